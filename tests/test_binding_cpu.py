"""The ctypes face of the library against include/polypolish_hip.h (no GPU; needs only the built library): the one table of
signatures (polypolish_amd/_abi.py: SIGNATURES) has every declared symbol with as many argtypes as the declaration has
parameters, and a restype wherever the ctypes default (int) would truncate or invent a value; the internal hooks the Python side
uses (HOOKS) exist in the built library; and the package still has every public name it had before the binding was folded."""
import ctypes as C
import os
import re

import polypolish_amd as pp


def _declarations():
    """[(name, return type, number of parameters)] of every pp_* function the header declares, in its order"""
    text = open(os.path.join(pp.ROOT, "include", "polypolish_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    text = re.sub(r"^\s*#[^\n]*", "", text, flags=re.M)
    out = []
    for m in re.finditer(r"\b(pp_[a-z0-9_]+)\s*\(", text):
        depth, i = 1, m.end()
        while depth:  # the parameter list up to the matching parenthesis
            depth += {"(": 1, ")": -1}.get(text[i], 0)
            i += 1
        params = text[m.end():i - 1].strip()
        commas = sum(1 for j, ch in enumerate(params) if ch == "," and params.count("(", 0, j) == params.count(")", 0, j))
        start = max(text.rfind(ch, 0, m.start()) for ch in ";{}") + 1
        out.append((m.group(1), " ".join(text[start:m.start()].split()), 0 if params in ("", "void") else commas + 1))
    return out


def test_every_declared_symbol_has_its_signature():
    decl = _declarations()
    names = [d[0] for d in decl]
    assert len(names) == len(set(names)) and len(names) >= 120
    assert list(pp.SIGNATURES) == names, "the table lists the header's symbols, in the header's order"
    assert pp.EXPORTS == names
    L = pp.lib()
    wrong = {}
    for name, ret, n_params in decl:
        restype, argtypes = pp.SIGNATURES[name]
        if len(argtypes) != n_params:
            wrong[name] = f"{len(argtypes)} argtypes for {n_params} parameters"
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes or ()) == list(argtypes), f"lib() did not apply the table to {name}"
        if ret.endswith("*") or ret.split()[-1] in ("uint64_t", "uint32_t", "void"):
            assert restype is not C.c_int, f"{name} returns {ret}: the ctypes default would cut it to an int"
            assert (restype is None) == (ret == "void"), name
        else:
            assert ret == "int" and restype is C.c_int, (name, ret)
    assert not wrong, wrong
    for name, restype in (("pp_assembly_n_contigs", C.c_uint32), ("pp_names_count", C.c_uint64), ("pp_bam_offs_count", C.c_uint64)):
        assert pp.SIGNATURES[name][0] is restype, name
    for name in ("pp_device_count", "pp_version", "pp_bam_last_error"):
        assert pp.SIGNATURES[name][1] == [], name
    assert pp.SIGNATURES["pp_polish_reserve"][1] == [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64]
    assert pp.SIGNATURES["pp_debug_extra_free"][0] is None


def test_every_hook_is_in_the_built_library():
    L = pp.lib()
    assert not set(pp.HOOKS) & set(pp.SIGNATURES)
    for name, (restype, argtypes) in pp.HOOKS.items():
        assert name.endswith("_") and hasattr(L, name), f"{name}: an internal hook the binding uses is not in the library"
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == list(argtypes), name


# dir(polypolish_amd) of the commit before the binding was folded, without the underscore names and the imported modules
PUBLIC = """AlnBatch BamOffsets BamRecords Bgzf Bytes COMM_ID_BYTES Context ContigStats ERR_ARG ERR_HIP ERR_LIMIT ERR_NOT_ASCII ERR_PANIC
ERR_QUIT EXPORTS FILTER_RAW_FIELDS FilterFile FilterFileCounts FilterInput FilterLoaded FilterLoadedDevice FilterReport GatedBatch HERE
KernelTimes LIB_PATH MEM_DEVICE MEM_HOST MEM_PEER Names OK OPS PP_MAX_KERNELS Params Plan PolishOptions PolypolishError PositionsOut
PreparedBatch RAW_FIELDS REC_FIELDS ROOT RawBatch STATUS SamCounts ShardPart ShardPlan WO_DTYPE WO_MULTI_RUN aln_batch annotations bam_header
bam_walk bam_walk_device bam_walk_geometry bgzf_walk comm_unique_id filter filter_records gate_records ingest ingest_device lib pack_names
pack_seq4 polish prepare_batch prepare_records shard_count shard_split_host split_records window_order_mirror""".split()


def test_the_package_keeps_its_public_face():
    assert len(PUBLIC) == 72
    missing = [n for n in PUBLIC if not hasattr(pp, n)]
    assert not missing, missing
    for cls in (pp.ShardPart, pp.PreparedBatch, pp.GatedBatch, pp.Names, pp.BamOffsets, pp.Bgzf, pp.BamRecords, pp.Plan, pp.FilterLoaded,
                pp.FilterLoadedDevice, pp.Context):
        assert callable(cls.close) and cls.__doc__, cls
