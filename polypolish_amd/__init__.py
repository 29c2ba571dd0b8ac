"""polypolish_amd -- Python face of libpolypolish_hip.so (MI355X / gfx950).

The product is the C-ABI library (include/polypolish_hip.h) and the ``bin/polypolish`` CLI; this
package is a thin ctypes binding used by the tests, bench.py and anyone who wants to call the
hot path from Python.  It mirrors the reference's two drivers by name and argument meaning:

    polish(assembly, sam, ...)            <->  polish::polish  (src/polish.rs:26-38)
    filter(in1, in2, out1, out2, ...)     <->  filter::filter  (src/filter.rs:26-37)

There is no CPU fallback: importing works anywhere the shared library loads, but every compute
call needs a HIP device and raises ``PolypolishError`` otherwise.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os

import numpy as np

from ._abi import (COMM_ID_BYTES, HOOKS, PP_MAX_KERNELS, SIGNATURES, AlnBatch, Bytes, ContigStats, FilterFile, FilterFileCounts,  # noqa: F401
                   FilterInput, FilterReport, KernelTimes, Params, PolishOptions, PositionsOut, RawBatch, SamCounts, ShardPlan)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB_PATH = os.environ.get("PP_LIB_PATH") or os.path.join(HERE, "_build", "libpolypolish_hip.so")  # PP_LIB_PATH: kernel experiments

OK, ERR_QUIT, ERR_HIP, ERR_ARG, ERR_LIMIT, ERR_PANIC = 0, 1, 3, 4, 5, 101
ERR_NOT_ASCII = 6  # device text front ends only: bytes outside ASCII, the host parsers take such a file
MEM_HOST, MEM_DEVICE, MEM_PEER = 0, 1, 2
STATUS = ("kept", "changed", "low_depth", "none", "multiple", "too_close")
OPS = "MIDNSHP=X"


class PolypolishError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"[{code}] {msg}")
        self.code, self.msg = code, msg


_NONE = 0xFFFFFFFFFFFFFFFF  # what the C side leaves in a "which one was bad" output when there is none


def _no_index():
    return C.c_uint64(_NONE)


def _index(v):
    """a "which one was bad" output of a failed call: None when the C side named none"""
    return None if v.value == _NONE else int(v.value)


def _raise(rc, msg, **attrs):
    """raise PolypolishError(rc, msg) carrying the failed call's outputs as attributes (.bad_record, .n_rec, .end, ...)"""
    e = PolypolishError(rc, msg)
    for k, v in attrs.items():
        setattr(e, k, v)
    raise e


RAW_FIELDS = (("flag", np.uint16), ("read_id", np.uint64), ("contig", np.uint32), ("ref_start", np.uint32), ("nm", np.uint32),
              ("seq_off", np.uint64), ("seq_len", np.uint32), ("cig_off", np.uint64), ("n_cig", np.uint32), ("seq", np.uint8),
              ("cigar", np.uint32))


def _runs_of(b):
    """the run table of a batch's window-order mirror (pp_aln_batch.wo_run_end: HOST memory) as a numpy array"""
    if not b.wo_n_runs or not b.wo_run_end:
        return np.zeros(0, dtype=np.uint64)
    return np.ctypeslib.as_array(C.cast(b.wo_run_end, C.POINTER(C.c_uint64)), shape=(int(b.wo_n_runs),)).copy()


def aln_batch(n_aln, ptrs: dict, seq_bytes, n_cig_total):
    """pp_aln_batch from addresses (field name -> address; "seq4", "wo" optional) plus, optionally, ptrs["wo_runs"]: the ends
    of the mirror's runs (a sequence of integers, HOST: pp_aln_batch.wo_run_end)."""
    runs = ptrs.get("wo_runs")
    if runs is not None:
        runs = np.ascontiguousarray(runs, dtype=np.uint64)
    b = AlnBatch(n_aln, ptrs["contig"], ptrs["ref_start"], ptrs["k"], ptrs["seq_off"], ptrs["seq_len"],
                 ptrs["cig_off"], ptrs["n_cig"], ptrs["seq"], seq_bytes, ptrs["cigar"], n_cig_total, ptrs.get("seq4") or None,
                 ptrs.get("wo") or None, len(runs) if runs is not None and ptrs.get("wo") else 0,
                 runs.ctypes.data if runs is not None and len(runs) and ptrs.get("wo") else None)
    b._runs = runs  # (the C side reads it during pp_polish_add)
    return b


# one record of pp_aln_batch.wo (include/polypolish_hip.h: pp_wo_rec, 32 bytes)
WO_DTYPE = np.dtype([("contig", np.uint32), ("ref_start", np.uint32), ("k", np.uint32), ("seq_len", np.uint32),
                     ("seq_off", np.uint64), ("op0", np.uint32), ("file_idx", np.uint32)])
WO_MULTI_RUN = 0xFFFFFFFF


def window_order_mirror(recs, contig_off, used_per_file=None, window=2048):
    """pp_aln_batch.wo for a batch given as numpy arrays: its records in window order -- per SAM file (used_per_file: good
    records of every file; None = one file), the records that start in one 2048-position window adjacent, file order inside
    a window -- as the host ingest writes it."""
    n = len(recs["contig"])
    off = np.asarray(contig_off).astype(np.int64)
    n_win = max(1, (int(off[-1]) + window - 1) // window)
    c = np.minimum(recs["contig"].astype(np.int64), len(off) - 2)
    win = np.minimum((off[c] + recs["ref_start"].astype(np.int64)) // window, n_win - 1)
    file_of = np.zeros(n, dtype=np.int64)
    if used_per_file is not None:
        file_of = np.repeat(np.arange(len(used_per_file)), used_per_file)
    order = np.argsort(file_of * n_win + win, kind="stable")
    wo = np.zeros(n, dtype=WO_DTYPE)
    for k in ("contig", "ref_start", "k", "seq_len", "seq_off"):
        wo[k] = recs[k][order]
    first = recs["cigar"][np.minimum(recs["cig_off"][order].astype(np.int64), max(len(recs["cigar"]) - 1, 0))] if len(recs["cigar"]) else np.zeros(n, np.uint32)
    wo["op0"] = np.where(recs["n_cig"][order] == 1, first, WO_MULTI_RUN)
    wo["file_idx"] = order.astype(np.uint32)
    return wo


# every symbol include/polypolish_hip.h declares (tests check that the library exports them all)
EXPORTS = list(SIGNATURES)

_lib = None


def lib():
    """Load the HIP library; fails loudly if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: run `make` (or __graft_entry__.build()) first; "
                              "polypolish_amd has no pure-Python or CPU path")
        L = C.CDLL(LIB_PATH)
        for table, declared in ((SIGNATURES, True), (HOOKS, False)):
            for name, (restype, argtypes) in table.items():
                if declared or hasattr(L, name):  # (a declared symbol that is missing raises here)
                    f = getattr(L, name)
                    f.restype, f.argtypes = restype, argtypes
        _lib = L
    return _lib


REC_FIELDS = (("contig", np.uint32), ("ref_start", np.uint32), ("k", np.uint32), ("seq_off", np.uint64),
              ("seq_len", np.uint32), ("cig_off", np.uint64), ("n_cig", np.uint32), ("seq", np.uint8),
              ("cigar", np.uint32))


def _host(addr, n, dtype):
    """a numpy copy of n items of HOST memory at addr; no address or nothing there: an empty array"""
    dt = np.dtype(dtype)
    if not n or not addr:
        return np.zeros(0, dtype=dt)
    return np.ctypeslib.as_array(C.cast(addr, C.POINTER(C.c_uint8)), shape=(int(n) * dt.itemsize,)).copy().view(dt)


def _read_batch(b, fields, ctx=None, mirrors=(), full=False):
    """A batch view (AlnBatch / RawBatch) as {field: numpy array} over `fields` (REC_FIELDS / RAW_FIELDS): HOST pointers are
    copied (ctx None: an empty array where there is no pointer), DEVICE pointers downloaded through ctx (zeros where there is
    none).  mirrors: which of "seq4", "wo", "wo_runs" of an AlnBatch come along -- when the view has them, or always
    (zero-filled at their full size) with `full`."""
    get = _host if ctx is None else ctx.download
    n = int(b.n_rec if isinstance(b, RawBatch) else b.n_aln)
    sizes = {"seq": int(b.seq_bytes), "cigar": int(b.n_cig_total)}
    recs = {name: get(getattr(b, name), sizes.get(name, n), dt) for name, dt in fields}
    if "seq4" in mirrors and (full or b.seq4):  # the 4-bit mirror of the seq array (two bases per byte)
        recs["seq4"] = get(b.seq4, (sizes["seq"] + 1) // 2, np.uint8)
    if "wo" in mirrors and (full or (b.wo and n)):  # the window-order mirror of the records (pp_aln_batch.wo)
        recs["wo"] = get(b.wo, n, WO_DTYPE)
        if "wo_runs" in mirrors:
            recs["wo_runs"] = _runs_of(b) if b.wo else np.zeros(0, dtype=np.uint64)
    return recs


def _ptrs_of(b, fields, mirrors=False):
    """field name -> address (0 = none) of a batch view; mirrors: an AlnBatch's "seq4", "wo" and "wo_runs" (the run ends
    themselves, as aln_batch takes them) where it has them"""
    ptrs = {name: getattr(b, name) or 0 for name, _ in fields}
    if mirrors and b.seq4:
        ptrs["seq4"] = b.seq4
    if mirrors and b.wo:
        ptrs["wo"], ptrs["wo_runs"] = b.wo, _runs_of(b)
    return ptrs


class _Owned:
    """An object of the library that the Python object owns: ._p its handle, ._ctx the context it lives on (kept alive with
    it; None for host objects).  Subclasses name the symbol that frees it and, where there is one, its pp_*_kernel_ms."""
    _free = None
    _kernel_ms = None

    def __init__(self, ctx=None, handle=C.c_void_p):
        self._p, self._ctx = handle(), ctx

    def close(self):
        if self._p:
            getattr(lib(), self._free)(self._p)
            self._p = type(self._p)()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def kernel_ms(self):
        ms = C.c_float()
        self._ctx._chk(getattr(lib(), self._kernel_ms)(self._p, C.byref(ms)))
        return float(ms.value)

    def _stage_ms(self, hook, names, when=""):
        """the per-stage HIP-event times an internal hook (HOOKS) reports, one float per name"""
        ms = (C.c_float * len(names))()
        if getattr(lib(), hook)(self._p, ms):
            raise PolypolishError(ERR_ARG, "the context had no profiling on" + when)
        return {k: float(v) for k, v in zip(names, ms)}


def split_records(recs, cuts):
    """The records cut at the indices `cuts` into batches that are valid on their own: seq_off / cig_off relative to
    each batch's seq / cigar arrays (which hold exactly the bytes / runs its records refer to, re-packed)."""
    n = len(recs["contig"])
    edges = [0] + sorted(int(c) for c in (cuts or []) if 0 < int(c) < n) + [n]
    if len(edges) == 2:
        return [recs]
    out = []
    for lo, hi in zip(edges[:-1], edges[1:]):
        sl = recs["seq_len"][lo:hi].astype(np.int64)
        so = recs["seq_off"][lo:hi].astype(np.int64)
        nc = recs["n_cig"][lo:hi].astype(np.int64)
        co = recs["cig_off"][lo:hi].astype(np.int64)
        new_so = np.concatenate([[0], np.cumsum(sl)[:-1]]) if hi > lo else np.zeros(0, np.int64)
        new_co = np.concatenate([[0], np.cumsum(nc)[:-1]]) if hi > lo else np.zeros(0, np.int64)
        seq_idx = np.repeat(so - new_so, sl) + np.arange(int(sl.sum())) if hi > lo else np.zeros(0, np.int64)
        cig_idx = np.repeat(co - new_co, nc) + np.arange(int(nc.sum())) if hi > lo else np.zeros(0, np.int64)
        part = {k: np.ascontiguousarray(recs[k][lo:hi]) for k in ("contig", "ref_start", "k", "seq_len", "n_cig")}
        part["seq_off"] = new_so.astype(np.uint64)
        part["cig_off"] = new_co.astype(np.uint64)
        part["seq"] = np.ascontiguousarray(recs["seq"][seq_idx]) if len(seq_idx) else np.zeros(0, np.uint8)
        part["cigar"] = np.ascontiguousarray(recs["cigar"][cig_idx]) if len(cig_idx) else np.zeros(0, np.uint32)
        out.append(part)
    return out


def _verdict_args(verdicts, i):
    """(pointer, count, the array it points into) of file i's filter verdicts: one byte per aligned record.  No verdicts for
    the file (None): (None, 0, None).  An empty array is a real pointer with a count of zero."""
    if verdicts is None or verdicts[i] is None:
        return None, 0, None
    v = np.ascontiguousarray(verdicts[i], dtype=np.uint8)
    buf = np.zeros(max(len(v), 1), dtype=np.uint8)
    buf[:len(v)] = v
    return buf.ctypes.data, len(v), buf


def _ingest(ctx, assembly, sams, max_errors, careful, seq_layout, expect, verdicts):
    """ingest() (ctx None: pp_ingest_*, errors in a text buffer) and ingest_device() (pp_dev_ingest_*, errors on the context)"""
    L = lib()
    err = C.create_string_buffer(1024)

    def chk_err(rc):
        if rc:
            raise PolypolishError(rc, err.value.decode())
    if ctx is None:  # only the host ingest's file calls report: a create that failed shows at the first file
        fn, head, tail, chk, chk_setup, mirrors = "pp_ingest_", (), (err, 1024), chk_err, (lambda rc: None), ("wo", "wo_runs")
    else:
        fn, head, tail, chk, chk_setup, mirrors = "pp_dev_ingest_", (ctx._h,), (), ctx._chk, ctx._chk, ("seq4", "wo", "wo_runs")
    a, g = C.c_void_p(), C.c_void_p()
    chk_err(L.pp_assembly_load(str(assembly).encode(), C.byref(a), err, 1024))
    try:
        n = L.pp_assembly_n_contigs(a)
        names = [L.pp_assembly_name(a, i).decode() for i in range(n)]
        descs = [L.pp_assembly_description(a, i).decode() for i in range(n)]
        off = np.ctypeslib.as_array(L.pp_assembly_offsets(a), shape=(n + 1,)).copy()
        bases = np.ctypeslib.as_array(L.pp_assembly_bases(a), shape=(int(off[-1]),)).copy()
        chk_setup(getattr(L, fn + "create")(*head, a, max_errors, int(careful), C.byref(g)))
        if seq_layout is not None:
            chk_setup(getattr(L, fn + "set_seq_layout")(g, int(seq_layout)))
        if expect is not None:
            chk_setup(L.pp_dev_ingest_expect(g, int(expect)))
        counts = []
        for s in sams:
            c = SamCounts()
            vp, nv, _keep = _verdict_args(verdicts, len(counts))
            if _keep is not None:
                chk(getattr(L, fn + "sam_filtered")(g, str(s).encode(), vp, nv, C.byref(c), *tail))
            else:
                chk(getattr(L, fn + "sam")(g, str(s).encode(), C.byref(c), *tail))
            counts.append((c.alignments, c.used, c.reads))
        b = AlnBatch()
        getattr(L, fn + "batch")(g, C.byref(b))
        return names, descs, off, bases, _read_batch(b, REC_FIELDS, ctx, mirrors), counts
    finally:
        if g:
            getattr(L, fn + "free")(g)
        L.pp_assembly_free(a)


def ingest(assembly, sams, max_errors=10, careful=False, seq_layout=None, verdicts=None):
    """Host ingest only (no GPU needed): FASTA + SAM text -> (names, descs, contig_off, bases, recs, counts).
    seq_layout: None = the library's default (window-grouped unless PP_SEQ_LAYOUT=file), 0 = SEQ bytes in file order,
    1 = window-grouped (pp_ingest_set_seq_layout).  verdicts: per file None or the filter's verdict byte of every aligned
    record (pp_ingest_sam_filtered)."""
    return _ingest(None, assembly, sams, max_errors, careful, seq_layout, None, verdicts)


_SEQ4_LUT = np.full(256, 15, dtype=np.uint8)
for _c, _v in ((ord("A"), 0), (ord("C"), 1), (ord("T"), 2), (ord("G"), 3), (ord("N"), 4), (ord("-"), 5)):
    _SEQ4_LUT[_c] = _v


def pack_seq4(seq):
    """The 4-bit mirror of a seq array (pp_aln_batch.seq4): base i in bits 4*(i&1).. of byte i >> 1, codes PP_SEQ4_*;
    32 bytes of slack behind, as the header asks for."""
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    codes = _SEQ4_LUT[seq]
    if codes.size & 1:
        codes = np.concatenate([codes, np.zeros(1, np.uint8)])
    out = np.zeros(codes.size // 2 + 32, dtype=np.uint8)
    out[:codes.size // 2] = codes[0::2] | (codes[1::2] << 4)
    return out


def ingest_device(ctx, assembly, sams, max_errors=10, careful=False, seq_layout=None, expect=None, verdicts=None):
    """The device tokenizer (pp_dev_ingest_*): same return value as ingest(), the records copied back from HBM.
    seq_layout: None = the library's default (window-grouped unless PP_SEQ_LAYOUT=file), 0 = SEQ bytes in file order,
    1 = window-grouped (pp_dev_ingest_set_seq_layout).  expect: the text bytes of all the files, announced before the first
    one (pp_dev_ingest_expect).  verdicts: per file None or the filter's verdict byte of every aligned record
    (pp_dev_ingest_sam_filtered)."""
    return _ingest(ctx, assembly, sams, max_errors, careful, seq_layout, expect, verdicts)


class Plan(_Owned):
    """pp_shard_plan: which rank polishes which contig / window of a contig (no GPU needed).
    aln_per_contig: alignment records per contig (e.g. np.bincount(recs["contig"], minlength=n_contigs))."""
    _free = "pp_shard_plan_free"

    def __init__(self, contig_off, aln_per_contig, world, min_window=0):
        self.contig_off = np.ascontiguousarray(contig_off, dtype=np.uint64)
        self.n_contigs = len(self.contig_off) - 1
        cnt = np.ascontiguousarray(aln_per_contig, dtype=np.uint64)
        assert len(cnt) == self.n_contigs
        super().__init__(None, C.POINTER(ShardPlan))
        rc = lib().pp_shard_plan_create(self.n_contigs, self.contig_off.ctypes.data, cnt.ctypes.data, world, min_window,
                                        C.byref(self._p))
        if rc:
            raise PolypolishError(rc, "pp_shard_plan_create failed")
        p = self._p.contents
        n = p.n_units
        self.world = world
        self.unit_contig = np.ctypeslib.as_array(p.contig, shape=(n,)).copy()
        self.unit_lo = np.ctypeslib.as_array(p.lo, shape=(n,)).copy()
        self.unit_hi = np.ctypeslib.as_array(p.hi, shape=(n,)).copy()
        self.unit_rank = np.ctypeslib.as_array(p.rank, shape=(n,)).copy()

    def emit_ranges(self, rank):
        """(n_contigs, 2) array of [lo, hi) the rank emits per contig (pp_polish_set_emit's form)."""
        lo = np.zeros(self.n_contigs, dtype=np.uint64)
        hi = np.zeros(self.n_contigs, dtype=np.uint64)
        rc = lib().pp_shard_emit_ranges(self._p, rank, lo.ctypes.data, hi.ctypes.data)
        if rc:
            raise PolypolishError(rc, "pp_shard_emit_ranges failed")
        return np.stack([lo, hi], axis=1)

    def assemble(self, rank_bytes, rank_contig_off):
        """Polished bytes of all ranks (what each rank's Context.result() gave) -> (bytes in assembly order, offsets)."""
        bufs = [np.frombuffer(b, dtype=np.uint8) if len(b) else np.zeros(1, np.uint8) for b in rank_bytes]
        offs = [np.ascontiguousarray(o, dtype=np.uint64) for o in rank_contig_off]
        bp = (C.c_void_p * self.world)(*[b.ctypes.data for b in bufs])
        op = (C.c_void_p * self.world)(*[o.ctypes.data for o in offs])
        out_off = np.zeros(self.n_contigs + 1, dtype=np.uint64)
        L = lib()
        rc = L.pp_shard_assemble(self._p, bp, op, None, out_off.ctypes.data)
        out = np.zeros(max(int(out_off[-1]), 1), dtype=np.uint8)
        if rc == 0:
            rc = L.pp_shard_assemble(self._p, bp, op, out.ctypes.data, out_off.ctypes.data)
        if rc:
            raise PolypolishError(rc, "pp_shard_assemble failed")
        return out[:int(out_off[-1])].tobytes(), out_off


class ShardPart(_Owned):
    """pp_shard_split: the records of a batch that rank `dest` of a plan needs (its contigs' records; on a tiled contig
    its window's records plus those that reach in from the neighbours).  The batch is given as raw pointers
    (`ptrs`: field name -> address, host or device as `mem` says); `ctx` may be None for host memory.
      .n_aln, .seq_bytes, .n_cig_total, .ptrs (field name -> address of the part's arrays, same memory kind), .orig_ptr
      .host() -> (recs dict of numpy arrays, orig) for a host part.
    wo_idx_base (internal hook, pp_shard_split_view_): what the file_idx of the batch's mirror count from, for a batch that is
    a view on records [lo, hi) of a larger one (the one-process multi-GPU driver's pieces)."""
    _free = "pp_shard_part_free"

    def __init__(self, ctx, plan, dest, n_aln, ptrs, seq_bytes, n_cig_total, mem, wo_idx_base=0):
        L = lib()
        b = aln_batch(n_aln, ptrs, seq_bytes, n_cig_total)  # (ptrs["wo_runs"]: the mirror's runs go along, restricted)
        super().__init__(ctx)  # (the context, and with it the part's device memory, stays alive)
        h = ctx._h if ctx is not None else None
        if wo_idx_base:
            rc = L.pp_shard_split_view_(h, plan._p, dest, C.byref(b), mem, wo_idx_base, C.byref(self._p))
        else:
            rc = L.pp_shard_split(h, plan._p, dest, C.byref(b), mem, C.byref(self._p))
        if rc:
            raise PolypolishError(rc, L.pp_last_error(ctx._h).decode() if ctx is not None else "pp_shard_split failed")
        out, orig = AlnBatch(), C.c_void_p()
        L.pp_shard_part_batch(self._p, C.byref(out), C.byref(orig))
        self.mem, self._view = mem, out
        self.n_aln, self.seq_bytes, self.n_cig_total = int(out.n_aln), int(out.seq_bytes), int(out.n_cig_total)
        # a device part brings the 4-bit mirror of its seq array, and every part the window-order mirror of its records when the
        # source batch has one -- with its runs, when the source's are known: the part takes the direct path too
        self.ptrs = _ptrs_of(out, REC_FIELDS, mirrors=True)
        if "wo_runs" in self.ptrs and not len(self.ptrs["wo_runs"]):
            del self.ptrs["wo_runs"]
        self.orig_ptr = orig.value or 0

    def host(self):
        assert self.mem == MEM_HOST
        return _read_batch(self._view, REC_FIELDS, None, ("wo",)), _host(self.orig_ptr, self.n_aln, np.uint32)


def shard_split_host(plan, dest, recs, wo_idx_base=0):
    """Host numpy SoA -> (recs of the part, orig).  recs["wo"] (the window-order mirror, WO_DTYPE) goes along when it is there,
    and recs["wo_runs"] (the ends of its runs) with it.  wo_idx_base: see ShardPart."""
    keep = {k: np.ascontiguousarray(recs[k], dtype=dt) for k, dt in REC_FIELDS}
    ptrs = {k: v.ctypes.data for k, v in keep.items()}
    if "wo" in recs and len(recs["wo"]):
        keep["wo"] = np.ascontiguousarray(recs["wo"])
        ptrs["wo"] = keep["wo"].ctypes.data
        if recs.get("wo_runs") is not None and len(recs["wo_runs"]):  # the mirror's runs: restricted along with it
            ptrs["wo_runs"] = recs["wo_runs"]
    part = ShardPart(None, plan, dest, len(keep["contig"]), ptrs, len(keep["seq"]),
                     len(keep["cigar"]), MEM_HOST, wo_idx_base)
    out = part.host()
    if "wo_runs" in part.ptrs and "wo" in out[0]:
        out[0]["wo_runs"] = part.ptrs["wo_runs"]
    part.close()
    return out


class PreparedBatch(_Owned):
    """pp_batch_prepare: any valid batch (raw pointers `ptrs`: field name -> address, host or device as `mem` says) laid out
    on the device as the library's ingests lay theirs out -- window-grouped SEQ rooms, the 4-bit mirror, the window-order mirror
    as one run -- and owned by this object: the way to the direct path for a batch the caller made.
      .n_aln, .seq_bytes, .n_cig_total
      .ptrs()       what Context.polish_add_ptrs / prepared_job take, with mem = MEM_DEVICE (valid until close())
      .host()       numpy copies of every array, "wo", "wo_runs" and "seq4" included
      .kernel_ms()  HIP-event time of the prepare's kernels (the context had set_profiling on)"""
    _free, _kernel_ms = "pp_prepared_free", "pp_prepared_kernel_ms"

    def __init__(self, ctx, contig_off, n_aln, ptrs, seq_bytes, n_cig_total, mem):
        L = lib()
        off = np.ascontiguousarray(contig_off, dtype=np.uint64)
        b = aln_batch(n_aln, ptrs, seq_bytes, n_cig_total)
        super().__init__(ctx)  # (the context, and with it the batch's device memory, stays alive)
        ctx._chk(L.pp_batch_prepare(ctx._h, len(off) - 1, off.ctypes.data, C.byref(b), mem, C.byref(self._p)))
        out = AlnBatch()
        L.pp_prepared_batch(self._p, C.byref(out))
        self.mem, self._view = MEM_DEVICE, out
        self.n_aln, self.seq_bytes, self.n_cig_total = int(out.n_aln), int(out.seq_bytes), int(out.n_cig_total)
        self._ptrs = _ptrs_of(out, REC_FIELDS, mirrors=True)

    def ptrs(self):
        return dict(self._ptrs)

    def host(self):
        return _read_batch(self._view, REC_FIELDS, self._ctx, ("seq4", "wo", "wo_runs"), full=True)


def prepare_batch(ctx, contig_off, n_aln, ptrs, seq_bytes, n_cig_total, mem):
    """pp_batch_prepare on a batch given by pointers: returns a PreparedBatch."""
    return PreparedBatch(ctx, contig_off, n_aln, ptrs, seq_bytes, n_cig_total, mem)


def prepare_records(ctx, contig_off, recs):
    """pp_batch_prepare on host numpy records (field names of pp_aln_batch, REC_FIELDS), as Context.polish_records takes them."""
    keep = {k: np.ascontiguousarray(recs[k], dtype=dt) for k, dt in REC_FIELDS}
    ptrs = {k: v.ctypes.data for k, v in keep.items()}
    return PreparedBatch(ctx, contig_off, len(keep["contig"]), ptrs, len(keep["seq"]), len(keep["cigar"]), MEM_HOST)


def _raw_batch(raw, host, fields):
    """(RawBatch, what it points into) of raw records.  host: raw = numpy arrays by the names of `fields` -- those of RAW_FIELDS the
    callee reads; without "seq" among them seq_bytes is 0.  Else raw = device addresses, those of `fields` at least, plus "n_rec",
    "seq_bytes" and "n_cig_total"."""
    if host:
        keep = {k: np.ascontiguousarray(raw[k], dtype=dt) for k, dt in fields}
        ptrs = {k: v.ctypes.data for k, v in keep.items()}
        n_rec, seq_bytes, n_cig_total = len(keep["flag"]), len(keep["seq"]) if "seq" in keep else 0, len(keep["cigar"])
    else:
        keep, ptrs, n_rec, seq_bytes, n_cig_total = None, raw, int(raw["n_rec"]), int(raw["seq_bytes"]), int(raw["n_cig_total"])
    need = {k for k, _ in fields}
    arrays = {k: ptrs[k] if k in need else ptrs.get(k) for k, _ in RAW_FIELDS}
    return RawBatch(n_rec=n_rec, seq_bytes=seq_bytes, n_cig_total=n_cig_total, **arrays), keep


class GatedBatch(_Owned):
    """pp_batch_gate: the good records of one SAM file's raw records (process_one_read on the device), owned by this object.
      .n_aln, .seq_bytes, .n_cig_total
      .counts       (alignments, used, reads) as add_to_pileup counts them
      .ptrs()       what Context.polish_add_ptrs / prepare_batch take, with mem = MEM_DEVICE (valid until close())
      .host()       numpy copies of the nine arrays
      .orig()       the index in the raw batch of every good record
      .kernel_ms()  HIP-event time of the gate's kernels (the context had set_profiling on)"""
    _free, _kernel_ms = "pp_gated_free", "pp_gated_kernel_ms"

    def __init__(self, ctx, raw, max_errors=10, careful=False, passed=None, mem=MEM_HOST):
        L = lib()
        b, _keep = _raw_batch(raw, mem == MEM_HOST, RAW_FIELDS)
        v = None if passed is None else np.ascontiguousarray(passed, dtype=np.uint8)
        super().__init__(ctx)
        bad = _no_index()
        rc = L.pp_batch_gate(ctx._h, C.byref(b), mem, max_errors, int(bool(careful)), v.ctypes.data if v is not None else None,
                             len(v) if v is not None else 0, C.byref(self._p), C.byref(bad))
        if rc:
            _raise(rc, L.pp_last_error(ctx._h).decode(), bad_record=_index(bad))
        out, orig, cnt = AlnBatch(), C.c_void_p(), SamCounts()
        L.pp_gated_batch(self._p, C.byref(out), C.byref(orig))
        L.pp_gated_counts(self._p, C.byref(cnt))
        self.mem, self._view = MEM_DEVICE, out
        self.counts = (int(cnt.alignments), int(cnt.used), int(cnt.reads))
        self.n_aln, self.seq_bytes, self.n_cig_total = int(out.n_aln), int(out.seq_bytes), int(out.n_cig_total)
        self._ptrs = _ptrs_of(out, REC_FIELDS)
        self._orig = orig.value or 0

    def ptrs(self):
        return dict(self._ptrs)

    def host(self):
        return _read_batch(self._view, REC_FIELDS, self._ctx)

    def orig(self):
        return self._ctx.download(self._orig, self.n_aln, np.uint32)


def gate_records(ctx, raw: dict, max_errors=10, careful=False, passed=None, mem=MEM_HOST):
    """pp_batch_gate on the raw records of ONE SAM file.  mem = MEM_HOST: raw = numpy arrays by the field names of pp_raw_batch
    (RAW_FIELDS); MEM_DEVICE: raw = their device addresses plus "n_rec", "seq_bytes", "n_cig_total".  passed: None or the
    filter's verdict byte of every aligned record (host).  A failing call raises PolypolishError with .bad_record."""
    return GatedBatch(ctx, raw, max_errors, careful, passed, mem)


class Regrouped(_Owned):
    """pp_batch_regroup: the raw records of ONE file with every read's records brought together (groups in the order of their first
    record, file order inside a group), in DEVICE memory.  With mem = MEM_DEVICE seq and cigar stay borrowed from `raw`, which must
    outlive this object, and when nothing moves the view is raw's own arrays.
      .n_rec, .seq_bytes, .n_cig_total
      .raw()               the device-address dict gate_records(..., mem=MEM_DEVICE) takes (valid until close())
      .host()              numpy copies of the view's arrays
      .perm()              np.uint32: output record j is raw record perm[j]
      .counts()            (distinct read_ids, records that changed place)
      .carry_pass(passed)  one byte per ALIGNED record of `raw` -> the same verdicts in the numbering of the regrouped records
      .kernel_ms()         HIP-event time of the kernels (the context had set_profiling on); .stage_ms(): intern | sort | gather"""
    _free, _kernel_ms = "pp_regrouped_free", "pp_regrouped_kernel_ms"

    def __init__(self, ctx, raw, mem=MEM_HOST):
        L = lib()
        b, _keep = _raw_batch(raw, mem == MEM_HOST, RAW_FIELDS)
        super().__init__(ctx)
        ctx._chk(L.pp_batch_regroup(ctx._h, C.byref(b), mem, C.byref(self._p)))
        out = self._view = RawBatch()
        L.pp_regrouped_raw(self._p, C.byref(out))
        self.n_rec, self.seq_bytes, self.n_cig_total = int(out.n_rec), int(out.seq_bytes), int(out.n_cig_total)
        self._ptrs = _ptrs_of(out, RAW_FIELDS)

    def raw(self):
        return dict(self._ptrs, n_rec=self.n_rec, seq_bytes=self.seq_bytes, n_cig_total=self.n_cig_total)

    def host(self):
        return _read_batch(self._view, RAW_FIELDS, self._ctx)

    def perm(self):
        return self._ctx.download(lib().pp_regrouped_perm(self._p), self.n_rec, np.uint32)

    def counts(self):
        g, m = C.c_uint64(0), C.c_uint64(0)
        lib().pp_regrouped_counts(self._p, C.byref(g), C.byref(m))
        return int(g.value), int(m.value)

    def carry_pass(self, passed):
        v = np.ascontiguousarray(passed, dtype=np.uint8)
        out = np.zeros(max(len(v), 1), dtype=np.uint8)
        self._ctx._chk(lib().pp_regrouped_pass(self._p, v.ctypes.data if len(v) else None, len(v), out.ctypes.data))
        return out[:len(v)]

    def stage_ms(self):
        return self._stage_ms("pp_regrouped_stage_ms_", ("intern", "sort", "gather"), " when the batch was regrouped")


def regroup_records(ctx, raw: dict, mem=MEM_HOST):
    """pp_batch_regroup on the raw records of ONE file (in front of gate_records, for a file whose reads do not stand together:
    coordinate-sorted BAM).  raw and mem as gate_records takes them.  Returns a Regrouped."""
    return Regrouped(ctx, raw, mem)


def regroup_geometry():
    """records per tile of the regroup's radix sort: the seam its tests are built on"""
    t = C.c_uint32()
    lib().pp_regroup_geometry_(C.byref(t))
    return int(t.value)


def pack_names(names):
    """a list of bytes / str -> (bytes, off, len): the names back to back, as pp_names_ids takes them"""
    raw = [n.encode() if isinstance(n, str) else bytes(n) for n in names]
    ln = np.array([len(r) for r in raw], dtype=np.uint32)
    off = (np.cumsum(ln, dtype=np.uint64) - ln).astype(np.uint64)
    return np.frombuffer(b"".join(raw), dtype=np.uint8), off, ln


class Names(_Owned):
    """pp_names: a set of byte strings with dense ids on the device -- QNAME -> pp_raw_batch.read_id, RNAME -> .contig.
      .ids(names)   names = a list of bytes / str, or (bytes, off, len): numpy arrays (mem = MEM_HOST) or device addresses
                    (MEM_DEVICE, with n = names, n_bytes = bytes of the array, out = device address of n uint64 -- or, with
                    out left None, out32 = device address of n uint32: SamRecords.contig_ptr).  Returns the
                    ids as a np.uint64 array: the number of distinct names in front of a name's first occurrence, over all calls.
                    A name whose range lies outside the array raises PolypolishError with .bad = its index.
      .count        distinct names held
      .name(id)     the bytes of a name
      .kernel_ms()  HIP-event time of the last ids() (the context had set_profiling on)"""
    _free, _kernel_ms = "pp_names_free", "pp_names_kernel_ms"

    def __init__(self, ctx, expect=0):
        super().__init__(ctx)
        ctx._chk(lib().pp_names_create(ctx._h, int(expect), C.byref(self._p)))

    def ids(self, names, mem=MEM_HOST, n=None, n_bytes=None, out=None, out32=None):
        L = lib()
        if isinstance(names, tuple) and len(names) == 3 and mem != MEM_HOST and out is None and out32:
            bp, op, lp = names      # the ids as n uint32 at out32 (pp_raw_batch.contig): id32 alone
            bad = _no_index()
            rc = L.pp_names_ids(self._p, bp, int(n_bytes), op, lp, int(n), mem, None, out32, C.byref(bad))
            if rc:
                _raise(rc, L.pp_last_error(self._ctx._h).decode(), bad=_index(bad))
            return self._ctx.download(out32, int(n), np.uint32).astype(np.uint64)
        if isinstance(names, tuple) and len(names) == 3 and mem != MEM_HOST:
            bp, op, lp = names
            n, n_bytes = int(n), int(n_bytes)
            res, dst = np.zeros(n, dtype=np.uint64), out
        else:
            if not (isinstance(names, tuple) and len(names) == 3 and all(isinstance(a, np.ndarray) for a in names)):
                names = pack_names(names)
            b, o, ln = (np.ascontiguousarray(a, dtype=dt) for a, dt in zip(names, (np.uint8, np.uint64, np.uint32)))
            n, n_bytes = len(o), len(b)
            res = np.zeros(n, dtype=np.uint64)
            bp, op, lp, dst = (b.ctypes.data if n_bytes else None), o.ctypes.data, ln.ctypes.data, res.ctypes.data
        bad = _no_index()
        rc = L.pp_names_ids(self._p, bp, n_bytes, op, lp, n, mem, dst, None, C.byref(bad))
        if rc:
            _raise(rc, L.pp_last_error(self._ctx._h).decode(), bad=_index(bad))
        return res if mem == MEM_HOST else self._ctx.download(dst, n, np.uint64)

    @property
    def count(self):
        return int(lib().pp_names_count(self._p))

    def name(self, id):  # noqa: A002 (the header's word)
        ln = C.c_uint32(0)
        buf = np.zeros(256, dtype=np.uint8)
        rc = lib().pp_names_name(self._p, int(id), buf.ctypes.data, len(buf), C.byref(ln))
        if rc and int(id) < self.count and ln.value > len(buf):     # a long name: once more with room for it
            buf = np.zeros(ln.value, dtype=np.uint8)
            rc = lib().pp_names_name(self._p, int(id), buf.ctypes.data, len(buf), C.byref(ln))
        self._ctx._chk(rc)
        return buf[:ln.value].tobytes()


def _bam_bytes(data):
    """uncompressed BAM bytes as a contiguous uint8 array (no copy of an array that already is one)"""
    if isinstance(data, np.ndarray):
        return np.ascontiguousarray(data, dtype=np.uint8)
    return np.frombuffer(bytes(data), dtype=np.uint8)


def bam_header(data):
    """pp_bam_header (no device needed): {"names": [bytes], "name_off", "name_len", "ref_len": numpy arrays, "records_at": int} of
    uncompressed BAM bytes; a truncated or inconsistent header raises PolypolishError(ERR_ARG)."""
    L = lib()
    b = _bam_bytes(data)
    n_ref, at = C.c_uint32(0), C.c_uint64(0)
    rc = L.pp_bam_header(b.ctypes.data if len(b) else None, len(b), 0, C.byref(n_ref), None, None, None, C.byref(at))
    n = int(n_ref.value)
    off, ln, rl = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    if n:
        rc = L.pp_bam_header(b.ctypes.data, len(b), n, C.byref(n_ref), off.ctypes.data, ln.ctypes.data, rl.ctypes.data, C.byref(at))
    if rc:
        raise PolypolishError(rc, L.pp_bam_last_error().decode())
    return {"names": [b[int(o):int(o) + int(k)].tobytes() for o, k in zip(off, ln)], "name_off": off, "name_len": ln, "ref_len": rl,
            "records_at": int(at.value)}


def _walk_host(fn, data, start, extra, count):
    """The two passes of a host chain walk (pp_bam_walk, pp_bgzf_walk): count the links, then fill one uint64 array per entry of
    `extra`, of links + extra entries.  -> (arrays, end).  A chain that breaks raises with .<count> = the links in front of the
    break and .end = its offset."""
    L = lib()
    b = _bam_bytes(data)
    n, end = C.c_uint64(0), C.c_uint64(0)
    bp = b.ctypes.data if len(b) else None
    rc = fn(bp, len(b), int(start), *[None] * len(extra), 0, C.byref(n), C.byref(end))
    if rc:
        _raise(rc, L.pp_bam_last_error().decode(), **{count: int(n.value), "end": int(end.value)})
    out = [np.zeros(int(n.value) + x, np.uint64) for x in extra]
    if n.value:
        rc = fn(bp, len(b), int(start), *[a.ctypes.data for a in out], int(n.value), C.byref(n), C.byref(end))
        if rc:
            raise PolypolishError(rc, L.pp_bam_last_error().decode())
    return out, int(end.value)


def bam_walk(data, start=0):
    """pp_bam_walk (no device needed): (rec_off: np.uint64 array, end) -- the offset of every record's block_size word from `start`
    on, and the first byte not consumed.  A chain that breaks raises PolypolishError(ERR_ARG) with .n_rec = the records in front
    of the break and .end = its offset."""
    (off,), end = _walk_host(lib().pp_bam_walk, data, start, (0,), "n_rec")
    return off, end


def _bytes_and_offsets(data, off, mem):
    """(bytes_ptr, n_bytes, off_ptr, n, what the pointers point into) of "bytes plus optional offsets".  MEM_HOST: data = bytes /
    a uint8 array, off = None or the offsets; else data = (device address, n_bytes), off = None or (device address of n uint64, n)."""
    if mem != MEM_HOST:
        op, n = (None, 0) if off is None else (int(off[0]), int(off[1]))
        return int(data[0]) or None, int(data[1]), op, n, None
    b = _bam_bytes(data)
    o = None if off is None else np.ascontiguousarray(off, dtype=np.uint64)
    n = 0 if o is None else len(o)
    if o is not None and n == 0:
        o = np.zeros(1, dtype=np.uint64)     # (an array without entries still is one: no walk)
    return (b.ctypes.data if len(b) else None), len(b), (None if o is None else o.ctypes.data), n, (b, o)


class BamOffsets(_Owned):
    """pp_bam_walk_device: the block_size chain of uncompressed BAM bytes walked on the device; the offsets stay in DEVICE memory,
    owned by this object.
      data           mem = MEM_HOST: bytes / a uint8 array; MEM_DEVICE: (device address, n_bytes), borrowed for the call
      .ptr, .n_rec   BamRecords(ctx, (bytes_ptr, n_bytes), (offs.ptr, offs.n_rec), ref_map, mem=MEM_DEVICE)
      .end           the first byte not consumed
      .host()        a numpy copy of the offsets (a download)
      .kernel_ms()   HIP-event time of the walk's kernels (the context had set_profiling on); .stage_ms(): tables | chain | offsets
      .stats()       along the true chain: {"chain": chunks on it, "zone": entered through a zone table, "slow": walked record by
                     record behind a zone, "pass": passed through}
    A chain that breaks raises PolypolishError(ERR_ARG) with .n_rec = the records in front of the break and .end = its offset, as
    bam_walk does; the text behind "pp_bam_walk_device: " is bam_walk's."""
    _free, _kernel_ms = "pp_bam_offs_free", "pp_bam_offs_kernel_ms"

    def __init__(self, ctx, data, start=0, mem=MEM_HOST):
        L = lib()
        bp, n_bytes, _, _, _keep = _bytes_and_offsets(data, None, mem)
        super().__init__(ctx)
        n, end = C.c_uint64(0), C.c_uint64(0)
        rc = L.pp_bam_walk_device(ctx._h, bp, n_bytes, int(start), mem, C.byref(self._p), C.byref(n), C.byref(end))
        if rc:
            _raise(rc, L.pp_last_error(ctx._h).decode(), n_rec=int(n.value), end=int(end.value))
        self.ptr, self.n_rec, self.end = L.pp_bam_offs_dev(self._p) or 0, int(L.pp_bam_offs_count(self._p)), int(end.value)

    def host(self):
        return self._ctx.download(self.ptr, self.n_rec, np.uint64)

    def stage_ms(self):
        return self._stage_ms("pp_bam_offs_stage_ms_", ("tables", "chain", "offsets"), " when the chain was walked")

    def stats(self):
        out = (C.c_uint64 * 4)()
        if lib().pp_bam_offs_stats_(self._p, out):
            raise PolypolishError(ERR_ARG, "pp_bam_offs_stats_: no object")
        return {"chain": int(out[0]), "zone": int(out[1]), "slow": int(out[2]), "pass": int(out[3])}


def bam_walk_device(ctx, data, start=0, mem=MEM_HOST):
    """pp_bam_walk_device: -> BamOffsets"""
    return BamOffsets(ctx, data, start, mem)


def bam_walk_geometry():
    """(bytes per chunk, offsets of a chunk's entry zone, chunks per group) of the device walk: the seams its tests are built on"""
    c, z, g = C.c_uint32(), C.c_uint32(), C.c_uint32()
    lib().pp_bam_walk_geometry_(C.byref(c), C.byref(z), C.byref(g))
    return int(c.value), int(z.value), int(g.value)


def bgzf_walk(data, start=0):
    """pp_bgzf_walk (no device needed): (blk_off, out_off, end) -- the offset of every BGZF block from `start` on, the sum of the
    ISIZEs in front of every block (one more entry: the sum of all), and the first byte not consumed.  A chain that breaks raises
    PolypolishError(ERR_ARG) with .n_blk = the blocks in front of the break and .end = its offset."""
    (off, out), end = _walk_host(lib().pp_bgzf_walk, data, start, (0, 1), "n_blk")
    return off, out, end


ALN_SAM, ALN_BAM, ALN_BAM_RAW, ALN_SAM_BGZF = 0, 1, 2, 3


def aln_file_kind(path):
    """pp_aln_file_kind (no device needed): ALN_SAM, ALN_BAM (BGZF that holds BAM) or ALN_BAM_RAW (uncompressed BAM), told by the
    head of the file.  gzip that is not BGZF, BGZF that does not hold BAM, a file cut inside its gzip header and a path that cannot be
    read raise PolypolishError(ERR_QUIT).  Context.polish_files / filter_files / filter_polish_files ask this themselves."""
    L = lib()
    kind = C.c_int(0)
    rc = L.pp_aln_file_kind(os.fsencode(path), C.byref(kind))
    if rc:
        raise PolypolishError(rc, L.pp_bam_last_error().decode())
    return int(kind.value)


def aln_file_kind_text(path):
    """pp_aln_file_kind_text (no device needed): aln_file_kind for a caller who reads bgzipped SAM text as well -- BGZF that does not
    hold BAM is ALN_SAM_BGZF instead of an error.  What the commands ask with text_chain=True."""
    L = lib()
    kind = C.c_int(0)
    rc = L.pp_aln_file_kind_text(os.fsencode(path), C.byref(kind))
    if rc:
        raise PolypolishError(rc, L.pp_bam_last_error().decode())
    return int(kind.value)


class Bgzf(_Owned):
    """pp_bgzf_inflate: the BGZF blocks of a file inflated into one dense array in DEVICE memory, owned by this object.
      data, blk_off  mem = MEM_HOST: bytes / a uint8 array, and the blocks' offsets (None: the library walks the chain from offset 0);
                     MEM_DEVICE: data = (device address, n_bytes), blk_off = (device address of n uint64, n)
      .n_bytes, .bytes_ptr   the inflated bytes: BamRecords(ctx, (z.bytes_ptr, z.n_bytes), (rec_off_ptr, n_rec), ref_map, mem=MEM_DEVICE)
      .host(lo, hi)  a numpy copy of the inflated bytes [lo, hi) (a download)
      .bam_walk(start)   pp_bgzf_bam_walk: (rec_off_ptr, n_rec, end); a chain that breaks raises with .n_rec and .end
      .kernel_ms()   HIP-event time of the stages so far (the context had set_profiling on); .stage_ms(): inflate | crc | walk (the
                     kernels of .bam_walk; "staging" is the same value under its earlier name)
    A failing call raises PolypolishError with .bad_block."""
    _free, _kernel_ms = "pp_bgzf_free", "pp_bgzf_kernel_ms"

    def __init__(self, ctx, data, blk_off=None, mem=MEM_HOST):
        L = lib()
        bp, n_bytes, op, n, _keep = _bytes_and_offsets(data, blk_off, mem)
        super().__init__(ctx)
        bad = _no_index()
        rc = L.pp_bgzf_inflate(ctx._h, bp, n_bytes, op, n, mem, C.byref(self._p), C.byref(bad))
        if rc:
            _raise(rc, L.pp_last_error(ctx._h).decode(), bad_block=_index(bad))
        dev, nb = C.c_void_p(), C.c_uint64(0)
        L.pp_bgzf_bytes(self._p, C.byref(dev), C.byref(nb))
        self.bytes_ptr, self.n_bytes = dev.value or 0, int(nb.value)

    def host(self, lo=0, hi=None):
        hi = self.n_bytes if hi is None else min(int(hi), self.n_bytes)
        lo = min(int(lo), hi)
        return self._ctx.download(self.bytes_ptr + lo, hi - lo, np.uint8)

    def bam_walk(self, start=0):
        L = lib()
        n, end = C.c_uint64(0), C.c_uint64(0)
        rc = L.pp_bgzf_bam_walk(self._p, int(start), C.byref(n), C.byref(end))
        if rc:
            _raise(rc, L.pp_last_error(self._ctx._h).decode(), n_rec=int(n.value), end=int(end.value))
        return L.pp_bgzf_rec_off(self._p) or 0, int(n.value), int(end.value)

    def stage_ms(self):
        ms = self._stage_ms("pp_bgzf_stage_ms_", ("inflate", "crc", "staging"), " when the blocks were inflated")
        return dict(ms, walk=ms["staging"])


class BamRecords(_Owned):
    """pp_bam_records: the alignment records of uncompressed BAM bytes as a raw batch in DEVICE memory, owned by this object.
      data, rec_off  mem = MEM_HOST: bytes / a uint8 array, and the records' offsets (None: the library walks the chain from offset 0);
                     MEM_DEVICE: data = (device address, n_bytes), rec_off = (device address of n uint64, n)
      ref_map        None, or n_ref + 1 contig ids (host): entry n_ref answers refID -1
      .n_rec, .seq_bytes, .n_cig_total
      .raw()         the device-address dict gate_records(..., mem=MEM_DEVICE) / filter_records(..., mem=MEM_DEVICE) take
      .names()       keyword arguments for Names.ids(mem=MEM_DEVICE, out=.read_id_ptr): the QNAMEs' ranges in the device bytes
      .read_id_ptr   device address of raw()["read_id"]: n_rec uint64, zero until filled
      .zp            np.uint8, one per ALIGNED record, 0 = the record carries ZP:Z:fail: gate_records' `passed` (AND the filter's)
      .host()        numpy copies of the arrays, and "name_off" / "name_len"
      .kernel_ms()   HIP-event time of the decode's kernels (the context had set_profiling on)
    A failing call raises PolypolishError with .bad_record."""
    _free, _kernel_ms = "pp_bam_free", "pp_bam_kernel_ms"

    def __init__(self, ctx, data, rec_off=None, ref_map=None, mem=MEM_HOST):
        L = lib()
        bp, n_bytes, op, n, _keep = _bytes_and_offsets(data, rec_off, mem)
        m = None if ref_map is None else np.ascontiguousarray(ref_map, dtype=np.uint32)
        super().__init__(ctx)
        bad = _no_index()
        rc = L.pp_bam_records(ctx._h, bp, n_bytes, op, n, mem, m.ctypes.data if m is not None else None, len(m) - 1 if m is not None else 0,
                              C.byref(self._p), C.byref(bad))
        if rc:
            _raise(rc, L.pp_last_error(ctx._h).decode(), bad_record=_index(bad))
        out = self._view = RawBatch()
        L.pp_bam_raw(self._p, C.byref(out))
        self.n_rec, self.seq_bytes, self.n_cig_total = int(out.n_rec), int(out.seq_bytes), int(out.n_cig_total)
        self._ptrs = _ptrs_of(out, RAW_FIELDS)
        self.read_id_ptr = L.pp_bam_read_id(self._p) or 0
        nb, nbytes, no, nl = C.c_void_p(), C.c_uint64(0), C.c_void_p(), C.c_void_p()
        L.pp_bam_names(self._p, C.byref(nb), C.byref(nbytes), C.byref(no), C.byref(nl))
        self._names = (nb.value or 0, no.value or 0, nl.value or 0)
        self.n_bytes = int(nbytes.value)
        zp, n_al = C.c_void_p(), C.c_uint64(0)
        L.pp_bam_pass(self._p, C.byref(zp), C.byref(n_al))
        self.zp = _host(zp.value, n_al.value, np.uint8)

    def raw(self):
        return dict(self._ptrs, n_rec=self.n_rec, seq_bytes=self.seq_bytes, n_cig_total=self.n_cig_total)

    def names(self):
        return {"names": self._names, "n": self.n_rec, "n_bytes": self.n_bytes}

    def host(self):
        out = _read_batch(self._view, RAW_FIELDS, self._ctx)
        out["name_off"] = self._ctx.download(self._names[1], self.n_rec, np.uint64)
        out["name_len"] = self._ctx.download(self._names[2], self.n_rec, np.uint32)
        return out


class SamRecords(_Owned):
    """pp_sam_records: the lines of SAM text as a raw batch in DEVICE memory, owned by this object -- the text twin of BamRecords.  The
    object keeps its own device copy of the text: raw()["seq"] IS that copy (seq_off = the offset of a record's SEQ column in it, any
    case, no rooms), and the name ranges point into it.
      data           mem = MEM_HOST: bytes / a uint8 array; MEM_DEVICE: (device address, n_bytes), free again when the call returns
      n_lines        None, or pp_sam_records_lines: the first n_lines lines only; nothing from line n_lines on is looked at, and the
                     object is that of the prefix (.n_bytes = the prefix's length)
      .n_rec, .seq_bytes (= .n_bytes, the text's), .n_cig_total
      .raw()         the device-address dict gate_records / regroup_records / filter_records(..., mem=MEM_DEVICE) take
      .names()       keyword arguments for Names.ids(mem=MEM_DEVICE, out=.read_id_ptr): the QNAMEs' ranges in the device copy
      .rnames()      ... for Names.ids(mem=MEM_DEVICE, out32=.contig_ptr) on a table seeded with the FASTA names: the RNAMEs' ranges
      .read_id_ptr, .contig_ptr   device addresses of raw()["read_id"] (n_rec uint64) and raw()["contig"] (n_rec uint32): zero until filled
      .zp            np.uint8, one per ALIGNED record, 0 = the line carries ZP:Z:fail: gate_records' `passed` (AND the filter's)
      .lines()       np.uint32: the 0-based line of every record (a later link's bad_record -> the file's own line)
      .first_empty_line()   pp_sam_first_empty_line: the 0-based line of the first empty (or "\r"-only) line, None without one
      .host()        numpy copies of the arrays, and "name_off" / "name_len" / "rname_off" / "rname_len" / "line"
      .kernel_ms()   HIP-event time of the decode's kernels (the context had set_profiling on); .stage_ms(): copy | newline_index |
                     scan | place | cigar
      .tagged(pass_) pp_sam_tagged_records: the text with the filter's verdicts written back -> SamOut (no second upload)
      .bam()         pp_sam_bam_records: the text encoded as uncompressed BAM -> BamEncoded (no second upload)
    A refused text raises PolypolishError with .bad_record = the 0-based line (None where the refusal names none)."""
    _free, _kernel_ms = "pp_sam_free", "pp_sam_kernel_ms"

    def __init__(self, ctx, data, mem=MEM_HOST, n_lines=None):
        L = lib()
        bp, n_bytes, _, _, _keep = _bytes_and_offsets(data, None, mem)
        super().__init__(ctx)
        bad = _no_index()
        if n_lines is None:
            rc = L.pp_sam_records(ctx._h, bp, n_bytes, mem, C.byref(self._p), C.byref(bad))
        else:
            rc = L.pp_sam_records_lines(ctx._h, bp, n_bytes, mem, int(n_lines), C.byref(self._p), C.byref(bad))
        if rc:
            _raise(rc, L.pp_last_error(ctx._h).decode(), bad_record=_index(bad))
        out = self._view = RawBatch()
        L.pp_sam_raw(self._p, C.byref(out))
        self.n_rec, self.seq_bytes, self.n_cig_total = int(out.n_rec), int(out.seq_bytes), int(out.n_cig_total)
        self._ptrs = _ptrs_of(out, RAW_FIELDS)
        self.read_id_ptr, self.contig_ptr = L.pp_sam_read_id(self._p) or 0, L.pp_sam_contig(self._p) or 0
        self._ranges = []
        for fn in (L.pp_sam_names, L.pp_sam_rnames):
            nb, nbytes, no, nl = C.c_void_p(), C.c_uint64(0), C.c_void_p(), C.c_void_p()
            fn(self._p, C.byref(nb), C.byref(nbytes), C.byref(no), C.byref(nl))
            self._ranges.append((nb.value or 0, no.value or 0, nl.value or 0))
            self.n_bytes = int(nbytes.value)
        self._lines = L.pp_sam_lines(self._p) or 0
        zp, n_al = C.c_void_p(), C.c_uint64(0)
        L.pp_sam_pass(self._p, C.byref(zp), C.byref(n_al))
        self.zp = _host(zp.value, n_al.value, np.uint8)

    def raw(self):
        return dict(self._ptrs, n_rec=self.n_rec, seq_bytes=self.seq_bytes, n_cig_total=self.n_cig_total)

    def names(self):
        return {"names": self._ranges[0], "n": self.n_rec, "n_bytes": self.n_bytes}

    def rnames(self):
        return {"names": self._ranges[1], "n": self.n_rec, "n_bytes": self.n_bytes}

    def lines(self):
        return self._ctx.download(self._lines, self.n_rec, np.uint32)

    def first_empty_line(self):
        line = C.c_uint64(0)
        return int(line.value) if lib().pp_sam_first_empty_line(self._p, C.byref(line)) else None

    def host(self):
        out = _read_batch(self._view, RAW_FIELDS, self._ctx)
        for k, (_, off, ln) in zip(("name", "rname"), self._ranges):
            out[k + "_off"] = self._ctx.download(off, self.n_rec, np.uint64)
            out[k + "_len"] = self._ctx.download(ln, self.n_rec, np.uint32)
        out["line"] = self.lines()
        return out

    def stage_ms(self):
        return self._stage_ms("pp_sam_stage_ms_", ("copy", "newline_index", "scan", "place", "cigar"), " when the text was decoded")

    def tagged(self, pass_):
        """pp_sam_tagged_records: the object's own device copy of the text with the verdicts written back -> SamOut"""
        return SamOut(self._ctx, pass_=pass_, records=self)

    def bam(self):
        """pp_sam_bam_records: the object's own device copy of the text encoded as uncompressed BAM -> BamEncoded"""
        return BamEncoded(self._ctx, records=self)


class FastaRecords(_Owned):
    """pp_fasta_records: FASTA text as contig bases in DEVICE memory, owned by this object -- the device twin of pp_assembly_load, next
    to SamRecords.  The text is read once; the object owns its output only.
      data           mem = MEM_HOST: bytes / a uint8 array; MEM_DEVICE: (device address, n_bytes), free again when the call returns
      .bases         (device address, n_bases): the bases of all contigs one behind the other, upper-cased: what a polish job takes
      .n_bases, .n_contigs
      .offsets       np.uint64, n_contigs + 1: contig i is bases[offsets[i] : offsets[i + 1]]
      .names, .descriptions   lists of bytes
      .host()        {"bases": the bases as bytes (one download), "offsets", "names", "descriptions"}
      .kernel_ms()   HIP-event time of the kernels (the context had set_profiling on); .stage_ms(): copy | sums | place | headers
    A refused text raises PolypolishError with .bad_record = the 0-based line (None where the refusal names none)."""
    _free, _kernel_ms = "pp_fasta_free", "pp_fasta_kernel_ms"

    def __init__(self, ctx, data, mem=MEM_HOST):
        L = lib()
        bp, n_bytes, _, _, _keep = _bytes_and_offsets(data, None, mem)
        super().__init__(ctx)
        bad = _no_index()
        rc = L.pp_fasta_records(ctx._h, bp, n_bytes, mem, C.byref(self._p), C.byref(bad))
        if rc:
            _raise(rc, L.pp_last_error(ctx._h).decode(), bad_record=_index(bad))
        dev, nb = C.c_void_p(), C.c_uint64(0)
        L.pp_fasta_bases(self._p, C.byref(dev), C.byref(nb))
        self.n_bases, self.n_contigs = int(nb.value), int(L.pp_fasta_n_contigs(self._p))
        self.bases = (dev.value or 0, self.n_bases)
        self.offsets = _host(L.pp_fasta_offsets(self._p), self.n_contigs + 1, np.uint64)
        self.names = [L.pp_fasta_name(self._p, i) for i in range(self.n_contigs)]
        self.descriptions = [L.pp_fasta_description(self._p, i) for i in range(self.n_contigs)]

    def host(self):
        b = self._ctx.download(self.bases[0], self.n_bases, np.uint8).tobytes() if self.n_bases else b""
        return {"bases": b, "offsets": self.offsets, "names": self.names, "descriptions": self.descriptions}

    def stage_ms(self):
        return self._stage_ms("pp_fasta_stage_ms_", ("copy", "sums", "place", "headers"), " when the text was parsed")


def fasta_geometry():
    """(bytes per lane, bytes per tile T, bytes per workgroup W) of pp_fasta_records: the seams its tests aim at.  Tiles are cut at
    multiples of the lane's bytes of ADDRESS: a device text whose first byte lies s bytes behind such a multiple has its seams at
    the text offsets k * T - s."""
    a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
    lib().pp_fasta_geometry_(C.byref(a), C.byref(b), C.byref(c))
    return int(a.value), int(b.value), int(c.value)


def _take_bytes(b):
    """the bytes of a pp_bytes the library allocated, which is released"""
    data = C.string_at(b.data, b.len) if b.len else b""
    lib().pp_bytes_free(C.byref(b))
    return data


class FastaText(_Owned):
    """pp_fasta_text: contig bases as FASTA text at a chosen line width in DEVICE memory, owned by this object -- the mirror of
    FastaRecords and the link in front of BgzfDeflated (tests/fasta_text_model.py defines the bytes).
      bases          mem = MEM_HOST: bytes / a uint8 array; MEM_DEVICE: (device address, n_bytes), borrowed for the call (what a
                     polish job leaves behind); the contigs one behind the other
      contig_off     n + 1 offsets into bases (host)
      headers        n header lines (bytes) without their '>' and their newline
      width          0: one line per contig, else the line width
      .dev()         (device address, n_bytes) of the text: what BgzfDeflated / FastaRecords take with mem=MEM_DEVICE
      .bytes()       the text as bytes (a download)
      .fai()         its .fai index as bytes
      .deflate()     pp_bgzf_deflate on the device bytes -> BgzfDeflated (.gzi(): its .gzi index)
      .write(path)   pp_fasta_out_write: the text on disk
      .kernel_ms()   HIP-event time of the kernel (the context had set_profiling on); .stage_ms(): copy | text"""
    _free, _kernel_ms = "pp_fasta_out_free", "pp_fasta_out_kernel_ms"

    def __init__(self, ctx, bases, contig_off, headers, width=0, mem=MEM_HOST):
        L = lib()
        bp, _, _, _, _keep = _bytes_and_offsets(bases, None, mem)
        off = np.ascontiguousarray(contig_off, dtype=np.uint64)
        n = len(off) - 1
        hb = np.frombuffer(b"".join(headers) + b"\0", dtype=np.uint8)
        ho = np.zeros(n + 1, dtype=np.uint64)
        ho[1:] = np.cumsum([len(h) for h in headers], dtype=np.uint64)
        super().__init__(ctx)
        ctx._chk(L.pp_fasta_text(ctx._h, bp, mem, n, off.ctypes.data, hb.ctypes.data, ho.ctypes.data, int(width), C.byref(self._p)))
        dev, nb = C.c_void_p(), C.c_uint64(0)
        L.pp_fasta_out_bytes(self._p, C.byref(dev), C.byref(nb))
        self.bytes_ptr, self.n_bytes = dev.value or 0, int(nb.value)

    def dev(self):
        return self.bytes_ptr, self.n_bytes

    def bytes(self):
        return self._ctx.download(self.bytes_ptr, self.n_bytes, np.uint8).tobytes() if self.n_bytes else b""

    def fai(self):
        b = Bytes()
        self._ctx._chk(lib().pp_fasta_out_fai(self._p, C.byref(b)))
        return _take_bytes(b)

    def deflate(self):
        return BgzfDeflated(self._ctx, self.dev(), mem=MEM_DEVICE)

    def write(self, path):
        self._ctx._chk(lib().pp_fasta_out_write(self._p, os.fsencode(path)))

    def stage_ms(self):
        return self._stage_ms("pp_fasta_out_stage_ms_", ("copy", "text"), " when the text was made")


class Vcf(_Owned):
    """pp_polish_vcf: the edits of the context's finished polish job as VCF 4.2 text in DEVICE memory, owned by this object
    (tests/vcf_model.py defines the bytes).  Valid after polish_finish and until the next polish_begin, with or without debug records.
      names          one contig name (bytes / str) per contig of the job
      .n_records     the records (runs of edited positions)
      .dev()         (device address, n_bytes) of the text: what BgzfDeflated takes with mem=MEM_DEVICE
      .bytes()       the text as bytes (a download)
      .deflate()     pp_bgzf_deflate on the device bytes -> BgzfDeflated
      .write(path)   pp_vcf_out_write: the text on disk
      .kernel_ms()   HIP-event time of the kernels (the context had set_profiling on); .stage_ms(): mark | runs | records | text"""
    _free, _kernel_ms = "pp_vcf_out_free", "pp_vcf_out_kernel_ms"

    def __init__(self, ctx, names):
        L = lib()
        enc = [n.encode() if isinstance(n, str) else bytes(n) for n in names]
        arr = (C.c_char_p * max(len(enc), 1))(*enc)
        super().__init__(ctx)
        ctx._chk(L.pp_polish_vcf(ctx._h, arr, C.byref(self._p)))
        dev, nb, nr = C.c_void_p(), C.c_uint64(0), C.c_uint64(0)
        L.pp_vcf_out_bytes(self._p, C.byref(dev), C.byref(nb), C.byref(nr))
        self.bytes_ptr, self.n_bytes, self.n_records = dev.value or 0, int(nb.value), int(nr.value)

    def dev(self):
        return self.bytes_ptr, self.n_bytes

    def bytes(self):
        return self._ctx.download(self.bytes_ptr, self.n_bytes, np.uint8).tobytes() if self.n_bytes else b""

    def deflate(self):
        return BgzfDeflated(self._ctx, self.dev(), mem=MEM_DEVICE)

    def write(self, path):
        self._ctx._chk(lib().pp_vcf_out_write(self._p, os.fsencode(path)))

    def stage_ms(self):
        return self._stage_ms("pp_vcf_out_stage_ms_", ("mark", "runs", "records", "text"), " when the text was made")


def vcf_geometry():
    """(positions per thread, positions per workgroup, text bytes per store, text bytes per workgroup) of pp_polish_vcf: the position
    passes cut the assembly, the text pass cuts the text -- the seams its tests aim at."""
    v = [C.c_uint32() for _ in range(4)]
    lib().pp_vcf_geometry_(*[C.byref(x) for x in v])
    return tuple(int(x.value) for x in v)


STATUS_WORDS = ("kept", "changed", "low_depth", "none", "multiple", "too_close")  # PP_ST_* in order: the reference's own words
BED_UNDECIDED = (1 << 2) | (1 << 3) | (1 << 4) | (1 << 5)  # PP_BED_UNDECIDED: low_depth, none, multiple, too_close


def bed_status_mask(bed_status):
    """the status mask of a bed_status= argument: None (the four undecided ones), an int mask, a comma-separated list of the six
    words (the commands' --bed_status) or a sequence of them"""
    if bed_status is None:
        return BED_UNDECIDED
    if isinstance(bed_status, (int, np.integer)):
        return int(bed_status)
    words = (bed_status.split(",") if bed_status else []) if isinstance(bed_status, str) else list(bed_status)
    if not words:
        raise PolypolishError(ERR_QUIT, "bed_status: an empty status list")
    mask = 0
    for w in words:
        if w not in STATUS_WORDS:
            raise PolypolishError(ERR_QUIT, f"bed_status: '{w}' is not one of {', '.join(STATUS_WORDS)}")
        mask |= 1 << STATUS_WORDS.index(w)
    return mask


class StatusBed(_Owned):
    """pp_polish_bed / pp_status_bed: the runs of equal per-position status as BED text in DEVICE memory, owned by this object
    (tests/bed_model.py defines the bytes).
      StatusBed(ctx, names, mask)                      of the context's finished job (it ran with debug records: polish_records(debug=True))
      StatusBed(ctx, names, mask, status, contig_off)  of a caller's status bytes: a numpy uint8 array (mem=MEM_HOST) or a device
                                                       address (mem=MEM_DEVICE); .bad_pos holds the first bad position when refused
      names          one contig name (bytes / str) per contig;  mask: bits 1 << PP_ST_x (default: the four undecided ones)
      .n_records, .n_bytes, .counts (positions per status inside the records)
      .dev() / .bytes() / .deflate() / .write(path) / .kernel_ms() / .stage_ms() (runs | records | text): as Vcf"""
    _free, _kernel_ms = "pp_bed_out_free", "pp_bed_out_kernel_ms"

    def __init__(self, ctx, names, mask=BED_UNDECIDED, status=None, contig_off=None, mem=MEM_HOST):
        L = lib()
        enc = [n.encode() if isinstance(n, str) else bytes(n) for n in names]
        arr = (C.c_char_p * max(len(enc), 1))(*enc)
        super().__init__(ctx)
        self.bad_pos = None
        if status is None:
            ctx._chk(L.pp_polish_bed(ctx._h, C.cast(arr, C.c_void_p), int(mask), C.byref(self._p)))
        else:
            off = np.ascontiguousarray(contig_off, dtype=np.uint64)
            if mem == MEM_HOST:
                keep = np.ascontiguousarray(status, dtype=np.uint8)
                ptr = keep.ctypes.data if keep.size else C.addressof(C.c_uint8())  # (nobody reads it: any address but NULL)
            else:
                ptr = int(status)
            bad = C.c_uint64(0)
            rc = L.pp_status_bed(ctx._h, ptr, mem, len(off) - 1, off.ctypes.data, C.cast(arr, C.c_void_p), int(mask), C.byref(self._p), C.byref(bad))
            if rc:
                self.bad_pos = int(bad.value)
                e = PolypolishError(rc, L.pp_last_error(ctx._h).decode())
                e.bad_pos = self.bad_pos
                raise e
        dev, nb, nr = C.c_void_p(), C.c_uint64(0), C.c_uint64(0)
        L.pp_bed_out_bytes(self._p, C.byref(dev), C.byref(nb), C.byref(nr))
        self.bytes_ptr, self.n_bytes, self.n_records = dev.value or 0, int(nb.value), int(nr.value)
        cnt = (C.c_uint64 * 6)()
        L.pp_bed_out_counts(self._p, cnt)
        self.counts = tuple(int(x) for x in cnt)

    def dev(self):
        return self.bytes_ptr, self.n_bytes

    def bytes(self):
        return self._ctx.download(self.bytes_ptr, self.n_bytes, np.uint8).tobytes() if self.n_bytes else b""

    def deflate(self):
        return BgzfDeflated(self._ctx, self.dev(), mem=MEM_DEVICE)

    def write(self, path):
        self._ctx._chk(lib().pp_bed_out_write(self._p, os.fsencode(path)))

    def stage_ms(self):
        return self._stage_ms("pp_bed_out_stage_ms_", ("runs", "records", "text"), " when the text was made")


class Masked(_Owned):
    """pp_polish_masked: a copy of the finished job's polished bytes in DEVICE memory in which every byte emitted by a position whose
    status is selected by `mask` is in lower case (the job ran with debug records).  .dev(): (address, n_bytes); .bytes(): a download;
    .kernel_ms(): the copy and the mask pass (the context had set_profiling on).  The job's own bytes are untouched."""
    _free, _kernel_ms = "pp_masked_free", "pp_masked_kernel_ms"

    def __init__(self, ctx, mask=BED_UNDECIDED):
        L = lib()
        super().__init__(ctx)
        ctx._chk(L.pp_polish_masked(ctx._h, int(mask), C.byref(self._p)))
        dev, nb = C.c_void_p(), C.c_uint64(0)
        L.pp_masked_bytes(self._p, C.byref(dev), C.byref(nb))
        self.bytes_ptr, self.n_bytes = dev.value or 0, int(nb.value)

    def dev(self):
        return self.bytes_ptr, self.n_bytes

    def bytes(self):
        return self._ctx.download(self.bytes_ptr, self.n_bytes, np.uint8).tobytes() if self.n_bytes else b""


def bed_geometry():
    """(positions per thread P, positions per workgroup T, text bytes per store, text bytes per workgroup) of pp_status_bed: the position
    passes cut the status array, the text pass cuts the text -- the seams its tests aim at."""
    v = [C.c_uint32() for _ in range(4)]
    lib().pp_bed_geometry_(*[C.byref(x) for x in v])
    return tuple(int(x.value) for x in v)


class DepthTrack(_Owned):
    """pp_polish_depth / pp_depth_bedgraph: a per-position read depth as bedGraph text in DEVICE memory, owned by this object
    (tests/depth_model.py defines the bytes): the runs of equal printed depth (bin=0) or the mean printed depth of bins of `bin`
    positions.
      DepthTrack(ctx, names, bin)                     of the context's finished job (it ran with debug records: polish_records(debug=True))
      DepthTrack(ctx, names, bin, depth, contig_off)  of a caller's depths: a numpy float64 array (mem=MEM_HOST) or a device address
                                                      (mem=MEM_DEVICE); .bad_pos holds the first bad position when refused
      names          one contig name (bytes / str) per contig
      .n_records, .n_bytes
      .bytes()       the text as bytes (a download);  .dev(): (device address, n_bytes);  .deflate(): pp_bgzf_deflate on the device bytes
      .summary()     {"zero_positions", "max_tenths", "sum_tenths"}: positions that print 0.0, the largest and the summed tenths
      .write(path)   pp_depth_out_write: the text on disk
      .kernel_ms()   HIP-event time of the kernels (the context had set_profiling on); .stage_ms(): values | records | lengths | text
      .close()       frees the text"""
    _free, _kernel_ms = "pp_depth_out_free", "pp_depth_out_kernel_ms"

    def __init__(self, ctx, names, bin=0, depth=None, contig_off=None, mem=MEM_HOST):  # noqa: A002 (the C argument's name)
        L = lib()
        enc = [n.encode() if isinstance(n, str) else bytes(n) for n in names]
        arr = (C.c_char_p * max(len(enc), 1))(*enc)
        super().__init__(ctx)
        self.bad_pos = None
        if depth is None:
            ctx._chk(L.pp_polish_depth(ctx._h, C.cast(arr, C.c_void_p), int(bin), C.byref(self._p)))
        else:
            off = np.ascontiguousarray(contig_off, dtype=np.uint64)
            if mem == MEM_HOST:
                keep = np.ascontiguousarray(depth, dtype=np.float64)
                ptr = keep.ctypes.data if keep.size else C.addressof(C.c_double())  # (nobody reads it: any address but NULL)
            else:
                ptr = int(depth)
            bad = C.c_uint64(0)
            rc = L.pp_depth_bedgraph(ctx._h, ptr, mem, len(off) - 1, off.ctypes.data, C.cast(arr, C.c_void_p), int(bin), C.byref(self._p), C.byref(bad))
            if rc:
                self.bad_pos = int(bad.value)
                e = PolypolishError(rc, L.pp_last_error(ctx._h).decode())
                e.bad_pos = self.bad_pos
                raise e
        dev, nb, nr = C.c_void_p(), C.c_uint64(0), C.c_uint64(0)
        L.pp_depth_out_bytes(self._p, C.byref(dev), C.byref(nb), C.byref(nr))
        self.bytes_ptr, self.n_bytes, self.n_records = dev.value or 0, int(nb.value), int(nr.value)

    def dev(self):
        return self.bytes_ptr, self.n_bytes

    def bytes(self):
        return self._ctx.download(self.bytes_ptr, self.n_bytes, np.uint8).tobytes() if self.n_bytes else b""

    def summary(self):
        z, m, s = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        lib().pp_depth_out_summary(self._p, C.byref(z), C.byref(m), C.byref(s))
        return {"zero_positions": int(z.value), "max_tenths": int(m.value), "sum_tenths": int(s.value)}

    def deflate(self):
        return BgzfDeflated(self._ctx, self.dev(), mem=MEM_DEVICE)

    def write(self, path):
        self._ctx._chk(lib().pp_depth_out_write(self._p, os.fsencode(path)))

    def stage_ms(self):
        return self._stage_ms("pp_depth_out_stage_ms_", ("values", "records", "lengths", "text"), " when the text was made")


def depth_geometry():
    """(positions per thread P, positions per workgroup T, text bytes per store, text bytes per workgroup) of pp_depth_bedgraph: the
    position passes cut the depth array, the text pass cuts the text -- the seams its tests aim at."""
    v = [C.c_uint32() for _ in range(4)]
    lib().pp_depth_geometry_(*[C.byref(x) for x in v])
    return tuple(int(x.value) for x in v)


def fasta_out_geometry():
    """(bytes per store S, bytes per workgroup G) of pp_fasta_text: a lane writes S bytes of TEXT with one aligned store, a workgroup
    owns the text offsets [k * G, (k + 1) * G): the seams its tests aim at."""
    a, b = C.c_uint32(), C.c_uint32()
    lib().pp_fasta_out_geometry_(C.byref(a), C.byref(b))
    return int(a.value), int(b.value)


class BamTagged(_Owned):
    """pp_bam_tagged: the filter's verdicts written back as a BAM file (level-0 BGZF) in DEVICE memory, owned by this object.
      data, rec_off  mem = MEM_HOST: bytes / a uint8 array of uncompressed BAM, and the records' offsets; MEM_DEVICE: data = (device
                     address, n_bytes), rec_off = (device address of n uint64, n), both borrowed for the call
      records_at     where the header ends (bam_header(...)["records_at"])
      passed         None or one byte per ALIGNED record (host): the filter's own verdict, filter_records(...)["pass"][f] -- not ANDed
                     with BamRecords.zp
      head           None, or bytes (host): pp_bam_tagged_head -- the stream starts with them instead of data[0, records_at)
      .n_bytes, .bytes_ptr   the file: Bgzf(ctx, (t.bytes_ptr, t.n_bytes), (blk_off_ptr, n_blocks), mem=MEM_DEVICE) with blk_off[b] =
                     b * 65,311 reads it back
      .counts        (passed, failed, blocks without the EOF block)
      .host(lo, hi)  a numpy copy of the file's bytes [lo, hi) (a download)
      .write(path)   pp_bam_out_write: the file on disk
      .deflate()     pp_bam_out_deflate: the same file compressed -> BgzfDeflated
      .kernel_ms()   HIP-event time of the kernels (the context had set_profiling on); .stage_ms(): pass_a | scans | pass_b
    A failing call raises PolypolishError with .bad_record."""
    _free, _kernel_ms = "pp_bam_out_free", "pp_bam_out_kernel_ms"

    def __init__(self, ctx, data, records_at, rec_off, passed, mem=MEM_HOST, head=None):
        L = lib()
        bp, n_bytes, op, n, _keep = _bytes_and_offsets(data, rec_off, mem)
        v = None if passed is None else np.ascontiguousarray(passed, dtype=np.uint8)
        super().__init__(ctx)
        bad = _no_index()
        args = (ctx._h, bp, n_bytes, int(records_at), op, n, mem, v.ctypes.data if v is not None else None, len(v) if v is not None else 0)
        if head is None:
            rc = L.pp_bam_tagged(*args, C.byref(self._p), C.byref(bad))
        else:
            h = _bam_bytes(head)
            rc = L.pp_bam_tagged_head(*args, h.ctypes.data if len(h) else None, len(h), C.byref(self._p), C.byref(bad))
        if rc:
            _raise(rc, L.pp_last_error(ctx._h).decode(), bad_record=_index(bad))
        dev, nb = C.c_void_p(), C.c_uint64(0)
        L.pp_bam_out_bytes(self._p, C.byref(dev), C.byref(nb))
        self.bytes_ptr, self.n_bytes = dev.value or 0, int(nb.value)
        p, f, k = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        L.pp_bam_out_counts(self._p, C.byref(p), C.byref(f), C.byref(k))
        self.counts = (int(p.value), int(f.value), int(k.value))

    def host(self, lo=0, hi=None):
        hi = self.n_bytes if hi is None else min(int(hi), self.n_bytes)
        lo = min(int(lo), hi)
        return self._ctx.download(self.bytes_ptr + lo, hi - lo, np.uint8)

    def write(self, path):
        self._ctx._chk(lib().pp_bam_out_write(self._p, os.fsencode(path)))

    def stage_ms(self):
        return self._stage_ms("pp_bam_out_stage_ms_", ("pass_a", "scans", "pass_b"), " when the records were tagged")

    def deflate(self):
        return BgzfDeflated(self._ctx, tagged=self)


class BamSorted(_Owned):
    """pp_bam_sort: the coordinate order of BAM records -- reference id, position, reverse strand, input order -- in DEVICE memory,
    owned by this object.  data, records_at, rec_off and mem as BamTagged takes them.
      .n_rec
      .perm()              np.uint32: sorted record j is input record perm[j]; .perm_ptr its device address
      .rec_off()           np.uint64: rec_off[perm[j]]; .rec_off_ptr its device address -- (s.rec_off_ptr, s.n_rec) is the rec_off of
                           BamTagged(..., mem=MEM_DEVICE, head=s.head)
      .head                bytes: the header with its first text line made to say SO:coordinate
      .counts()            (records that changed place, records with ref_id == -1)
      .carry_pass(passed)  one byte per ALIGNED input record -> the same verdicts in the numbering of the sorted records
      .kernel_ms()         HIP-event time of the kernels (the context had set_profiling on); .stage_ms(): keys | sort | gather
    A failing call raises PolypolishError with .bad_record."""
    _free, _kernel_ms = "pp_bam_sorted_free", "pp_bam_sorted_kernel_ms"

    def __init__(self, ctx, data, records_at, rec_off, mem=MEM_HOST):
        L = lib()
        bp, n_bytes, op, n, _keep = _bytes_and_offsets(data, rec_off, mem)
        super().__init__(ctx)
        bad = _no_index()
        rc = L.pp_bam_sort(ctx._h, bp, n_bytes, int(records_at), op, n, mem, C.byref(self._p), C.byref(bad))
        if rc:
            _raise(rc, L.pp_last_error(ctx._h).decode(), bad_record=_index(bad))
        self.n_rec = n
        self.perm_ptr, self.rec_off_ptr = L.pp_bam_sorted_perm(self._p) or 0, L.pp_bam_sorted_rec_off(self._p) or 0
        hp, hn = C.c_void_p(), C.c_uint64(0)
        L.pp_bam_sorted_head(self._p, C.byref(hp), C.byref(hn))
        self.head = _host(hp.value, int(hn.value), np.uint8).tobytes()

    def perm(self):
        return self._ctx.download(self.perm_ptr, self.n_rec, np.uint32)

    def rec_off(self):
        return self._ctx.download(self.rec_off_ptr, self.n_rec, np.uint64)

    def counts(self):
        m, u = C.c_uint64(0), C.c_uint64(0)
        lib().pp_bam_sorted_counts(self._p, C.byref(m), C.byref(u))
        return int(m.value), int(u.value)

    def carry_pass(self, passed):
        v = np.ascontiguousarray(passed, dtype=np.uint8)
        out = np.zeros(max(len(v), 1), dtype=np.uint8)
        self._ctx._chk(lib().pp_bam_sorted_pass(self._p, v.ctypes.data if len(v) else None, len(v), out.ctypes.data))
        return out[:len(v)]

    def stage_ms(self):
        return self._stage_ms("pp_bam_sorted_stage_ms_", ("keys", "sort", "gather"), " when the records were sorted")


class BamIndex(_Owned):
    """pp_bam_index: the .bai of the file BamTagged(ctx, data, ..., rec_off, passed, mem, head=...) makes, made on the device.
      data, rec_off, passed, mem   as BamTagged takes them; the records in coordinate order (BamSorted.rec_off_ptr, .carry_pass)
      n_head         the header's length in the stream (len(head); records_at for a BamTagged without head)
      n_ref          the header's references
      blk_off        the file's n_blocks + 1 block offsets: a host array, or (device address, n_blocks) -- BgzfDeflated.blk_off_ptr
      .bytes         the index
    A failing call raises PolypolishError with .bad_record.  (The object owns nothing once it is made: close() does nothing.)"""

    def __init__(self, ctx, data, n_head, rec_off, passed, n_ref, blk_off, mem=MEM_HOST):
        L = lib()
        bp, n_bytes, op, n, _keep = _bytes_and_offsets(data, rec_off, mem)
        v = None if passed is None else np.ascontiguousarray(passed, dtype=np.uint8)
        if isinstance(blk_off, tuple):
            kp, n_blk, blk_mem, _kb = int(blk_off[0]), int(blk_off[1]), MEM_DEVICE, None
        else:
            _kb = np.ascontiguousarray(blk_off, dtype=np.uint64)
            kp, n_blk, blk_mem = _kb.ctypes.data, len(_kb) - 1, MEM_HOST
        super().__init__(ctx)
        out, bad = Bytes(), _no_index()
        rc = L.pp_bam_index(ctx._h, bp, n_bytes, int(n_head), op, n, mem, v.ctypes.data if v is not None else None, len(v) if v is not None else 0,
                            int(n_ref), kp, n_blk, blk_mem, C.byref(out), C.byref(bad))
        if rc:
            _raise(rc, L.pp_last_error(ctx._h).decode(), bad_record=_index(bad))
        self.bytes = _take_bytes(out)

    def close(self):
        pass

    def stage_ms(self):
        """scans | records | chunks | linear of the context's LAST pp_bam_index (the context had set_profiling on)"""
        ms = (C.c_float * 4)()
        if lib().pp_bam_index_stage_ms_(self._ctx._h, ms):
            raise PolypolishError(ERR_ARG, "the context had no profiling on when the records were indexed")
        return {k: float(v) for k, v in zip(("scans", "records", "chunks", "linear"), ms)}


TBX_VCF, TBX_BED = 0, 1
TBI_TRACKS = ("vcf", "bed", "depth")  # PP_TBI_VCF, PP_TBI_BED, PP_TBI_DEPTH
TBX_LANE_BYTES = 64  # PP_TBX_LANE_BYTES


def tabix_index(ctx, text, preset, blk_off, mem=MEM_HOST, raw=True):
    """pp_tabix_index: the .tbi of the file BgzfDeflated(ctx, text, mem) makes of a position-sorted, tab-separated text, made on the
    device (tests/tabix_model.py defines the bytes).
      text           the UNCOMPRESSED text.  mem = MEM_HOST: bytes / a uint8 array; MEM_DEVICE: (device address, n_bytes), borrowed
      preset         TBX_VCF or TBX_BED (bedGraph too)
      blk_off        the file's n_blocks + 1 block offsets: a host array, or (device address, n_blocks) -- BgzfDeflated.blk_off_ptr
    -> (tbi, raw): the bytes of "<file>.tbi" and the index uncompressed (None with raw=False).  A failing call raises
    PolypolishError with .bad_line."""
    L = lib()
    bp, n_bytes, _, _, _keep = _bytes_and_offsets(text, None, mem)
    if isinstance(blk_off, tuple):
        kp, n_blk, blk_mem, _kb = int(blk_off[0]), int(blk_off[1]), MEM_DEVICE, None
    else:
        _kb = np.ascontiguousarray(blk_off, dtype=np.uint64)
        kp, n_blk, blk_mem = _kb.ctypes.data, len(_kb) - 1, MEM_HOST
    tbi, rw, bad = Bytes(), Bytes(), _no_index()
    rc = L.pp_tabix_index(ctx._h, bp, n_bytes, mem, int(preset), kp, n_blk, blk_mem, C.byref(tbi), C.byref(rw) if raw else None, C.byref(bad))
    if rc:
        _raise(rc, L.pp_last_error(ctx._h).decode(), bad_line=_index(bad))
    return _take_bytes(tbi), (_take_bytes(rw) if raw else None)


def tabix_stage_ms(ctx):
    """newline index | rows | names | chunks | linear of the context's LAST pp_tabix_index (the context had set_profiling on)"""
    ms = (C.c_float * 5)()
    if lib().pp_tabix_stage_ms_(ctx._h, ms):
        raise PolypolishError(ERR_ARG, "the context had no profiling on when the text was indexed")
    return {k: float(v) for k, v in zip(("newlines", "rows", "names", "chunks", "linear"), ms)}


class BgzfDeflated(_Owned):
    """pp_bgzf_deflate / pp_bam_out_deflate: bytes compressed into a BGZF file in DEVICE memory, owned by this object.  The bytes are
    cut every 65,280; each piece is one BGZF block around one DEFLATE block, the EOF block is the last (tests/bgzf_deflate_model.py
    defines the bytes).
      data           mem = MEM_HOST: bytes / a uint8 array; MEM_DEVICE: (device address, n_bytes), borrowed for the call; or
                     tagged = a BamTagged (BamTagged.deflate()): the uncompressed stream of its level-0 file
      .n_bytes, .bytes_ptr        the file
      .n_blocks, .blk_off_ptr     the blocks without the EOF block, and the device address of n_blocks + 1 uint64 offsets (the EOF
                     block's last): Bgzf(ctx, (z.bytes_ptr, z.n_bytes), (z.blk_off_ptr, z.n_blocks), mem=MEM_DEVICE) reads it back
      .counts        blocks by form: (stored, fixed, dynamic)
      .host(lo, hi)  a numpy copy of the file's bytes [lo, hi) (a download); .blk_off(): of the n_blocks + 1 offsets
      .write(path)   pp_bgzf_out_write: the file on disk
      .gzi()         pp_bgzf_out_gzi: the file's .gzi index as bytes
      .kernel_ms()   HIP-event time of the kernels (the context had set_profiling on); .stage_ms(): pieces | scan | place"""
    _free, _kernel_ms = "pp_bgzf_out_free", "pp_bgzf_out_kernel_ms"

    def __init__(self, ctx, data=None, mem=MEM_HOST, tagged=None):
        L = lib()
        super().__init__(ctx)
        if tagged is not None:
            rc = L.pp_bam_out_deflate(ctx._h, tagged._p, C.byref(self._p))
        else:
            bp, n_bytes, _, _, _keep = _bytes_and_offsets(data, None, mem)
            rc = L.pp_bgzf_deflate(ctx._h, bp, n_bytes, mem, C.byref(self._p))
        ctx._chk(rc)
        dev, nb, k = C.c_void_p(), C.c_uint64(0), C.c_uint64(0)
        L.pp_bgzf_out_bytes(self._p, C.byref(dev), C.byref(nb))
        self.bytes_ptr, self.n_bytes = dev.value or 0, int(nb.value)
        self.blk_off_ptr = L.pp_bgzf_out_blk_off(self._p, C.byref(k)) or 0
        self.n_blocks = int(k.value)
        s, f, d = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        L.pp_bgzf_out_counts(self._p, C.byref(s), C.byref(f), C.byref(d))
        self.counts = (int(s.value), int(f.value), int(d.value))

    def host(self, lo=0, hi=None):
        hi = self.n_bytes if hi is None else min(int(hi), self.n_bytes)
        lo = min(int(lo), hi)
        return self._ctx.download(self.bytes_ptr + lo, hi - lo, np.uint8)

    def blk_off(self):
        return self._ctx.download(self.blk_off_ptr, self.n_blocks + 1, np.uint64)

    def write(self, path):
        self._ctx._chk(lib().pp_bgzf_out_write(self._p, os.fsencode(path)))

    def gzi(self):
        """pp_bgzf_out_gzi: the file's .gzi index as bytes (per block except the first: its offset, the uncompressed bytes in front)"""
        b = Bytes()
        self._ctx._chk(lib().pp_bgzf_out_gzi(self._p, C.byref(b)))
        return _take_bytes(b)

    def stage_ms(self):
        return self._stage_ms("pp_bgzf_out_stage_ms_", ("pieces", "scan", "place"), " when the bytes were compressed")


class SamOut(_Owned):
    """pp_sam_tagged / pp_sam_tagged_records: the filter's verdicts written back as SAM text in DEVICE memory, owned by this object --
    byte for byte what pp_filter_write_text writes; the text twin of BamTagged.  Made by SamOut.tagged(ctx, text, pass_, mem=...) or
    SamRecords.tagged(pass_).  pp_bam_sam / pp_bam_sam_encoded make the same object from uncompressed BAM
    (tests/bam_sam_model.py defines the bytes): SamOut.from_bam(ctx, data, records_at, rec_off, pass_=None, mem=...) or
    BamEncoded.sam(pass_); there pass_=None appends no tag at all, and a refused record raises PolypolishError with .bad_record.
      text           mem = MEM_HOST: bytes / a uint8 array; MEM_DEVICE: (device address, n_bytes), borrowed for the call
      pass_          None or one byte per ALIGNED line (host): the filter's own verdict, filter_records(...)["pass"][f]
      .dev()         (device address, n_bytes) of the text: what Bgzf / BgzfDeflated / SamRecords take with mem=MEM_DEVICE
      .bytes()       the text as bytes (a download)
      .counts()      (passed, failed, lines)
      .write(path)   pp_sam_out_write: the file on disk
      .deflate()     pp_bgzf_deflate on the device bytes -> BgzfDeflated: the bgzipped file
      .kernel_ms()   HIP-event time of the kernels (the context had set_profiling on); .stage_ms(): newline_index | pass_a | scans |
                     pass_b"""
    _free, _kernel_ms = "pp_sam_out_free", "pp_sam_out_kernel_ms"

    def __init__(self, ctx, text=None, pass_=None, mem=MEM_HOST, records=None, bam=None, encoded=None):
        L = lib()
        v = None if pass_ is None else np.ascontiguousarray(pass_, dtype=np.uint8)
        vp, vn = (v.ctypes.data if v is not None and len(v) else None), (len(v) if v is not None else 0)
        super().__init__(ctx)
        if bam is not None or encoded is not None:
            if v is not None and not len(v):
                v = np.zeros(1, np.uint8)    # (no verdicts is None; an empty array still is an array of verdicts)
                vp = v.ctypes.data
            bad = _no_index()
            if encoded is not None:
                rc = L.pp_bam_sam_encoded(ctx._h, encoded._p, vp, vn, C.byref(self._p), C.byref(bad))
            else:
                data, records_at, rec_off = bam
                bp, n_bytes, op, n, _keep = _bytes_and_offsets(data, rec_off, mem)
                rc = L.pp_bam_sam(ctx._h, bp, n_bytes, int(records_at), op, n, mem, vp, vn, C.byref(self._p), C.byref(bad))
            if rc:
                _raise(rc, L.pp_last_error(ctx._h).decode(), bad_record=_index(bad))
        elif records is not None:
            rc = L.pp_sam_tagged_records(ctx._h, records._p, vp, vn, C.byref(self._p))
        else:
            bp, n_bytes, _, _, _keep = _bytes_and_offsets(text, None, mem)
            rc = L.pp_sam_tagged(ctx._h, bp, n_bytes, mem, vp, vn, C.byref(self._p))
        ctx._chk(rc)
        dev, nb = C.c_void_p(), C.c_uint64(0)
        L.pp_sam_out_bytes(self._p, C.byref(dev), C.byref(nb))
        self.bytes_ptr, self.n_bytes = dev.value or 0, int(nb.value)
        p, f, k = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        L.pp_sam_out_counts(self._p, C.byref(p), C.byref(f), C.byref(k))
        self._counts = (int(p.value), int(f.value), int(k.value))

    @classmethod
    def tagged(cls, ctx, text, pass_, mem=MEM_HOST):
        return cls(ctx, text, pass_, mem)

    @classmethod
    def from_bam(cls, ctx, data, records_at, rec_off, pass_=None, mem=MEM_HOST):
        """pp_bam_sam: data / rec_off as BamTagged takes them (MEM_DEVICE: (address, n_bytes) and (address of n uint64, n))"""
        return cls(ctx, pass_=pass_, mem=mem, bam=(data, records_at, rec_off))

    def dev(self):
        return self.bytes_ptr, self.n_bytes

    def bytes(self):
        return self._ctx.download(self.bytes_ptr, self.n_bytes, np.uint8).tobytes()

    def counts(self):
        return self._counts

    def write(self, path):
        self._ctx._chk(lib().pp_sam_out_write(self._p, os.fsencode(path)))

    def stage_ms(self):
        return self._stage_ms("pp_sam_out_stage_ms_", ("newline_index", "pass_a", "scans", "pass_b"), " when the text was tagged")

    def deflate(self):
        return BgzfDeflated(self._ctx, self.dev(), mem=MEM_DEVICE)


def sam_header(text):
    """pp_sam_header (no device needed): {"names": [bytes], "name_off", "name_len", "ref_len": numpy arrays, "header_end": int} of SAM
    text; a refused @SQ line raises PolypolishError(ERR_QUIT) with the 1-based line in its message."""
    L = lib()
    b = _bam_bytes(text)
    bp = b.ctypes.data if len(b) else None
    n_ref, end = C.c_uint32(0), C.c_uint64(0)
    rc = L.pp_sam_header(bp, len(b), 0, C.byref(n_ref), None, None, None, C.byref(end))
    n = int(n_ref.value)
    off, ln, rl = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    if n and rc == ERR_ARG:
        rc = L.pp_sam_header(bp, len(b), n, C.byref(n_ref), off.ctypes.data, ln.ctypes.data, rl.ctypes.data, C.byref(end))
    if rc:
        raise PolypolishError(rc, L.pp_bam_last_error().decode())
    return {"names": [b[int(o):int(o) + int(k)].tobytes() for o, k in zip(off, ln)], "name_off": off, "name_len": ln, "ref_len": rl,
            "header_end": int(end.value)}


class BamEncoded(_Owned):
    """pp_sam_bam / pp_sam_bam_records: SAM text encoded as uncompressed BAM in DEVICE memory, owned by this object
    (tests/sam_bam_model.py defines the bytes).  Made by BamEncoded(ctx, text, mem=...) or SamRecords.bam().
      text           mem = MEM_HOST: bytes / a uint8 array; MEM_DEVICE: (device address, n_bytes), borrowed for the call
      .dev()         (device address, n_bytes) of the BAM bytes: what BamRecords / BamTagged / bam_walk_device take with MEM_DEVICE
      .bytes()       the BAM bytes (a download)
      .records_at    where the header ends
      .n_rec, .rec_off_ptr   the records, and the device address of their n_rec uint64 offsets; .rec_off(): a numpy copy
      .tagged(pass_) pp_bam_tagged on the device bytes -> BamTagged (then .deflate().write(path): the compressed file)
      .records(ref_map)      pp_bam_records on the device bytes -> BamRecords
      .sam(pass_)    pp_bam_sam_encoded: the bytes decoded back to SAM text -> SamOut
      .kernel_ms()   HIP-event time of the kernels (the context had set_profiling on); .stage_ms(): newline_index | pass_a | names |
                     scans | pass_b
    A refused text raises PolypolishError with .bad_record = the 0-based line (None where the refusal names none)."""
    _free, _kernel_ms = "pp_bam_enc_free", "pp_bam_enc_kernel_ms"

    def __init__(self, ctx, text=None, mem=MEM_HOST, records=None):
        L = lib()
        super().__init__(ctx)
        bad = _no_index()
        if records is not None:
            rc = L.pp_sam_bam_records(ctx._h, records._p, C.byref(self._p), C.byref(bad))
        else:
            bp, n_bytes, _, _, _keep = _bytes_and_offsets(text, None, mem)
            rc = L.pp_sam_bam(ctx._h, bp, n_bytes, mem, C.byref(self._p), C.byref(bad))
        if rc:
            _raise(rc, L.pp_last_error(ctx._h).decode(), bad_record=_index(bad))
        dev, nb, at, k = C.c_void_p(), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        L.pp_bam_enc_bytes(self._p, C.byref(dev), C.byref(nb), C.byref(at))
        self.bytes_ptr, self.n_bytes, self.records_at = dev.value or 0, int(nb.value), int(at.value)
        self.rec_off_ptr = L.pp_bam_enc_rec_off(self._p, C.byref(k)) or 0
        self.n_rec = int(k.value)

    def dev(self):
        return self.bytes_ptr, self.n_bytes

    def bytes(self):
        return self._ctx.download(self.bytes_ptr, self.n_bytes, np.uint8).tobytes()

    def rec_off(self):
        return self._ctx.download(self.rec_off_ptr, self.n_rec, np.uint64)

    def tagged(self, pass_):
        return BamTagged(self._ctx, self.dev(), self.records_at, (self.rec_off_ptr, self.n_rec), pass_, mem=MEM_DEVICE)

    def records(self, ref_map=None):
        return BamRecords(self._ctx, self.dev(), (self.rec_off_ptr, self.n_rec), ref_map, mem=MEM_DEVICE)

    def sam(self, pass_=None):
        """pp_bam_sam_encoded: the bytes decoded back to SAM text -> SamOut"""
        return SamOut(self._ctx, pass_=pass_, encoded=self)

    def stage_ms(self):
        return self._stage_ms("pp_bam_enc_stage_ms_", ("newline_index", "pass_a", "names", "scans", "pass_b"), " when the text was encoded")


def sam_bam_geometry():
    """(lines per workgroup of the placing kernel, output bytes per workgroup of pass B, bytes per store) of pp_sam_bam: the seams
    its tests are built on"""
    a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
    lib().pp_sam_bam_geometry_(C.byref(a), C.byref(b), C.byref(c))
    return int(a.value), int(b.value), int(c.value)


def bam_sam_geometry():
    """(records per workgroup of pass A, output bytes per workgroup of pass B, bytes per store, output bytes per lane and step of the
    wide parts, lanes per record's group there) of pp_bam_sam: the seams its tests are built on"""
    v = [C.c_uint32() for _ in range(5)]
    lib().pp_bam_sam_geometry_(*[C.byref(x) for x in v])
    return tuple(int(x.value) for x in v)


def sam_out_geometry():
    """(lines per workgroup of pass A, output bytes per workgroup of pass B, bytes per store) of pp_sam_tagged: the seams its tests
    are built on"""
    a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
    lib().pp_sam_out_geometry_(C.byref(a), C.byref(b), C.byref(c))
    return int(a.value), int(b.value), int(c.value)


def _report_dict(rep):
    return {"before": int(rep.before_count), "after": int(rep.after_count), "low": int(rep.low_threshold), "high": int(rep.high_threshold),
            "orientation": ("fr", "rf", "ff", "rr")[rep.orientation] if 0 <= rep.orientation < 4 else None,
            "counts": [int(c) for c in rep.orientation_counts]}


# the arrays of pp_raw_batch the filter reads (nm and seq* are not looked at and may be missing)
FILTER_RAW_FIELDS = tuple((k, dt) for k, dt in RAW_FIELDS if k in ("flag", "read_id", "contig", "ref_start", "cig_off", "n_cig", "cigar"))


def filter_records(ctx, raw1, raw2, orientation="auto", low=0.1, high=99.9, mem=MEM_HOST):
    """pp_filter_records: the whole filter over the raw records of the two SAM files -- the dicts gate_records takes next
    (MEM_HOST: numpy arrays by the field names of pp_raw_batch; MEM_DEVICE: their device addresses plus "n_rec", "seq_bytes",
    "n_cig_total").  contig is the RNAME as an id, compared for equality only: names that are not in the assembly need distinct
    ids.  Returns {"pass": (p1, p2), "counts": [(alignments, reads)] * 2, "report": dict}; p1 / p2 (uint8, one per aligned
    record) are gate_records' `passed`."""
    pairs = [_raw_batch(raw, mem != MEM_DEVICE, FILTER_RAW_FIELDS) for raw in (raw1, raw2)]  # (the arrays stay alive in here)
    batches = (RawBatch * 2)(*[b for b, _ in pairs])
    passed = [np.zeros(int(b.n_rec), dtype=np.uint8) for b in batches]  # (room for every record: the aligned ones are a prefix of it)
    cnt, rep = (FilterFileCounts * 2)(), FilterReport()
    ctx._chk(lib().pp_filter_records(ctx._h, batches, mem, orientation.encode(), low, high, passed[0].ctypes.data, passed[1].ctypes.data, cnt, C.byref(rep)))
    return {"pass": tuple(p[:int(c.alignments)].copy() for p, c in zip(passed, cnt)),
            "counts": [(int(c.alignments), int(c.reads)) for c in cnt], "report": _report_dict(rep)}


def shard_count(ctx, n_aln, contig_ptr, mem, n_contigs, ptrs=None, into=None):
    """pp_shard_count: alignment records per contig of a batch given by pointers, ADDED to `into` (uint64, n_contigs; default:
    zeros)."""
    p = ptrs or {}
    one = contig_ptr
    b = AlnBatch(n_aln, contig_ptr, p.get("ref_start", one), p.get("k", one), p.get("seq_off", one), p.get("seq_len", one),
                 p.get("cig_off", one), p.get("n_cig", one), p.get("seq", one), 0, p.get("cigar", one), 0)
    cnt = np.zeros(n_contigs, dtype=np.uint64) if into is None else into
    assert cnt.dtype == np.uint64 and len(cnt) == n_contigs and cnt.flags.c_contiguous
    rc = lib().pp_shard_count(ctx._h if ctx is not None else None, C.byref(b), mem, n_contigs, cnt.ctypes.data)
    if rc:
        raise PolypolishError(rc, "pp_shard_count failed")
    return cnt


def comm_unique_id() -> bytes:
    """ncclUniqueId for pp_comm_init (rank 0 makes it, the launcher hands it to every rank)."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    rc = lib().pp_comm_unique_id(buf)
    if rc:
        raise PolypolishError(rc, "pp_comm_unique_id failed (librccl not loadable?)")
    return buf.raw


# pp_filter_file's arrays; "cigar" holds n_cig_total entries, "grp_off" n_reads + 1, every other one n_aln
_FILTER_FILE_FIELDS = (("ref_id", np.uint32), ("ref_start", np.uint32), ("flags", np.uint32), ("ref_end", np.uint64), ("cig_off", np.uint64),
                       ("n_cig", np.uint32), ("cigar", np.uint32), ("read", np.uint32), ("grp_off", np.uint32), ("grp_idx", np.uint32))


class _FilterLoad(_Owned):
    """what FilterLoaded and FilterLoadedDevice share: .counts from the load's pp_filter_file_counts, and .input / .n_reads /
    .files from the pp_filter_input the library hands out, read with `get` (_host or Context.download), without `skip`"""

    def _loaded(self, rc, fc, msg):
        self.counts = [(c.alignments, c.reads) if c.loaded else None for c in fc]
        if rc:
            self._p = C.c_void_p()
            raise PolypolishError(rc, msg())

    def _read_input(self, input_fn, get, skip):
        self.input = FilterInput()
        input_fn(self._p, C.byref(self.input))
        self.n_reads = int(self.input.n_reads)
        self.files = []
        for d in self.input.file:
            sizes = {"cigar": int(d.n_cig_total), "grp_off": self.n_reads + 1}
            self.files.append({k: get(getattr(d, k), sizes.get(k, int(d.n_aln)), dt) for k, dt in _FILTER_FILE_FIELDS if k not in skip})


class FilterLoaded(_FilterLoad):
    """Host half of the filter (pp_filter_load / pp_filter_write; no GPU needed): `files[f]` holds the SoA
    of pp_filter_file as numpy copies, `counts[f]` = (alignments, distinct read names)."""
    _free = "pp_filter_loaded_free"

    def __init__(self, in1, in2):
        L = lib()
        super().__init__()
        err = C.create_string_buffer(1400)
        fc = (FilterFileCounts * 2)()
        rc = L.pp_filter_load(str(in1).encode(), str(in2).encode(), C.byref(self._p), fc, err, 1400)
        self._loaded(rc, fc, lambda: err.value.decode())
        self._read_input(L.pp_filter_loaded_input, _host, ("ref_end",))

    def write(self, f, passed, path):
        passed = np.ascontiguousarray(passed, dtype=np.uint8)
        err = C.create_string_buffer(1400)
        p_, f_ = C.c_uint64(), C.c_uint64()
        rc = lib().pp_filter_write(self._p, f, passed.ctypes.data, str(path).encode(), C.byref(p_), C.byref(f_), err, 1400)
        if rc:
            raise PolypolishError(rc, err.value.decode())
        return p_.value, f_.value


class FilterLoadedDevice(_FilterLoad):
    """pp_filter_load_device: the same load on the GPU; `files[f]` holds copies of the device arrays
    (ref_end instead of the CIGAR arrays), `counts[f]` = (alignments, distinct read names)."""
    _free = "pp_filter_dev_free"

    def __init__(self, ctx, in1, in2):
        L = lib()
        super().__init__()
        fc = (FilterFileCounts * 2)()
        rc = L.pp_filter_load_device(ctx._h, str(in1).encode(), str(in2).encode(), C.byref(self._p), fc)
        self._loaded(rc, fc, lambda: L.pp_last_error(ctx._h).decode())
        self._read_input(L.pp_filter_dev_input, ctx.download, ("cig_off", "n_cig", "cigar"))


class Context:
    """One HIP device + stream (pp_ctx)."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        rc = lib().pp_ctx_create(device, C.byref(self._h))
        if rc:
            raise PolypolishError(rc, f"pp_ctx_create({device}) failed: no usable HIP device (there is no CPU path)")
        self._keep = []

    def close(self):
        if self._h:
            lib().pp_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc:
            raise PolypolishError(rc, lib().pp_last_error(self._h).decode())

    def download(self, addr, n, dtype):
        """n items of DEVICE memory at addr as a numpy array (pp_ctx_download); zeros when n == 0 or there is no address"""
        arr = np.zeros(int(n), dtype=dtype)
        if arr.size and addr:
            self._chk(lib().pp_ctx_download(self._h, arr.ctypes.data, addr, arr.nbytes))
        return arr

    def sync(self):
        self._chk(lib().pp_ctx_sync(self._h))

    def set_profiling(self, on=True):
        """False/0 off, True/1 every kernel group, 2 only the dominant kernel (one event pair per job)."""
        lib().pp_ctx_set_profiling(self._h, int(on))

    def set_regroup(self, on=True):
        """pp_ctx_set_regroup: polish_files and the polish half of filter_polish_files regroup every BAM file's records in front of
        the gate (coordinate-sorted BAM; the commands' --regroup)."""
        self._chk(lib().pp_ctx_set_regroup(self._h, int(bool(on))))

    def set_text_chain(self, on=True):
        """pp_ctx_set_text_chain: polish_files, filter_files and filter_polish_files take SAM text inputs, plain or bgzipped, through
        the record chain on the device (the commands' --text_chain); regrouping is then accepted on text."""
        self._chk(lib().pp_ctx_set_text_chain(self._h, int(bool(on))))

    def set_out_bam(self, on=True):
        """pp_ctx_set_out_bam: filter_files / filter_polish_files write the outputs of SAM text inputs as compressed BAM (the
        commands' --out_bam)."""
        self._chk(lib().pp_ctx_set_out_bam(self._h, int(bool(on))))

    def set_out_sam(self, on=True):
        """pp_ctx_set_out_sam: filter_files / filter_polish_files write the outputs of BAM inputs as SAM text (the commands'
        --out_sam)."""
        self._chk(lib().pp_ctx_set_out_sam(self._h, int(bool(on))))

    # ---- seam B -------------------------------------------------------------------------------
    def polish_begin(self, contig_off, bases_ptr, bases_mem, min_depth=5, fraction_valid=0.5, fraction_invalid=0.2):
        off = np.ascontiguousarray(contig_off, dtype=np.uint64)
        p = Params(min_depth, fraction_valid, fraction_invalid)
        self._n_contigs = len(off) - 1
        self._G = int(off[-1])
        self._chk(lib().pp_polish_begin(self._h, self._n_contigs, off.ctypes.data, bases_ptr, bases_mem, C.byref(p)))

    def polish_add_ptrs(self, n_aln, ptrs: dict, seq_bytes, n_cig_total, mem):
        b = aln_batch(n_aln, ptrs, seq_bytes, n_cig_total)
        self._chk(lib().pp_polish_add(self._h, C.byref(b), mem))

    def polish_finish(self):
        self._chk(lib().pp_polish_finish(self._h))

    def prepared_job(self, contig_off, bases_ptr, bases_mem, n_aln, ptrs: dict, seq_bytes, n_cig_total, mem,
                     min_depth=5, fraction_valid=0.5, fraction_invalid=0.2, emit=None):
        """begin + (set_emit) + add + finish of ONE job with every argument marshalled once: returns run(), which makes
        the three (four) C calls and nothing else.  For callers that repeat a job on resident data (bench.py's steps): the
        Python side of polish_begin / polish_add_ptrs costs tens of microseconds per call, during which the GPU idles."""
        L = lib()
        off = np.ascontiguousarray(contig_off, dtype=np.uint64)
        p = Params(min_depth, fraction_valid, fraction_invalid)
        b = aln_batch(n_aln, ptrs, seq_bytes, n_cig_total)
        n_contigs, G = len(off) - 1, int(off[-1])
        h, off_p, p_ref, b_ref = self._h, off.ctypes.data, C.byref(p), C.byref(b)
        begin, add, finish, set_emit = L.pp_polish_begin, L.pp_polish_add, L.pp_polish_finish, L.pp_polish_set_emit
        if emit is not None:
            e = np.ascontiguousarray(emit, dtype=np.uint64).reshape(n_contigs, 2)
            lo, hi = np.ascontiguousarray(e[:, 0]), np.ascontiguousarray(e[:, 1])
            lo_p, hi_p = lo.ctypes.data, hi.ctypes.data
        keep = (off, p, b, emit is not None and (lo, hi))  # the C side reads these during the calls

        def run():
            self._n_contigs, self._G = n_contigs, G
            rc = begin(h, n_contigs, off_p, bases_ptr, bases_mem, p_ref)
            if rc == 0 and emit is not None:
                rc = set_emit(h, lo_p, hi_p)
            if rc == 0:
                rc = add(h, b_ref, mem)
            if rc == 0:
                rc = finish(h)
            if rc:
                self._chk(rc)
        run._keep = keep
        return run

    def result_size(self):
        n = C.c_uint64()
        self._chk(lib().pp_polish_result_size(self._h, C.byref(n)))
        return n.value

    def result_device_ptr(self):
        return lib().pp_polish_result_device(self._h)

    def result(self):
        n = self.result_size()
        out = np.zeros(max(n, 1), dtype=np.uint8)
        offs = np.zeros(self._n_contigs + 1, dtype=np.uint64)
        stats = (ContigStats * self._n_contigs)()
        self._chk(lib().pp_polish_result(self._h, out.ctypes.data, MEM_HOST, offs.ctypes.data, stats))
        st = [dict(polished_len=s.polished_len, changed=s.changed, zero_depth=s.zero_depth, depth_sum=s.depth_sum)
              for s in stats]
        return out[:n].tobytes(), offs, st

    def trust_mirrors(self, on=True):
        """(internal hook, pp_ctx_trust_mirrors_) every window-order mirror this context is given counts as one of the library's
        own: it is not compared with the arrays before the kernels read the records through it.  For callers that lay their
        batches out exactly as the library's ingests do (bench.py's resident job; tests/test_synthjob_cpu.py checks that it does)."""
        self._chk(lib().pp_ctx_trust_mirrors_(self._h, int(bool(on))))

    def took_direct_path(self):
        """True when the last pp_polish_finish took its bulk straight from the window-order mirror (pp_aln_batch.wo_run_end)."""
        return bool(lib().pp_polish_took_direct_path(self._h))

    def kernel_times(self):
        kt = KernelTimes()
        lib().pp_polish_kernel_times(self._h, C.byref(kt))
        return kt.as_dict()

    def first_kernel_ms(self):
        """(name as bytes, milliseconds) of the first kernel group the last job timed, or None: what bench.py's timed steps read
        after every job (profiling level 2: the dominant kernel alone) -- one C call into a structure that is kept, no dictionaries."""
        kt = getattr(self, "_kt", None)
        if kt is None:
            kt = self._kt = KernelTimes()
            self._kt_ref = C.byref(kt)
            self._kt_fn = lib().pp_polish_kernel_times
        self._kt_fn(self._h, self._kt_ref)
        return (kt.name[0], kt.ms[0]) if kt.n else None

    def positions(self):
        G = self._G
        arrs = {"depth": np.zeros(G, np.float64), "status": np.zeros(G, np.uint8)}
        for k in ("count_a", "count_c", "count_g", "count_t", "count_other", "valid_thr", "invalid_thr"):
            arrs[k] = np.zeros(G, np.uint32)
        po = PositionsOut(*[arrs[k].ctypes.data for k in ("depth", "count_a", "count_c", "count_g", "count_t",
                                                          "count_other", "valid_thr", "invalid_thr", "status")])
        self._chk(lib().pp_polish_positions(self._h, C.byref(po)))
        return arrs

    def debug_tsv(self, contig_names, lo=0, hi=None, chunk=64 << 20) -> bytes:
        """The --debug TSV lines (no header) of positions [lo, hi) of the last job, formatted on the device
        (pp_polish_debug_tsv): the job must have run with per-position records (polish_records(..., positions=True)).
        A context with emit ranges gives the lines of the positions it emits.  Fetched `chunk` bytes at a time."""
        names = [n.encode() if isinstance(n, str) else bytes(n) for n in contig_names]
        if len(names) != self._n_contigs:
            raise PolypolishError(ERR_ARG, "debug_tsv: one name per contig")
        arr = (C.c_char_p * max(len(names), 1))(*names)
        hi = self._G if hi is None else int(hi)
        buf = np.empty(max(int(chunk), 1), dtype=np.uint8)
        n, nxt = C.c_uint64(), C.c_uint64()
        parts, p = [], int(lo)
        while True:
            self._chk(lib().pp_polish_debug_tsv(self._h, C.cast(arr, C.c_void_p), p, hi, buf.ctypes.data, MEM_HOST, len(buf),
                                                C.byref(n), C.byref(nxt)))
            parts.append(buf[:n.value].tobytes())
            if nxt.value >= hi or nxt.value == p:
                return b"".join(parts)
            p = nxt.value

    def set_emit(self, emit):
        """emit: None or an (n_contigs, 2) array of [lo, hi) positions each contig emits (pp_polish_set_emit)."""
        if emit is None:
            self._chk(lib().pp_polish_set_emit(self._h, None, None))
            return
        e = np.ascontiguousarray(emit, dtype=np.uint64).reshape(-1, 2)
        lo, hi = np.ascontiguousarray(e[:, 0]), np.ascontiguousarray(e[:, 1])
        if len(lo) != self._n_contigs:
            raise PolypolishError(ERR_ARG, "set_emit: one range per contig")
        self._chk(lib().pp_polish_set_emit(self._h, lo.ctypes.data, hi.ctypes.data))

    def comm_init(self, rank, world, unique_id: bytes):
        """Join the RCCL communicator of the job (pp_comm_init): one context per rank / GPU."""
        self._chk(lib().pp_comm_init(self._h, rank, world, C.c_char_p(unique_id)))
        self._comm = (rank, world)

    def gather(self, gathered_ptr, cap):
        """pp_polish_gather: the polished bytes of all ranks -> rank 0's DEVICE buffer (rank-major).
        Returns (rank_len, rank_contig_off) as numpy arrays (on every rank)."""
        rank, world = self._comm
        lens = np.zeros(world, dtype=np.uint64)
        offs = np.zeros((world, self._n_contigs + 1), dtype=np.uint64)
        self._chk(lib().pp_polish_gather(self._h, gathered_ptr, cap, lens.ctypes.data, offs.ctypes.data))
        return lens, offs

    def polish_records(self, contig_off, bases, recs, min_depth=5, fraction_valid=0.5, fraction_invalid=0.2,
                       positions=False, emit=None, cuts=None, debug=False):
        """Host numpy SoA (field names of pp_aln_batch) -> polished bytes, offsets, stats.
        cuts: optional record indices at which the records are cut into several pp_polish_add batches.
        positions: True = the per-position records of --debug; 3 = the records of what the pileup kernel itself decides
        (test hook: positions with inexact depth shares settled by its interval test are not replayed).
        debug: True = the job keeps the --debug records on the device for debug_tsv() without fetching them."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        keep = {k: np.ascontiguousarray(recs[k], dtype=dt) for k, dt in REC_FIELDS}
        lib().pp_polish_set_debug(self._h, int(positions) if positions else int(bool(debug)))
        self.polish_begin(contig_off, bases.ctypes.data, MEM_HOST, min_depth, fraction_valid, fraction_invalid)
        if emit is not None:
            self.set_emit(emit)
        for part in split_records(keep, cuts):
            ptrs = {k: v.ctypes.data for k, v in part.items()}
            if cuts is None and recs.get("wo") is not None and len(recs["wo"]) == len(keep["contig"]) and len(recs["wo"]):
                # the window-order mirror of the records (WO_DTYPE) and, optionally, the ends of its runs
                keep["wo"] = np.ascontiguousarray(recs["wo"])
                ptrs["wo"] = keep["wo"].ctypes.data
                if recs.get("wo_runs") is not None and len(recs["wo_runs"]):
                    ptrs["wo_runs"] = recs["wo_runs"]
            self.polish_add_ptrs(len(part["contig"]), ptrs, len(part["seq"]), len(part["cigar"]), MEM_HOST)
        self.polish_finish()
        polished, offs, stats = self.result()
        res = {"polished": polished, "offsets": offs, "stats": stats, "positions": None}
        if positions:
            res["positions"] = self.positions()
        lib().pp_polish_set_debug(self._h, 0)
        return res

    def polish_raw(self, contig_off, bases, raws, max_errors=10, careful=False, passed=None, prepare=False, min_depth=5,
                   fraction_valid=0.5, fraction_invalid=0.2, positions=False, regroup=False):
        """The record chain (regroup ->) gate -> (prepare) -> polish: raws = the raw records of every SAM file (host numpy, RAW_FIELDS), in
        argv order; passed = None or one entry per file (None or the filter's verdicts).  Every file is gated on the device
        (gate_records; with `regroup` behind regroup_records, the verdicts carried along: for files whose reads do not stand
        together), the gated batches -- each through pp_batch_prepare when `prepare` -- are added one after the other.
        Returns what polish_records returns, plus "counts": (alignments, used, reads) per file."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        gated = []
        for f, raw in enumerate(raws):
            v = None if passed is None else passed[f]
            if regroup:
                g = regroup_records(self, raw)
                try:
                    gated.append(gate_records(self, g.raw(), max_errors, careful, None if v is None else g.carry_pass(v), MEM_DEVICE))
                finally:
                    g.close()
            else:
                gated.append(gate_records(self, raw, max_errors, careful, v))
        batches = [prepare_batch(self, contig_off, g.n_aln, g.ptrs(), g.seq_bytes, g.n_cig_total, MEM_DEVICE) for g in gated] if prepare else gated
        lib().pp_polish_set_debug(self._h, int(positions) if positions else 0)
        try:
            self.polish_begin(contig_off, bases.ctypes.data, MEM_HOST, min_depth, fraction_valid, fraction_invalid)
            for b in batches:
                if b.n_aln:  # (a file without a good record adds nothing)
                    self.polish_add_ptrs(b.n_aln, b.ptrs(), b.seq_bytes, b.n_cig_total, MEM_DEVICE)
            self.polish_finish()
            polished, offs, stats = self.result()
            res = {"polished": polished, "offsets": offs, "stats": stats, "positions": self.positions() if positions else None,
                   "counts": [g.counts for g in gated]}
        finally:
            lib().pp_polish_set_debug(self._h, 0)
            for b in batches + gated:
                b.close()
        return res

    def filter_thresholds(self, orientation="auto", low=0.1, high=99.9):
        """pp_filter_thresholds after pp_filter_begin: orientation counts, the correct orientation and the two insert size
        thresholds from the samples in device memory -> {"counts", "orientation", "low", "high", "before", "after": 0}."""
        rep = FilterReport()
        self._chk(lib().pp_filter_thresholds(self._h, orientation.encode(), low, high, C.byref(rep)))
        return _report_dict(rep)

    # ---- whole commands -----------------------------------------------------------------------
    @contextlib.contextmanager
    def _regrouping(self, regroup):
        """regroup=True switches the context's regrouping on for one command; False leaves what set_regroup chose"""
        if not regroup:
            yield
            return
        was = bool(lib().pp_ctx_regroup_(self._h))
        self.set_regroup(True)
        try:
            yield
        finally:
            self.set_regroup(was)

    @contextlib.contextmanager
    def _chaining_text(self, text_chain):
        """text_chain=True switches pp_ctx_set_text_chain on for one command; False leaves what set_text_chain chose"""
        if not text_chain:
            yield
            return
        was = bool(lib().pp_ctx_text_chain_(self._h))
        self.set_text_chain(True)
        try:
            yield
        finally:
            self.set_text_chain(was)

    @contextlib.contextmanager
    def _fasta_form(self, wrap, bgzf, out, index):
        """wrap= (a line width, 0: one line per contig), bgzf=, out= (a path) and index= of one command: pp_ctx_set_fasta_form for its
        duration; behind it the FASTA the command returned is written to `out`, with `out`.fai (and `out`.gzi under bgzf) for index.
        The command hands its bytes to the function this yields."""
        if index and out is None:
            raise PolypolishError(ERR_QUIT, "index=True needs out=<path>: the indexes are written next to the file")
        L = lib()
        on = wrap is not None or bgzf or index
        if on:
            self._chk(L.pp_ctx_set_fasta_form(self._h, int(wrap or 0), int(bool(bgzf))))
        L.pp_ctx_set_fasta_out_name_(self._h, os.fsencode(out) if out is not None else None)

        def deliver(data):
            if out is None:
                return
            try:
                with open(out, "wb") as f:
                    f.write(data)
                if index:
                    fai, gzi = self.fasta_index()
                    with open(os.fspath(out) + ".fai", "wb") as f:
                        f.write(fai)
                    if bgzf:
                        with open(os.fspath(out) + ".gzi", "wb") as f:
                            f.write(gzi)
            except OSError:
                raise PolypolishError(ERR_QUIT, f'unable to write the polished sequence to "{os.fspath(out)}"') from None
        try:
            yield deliver
        finally:
            if on:
                L.pp_ctx_set_fasta_form(self._h, -1, 0)
            L.pp_ctx_set_fasta_out_name_(self._h, None)

    def set_fasta_form(self, width, bgzf=False):
        """pp_ctx_set_fasta_form: polish_files and filter_polish_files return the FASTA made by pp_fasta_text at this line width (0:
        one line per contig; None: off, the host loop as before), compressed by pp_bgzf_deflate with bgzf."""
        self._chk(lib().pp_ctx_set_fasta_form(self._h, -1 if width is None else int(width), int(bool(bgzf))))

    def fasta_index(self):
        """pp_ctx_fasta_index: (.fai bytes, .gzi bytes) of the last FASTA a command made on this context with the form set"""
        fai, gzi = Bytes(), Bytes()
        self._chk(lib().pp_ctx_fasta_index(self._h, C.byref(fai), C.byref(gzi)))
        return _take_bytes(fai), _take_bytes(gzi)

    def set_vcf(self, on=True, bgzf=False):
        """pp_ctx_set_vcf: polish_files and filter_polish_files run pp_polish_vcf behind their polish (bgzf: pp_bgzf_deflate behind it);
        vcf() fetches the file"""
        self._chk(lib().pp_ctx_set_vcf(self._h, int(bool(on)), int(bool(bgzf))))

    def vcf(self):
        """pp_ctx_vcf: the VCF file (bytes) of the last command that made one on this context"""
        b = Bytes()
        self._chk(lib().pp_ctx_vcf(self._h, C.byref(b)))
        return _take_bytes(b)

    @contextlib.contextmanager
    def _making_vcf(self, vcf, vcf_bgzf):
        """vcf= (a path) and vcf_bgzf= of one command: pp_ctx_set_vcf for its duration; the function this yields writes the file once
        the command has succeeded"""
        if vcf_bgzf and vcf is None:
            raise PolypolishError(ERR_QUIT, "vcf_bgzf=True needs vcf=<path>: it compresses the VCF file")
        if vcf is None:
            yield lambda: None
            return
        self.set_vcf(True, vcf_bgzf)

        def deliver():
            data = self.vcf()
            try:
                with open(vcf, "wb") as f:
                    f.write(data)
            except OSError:
                raise PolypolishError(ERR_QUIT, f'unable to write the VCF to "{os.fspath(vcf)}"') from None
        try:
            yield deliver
        finally:
            self.set_vcf(False)

    def set_bed(self, on=True, mask=BED_UNDECIDED, bgzf=False):
        """pp_ctx_set_bed: polish_files and filter_polish_files keep the per-position status and run pp_polish_bed behind their polish
        (bgzf: pp_bgzf_deflate behind it); bed() fetches the file"""
        self._chk(lib().pp_ctx_set_bed(self._h, int(bool(on)), int(mask) if on else 0, int(bool(bgzf))))

    def bed(self):
        """pp_ctx_bed: the BED file (bytes) of the last command that made one on this context"""
        b = Bytes()
        self._chk(lib().pp_ctx_bed(self._h, C.byref(b)))
        return _take_bytes(b)

    def set_soft_mask(self, mask=BED_UNDECIDED):
        """pp_ctx_set_soft_mask: the FASTA of polish_files and filter_polish_files has the bytes of positions with a selected status in
        lower case (pp_polish_masked); 0 / None / False: off"""
        self._chk(lib().pp_ctx_set_soft_mask(self._h, int(mask or 0)))

    @contextlib.contextmanager
    def _making_bed(self, bed, bed_bgzf, bed_status, soft_mask):
        """bed= (a path), bed_bgzf=, bed_status= and soft_mask= of one command: pp_ctx_set_bed / pp_ctx_set_soft_mask for its duration;
        the function this yields writes the BED once the command has succeeded"""
        if bed_bgzf and bed is None:
            raise PolypolishError(ERR_QUIT, "bed_bgzf=True needs bed=<path>: it compresses the BED file")
        if bed_status is not None and bed is None and not soft_mask:
            raise PolypolishError(ERR_QUIT, "bed_status= needs bed=<path> or soft_mask=True: it chooses what they select")
        if bed is None and not soft_mask:
            yield lambda: None
            return
        mask = bed_status_mask(bed_status)
        if bed is not None:
            self.set_bed(True, mask, bed_bgzf)
        if soft_mask:
            self.set_soft_mask(mask)

        def deliver():
            if bed is None:
                return
            data = self.bed()
            try:
                with open(bed, "wb") as f:
                    f.write(data)
            except OSError:
                raise PolypolishError(ERR_QUIT, f'unable to write the BED to "{os.fspath(bed)}"') from None
        try:
            yield deliver
        finally:
            self.set_bed(False)
            self.set_soft_mask(0)

    def depth_bedgraph(self, depth, contig_off, names, bin=0, mem=MEM_HOST):  # noqa: A002
        """pp_depth_bedgraph: a caller's per-position depths (numpy float64, or a device address with mem=MEM_DEVICE) -> DepthTrack"""
        return DepthTrack(self, names, bin, depth, contig_off, mem)

    def polish_depth(self, names, bin=0):  # noqa: A002
        """pp_polish_depth: the finished job's own depth plane (it ran with debug records) -> DepthTrack"""
        return DepthTrack(self, names, bin)

    def set_depth(self, on=True, bin=0, bgzf=False):  # noqa: A002
        """pp_ctx_set_depth: polish_files and filter_polish_files keep the per-position depth and run pp_polish_depth behind their
        polish (bgzf: pp_bgzf_deflate behind it); depth() fetches the file"""
        self._chk(lib().pp_ctx_set_depth(self._h, int(bool(on)), int(bin) if on else 0, int(bool(bgzf))))

    def depth(self):
        """pp_ctx_depth: the depth track (bytes) of the last command that made one on this context"""
        b = Bytes()
        self._chk(lib().pp_ctx_depth(self._h, C.byref(b)))
        return _take_bytes(b)

    @contextlib.contextmanager
    def _making_depth(self, depth, depth_bin, depth_bgzf):
        """depth= (a path), depth_bin= and depth_bgzf= of one command: pp_ctx_set_depth for its duration; the function this yields
        writes the file once the command has succeeded"""
        if depth_bin is not None and depth is None:
            raise PolypolishError(ERR_QUIT, "depth_bin= needs depth=<path>: it chooses the form of the depth track")
        if depth_bgzf and depth is None:
            raise PolypolishError(ERR_QUIT, "depth_bgzf=True needs depth=<path>: it compresses the depth track")
        if depth is None:
            yield lambda: None
            return
        w = 0 if depth_bin is None else depth_bin
        if isinstance(w, bool) or not isinstance(w, (int, np.integer)) or not 0 <= int(w) <= 1 << 24:
            raise PolypolishError(ERR_QUIT, f"depth_bin: {w!r} is not an integer in 0..16777216")
        self.set_depth(True, int(w), depth_bgzf)

        def deliver():
            data = self.depth()
            try:
                with open(depth, "wb") as f:
                    f.write(data)
            except OSError:
                raise PolypolishError(ERR_QUIT, f'unable to write the depth track to "{os.fspath(depth)}"') from None
        try:
            yield deliver
        finally:
            self.set_depth(False)

    def set_tbi(self, vcf=False, bed=False, depth=False):
        """pp_ctx_set_tbi: polish_files and filter_polish_files run pp_tabix_index behind the pp_bgzf_deflate of the tracks named;
        tbi(which) fetches an index"""
        self._chk(lib().pp_ctx_set_tbi(self._h, int(bool(vcf)), int(bool(bed)), int(bool(depth))))

    def tbi(self, which):
        """pp_ctx_tbi: the .tbi (bytes) of the VCF, BED or depth track ("vcf" | "bed" | "depth", or PP_TBI_*) of the last command
        that made one on this context"""
        b = Bytes()
        self._chk(lib().pp_ctx_tbi(self._h, TBI_TRACKS.index(which) if which in TBI_TRACKS else int(which), C.byref(b)))
        return _take_bytes(b)

    @contextlib.contextmanager
    def _making_tbi(self, tbi, paths, bgzf):
        """tbi= of one command -- True: every bgzipped track; or the tracks by name, "vcf", "bed", "depth" --: pp_ctx_set_tbi for its
        duration; the function this yields writes <track path>.tbi once the command has succeeded and the tracks are written"""
        if not tbi:
            yield lambda: None
            return
        names = [t for t in TBI_TRACKS if bgzf[t] and paths[t] is not None] if tbi is True else ([tbi] if isinstance(tbi, str) else list(tbi))
        for t in names:
            if t not in TBI_TRACKS:
                raise PolypolishError(ERR_QUIT, f"tbi: {t!r} is not one of vcf, bed, depth")
            if not bgzf[t] or paths[t] is None:
                raise PolypolishError(ERR_QUIT, f"tbi={t!r} needs {t}_bgzf=True: a .tbi indexes the bgzipped file")
        if not names:
            raise PolypolishError(ERR_QUIT, "tbi=True needs a bgzipped track (vcf_bgzf, bed_bgzf or depth_bgzf): a .tbi indexes a bgzipped file")
        self.set_tbi(*[t in names for t in TBI_TRACKS])

        def deliver():
            for t in names:
                to = os.fspath(paths[t]) + ".tbi"
                data = self.tbi(t)
                try:
                    with open(to, "wb") as f:
                        f.write(data)
                except OSError:                                 # (no track and no index are left behind)
                    for junk in (to, paths[t]):
                        with contextlib.suppress(OSError):
                            os.remove(junk)
                    raise PolypolishError(ERR_QUIT, f'unable to write the index of the {t} track to "{to}"') from None
        try:
            yield deliver
        finally:
            self.set_tbi(False, False, False)

    @contextlib.contextmanager
    def _writing_bam(self, out_bam):
        """out_bam=True switches pp_ctx_set_out_bam on for one command and off again behind it"""
        if not out_bam:
            yield
            return
        self.set_out_bam(True)
        try:
            yield
        finally:
            self.set_out_bam(False)

    def set_sort_out(self, on=True, index=False):
        """pp_ctx_set_sort_out: the filter commands write their BAM outputs in coordinate order, with index a .bai next to each"""
        self._chk(lib().pp_ctx_set_sort_out(self._h, int(bool(on)), int(bool(index))))

    @contextlib.contextmanager
    def _sorting_out(self, sort_out, out_bai):
        """sort_out / out_bai switch pp_ctx_set_sort_out on for one command and off again behind it"""
        if not sort_out and not out_bai:
            yield
            return
        self.set_sort_out(sort_out, out_bai)
        try:
            yield
        finally:
            self.set_sort_out(False, False)

    @contextlib.contextmanager
    def _writing_sam(self, out_sam):
        """out_sam=True switches pp_ctx_set_out_sam on for one command and off again behind it"""
        if not out_sam:
            yield
            return
        self.set_out_sam(True)
        try:
            yield
        finally:
            self.set_out_sam(False)

    def polish_files(self, assembly, sams, fraction_invalid=0.2, fraction_valid=0.5, max_errors=10, min_depth=5,
                     careful=False, debug=None, quiet=True, regroup=False, text_chain=False, wrap=None, bgzf=False, out=None,
                     index=False, vcf=None, vcf_bgzf=False, bed=None, bed_bgzf=False, bed_status=None, soft_mask=False,
                     depth=None, depth_bin=None, depth_bgzf=False, tbi=False):
        """polish::polish (pp_polish_files): the FASTA bytes.  wrap / bgzf / out / index (not in the reference): the FASTA at a line
        width (0: one line per contig) and bgzipped, made on the device (pp_fasta_text, pp_bgzf_deflate); also written to `out`,
        with out.fai (and out.gzi) for index.  `sams` are SAM text files, or all of them BAM files (BGZF or
        uncompressed; told by content, aln_file_kind): those go through the record chain on the device, inside the driver.
        regroup: for this call, as set_regroup (coordinate-sorted BAM).  text_chain: for this call, as set_text_chain (SAM text,
        plain or bgzipped, through the record chain as well).  vcf / vcf_bgzf (not in the reference): the polish's edits written to
        the path `vcf` as VCF 4.2 made on the device (pp_polish_vcf), bgzipped with vcf_bgzf.  bed / bed_bgzf / bed_status / soft_mask
        (not in the reference): the runs of undecided positions written to the path `bed` as BED made on the device (pp_polish_bed),
        bgzipped with bed_bgzf; soft_mask: their bases in lower case in the FASTA (pp_polish_masked); bed_status: the statuses both
        select (bed_status_mask; default the four undecided ones).  depth / depth_bin / depth_bgzf (not in the reference): the read
        depth written to the path `depth` as bedGraph made on the device (pp_polish_depth) -- runs of equal depth, or with depth_bin=N
        the mean of bins of N positions --, bgzipped with depth_bgzf.  tbi (not in the reference): True, or some of "vcf", "bed",
        "depth": the tabix index of those bgzipped tracks, made on the device (pp_tabix_index), written to <track path>.tbi."""
        opt = PolishOptions(fraction_invalid, fraction_valid, max_errors, min_depth, int(careful),
                            str(debug).encode() if debug else None, int(quiet))
        arr = (C.c_char_p * max(len(sams), 1))(*[str(s).encode() for s in sams])
        res = Bytes()
        with self._regrouping(regroup), self._chaining_text(text_chain), self._making_vcf(vcf, vcf_bgzf) as deliver_vcf, \
                self._making_bed(bed, bed_bgzf, bed_status, soft_mask) as deliver_bed, \
                self._making_depth(depth, depth_bin, depth_bgzf) as deliver_depth, \
                self._making_tbi(tbi, dict(vcf=vcf, bed=bed, depth=depth), dict(vcf=vcf_bgzf, bed=bed_bgzf, depth=depth_bgzf)) as deliver_tbi, \
                self._fasta_form(wrap, bgzf, out, index) as deliver:
            self._chk(lib().pp_polish_files(self._h, str(assembly).encode(), arr, len(sams), C.byref(opt), C.byref(res)))
            data = _take_bytes(res)
            deliver_vcf()
            deliver_bed()
            deliver_depth()
            deliver_tbi()
            deliver(data)
        return data

    def filter_polish_files(self, assembly, in1, in2, out1=None, out2=None, orientation="auto", low=0.1, high=99.9,
                            fraction_invalid=0.2, fraction_valid=0.5, max_errors=10, min_depth=5, careful=False,
                            debug=None, quiet=True, regroup=False, out_bam=False, out_sam=False, text_chain=False, wrap=None,
                            bgzf=False, out=None, index=False, sort_out=False, out_bai=False, vcf=None, vcf_bgzf=False, bed=None,
                            bed_bgzf=False, bed_status=None, soft_mask=False, depth=None, depth_bin=None, depth_bgzf=False, tbi=False):
        """filter + polish in one process (pp_filter_polish_files): returns (FASTA bytes, filter report).  wrap / bgzf / out / index:
        as polish_files.  Two BAM inputs are decoded
        once for both halves; out1 / out2 are then BAM files as well.  regroup: for this call, as set_regroup (the polish half).
        out_bam: for this call, as set_out_bam (SAM text inputs, out1 / out2 as compressed BAM).  out_sam: for this call, as
        set_out_sam (BAM inputs, out1 / out2 as SAM text).  text_chain: for this call, as set_text_chain.  sort_out / out_bai: for
        this call, as set_sort_out (BAM outputs in coordinate order, out1.bai / out2.bai next to them).  vcf / vcf_bgzf, bed /
        bed_bgzf / bed_status / soft_mask, depth / depth_bin / depth_bgzf, tbi: as polish_files."""
        opt = PolishOptions(fraction_invalid, fraction_valid, max_errors, min_depth, int(careful),
                            str(debug).encode() if debug else None, int(quiet))
        rep, res = FilterReport(), Bytes()
        enc = lambda x: str(x).encode() if x is not None else None
        with self._regrouping(regroup), self._writing_bam(out_bam), self._writing_sam(out_sam), self._chaining_text(text_chain), \
                self._sorting_out(sort_out, out_bai), self._making_vcf(vcf, vcf_bgzf) as deliver_vcf, \
                self._making_bed(bed, bed_bgzf, bed_status, soft_mask) as deliver_bed, \
                self._making_depth(depth, depth_bin, depth_bgzf) as deliver_depth, \
                self._making_tbi(tbi, dict(vcf=vcf, bed=bed, depth=depth), dict(vcf=vcf_bgzf, bed=bed_bgzf, depth=depth_bgzf)) as deliver_tbi, \
                self._fasta_form(wrap, bgzf, out, index) as deliver:
            self._chk(lib().pp_filter_polish_files(self._h, enc(assembly), enc(in1), enc(in2), enc(out1), enc(out2),
                                                   orientation.encode(), low, high, C.byref(opt), C.byref(rep), C.byref(res)))
            data = _take_bytes(res)
            deliver_vcf()
            deliver_bed()
            deliver_depth()
            deliver_tbi()
            deliver(data)
        return data, _report_dict(rep)

    def filter_files(self, in1, in2, out1, out2, orientation="auto", low=0.1, high=99.9, quiet=True, out_bam=False, out_sam=False,
                     text_chain=False, sort_out=False, out_bai=False):
        """filter::filter (pp_filter_files): writes out1 / out2, returns the report.  in1 / in2 are both SAM text, or both BAM:
        BAM in gives compressed BAM out (pp_bam_tagged -> pp_bam_out_deflate).  out_bam: for this call, as set_out_bam (SAM text
        in, compressed BAM out through pp_sam_bam).  out_sam: for this call, as set_out_sam (BAM in, SAM text out through
        pp_bam_sam).  text_chain: for this call, as set_text_chain (SAM text, plain or bgzipped, through the record chain; bgzipped
        in gives bgzipped out).  sort_out / out_bai: for this call, as set_sort_out (BAM outputs in coordinate order, out1.bai /
        out2.bai next to them; SAM text outputs are refused)."""
        rep = FilterReport()
        with self._writing_bam(out_bam), self._writing_sam(out_sam), self._chaining_text(text_chain), self._sorting_out(sort_out, out_bai):
            self._chk(lib().pp_filter_files(self._h, str(in1).encode(), str(in2).encode(), str(out1).encode(),
                                            str(out2).encode(), orientation.encode(), low, high, int(quiet),
                                            C.byref(rep)))
        return _report_dict(rep)


_default_ctx = None


def _ctx():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(int(os.environ.get("PP_DEVICE", "0")))
    return _default_ctx


def polish(assembly, sam, debug=None, fraction_invalid=0.2, fraction_valid=0.5, max_errors=10, min_depth=5,
           careful=False, regroup=False, text_chain=False, wrap=None, bgzf=False, out=None, index=False, bed=None, bed_bgzf=False,
           bed_status=None, soft_mask=False, depth=None, depth_bin=None, depth_bgzf=False, tbi=False) -> bytes:
    """polish::polish (src/polish.rs:26-38): returns the FASTA bytes the reference prints to stdout.  regroup: coordinate-sorted
    BAM files (every read's records are brought together in front of the gate: the command's --regroup).  text_chain: SAM text,
    plain or bgzipped, through the record chain as well (the command's --text_chain; regroup then takes text too).  wrap / bgzf / out /
    index: the commands' --wrap, --out_bgzf, --out and --index; bed / bed_bgzf / bed_status / soft_mask: --bed, --bed_bgzf, --bed_status
    and --soft_mask; depth / depth_bin / depth_bgzf: --depth, --depth_bin and --depth_bgzf; tbi: --bed_tbi and --depth_tbi
    (Context.polish_files)."""
    return _ctx().polish_files(assembly, list(sam), fraction_invalid, fraction_valid, max_errors, min_depth, careful,
                               debug, regroup=regroup, text_chain=text_chain, wrap=wrap, bgzf=bgzf, out=out, index=index, bed=bed,
                               bed_bgzf=bed_bgzf, bed_status=bed_status, soft_mask=soft_mask, depth=depth, depth_bin=depth_bin,
                               depth_bgzf=depth_bgzf, tbi=tbi)


def filter(in1, in2, out1, out2, orientation="auto", low=0.1, high=99.9):  # noqa: A001 (reference name)
    """filter::filter (src/filter.rs:26-37): writes out1/out2, returns the before/after report."""
    return _ctx().filter_files(in1, in2, out1, out2, orientation, low, high)
