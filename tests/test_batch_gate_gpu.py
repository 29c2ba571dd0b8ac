"""pp_batch_gate (include/polypolish_hip.h, pp_gate.hip): process_one_read over a caller's raw records on the device, against
the plain models -- ingest_model.model() on every parse-clean named case, gate_model.gate() at the seams of the kernels -- byte
for byte, then down the chain gate -> (prepare) -> polish against the oracle on the SAM text.  tests/test_gate_model_cpu.py
pins gate_model to ingest_model and asserts the shape of the generated inputs.  Needs an MI355X: `-m gpu`."""
import os

import numpy as np
import pytest

import gate_model as gm
import ingest_model as im
import synth

pytestmark = pytest.mark.gpu
POS_KEYS = ("depth", "count_a", "count_c", "count_g", "count_t", "count_other", "valid_thr", "invalid_thr", "status")


@pytest.fixture(scope="module")
def pp():
    import polypolish_amd
    return polypolish_amd


@pytest.fixture(scope="module")
def ctx(pp):
    c = pp.Context(0)
    yield c
    c.close()


def _gate(pp, ctx, raw, source="host", **kw):
    """-> ({"recs", "orig", "counts"}, the GatedBatch); source "device": the raw arrays live in device memory"""
    if source == "host":
        g = pp.gate_records(ctx, raw, **kw)
    else:
        import torch
        dev = torch.device("cuda:0")
        signed = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64, np.dtype(np.uint8): np.uint8}
        t = {k: torch.from_numpy(np.ascontiguousarray(raw[k], dtype=dt).view(signed[np.dtype(dt)])).to(dev) for k, dt in pp.RAW_FIELDS}
        torch.cuda.synchronize()
        ptrs = {k: v.data_ptr() for k, v in t.items()}
        ptrs.update(n_rec=len(raw["flag"]), seq_bytes=len(raw["seq"]), n_cig_total=len(raw["cigar"]))
        g = pp.gate_records(ctx, ptrs, mem=pp.MEM_DEVICE, **kw)
        del t
    return {"recs": g.host(), "orig": g.orig(), "counts": g.counts}, g


def _same_as_model(got, want):
    gm.same(got["recs"], want["recs"])
    assert np.array_equal(got["orig"], want["orig"]) and got["counts"] == tuple(want["counts"])


def _assembly(contigs):
    off = np.concatenate([[0], np.cumsum([len(s) for _, s in contigs])]).astype(np.uint64)
    return off, np.frombuffer("".join(s for _, s in contigs).upper().encode(), np.uint8)


_raws = {}


def _case_raws(name):
    """per file of the named case: (raw, passed, expectation) or None for a file that is not parse-clean (built once)"""
    if name not in _raws:
        c, out = im.case(name), []
        for f, text in enumerate(c.texts):
            try:
                raw, zp = gm.raw_from_text(c.contigs, text)
            except gm.NotRaw:
                out.append(None)
                continue
            out.append((raw, gm.passed_for(c, f, zp), gm.expect_from_model(c, f, zp)))
        _raws[name] = out
    return _raws[name]


# ---- 1. the named cases of ingest_model ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ("host", "device"))
@pytest.mark.parametrize("name", sorted(im.CASES))
def test_named_case_is_the_model_byte_for_byte(pp, ctx, name, source):
    c = im.case(name)
    gated, all_ok = [], True
    for item in _case_raws(name):
        if item is None:
            all_ok = False
            continue
        raw, passed, want = item
        kw = dict(max_errors=c.max_errors, careful=c.careful, passed=passed)
        if want[0] == "error" or (want[0] == "contig" and passed is not None and len(passed) != int(((raw["flag"] & 4) == 0).sum())):
            ref = None
            try:
                gm.gate(raw, c.max_errors, c.careful, passed)
            except gm.GateError as e:
                ref = e
            with pytest.raises(pp.PolypolishError) as e:
                _gate(pp, ctx, raw, source, **kw)
            assert e.value.code == ref.code and e.value.bad_record == ref.bad_record, (name, str(e.value), ref)
            if ref.kind == "no_sequence":
                assert str(e.value).endswith(f"no alignments for read record {ref.bad_record} contain sequence")
            all_ok = False
            continue
        got, g = _gate(pp, ctx, raw, source, **kw)
        if want[0] == "ok":
            gm.same(got["recs"], want[1]["recs"])
            assert [got["counts"]] == [tuple(x) for x in want[1]["counts"]]
        _same_as_model(got, gm.gate(raw, c.max_errors, c.careful, passed))
        all_ok = all_ok and want[0] == "ok"
        gated.append(g)
    if all_ok and c.valid_job and source == "host" and sum(g.n_aln for g in gated):
        # the chain: every file's gated batch through pp_batch_prepare, added one after the other -> the direct path, and the
        # bytes the model's records give
        off, bases = _assembly(c.contigs)
        want = ctx.polish_records(off, bases, c.model()["recs"])["polished"]
        preps = [pp.prepare_batch(ctx, off, g.n_aln, g.ptrs(), g.seq_bytes, g.n_cig_total, pp.MEM_DEVICE) for g in gated if g.n_aln]
        ctx.polish_begin(off, bases.ctypes.data, pp.MEM_HOST)
        for p in preps:
            ctx.polish_add_ptrs(p.n_aln, p.ptrs(), p.seq_bytes, p.n_cig_total, pp.MEM_DEVICE)
        ctx.polish_finish()
        assert ctx.took_direct_path()
        assert ctx.result()[0] == want
        for p in preps:
            p.close()
    for g in gated:
        g.close()


# ---- 2. seams, against gate_model -----------------------------------------------------------------------------------------------
def _rng_rows(n, seed):
    rng = np.random.default_rng(seed)
    return rng, [gm._row(rng, 50 + i) for i in range(n)]


def _seam(name):
    """-> (rows, kwargs of the gate)"""
    rng = np.random.default_rng(20)
    if name == "one record":
        return [gm._row(rng, 1, n=101, lower=True)], {}
    if name == "generated":
        rows, passed = gm.seam_rows()
        return rows, {"passed": passed}
    if name == "generated, no verdicts":
        return gm.seam_rows()[0], {}
    if name == "generated, all ones":
        rows, passed = gm.seam_rows()
        return rows, {"passed": np.ones_like(passed)}
    if name == "one group of 3000":
        return gm.big_group_rows(), {}
    if name == "one group of 3000, careful":
        return gm.big_group_rows(), {"careful": True}
    if name == "only unaligned":
        return [gm._row(rng, i, flag=4 | (16 if i % 2 else 0), runs=[]) for i in range(70)], {}
    if name == "empty":
        return [], {}
    if name == "careful, groups of 1 and 2":
        rows = []
        for i in range(300):
            rows.append(gm._row(rng, i))
            if i % 2:
                rows.append(gm._row(rng, i, flag=256, seq=b"", runs=[24 << 4]))
        return rows, {"careful": True}
    if name == "nm at the bound":
        return [gm._row(rng, i, nm=nm) for i, nm in enumerate((9, 10, 11, 0, 0xFFFFFFFF))], {"max_errors": 10}
    if name == "nm and the bound at 2^32-1":
        return [gm._row(rng, i, nm=nm) for i, nm in enumerate((0, 0xFFFFFFFE, 0xFFFFFFFF))], {"max_errors": 0xFFFFFFFF}
    if name == "nine ops first and last":
        rows = []
        for op in range(9):
            rows.append(gm._row(rng, 2 * op, runs=[(4 << 4) | op, 20 << 4]))
            rows.append(gm._row(rng, 2 * op + 1, runs=[20 << 4, (4 << 4) | op]))
            rows.append(gm._row(rng, 100 + op, runs=[(24 << 4) | op]))
        return rows, {}
    if name == "all 128 ascii values on the other strand":
        s = bytes(range(128))
        return [gm._row(rng, 1, seq=s, runs=[128 << 4], flag=16), gm._row(rng, 1, seq=b"", runs=[128 << 4], flag=256),
                gm._row(rng, 1, seq=b"", runs=[128 << 4], flag=256 | 16), gm._row(rng, 2, seq=s + s[:5], runs=[133 << 4])], {}
    raise KeyError(name)


SEAMS = ("one record", "generated", "generated, no verdicts", "generated, all ones", "one group of 3000", "one group of 3000, careful",
         "only unaligned", "empty", "careful, groups of 1 and 2", "nm at the bound", "nm and the bound at 2^32-1",
         "nine ops first and last", "all 128 ascii values on the other strand")


@pytest.mark.parametrize("source", ("host", "device"))
@pytest.mark.parametrize("name", SEAMS)
def test_seam_against_the_model(pp, ctx, name, source):
    rows, kw = _seam(name)
    raw = gm.pack_raw(rows)
    want = gm.gate(raw, kw.get("max_errors", 10), kw.get("careful", False), kw.get("passed"))
    got, g = _gate(pp, ctx, raw, source, **kw)
    _same_as_model(got, want)
    if name == "all 128 ascii values on the other strand":
        from oracle import pyref
        rc = pyref.reverse_complement(gm.upper(bytes(range(128))).decode("latin-1")).encode("latin-1")
        assert got["recs"]["seq"][128:256].tobytes() == rc
    if name in ("only unaligned", "empty"):
        assert got["counts"] == (0, 0, 0) and g.n_aln == 0
    g.close()


def test_verdicts_one_byte_short_is_an_argument_error_behind_a_clean_gate(pp, ctx):
    rows, passed = gm.seam_rows()
    raw = gm.pack_raw(rows)
    with pytest.raises(pp.PolypolishError) as e:
        _gate(pp, ctx, raw, passed=passed[:-1])
    assert e.value.code == pp.ERR_ARG and e.value.bad_record is None
    rows[40] = gm._row(np.random.default_rng(0), 999_999, seq=b"", runs=[24 << 4])     # ... and behind a defect, the defect
    with pytest.raises(pp.PolypolishError) as e:
        _gate(pp, ctx, gm.pack_raw(rows), passed=passed[:-1])
    assert e.value.code == im.QUIT and e.value.bad_record == 40


# ---- 3. defects: ordinary error returns -------------------------------------------------------------------------------------------
def _defect_rows():
    rng, rows = _rng_rows(1200, 30)
    return rng, rows


def test_group_without_sequence_quits_and_is_silent_under_careful(pp, ctx):
    rng, rows = _defect_rows()
    rows[7] = gm._row(rng, 7, flag=4, runs=[])
    rows[8] = gm._row(rng, 8, seq=b"", runs=[24 << 4])
    rows[9] = gm._row(rng, 8, seq=b"", runs=[24 << 4], flag=256)
    raw = gm.pack_raw(rows)
    with pytest.raises(pp.PolypolishError) as e:
        _gate(pp, ctx, raw)
    assert e.value.code == im.QUIT and e.value.bad_record == 8
    assert str(e.value).endswith("no alignments for read record 8 contain sequence")
    got, g = _gate(pp, ctx, raw, careful=True)
    _same_as_model(got, gm.gate(raw, careful=True))
    g.close()


def test_empty_cigar_panics(pp, ctx):
    rng, rows = _defect_rows()
    rows[600] = gm._row(rng, 650, runs=[])
    rows[601] = gm._row(rng, 650, flag=256, runs=[24 << 4])
    rows[602] = gm._row(rng, 650, flag=256, runs=[])
    with pytest.raises(pp.PolypolishError) as e:
        _gate(pp, ctx, gm.pack_raw(rows))
    assert e.value.code == im.PANIC and e.value.bad_record == 600


def test_first_of_two_defects_in_file_order_wins(pp, ctx):
    rng, rows = _defect_rows()
    rows[5] = gm._row(rng, 55, runs=[])                                  # group 5: empty CIGAR (a panic)
    rows[900] = gm._row(rng, 950, seq=b"", runs=[24 << 4])               # group 900: no sequence (a quit)
    raw = gm.pack_raw(rows)
    assert [g[0] for g in gm.groups(raw)][5] == 5 and [g[0] for g in gm.groups(raw)][900] == 900
    with pytest.raises(pp.PolypolishError) as e:
        _gate(pp, ctx, raw)
    assert e.value.code == im.PANIC and e.value.bad_record == 5


@pytest.mark.parametrize("source", ("host", "device"))
def test_ranges_past_their_arrays_are_argument_errors(pp, ctx, source):
    rng, rows = _defect_rows()
    raw = gm.pack_raw(rows)
    for field, size, r in (("seq_off", len(raw["seq"]), 300), ("cig_off", len(raw["cigar"]), 1100)):
        for off in (size - int(raw["seq_len" if field == "seq_off" else "n_cig"][r]) + 1, 1 << 62, 0xFFFFFFFFFFFFFFFF):
            bad = {k: v.copy() for k, v in raw.items()}
            bad[field][r] = off
            with pytest.raises(pp.PolypolishError) as e:
                _gate(pp, ctx, bad, source)
            assert e.value.code == pp.ERR_ARG and e.value.bad_record == r, (field, off, str(e.value))
    got, g = _gate(pp, ctx, raw, source)          # the context is fine afterwards
    _same_as_model(got, gm.gate(raw))
    g.close()


# ---- 4. end to end: SAM text -> raw records -> gate -> (prepare) -> polish, against the oracle on the text --------------------------
@pytest.fixture(scope="module")
def dataset(tmp_path_factory, orc):
    d = tmp_path_factory.mktemp("gate_e2e")
    ds = synth.rich_dataset(str(d), seed=21, contig_lens=(4000, 2500), coverage=30, repeat_len=400, repeat_copies=3, zp_frac=0.02)
    contigs = [(c.name, c.assembly) for c in ds["contigs"]]
    sams = [ds["sam1"], ds["sam2"]]
    texts = [open(p, "rb").read() for p in sams]
    raws = [gm.raw_from_text(contigs, t) for t in texts]
    # the oracle filter's verdicts: the aligned lines of its outputs that came back with ZP:Z:fail appended
    outs = [os.path.join(str(d), f"filtered_{i}.sam") for i in (1, 2)]
    orc.filter_files(sams[0], sams[1], outs[0], outs[1])
    verdicts = []
    for t_in, p_out in zip(texts, outs):
        lin, lout = im._lines(t_in), im._lines(open(p_out, "rb").read())
        verdicts.append(np.array([0 if len(b) > len(a) else 1 for a, b in zip(lin, lout)
                                  if a and a[0] != "@" and not int(a.split("\t")[1]) & 4], np.uint8))
    return {"fasta": ds["fasta"], "sams": sams, "filtered": outs, "contigs": contigs, "raws": raws, "verdicts": verdicts}


@pytest.mark.parametrize("careful", (False, True))
@pytest.mark.parametrize("filtered", (False, True))
def test_chain_equals_the_oracle_on_the_text(pp, ctx, orc, dataset, filtered, careful):
    want = orc.polish_files(dataset["fasta"], dataset["filtered" if filtered else "sams"], careful=careful, positions=True)
    off, bases = _assembly(dataset["contigs"])
    passed = []
    for (raw, zp), v in zip(dataset["raws"], dataset["verdicts"]):
        assert len(v) == len(zp)
        passed.append(zp & v if filtered else zp)
    assert not filtered or any((v == 0).any() for v in dataset["verdicts"])
    for prepare in (False, True):
        got = ctx.polish_raw(off, bases, [r for r, _ in dataset["raws"]], careful=careful, passed=passed, prepare=prepare, positions=True)
        assert got["polished"] == im.seqs(want["fasta"])
        for k in POS_KEYS:
            assert np.array_equal(got["positions"][k], want["positions"][k]), (k, prepare)
        assert tuple(map(sum, zip(*got["counts"]))) == tuple(want["counts"])
        assert ctx.took_direct_path() == prepare


# ---- 5. large then small on one context --------------------------------------------------------------------------------------------
def test_two_gates_of_different_sizes_on_one_context(pp, ctx, orc):
    for seed, n in ((41, 9000), (42, 300)):
        g = im.Gen(seed, (6000,))
        T = im.Text()
        for i in range(n):
            T.add(g.line(name=f"r{i // 2}", n=40, flag=0 if i % 2 == 0 else 256, seq=None if i % 2 == 0 else "*", cigar="40M",
                         nm=11 if i % 7 == 0 else 0))
        text = T.bytes()
        raw, zp = gm.raw_from_text(g.contigs, text)
        want = im.model(g.contigs, [text])
        got, gb = _gate(pp, ctx, raw)
        gm.same(got["recs"], want["recs"])
        gb.close()
        off, bases = _assembly(g.contigs)
        res = ctx.polish_raw(off, bases, [raw], prepare=True)
        assert res["polished"] == orc.polish_records(off, bases, want["recs"])["polished"]
        assert res["counts"] == [tuple(want["counts"][0])]
