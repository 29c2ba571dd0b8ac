"""pp_polish_bed and pp_polish_masked (pp_k_bed.h) on a finished job through the C ABI, byte for byte against tests/bed_model.py.  The
model is fed from the ORACLE on the same records (oracle.polish_records: per-position status and emitted lengths, polished bytes), never
from the device; the device's polished bytes are the oracle's (asserted: the precondition).  The jobs are hand-built (tests/bed_jobs.py):
every status in runs, three of them across a workgroup boundary per job, insertions and deletions in front so that output offsets
differ from positions.  On the direct path and on the plain one, as tests/test_vcf_gpu.py chooses them.  Needs an MI355X: `-m gpu`."""
import ctypes as C

import numpy as np
import pytest

import bed_jobs as bj
import bed_model as bm

pytestmark = pytest.mark.gpu

T = 2048  # BED_TILE (polypolish_amd/csrc/pp_k_bed.h), checked against the library's own report below
MASKS = (bm.UNDECIDED, bm.ALL, (1 << bm.CHANGED) | (1 << bm.MULTIPLE))


@pytest.fixture(scope="module")
def pp():
    import polypolish_amd
    return polypolish_amd


@pytest.fixture(scope="module")
def ctx(pp):
    c = pp.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def jobs(pp, orc):
    assert pp.bed_geometry()[1] == T
    out = []
    for which in (0, 1):
        job = bj.job(T, which)
        res = orc.polish_records(job["off"], job["bases"], job["recs"], min_depth=1, positions=True)
        bj.check_oracle_made(job, res)
        at = np.concatenate([[0], np.cumsum(res["positions"]["emit_len"].astype(np.int64))])
        assert all(int(at[b]) != b for b in (T, 2 * T, 3 * T)), "output offsets differ from positions at every workgroup boundary"
        assert int(res["positions"]["emit_len"].max()) == 2 and int(res["positions"]["emit_len"].min()) == 0
        out.append((job, res))
    return out


def _first_diff(got, want):
    i = next((k for k, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    return len(got), len(want), i, got[max(0, i - 40):i + 40], want[max(0, i - 40):i + 40]


def _polish(pp, ctx, job, res, path="plain", debug=True, **kw):
    off, bases, recs = job["off"], job["bases"], job["recs"]
    if path == "plain":
        got = ctx.polish_records(off, bases, recs, min_depth=1, debug=debug, **kw)["polished"]
        assert not ctx.took_direct_path()
    else:
        prep = pp.prepare_records(ctx, off, recs)
        try:
            pp.lib().pp_polish_set_debug(ctx._h, int(debug))
            ctx.polish_begin(off, bases.ctypes.data, pp.MEM_HOST, min_depth=1)
            ctx.polish_add_ptrs(prep.n_aln, prep.ptrs(), prep.seq_bytes, prep.n_cig_total, pp.MEM_DEVICE)
            ctx.polish_finish()
            assert ctx.took_direct_path()
            got = ctx.result()[0]
        finally:
            pp.lib().pp_polish_set_debug(ctx._h, 0)
            prep.close()
    assert got == res["polished"], "the device's job is the oracle's"


def _check(pp, ctx, job, res):
    """the context's finished job against the model on the oracle's statuses and bytes, under three masks; the job's own bytes and its
    VCF are what they were"""
    pos, names = res["positions"], job["names"]
    v = pp.Vcf(ctx, names)
    vcf = v.bytes()
    v.close()
    for mask in MASKS:
        want = bm.bed(pos["status"], job["off"], names, mask)
        b = pp.StatusBed(ctx, names, mask)
        try:
            got = b.bytes()
            assert got == want, (mask, _first_diff(got, want))
            assert b.n_records == want.count(b"\n") and b.counts == bm.counts(pos["status"], job["off"], mask)
        finally:
            b.close()
        want = bm.masked(res["polished"], pos["emit_len"], pos["status"], mask)
        m = pp.Masked(ctx, mask)
        try:
            got = m.bytes()
            assert got == want, (mask, _first_diff(got, want))
            assert m.n_bytes == ctx.result_size() == len(res["polished"])
        finally:
            m.close()
        assert ctx.result()[0] == res["polished"], "the job's own bytes stay as they are"
    v = pp.Vcf(ctx, names)
    assert v.bytes() == vcf, "the VCF is unchanged by the mask"
    v.close()


@pytest.mark.parametrize("path", ["plain", "direct"])
@pytest.mark.parametrize("which", [0, 1])
def test_the_bed_and_the_masked_bytes_are_the_models(pp, ctx, jobs, which, path):
    job, res = jobs[which]
    _polish(pp, ctx, job, res, path)
    _check(pp, ctx, job, res)
    if which == 0 and path == "plain":
        recs = bm.parse(bm.bed(res["positions"]["status"], job["off"], job["names"], bm.ALL))
        assert (b"contig_1", T - 19, T - 10, b"changed") in recs and (b"contig_1", T - 10, T + 10, b"multiple") in recs, "two statuses side by side"
        assert (b"one", 0, 1, b"low_depth") in recs and recs[-1][2] == 2 * T - 5 and recs[-1][3] == b"low_depth", "a run to a contig's last position"
        assert (b"the third contig", 2 * T - 8 - (T + 38), 2 * T + 15 - (T + 38), b"none") in recs


def test_a_second_job_on_the_same_context(pp, jobs):
    c = pp.Context(0)
    try:
        for which in (0, 1, 0):
            job, res = jobs[which]
            _polish(pp, c, job, res)
            _check(pp, c, job, res)
    finally:
        c.close()


def test_times(pp, ctx, jobs):
    job, res = jobs[0]
    _polish(pp, ctx, job, res)
    m = pp.Masked(ctx)
    with pytest.raises(pp.PolypolishError) as e:
        m.kernel_ms()
    assert e.value.code == pp.ERR_ARG and "pp_ctx_set_profiling" in e.value.msg
    m.close()
    ctx.set_profiling(True)
    try:
        m = pp.Masked(ctx)
        assert m.kernel_ms() >= 0 and m.bytes() == bm.masked(res["polished"], res["positions"]["emit_len"], res["positions"]["status"])
        m.close()
        b = pp.StatusBed(ctx, job["names"])
        assert abs(b.kernel_ms() - sum(b.stage_ms().values())) < 1e-3
        b.close()
    finally:
        ctx.set_profiling(False)


def _refused(pp, fn, *words):
    with pytest.raises(pp.PolypolishError) as e:
        fn()
    assert e.value.code == pp.ERR_ARG and all(w in e.value.msg for w in words), e.value.msg


def test_refusals(pp, jobs):
    job, res = jobs[0]
    names = job["names"]
    c = pp.Context(0)
    try:
        L = pp.lib()
        for make, who in ((lambda: pp.StatusBed(c, names), "pp_polish_bed"), (lambda: pp.Masked(c), "pp_polish_masked")):
            _refused(pp, make, who, "no finished polish job")
        c.polish_begin(job["off"], job["bases"].ctypes.data, pp.MEM_HOST, min_depth=1)  # an open job is no finished one
        _refused(pp, lambda: pp.StatusBed(c, names), "no finished polish job")
        _refused(pp, lambda: pp.Masked(c), "no finished polish job")
        _polish(pp, c, job, res, debug=False)  # a job without per-position records
        _refused(pp, lambda: pp.StatusBed(c, names), "pp_polish_bed", "pp_polish_set_debug(ctx, 1)")
        _refused(pp, lambda: pp.Masked(c), "pp_polish_masked", "pp_polish_set_debug(ctx, 1)")
        lens = np.diff(job["off"]).astype(np.int64)
        c.polish_records(job["off"], job["bases"], job["recs"], min_depth=1, debug=True, emit=[(0, int(lens[0])), (0, 1), (0, int(lens[2]) // 2)])
        _refused(pp, lambda: pp.StatusBed(c, names), "pp_polish_set_emit", "edges")
        _refused(pp, lambda: pp.Masked(c), "pp_polish_set_emit", "edges")
        _polish(pp, c, job, res)
        for mask in (0, 64, 1 << 31):
            _refused(pp, lambda: pp.StatusBed(c, names, mask), "pp_polish_bed", "mask")
            _refused(pp, lambda: pp.Masked(c, mask), "pp_polish_masked", "mask")
        _refused(pp, lambda: pp.StatusBed(c, [b"a\tb", b"c", b"d"]), "tab or a newline")
        _refused(pp, lambda: pp.StatusBed(c, [b"a", b"c", b"d\n"]), "tab or a newline")
        p = C.c_void_p()
        arr = (C.c_char_p * 3)(b"a", None, b"c")
        assert L.pp_polish_bed(c._h, C.cast(arr, C.c_void_p), bm.ALL, C.byref(p)) == pp.ERR_ARG and not p.value and b"name is NULL" in L.pp_last_error(c._h)
        assert L.pp_polish_bed(c._h, None, bm.ALL, C.byref(p)) == pp.ERR_ARG and b"null argument" in L.pp_last_error(c._h)
        arr = (C.c_char_p * 3)(b"a", b"b", b"c")
        assert L.pp_polish_bed(c._h, C.cast(arr, C.c_void_p), bm.ALL, None) == pp.ERR_ARG and b"null argument" in L.pp_last_error(c._h)
        assert L.pp_polish_masked(c._h, bm.ALL, None) == pp.ERR_ARG and b"null argument" in L.pp_last_error(c._h)
        assert L.pp_polish_bed(None, C.cast(arr, C.c_void_p), bm.ALL, C.byref(p)) == pp.ERR_ARG and L.pp_polish_masked(None, bm.ALL, C.byref(p)) == pp.ERR_ARG
        _check(pp, c, job, res)  # ... and the context still makes both
    finally:
        c.close()
