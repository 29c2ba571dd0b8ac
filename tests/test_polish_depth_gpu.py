"""pp_polish_depth (pp_k_depth.h) on a finished job through the C ABI, byte for byte against tests/depth_model.py.  The model is fed from
the ORACLE's per-position depths on the same records (oracle.polish_records), never from the device alone; the device's polished bytes
and its own per-position depths are the oracle's (asserted: the precondition).  The jobs are the hand-built ones of tests/bed_jobs.py
(uncovered stretches across a workgroup boundary among them) and tests/long_sites.py, and one whose reads carry shares of 1, 1/3 and
1/4, so that depths are fractional and exact ties of the rounding occur.  On the direct path and on the plain one, in the runs form and
under two bins.  Needs an MI355X: `-m gpu`."""
import ctypes as C

import numpy as np
import pytest

import bed_jobs as bj
import bed_model as bm
import depth_model as dm
import long_sites as ls

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pp():
    import polypolish_amd
    return polypolish_amd


@pytest.fixture(scope="module")
def ctx(pp):
    c = pp.Context(0)
    yield c
    c.close()


def _shares_job(T):
    """bed_jobs' second job with the reads' shares set to 1, 1/3 and 1/4 in turn (k = 1, 3, 4 alignments per read)"""
    job = dict(bj.job(T, 1))
    recs = {k: np.array(v, copy=True) for k, v in job["recs"].items()}
    recs["k"] = np.array([(1, 3, 4)[i % 3] for i in range(len(recs["k"]))], recs["k"].dtype)
    job["recs"] = recs
    return job


@pytest.fixture(scope="module")
def jobs(pp, orc):
    T = pp.depth_geometry()[1]
    ppt, tile, _, _ = pp.vcf_geometry()
    out = {}
    for which in (0, 1):
        out["bed%d" % which] = dict(bj.job(T, which), kw=ls.MIN1)
    out["shares"] = dict(_shares_job(T), kw=ls.MIN1)
    out.update({"l1_small": ls.l1_job("small"), "dashed": ls.dashed_job(), "l2": ls.l2_job(tile, ppt)})
    made = {}
    for name, job in out.items():
        res = orc.polish_records(job["off"], job["bases"], job["recs"], positions=True, **job["kw"])
        depth = res["positions"]["depth"]
        want = {W: dm.bedgraph(depth, job["off"], job["names"], W) for W in (0, 100, T + 1)}
        made[name] = (job, res, want, dm.summary(depth))
    # what the jobs are chosen for
    d = made["bed1"][1]["positions"]["depth"]
    assert d[T - 1] == 0.0 and d[T] == 0.0 and d[T - 40] > 0 and d[T + 20] > 0, "an uncovered stretch across a workgroup boundary"
    d = made["shares"][1]["positions"]["depth"]
    frac = d * 10 - np.floor(d * 10)
    assert (frac == 0.5).sum() >= 50 and ((d % 1) != 0).sum() >= 1000, "fractional depths, exact ties of the rounding among them (2.25, 3.75)"
    assert len({len(j["off"]) for j, _, _, _ in made.values()}) >= 2, "jobs with different contig counts"
    return made, T


def _first_diff(got, want):
    i = next((k for k, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    return len(got), len(want), i, got[max(0, i - 40):i + 40], want[max(0, i - 40):i + 40]


def _polish(pp, ctx, job, res, path="plain", debug=True, **kw):
    off, bases, recs = job["off"], job["bases"], job["recs"]
    if path == "plain":
        got = ctx.polish_records(off, bases, recs, debug=debug, **job["kw"], **kw)["polished"]
        assert not ctx.took_direct_path()
    else:
        prep = pp.prepare_records(ctx, off, recs)
        try:
            pp.lib().pp_polish_set_debug(ctx._h, int(debug))
            ctx.polish_begin(off, bases.ctypes.data, pp.MEM_HOST, **job["kw"])
            ctx.polish_add_ptrs(prep.n_aln, prep.ptrs(), prep.seq_bytes, prep.n_cig_total, pp.MEM_DEVICE)
            ctx.polish_finish()
            assert ctx.took_direct_path()
            got = ctx.result()[0]
        finally:
            pp.lib().pp_polish_set_debug(ctx._h, 0)
            prep.close()
    assert got == res["polished"], "the device's job is the oracle's"


def _check(pp, ctx, made, T):
    """the context's finished job against the model on the oracle's depths, in the runs form and under two bins; the job's own bytes, its
    VCF and its BED are what they were"""
    job, res, want, summ = made
    names = job["names"]
    pp.lib().pp_polish_set_debug(ctx._h, 1)  # (pp_polish_positions asks for the setting as well as for the job's records)
    try:
        own = ctx.positions()["depth"]
    finally:
        pp.lib().pp_polish_set_debug(ctx._h, 0)
    assert np.array_equal(own.view(np.uint64), res["positions"]["depth"].view(np.uint64)), "the device's own depths are the oracle's, bit for bit"
    v, b = pp.Vcf(ctx, names), pp.StatusBed(ctx, names, bm.ALL)
    vcf, bed = v.bytes(), b.bytes()
    v.close()
    b.close()
    for W in (0, 100, T + 1):
        d = ctx.polish_depth(names, W)
        try:
            got = d.bytes()
            assert got == want[W], (W, _first_diff(got, want[W]))
            assert d.n_records == want[W].count(b"\n") and d.n_bytes == len(want[W]) and d.summary() == summ
        finally:
            d.close()
        assert ctx.result()[0] == res["polished"], "the job's own bytes stay as they are"
    v, b = pp.Vcf(ctx, names), pp.StatusBed(ctx, names, bm.ALL)
    assert v.bytes() == vcf and b.bytes() == bed, "the VCF and the BED are unchanged by the call"
    v.close()
    b.close()


@pytest.mark.parametrize("path", ["plain", "direct"])
@pytest.mark.parametrize("name", ["bed0", "bed1", "shares", "l1_small", "dashed", "l2"])
def test_the_depth_track_is_the_models(pp, ctx, jobs, name, path):
    made, T = jobs
    job, res = made[name][:2]
    _polish(pp, ctx, job, res, path)
    _check(pp, ctx, made[name], T)


def test_job_after_job_on_one_context(pp, jobs):
    made, T = jobs
    c = pp.Context(0)
    try:
        for name in ("bed0", "l1_small", "shares", "bed0"):  # (three contigs, then key_sites' own count, and back)
            _polish(pp, c, made[name][0], made[name][1])
            _check(pp, c, made[name], T)
    finally:
        c.close()


def _refused(pp, fn, *words):
    with pytest.raises(pp.PolypolishError) as e:
        fn()
    assert e.value.code == pp.ERR_ARG and all(w in e.value.msg for w in words), e.value.msg


def test_refusals(pp, jobs):
    made, T = jobs
    job, res = made["bed0"][:2]
    names = job["names"]
    c = pp.Context(0)
    try:
        L = pp.lib()
        _refused(pp, lambda: c.polish_depth(names), "pp_polish_depth", "no finished polish job")  # a context with no job
        c.polish_begin(job["off"], job["bases"].ctypes.data, pp.MEM_HOST, min_depth=1)  # an open job is no finished one
        _refused(pp, lambda: c.polish_depth(names), "no finished polish job")
        bad = {k: np.array(v, copy=True) for k, v in job["recs"].items()}
        bad["ref_start"][3] = int(job["off"][1]) - 10  # runs off its contig
        with pytest.raises(pp.PolypolishError):
            c.polish_records(job["off"], job["bases"], bad, min_depth=1, debug=True)
        _refused(pp, lambda: c.polish_depth(names), "no finished polish job", "ended in an error")
        _polish(pp, c, job, res, debug=False)  # a job without per-position records
        _refused(pp, lambda: c.polish_depth(names), "pp_polish_depth", "pp_polish_set_debug(ctx, 1)")
        lens = np.diff(job["off"]).astype(np.int64)
        c.polish_records(job["off"], job["bases"], job["recs"], min_depth=1, debug=True, emit=[(0, int(lens[0])), (0, 1), (0, int(lens[2]) // 2)])
        _refused(pp, lambda: c.polish_depth(names), "pp_polish_set_emit", "edges")
        _polish(pp, c, job, res)
        _refused(pp, lambda: c.polish_depth(names, (1 << 24) + 1), "pp_polish_depth", "2^24")
        _refused(pp, lambda: c.polish_depth([b"a\tb", b"c", b"d"]), "tab or a newline")
        _refused(pp, lambda: c.polish_depth([b"a", b"c", b"d\n"], 7), "tab or a newline")
        p = C.c_void_p()
        arr = (C.c_char_p * 3)(b"a", None, b"c")
        assert L.pp_polish_depth(c._h, C.cast(arr, C.c_void_p), 0, C.byref(p)) == pp.ERR_ARG and not p.value and b"name is NULL" in L.pp_last_error(c._h)
        assert L.pp_polish_depth(c._h, None, 0, C.byref(p)) == pp.ERR_ARG and b"null argument" in L.pp_last_error(c._h)
        arr = (C.c_char_p * 3)(b"a", b"b", b"c")
        assert L.pp_polish_depth(c._h, C.cast(arr, C.c_void_p), 0, None) == pp.ERR_ARG and b"null argument" in L.pp_last_error(c._h)
        assert L.pp_polish_depth(None, C.cast(arr, C.c_void_p), 0, C.byref(p)) == pp.ERR_ARG
        _check(pp, c, made["bed0"], T)  # ... and the context still makes the track
        c.set_profiling(True)
        try:
            d = c.polish_depth(names, 100)
            assert abs(d.kernel_ms() - sum(d.stage_ms().values())) < 1e-3 and d.bytes() == made["bed0"][2][100]
            d.close()
        finally:
            c.set_profiling(False)
    finally:
        c.close()
