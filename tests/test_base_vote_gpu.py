"""k_tile's own vote over A, C, G, T and "-" where the file order of the depth sum decides it, against the oracle.

A position under reads with shares like 1/3 has a depth that the kernel only bounds (pp_k_tile.h, pass 2 of tile_body): it
votes from the interval's two ends where the vote's three step functions agree, votes twice where exactly one of them moves
by a step (bytes-only jobs) and hands the rest to the ordered replay (pp_k_exact.h).  Exact depths take their thresholds from
the job's table (integers below 4096) or compute them.  The jobs come from base_sites.py (test_base_sites_cpu.py checks what
they hold): tallies on, one below and above a threshold that two file orders of the same reads put in two places; ties that
one read of a tiny or odd share tips; windows of exactly 2047, 2048 and 36,000 work items, where the unit of the fixed-point
tally changes; stacks around the table's end.  The expected result is always the oracle's on the same records in the same
file order, compared for equality.  Needs an MI355X."""
import numpy as np
import pytest

import base_sites as bs
import key_sites as ks
from test_gpu_parity import POS_KEYS, _compare_records, _polish_device_batch
from test_key_vote_gpu import _check_bytes, _flagged

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


def _same_positions(got, want, where, exact_depth):
    """Tallies, both thresholds and the status equal at every position; the depth bit for bit, or (debug level 3: what the
    pileup kernel decides by itself) within the bound test_gpu_parity._compare_records uses, reads * 2^-11 + 1e-9."""
    p = want["positions"]
    for k in POS_KEYS:
        if k == "depth" and not exact_depth:
            continue
        bad = np.nonzero(p[k] != got["positions"][k])[0]
        assert len(bad) == 0, (where, k, len(bad), bad[:8], p[k][bad[:8]], got["positions"][k][bad[:8]])
    if not exact_depth:
        reads = (p["count_a"].astype(np.int64) + p["count_c"] + p["count_g"] + p["count_t"] + p["count_other"]).astype(np.float64)
        err = np.abs(got["positions"]["depth"] - p["depth"])
        assert (err <= reads * 2.0 ** -11 + 1e-9).all(), (where, "interval depth", float(err.max()))
    assert got["polished"] == want["polished"], where


def _routes(ctx, pp, want, params, where, levels=(False, 3, True)):
    """One job as host records and as one device batch on the direct path, bytes-only, at debug level 3 and with the full
    per-position records.  Returns the level-3 records of the direct path."""
    off, bases, recs = want["job"]
    level3 = None
    for positions in levels:
        host = ctx.polish_records(off, bases, recs, positions=positions, **bs.kw(params))
        direct = _polish_device_batch(ctx, pp, off, bases, recs, True, positions=positions, wo=True, **bs.kw(params))
        assert ctx.took_direct_path(), (where, positions)
        for route, got in (("host records", host), ("direct path", direct)):
            at = f"{where}, {route}, positions={positions}"
            if positions:
                _same_positions(got, want, at, exact_depth=positions is True)
            else:
                _check_bytes(got, want, at)
        if positions == 3:
            level3 = host, direct
    return level3


# ---- A and B: small jobs at the finest unit, every route ---------------------------------------------------------------------

@pytest.mark.parametrize("which", [0, 1], ids=["order0", "order1"])
@pytest.mark.parametrize("family", ["A", "B"])
@pytest.mark.parametrize("params", bs.OPTION_SETS, ids=bs.IDS)
def test_sites_that_the_file_order_decides_on_every_route(ctx, orc, params, family, which):
    """A: tallies of the assembly's own base, a substituted base or "-" on the lower value of a threshold that the two file
    orders put in two places, one below it and above the higher one.  B: ties of m reads of k = 1 tipped by one or two reads
    of k = 2, 2^19, 2^20, 2^21, 3, 236, 237, 1000, 2^31; shares 1/2, 1/4, 1/8 only.  Host records, device batches with and
    without the 4-bit mirror, the window-order mirror with its run table, shuffled and without runs; bytes-only, level 3 and
    full per-position records; changed and zero_depth per contig (all in _compare_records).  Then, from the oracle's own two
    results: the two orders of an A job differ at the sites test_base_sites_cpu.py counts -- what is compared here IS decided
    by the file order."""
    job = (bs.family_a_job if family == "A" else bs.family_b_job)(orc, params)
    off, bases, recs = job.ordered(which)
    want, _ = _compare_records(ctx, orc, off, bases, recs, **bs.kw(params))
    mine = bs.expected(orc, job, which)
    assert want["polished"] == mine["polished"] and np.array_equal(want["positions"]["status"], mine["positions"]["status"])
    if family == "A":
        other = bs.expected(orc, job, 1 - which)
        sites = np.array([g for g, _ in job.contested()])
        differ = sites[want["positions"]["status"][sites] != other["positions"]["status"][sites]]
        st, by = bs.order_differences(orc, job)
        assert differ.tolist() == st and len(st) >= 8, (len(differ), len(st))
        assert len(by) >= (3 if params in bs.BYTE_SETS else 1) and want["polished"] != other["polished"], len(by)


# ---- C: the window's unit -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", [0, 1], ids=["order0", "order1"])
@pytest.mark.parametrize("params", bs.OPTION_SETS, ids=bs.IDS)
def test_windows_of_2047_2048_and_36000_items(ctx, pp, orc, params, which):
    """The sites of A and B in windows whose fixed-point unit is 2^-20 (2047 items), 2^-19 (2048: a read of k = 2^20 is off by
    exactly half a unit there, the edge of the interval's bound) and 2^-15 (36,000: a heavy window, whose helper blocks each
    add a part of every position's deficit; sites of 5,500 reads whose interval holds two steps at once).  Host records and
    the direct path; bytes-only (where the two-vote shortcut runs), level 3 and full records."""
    job = bs.family_c_job(orc, params)
    want = bs.expected(orc, job, which)
    host3, direct3 = _routes(ctx, pp, want, params, f"{params}, order {which}")
    # where the seam is: under a lone read of k = 3 the kernel's own depth is the share in the window's unit
    for window, b in ((bs.W_2047, 20), (bs.W_2048, 19)):
        (g,) = [g for g, s in job.sites if g // ks.WIN == window and s["family"] == "lone"]
        share = round(2.0 ** b / 3.0) / 2.0 ** b
        for got in (host3, direct3):
            assert got["positions"]["depth"][g] == share, (
                f"this only locates the seam of the unit: the window of {2047 + window - bs.W_2047} items should tally in 2^-{b}, "
                f"a third is then {share!r}, the kernel has {got['positions']['depth'][g]!r}")


# ---- D: the table's end -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ntot", bs.D_DEPTHS)
def test_depths_around_the_end_of_the_threshold_table(ctx, pp, orc, ntot):
    """4095 reads of k = 1 read their thresholds from the job's table, 4096 and 4097 compute them: a substituted base on and
    one below either threshold."""
    job = bs.family_d_job(orc, ntot)
    want = bs.expected(orc, job, 0)
    assert (want["positions"]["depth"][[g for g, _ in job.sites]] == float(ntot)).all()
    _routes(ctx, pp, want, job.params, f"depth {ntot}", levels=(False, True))


# ---- the shortcut, and job after job ---------------------------------------------------------------------------------------------

def test_one_moved_step_with_both_votes_equal_is_decided_in_the_pileup_kernel(ctx, orc):
    """A job of family-A sites at which one step function moves inside the interval and the vote comes out the same either
    way: the bytes-only job replays fewer positions than have a step inside their interval."""
    params = ks.DEFAULT
    job = bs.shortcut_job(orc, params)
    open_positions = sum(1 for c in bs.classify(job).values() if c != 0)
    assert open_positions == len(job.sites) >= 20
    for which in (0, 1):
        want = bs.expected(orc, job, which)
        got, flagged = _flagged(ctx, want["job"], params)
        _check_bytes(got, want, f"order {which}")
        assert flagged < open_positions, (f"{flagged} positions were replayed, {open_positions} sites have one step inside their interval: "
                                          "the two-vote shortcut is off (a cost, not a wrong result -- the bytes were right)")


@pytest.mark.parametrize("params", bs.OPTION_SETS, ids=bs.IDS)
def test_two_file_orders_of_one_job_one_after_the_other(pp, orc, params):
    """The same reads in two file orders on one context, bytes-only, each against its own oracle result: the second job
    inherits neither the first one's flagged positions nor its table of thresholds (another option set in between)."""
    job = bs.family_a_job(orc, params)
    between = bs.family_a_job(orc, bs.OPTION_SETS[(bs.OPTION_SETS.index(params) + 1) % len(bs.OPTION_SETS)])
    w0, w1 = bs.expected(orc, job, 0), bs.expected(orc, job, 1)
    assert w0["polished"] != w1["polished"]
    c = pp.Context(0)
    try:
        for step, (j, want) in enumerate(((job, w0), (job, w1), (between, bs.expected(orc, between, 0)), (job, w1), (job, w0))):
            off, bases, recs = want["job"]
            _check_bytes(c.polish_records(off, bases, recs, **bs.kw(j.params)), want, f"job {step}")
    finally:
        c.close()
