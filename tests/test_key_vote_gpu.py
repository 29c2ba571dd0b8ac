"""The string-keyed vote and the emission of its winners, against the oracle, where they can go wrong unnoticed.

Where the assembly lacks a base every read over the spot votes for a string key; a key that wins leaves more than one byte,
"-" none, and every byte behind depends on the emission's prefix sums.  Three pieces of code do this: the table vote inside
k_tile (vote_with_keys / pt_insert: only without per-position records), the grouping of distinct keys in k_exact (whatever
k_tile lists, and everything with per-position records), and k_emit (code_len, the all_one store, finalize_entries, the sums
at three levels).  The jobs come from key_sites.py (test_key_sites_cpu.py checks what they hold); the expected result is
the oracle's, compared for equality: bytes, offsets, changed / zero_depth per contig, every per-position record.
Needs an MI355X."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import key_sites as ks
from test_gpu_parity import _compare_records, _polish_device_batch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [f"{p[0]}-{p[1]}-{p[2]}" for p in ks.OPTION_SETS]


@pytest.fixture(scope="module")
def pp():
    import polypolish_amd
    return polypolish_amd


@pytest.fixture(scope="module")
def ctx(pp):
    c = pp.Context(0)
    yield c
    c.close()


def _kw(params):
    return dict(min_depth=params[0], fraction_valid=params[1], fraction_invalid=params[2])


def _expected(orc, job, params=ks.DEFAULT):
    """The oracle's bytes, offsets and per-contig changed / zero_depth of a job (and its records, made once)."""
    off, bases, recs = job.records()
    w = orc.polish_records(off, bases, recs, positions=True, **_kw(params))
    o = [int(x) for x in off]
    st, depth = w["positions"]["status"], w["positions"]["depth"]
    return {"job": (off, bases, recs), "polished": w["polished"], "offsets": w["offsets"],
            "changed": [int((st[o[c]:o[c + 1]] == 1).sum()) for c in range(len(o) - 1)],
            "zero_depth": [int((depth[o[c]:o[c + 1]] == 0.0).sum()) for c in range(len(o) - 1)],
            "positions": w["positions"]}


def _check_bytes(got, want, where):
    assert np.array_equal(np.asarray(got["offsets"], np.uint64), want["offsets"]), (where, got["offsets"], want["offsets"])
    if got["polished"] != want["polished"]:
        a, b = np.frombuffer(got["polished"], np.uint8), np.frombuffer(want["polished"], np.uint8)
        n = min(len(a), len(b))
        first = int(np.argmax(a[:n] != b[:n])) if (a[:n] != b[:n]).any() else n
        raise AssertionError(f"{where}: polished bytes differ from byte {first} on ({len(a)} vs {len(b)} bytes)")
    for c in range(len(want["changed"])):
        assert got["stats"][c]["changed"] == want["changed"][c], (where, c, got["stats"][c], want["changed"][c])
        assert got["stats"][c]["zero_depth"] == want["zero_depth"][c], (where, c, got["stats"][c], want["zero_depth"][c])


def _flagged(ctx, job, params=ks.DEFAULT):
    """Positions the plain bytes-only job handed to the replay kernels."""
    off, bases, recs = job
    ctx.set_profiling(1)
    try:
        got = ctx.polish_records(off, bases, recs, **_kw(params))
        return got, ctx.kernel_times()["n_flagged"]
    finally:
        ctx.set_profiling(0)


# ---- A. thresholds and competition -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("variant", ks.KEY2_VARIANTS + ("shares",))
@pytest.mark.parametrize("params", ks.OPTION_SETS, ids=IDS)
def test_key_counts_on_and_around_both_thresholds(ctx, orc, params, variant, sparse):
    """Sites whose keys have counts on, one below and far from both thresholds, competing with a second key (two bytes; the
    same key from a slow-class read; three bytes; N), with "-" and with the assembly's own base; at window positions 0, 1,
    2046, 2047 and a contig's last coverable position; with depth shares of 1, 1/2 and 1/3 ("shares").  dense: more keys per
    window than k_tile's table holds -- k_exact groups and votes them all.  sparse: every window's keys fit the table --
    k_tile votes them itself wherever the table accounts for the position's whole string-keyed row, in the runs without
    per-position records and at debug level 3."""
    for seed in ks.SEEDS[sparse]:
        job = ks.shares_job(orc, params, seed, sparse) if variant == "shares" else ks.threshold_job(orc, params, variant, seed, sparse)
        off, bases, recs = job.records()
        want, _ = _compare_records(ctx, orc, off, bases, recs, **_kw(params))
        sites = [g for g, _ in job.sites]
        assert len(set(want["positions"]["status"][sites].tolist())) >= 3, "the sites of one job end in at least three ways"
        if variant in ("two_byte", "slow_read"):
            # which of the two voted: with depth shares 1 and a table that holds the window's keys nothing is listed
            # (a slow-class read's key is in the table too) -- else every position a key could decide is
            p = want["positions"]
            could = sum(1 for g, plan in job.sites if p["status"][g] != 2
                        and 0 < sum(c for k, c in plan["keys"].items() if k != "-") >= p["invalid_thr"][g])
            _, flagged = _flagged(ctx, (off, bases, recs), params)
            assert flagged == 0 if sparse else flagged >= 0.5 * could, (seed, flagged, could, job.pairs)


# ---- B. the table's capacity ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_pairs", [9, 10, 11])
def test_nine_ten_and_eleven_keys_in_a_window(ctx, orc, n_pairs):
    """The table has 10 slots: 9 and 10 distinct (position, key) pairs are voted in k_tile, with 11 the table overflows and
    every string-keyed position of the window goes to k_exact.  The same bytes and records either way, and the plain job
    lists nothing, or every position a key could decide."""
    job = ks.capacity_job(n_pairs)
    off, bases, recs = job.records()
    want, _ = _compare_records(ctx, orc, off, bases, recs)
    p = want["positions"]
    assert (p["status"] == 1).sum() >= 1
    could = int(((p["count_other"] > 0) & (p["count_other"] >= p["invalid_thr"])).sum())
    got, flagged = _flagged(ctx, (off, bases, recs))
    assert got["polished"] == want["polished"]
    assert could == len(job.sites) and (flagged == 0 if n_pairs <= ks.PT_SLOTS else flagged >= could), (n_pairs, flagged, could)


def test_twelve_keys_at_one_position(ctx, orc):
    job = ks.one_position_job()
    off, bases, recs = job.records()
    want, _ = _compare_records(ctx, orc, off, bases, recs)
    assert want["positions"]["status"][job.sites[0][0]] == 3
    got, flagged = _flagged(ctx, (off, bases, recs))
    assert got["polished"] == want["polished"] and flagged >= 1, flagged


# ---- C. multi-byte winners and deletions at the emission's seams -----------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _seam(orc, name):
    return _expected(orc, {"small": ks.seam_job_small, "coarse": ks.seam_job_coarse, "big": ks.seam_job_big}[name]())


@pytest.mark.parametrize("name", ["small", "coarse"])
def test_winners_of_every_length_at_the_seams_of_the_emission(ctx, orc, name):
    """small: three windows -- winners of 2, 3, 126 and 127 bytes, "-", a key that ends in "-"; at window positions 15 / 16,
    1023 / 1024 and 2047; sixteen deleted positions that are one thread's; a contig that starts behind two winners and a
    deletion of its window; a contig that is deleted but for eight bases.  coarse: 66 windows -- contig starts inside
    windows 63 and 64, sites in windows 0 and 62..65, every kind of winner at every seam position in windows 1..43."""
    off, bases, recs = _seam(orc, name)["job"]
    want, _ = _compare_records(ctx, orc, off, bases, recs)
    assert want["polished"] == _seam(orc, name)["polished"]


BIG_CHILD = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np, torch
import polypolish_amd as pp, key_sites as ks
off, bases, recs = ks.seam_job_big().records()
want = np.load(sys.argv[1])
ctx = pp.Context(0)
got = ctx.polish_records(off, bases, recs)
assert np.array_equal(got["offsets"], want["offsets"]), (got["offsets"], want["offsets"])
assert got["polished"] == want["polished"].tobytes(), "polished bytes differ"
assert [s["changed"] for s in got["stats"]] == want["changed"].tolist()
ctx.close()
print("big ok")
"""


def test_second_level_of_the_sums_in_front_of_a_window(pp, orc, tmp_path):
    """4,098 windows (8.4 Mbp): windows 4096 and 4097 have a whole second-level group in front of them, contig starts lie
    inside windows 63, 64 and 4095, sites in windows 0, 62..65 and 4094..4097.  Bytes, offsets and per-contig figures on
    three routes: host batch; device batch with the mirror and its run table (the direct path); the scan kernel in front of
    the emission (PP_EMIT_FUSE=0, read once per process: a child).  On the same context the small job runs directly before
    the big one and after it: k_emit's finalize grid follows the winners of the job before -- too small once, too large once."""
    small, big = _seam(orc, "small"), _seam(orc, "big")
    ctx = pp.Context(0)
    try:
        for step, want in (("small", small), ("big", big), ("small", small), ("big", big)):
            off, bases, recs = want["job"]
            _check_bytes(ctx.polish_records(off, bases, recs), want, f"host batch, {step}")
        for step, want in (("small", small), ("big", big), ("small", small)):
            off, bases, recs = want["job"]
            got = _polish_device_batch(ctx, pp, off, bases, recs, True, wo=True)
            assert ctx.took_direct_path() or step == "small", step
            _check_bytes(got, want, f"direct path, {step}")
    finally:
        ctx.close()
    path = str(tmp_path / "want.npz")
    np.savez(path, polished=np.frombuffer(big["polished"], np.uint8), offsets=big["offsets"], changed=np.array(big["changed"]))
    code = BIG_CHILD % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code, path], capture_output=True, env=dict(os.environ, PP_EMIT_FUSE="0"), timeout=300)
    assert r.returncode == 0 and b"big ok" in r.stdout, (r.returncode, r.stderr.decode()[-3000:])


# ---- D. more winners than the first job's room -------------------------------------------------------------------------------

def test_more_two_byte_winners_than_a_fresh_context_has_room_for(pp, orc):
    """65,600 two-byte winners where a fresh context has room for 65,536: the oracle's bytes, in two passes on a fresh context
    (the rooms grow once) and in one when the job runs again on it.  42 sites in a window overflow the 10-slot key table, so
    every site is listed for k_exact: the first pass ends with listed positions 65,536 -> need 65,600, and k_exact votes
    nothing while the list has no room -- the room for the winners it will find has to grow with the list.  (Every read has
    an insertion and is cut into three work items: their room follows the CIGAR runs, or it would cost a pass of its own.)"""
    job = ks.many_winners_job()
    params = (1, 0.5, 0.2)
    want = _expected(orc, job, params)
    assert sum(want["changed"]) == 65_600
    off, bases, recs = want["job"]
    ctx = pp.Context(0)
    passes = []
    try:
        ctx.set_profiling(1)
        for run in ("a fresh context", "the same job again"):
            got = ctx.polish_records(off, bases, recs, **_kw(params))
            _check_bytes(got, want, run)
            passes.append(ctx.kernel_times()["n_passes"])
    finally:
        ctx.close()
    print("passes:", passes)
    assert passes[1] == 1, passes
    assert passes[0] == 2, passes
