"""The site generator (key_sites.py) against the oracle alone: the jobs test_key_vote_gpu.py runs hold what they are meant to
hold -- every outcome of the vote, key counts on and one below both thresholds, winners that change the length where
planned -- and are the same from run to run."""
from collections import Counter

import numpy as np
import pytest

import key_sites as ks


def _oracle(orc, job, params=ks.DEFAULT):
    off, bases, recs = job.records()
    md, fv, fi = params
    return orc.polish_records(off, bases, recs, min_depth=md, fraction_valid=fv, fraction_invalid=fi, positions=True)


def _same(a, b):
    (o1, b1, r1), (o2, b2, r2) = a.records(), b.records()
    return np.array_equal(o1, o2) and np.array_equal(b1, b2) and all(np.array_equal(r1[k], r2[k]) for k in r1)


def test_assembly_has_no_homopolymer_longer_than_three():
    a = ks.assembly(np.random.default_rng(1), 200_000)
    assert set(a.tolist()) == set(b"ACGT")
    assert not (a[3:] == a[2:-1])[(a[2:-1] == a[1:-2]) & (a[1:-2] == a[:-3])].any()
    assert ((a[2:] == a[1:-1]) & (a[1:-1] == a[:-2])).sum() > 1000  # (runs of three do occur)


def test_sites_may_not_overlap_or_leave_their_contig():
    job = ks.Job((200, 200), 1)
    job.site(100, [("plain", None, 1)] * 3)
    for g in (130, 81, 10, 190, 205):
        with pytest.raises(AssertionError):
            job.site(g, [("plain", None, 1)])
    job.site(140, [("del", 16, 1)])
    with pytest.raises(AssertionError):
        job.site(180, [("plain", None, 1)])  # (the deletion's reads reach up to 174)
    assert len(job.sites) == 2 and len(job.reads) == 4


def test_a_site_has_exactly_the_planned_tallies(orc):
    """What the generator says it planted is what the oracle counts: the site's depth is its own read count, its string-keyed
    row the planned key counts -- with every kind of read, at a window seam and at a contig's last coverable position."""
    for variant in ks.KEY2_VARIANTS:
        job = ks.threshold_job(orc, ks.DEFAULT, variant)
        p = _oracle(orc, job)["positions"]
        assert len(job.sites) >= 120
        for g, plan in job.sites:
            total = int(p["count_a"][g]) + int(p["count_c"][g]) + int(p["count_g"][g]) + int(p["count_t"][g]) + int(p["count_other"][g])
            assert total == plan["n"] and p["depth"][g] == float(plan["n"]), (variant, g, plan, total, p["depth"][g])
            assert int(p["count_other"][g]) == sum(plan["keys"].values()), (variant, g, plan, p["count_other"][g])
        ends = [int(e) - 3 for e in job.off[1:]]
        assert all(p["depth"][e] == 12.0 and p["depth"][e + 1] == 0.0 for e in ends), [p["depth"][e:e + 3] for e in ends]
        assert {g % ks.WIN for g, _ in job.sites} & {0, 1, 2046, 2047}
    assert {g % ks.WIN for v in ks.KEY2_VARIANTS for g, _ in ks.threshold_job(orc, ks.DEFAULT, v).sites} >= {0, 1, 2046, 2047}


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("params", ks.OPTION_SETS, ids=[f"{p[0]}-{p[1]}-{p[2]}" for p in ks.OPTION_SETS])
def test_threshold_jobs_hold_every_outcome_and_counts_on_both_thresholds(orc, params, sparse):
    """Over the key sites (count_other > 0) of an option set's jobs -- the four variants of key 2 and the depth-share job --:
    each of the statuses kept, changed, none, multiple and too close at 10 sites or more, low depth at 3 or more; a key's
    count equal to the valid threshold at 20 sites or more, one below it at 20 or more, and the same for the invalid
    threshold wherever it is at least 1.  (The thresholds are the oracle's at the site; the counts are the planned ones, which
    test_a_site_has_exactly_the_planned_tallies ties to the oracle's row.)  The same holds for the sparse jobs (three
    seeds each), in which no window has more pairs of position and two-byte key than k_tile's table holds."""
    status = Counter()
    on = Counter()
    n_sites = 0
    jobs = [ks.threshold_job(orc, params, v, seed, sparse) for v in ks.KEY2_VARIANTS for seed in ks.SEEDS[sparse]]
    jobs += [ks.shares_job(orc, params, seed, sparse) for seed in ks.SEEDS[sparse]]
    for job in jobs:
        assert (max(job.pairs.values()) <= ks.PT_SLOTS) == sparse, job.pairs
        p = _oracle(orc, job, params)["positions"]
        status.update(p["status"][p["count_other"] > 0].tolist())
        n_sites += len(job.sites)
        for g, plan in job.sites:
            counts = [c for c in plan["keys"].values() if c > 0]
            v, i = int(p["valid_thr"][g]), int(p["invalid_thr"][g])
            on["valid_thr"] += v in counts
            on["valid_thr - 1"] += v - 1 in counts
            if i >= 1:
                on["invalid_thr"] += i in counts
                on["invalid_thr - 1"] += i - 1 in counts
            else:
                on["invalid_thr == 0"] += 1
    print(f"\noptions {params}, {'sparse' if sparse else 'dense'}: {n_sites} sites; key positions per status "
          f"{ {orc.STATUS[s]: status[s] for s in sorted(status)} }; sites with a key count on {dict(on)}")
    for s in (0, 1, 3, 4, 5):
        assert status[s] >= 10, (orc.STATUS[s], status)
    assert status[2] >= 3, status
    for k in ("valid_thr", "valid_thr - 1", "invalid_thr", "invalid_thr - 1"):
        assert on[k] >= 20, (k, on)
    if params == ks.OPTION_SETS[1]:
        assert on["invalid_thr == 0"] >= 20, on  # (where every zero tally is intermediate, pileup.rs:79)


def test_shares_job_has_order_dependent_depths(orc):
    job = ks.shares_job(orc, ks.DEFAULT)
    p = _oracle(orc, job)["positions"]
    all3 = [g for g, plan in job.sites if set(plan["k"]) == {3} and plan["n"] >= 15]
    assert len(all3) >= 9 and {len(plan["k"]) for _, plan in job.sites} >= {15, 30, 45}
    assert any(p["depth"][g] == 4.999999999999999 and p["status"][g] == 2 for g in all3), p["depth"][all3]
    assert sum(1 for _, plan in job.sites if len(set(plan["k"])) == 3) >= 50


def test_capacity_jobs(orc):
    for n_pairs in (9, 10, 11):
        job = ks.capacity_job(n_pairs)
        assert sum(sum(c > 0 for c in plan["keys"].values()) for _, plan in job.sites) == n_pairs
        assert {g // ks.WIN for g, _ in job.sites} == {1}
        p = _oracle(orc, job)["positions"]
        st = Counter(p["status"][[g for g, _ in job.sites]].tolist())
        assert st[1] >= 1 and st[3] >= 1 and st[5] >= 1, st
    job = ks.one_position_job()
    w = _oracle(orc, job)
    (g, _), = job.sites
    assert w["positions"]["status"][g] == 3 and w["positions"]["count_other"][g] == 12 and w["polished"] == job.raw


LEN_CHANGE = {"two": 1, "del": -1, "del16": -16, "del22": -22, "ins2": 2, "ins125": 125, "ins126": 126, "dash": 0}


@pytest.mark.parametrize("make", [ks.seam_job_small, ks.seam_job_coarse, ks.seam_job_big], ids=["small", "coarse", "big"])
def test_seam_jobs_change_the_length_where_planned(orc, make):
    job = make()
    w = _oracle(orc, job)
    p = w["positions"]
    assert all(p["status"][g] == 1 for g, _ in job.sites), [(g, plan) for g, plan in job.sites if p["status"][g] != 1]
    off = [int(x) for x in job.off]
    for c in range(len(off) - 1):
        delta = sum(LEN_CHANGE[plan["kind"]] for g, plan in job.sites if off[c] <= g < off[c + 1])
        assert int(w["offsets"][c + 1]) - int(w["offsets"][c]) == off[c + 1] - off[c] + delta, (c, delta)
    at = {(g % ks.WIN, plan["kind"]) for g, plan in job.sites}
    windows = {g // ks.WIN for g, _ in job.sites}
    if make is ks.seam_job_small:
        assert {k for _, k in at} >= set(LEN_CHANGE)
        assert {q for q, _ in at} >= {16, 15, 1023, 1024, 2047}
        assert int(w["offsets"][2]) - int(w["offsets"][1]) == 8  # the short contig: its first two and its last six bases
    if make is ks.seam_job_coarse:
        assert windows >= {0, 62, 63, 64, 65}
        for q in (0, 15, 16, 1023, 1024, 2047):
            assert {k for qq, k in at if qq == q} >= set(ks.KINDS), (q, at)
        assert (off[1] // ks.WIN, off[2] // ks.WIN) == (63, 64) and off[1] - 3 in [g for g, _ in job.sites]
    if make is ks.seam_job_big:
        assert windows >= {0, 62, 63, 64, 65, 4094, 4095, 4096, 4097} and off[-1] == 4098 * ks.WIN
        assert [o // ks.WIN for o in off[1:4]] == [63, 64, 4095] and all(o % ks.WIN for o in off[1:4])


def test_many_winners_job(orc):
    job = ks.many_winners_job()
    off, bases, recs = job.records()
    w = orc.polish_records(off, bases, recs, min_depth=1, positions=True)
    g = np.array([g for g, _ in job.sites])
    p = w["positions"]
    assert len(g) == 65_600 and (p["status"][g] == 1).all() and (p["valid_thr"][g] == 2).all() and (p["invalid_thr"][g] == 1).all()
    assert len(w["polished"]) == len(bases) + 65_600 and (p["status"] == 1).sum() == 65_600


def test_the_generator_is_deterministic(orc):
    assert _same(ks.threshold_job(orc, ks.OPTION_SETS[2], "slow_read"), ks.threshold_job(orc, ks.OPTION_SETS[2], "slow_read"))
    assert _same(ks.shares_job(orc, ks.DEFAULT), ks.shares_job(orc, ks.DEFAULT))
    assert _same(ks.seam_job_small(), ks.seam_job_small()) and _same(ks.capacity_job(11), ks.capacity_job(11))
    off, bases, recs = ks.seam_job_small().records()
    assert (np.diff(recs["ref_start"].astype(np.int64)) < 0).any()  # (a random file order, not the order of the sites)
