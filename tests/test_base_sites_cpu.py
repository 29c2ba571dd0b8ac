"""The site generator (base_sites.py) against the oracle alone: the jobs test_base_vote_gpu.py runs hold what they are meant to
hold -- sites whose status and whose polished byte depend on the file order of the depth sum, windows of exactly 2047, 2048
and 32,768 work items, stacks around the end of the threshold table -- and a numpy model of the kernel's interval rule says
that they reach every branch of it.  The model only classifies; no expected result of a GPU test comes from it."""
from collections import Counter

import numpy as np
import pytest

import base_sites as bs
import key_sites as ks

FAMILIES = (("A", bs.family_a_job), ("B", bs.family_b_job), ("C", bs.family_c_job))
CLASS_NAMES = {"exact": "every share a multiple of the unit", 0: "ndiff 0", 1: "ndiff 1, votes equal", 2: "ndiff 1, votes differ",
               3: "ndiff 2 or 3"}


def _tallies(p, g, ref):
    rows = dict(zip(b"ACGT", (int(p["count_a"][g]), int(p["count_c"][g]), int(p["count_g"][g]), int(p["count_t"][g]))))
    out = {"own": rows[ref], "del": int(p["count_other"][g])}
    for i in range(3):
        out["sub%d" % i] = rows[ks.other_base(ref, i)]
    return out


@pytest.mark.parametrize("family", [f for f, _ in FAMILIES])
@pytest.mark.parametrize("params", bs.OPTION_SETS, ids=bs.IDS)
def test_a_site_has_the_planned_tallies_and_the_depth_of_its_file_order(orc, params, family):
    """What a spec says is what the oracle counts, in both file orders: the planned tally in every row, and as depth the f64
    sum of 1 / k over the site's reads in exactly the order the spec gives for that file order, bit for bit."""
    job = dict(FAMILIES)[family](orc, params)
    for which in (0, 1):
        p = bs.expected(orc, job, which)["positions"]
        for g, s in job.sites:
            order = s["perm"] if which else range(len(s["k"]))
            assert p["depth"][g] == bs.ordered_sum([s["k"][i] for i in order]), (family, which, g, s["family"], p["depth"][g])
            assert _tallies(p, g, job.raw[g]) == bs.counts_of(s), (family, which, g, _tallies(p, g, job.raw[g]), bs.counts_of(s))
    recs = bs.expected(orc, job, 0)["job"][2]
    assert (np.diff(recs["ref_start"].astype(np.int64)) < 0).any()   # (a shuffled file, not the order of the sites)


@pytest.mark.parametrize("params", bs.OPTION_SETS, ids=bs.IDS)
def test_family_a_sites_are_decided_by_the_file_order(orc, params):
    """Per option set at least 8 sites whose status the oracle gives differently for the two file orders, at least one for
    every step function that can move, and -- (5, 0.5, 0.2), (8, 0.7, 0.3), (2, 0.5, 0.25) -- at least 3 whose polished byte
    differs.  (1, 0.6, 0.05): the invalid threshold is 0 below a depth of 10 and nothing is ever invalid there; its tie lies
    at depths of 10, 30 and 50, the search goes up to 80 reads a site with at most 12 of k > 1.  min_depth = 1 cannot move:
    six or more shares from 1, 1/3, 1/5, 1/6, 1/7 add up to 1 only as six sixths or seven sevenths, the same in any order."""
    job = bs.family_a_job(orc, params)
    assert int(job.items_per_window().max()) <= 2047, "a small job: every window at the finest unit"
    st, by = bs.order_differences(orc, job)
    spec_of = dict(job.contested())
    moved = Counter(spec_of[g]["moved"] for g in st)
    deep = sum(1 for g in by if spec_of[g].get("deep"))
    print(f"\noptions {params}: {len(spec_of)} sites, status differs at {len(st)} ({dict(moved)}), polished byte at {len(by)} ({deep} of them deep sites)")
    assert len(st) >= 8, (params, len(st), dict(moved))
    for step in bs.STEPS[:2] + (bs.STEPS[2:] if params[0] > 1 else ()):
        assert moved[step] >= 1, (params, step, dict(moved))
    if params in bs.BYTE_SETS:
        assert len(by) >= 3, (params, len(by))
    else:
        # the deeper search finds three multisets (12, 17 and 79 reads; depths 10, 10 and 70), two sites each: the own base on
        # the lower value of the invalid threshold and above the higher one; at the first of each the polished byte differs
        found = sum(1 for s in spec_of.values() if s.get("deep"))
        assert (found, deep) == (6, 3) and len(by) >= 3, (
            f"sites of {bs.DEEP[0]}..{bs.DEEP[1]} reads with 2..12 of k in (3, 5, 6, 7), 6000 draws: {found} deep sites, "
            f"polished byte differs at {deep} of them and at {len(by)} sites in all")


@pytest.mark.parametrize("params", bs.OPTION_SETS, ids=bs.IDS)
def test_family_b_holds_every_share_class_on_both_candidate_thresholds(orc, params):
    """Every k of the seams of the share classes, each under a tally on either candidate threshold wherever m * fraction has a
    tie at all; dyadic sites with a fractional depth; the oracle's thresholds at the site are among the planned tallies."""
    job = bs.family_b_job(orc, params)
    assert int(job.items_per_window().max()) <= 2047
    p = bs.expected(orc, job, 0)["positions"]
    ties = [(g, s) for g, s in job.contested() if s["moved"] != "dyadic"]
    assert {s["extra"] for _, s in ties} == set(bs.EXTRA_KS)
    on = Counter()
    for g, s in ties:
        thr = int(p["valid_thr" if s["moved"] == "valid" else "invalid_thr"][g])
        on[s["extra"]] += s["tally"] == thr
    assert all(on[k] >= 1 for k in bs.EXTRA_KS), on
    dy = [(g, s) for g, s in job.contested() if s["moved"] == "dyadic"]
    assert len(dy) >= 12 and all(p["depth"][g] % 1.0 in (0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875) for g, _ in dy)
    assert all(set(s["k"]) <= {1, 2, 4, 8} for _, s in dy)


@pytest.mark.parametrize("params", bs.OPTION_SETS, ids=bs.IDS)
def test_family_c_windows_hold_exactly_the_planned_items(orc, params):
    """Counted from the records themselves: every read of windows 1 and 2 is one M run inside its window, 2047 and 2048 of
    them; window 3 has 32,768 reads and more, and is heavy (over 1.5 times the job's average, over 3072); the job stays
    under 45,000 reads; the 2048-item window has a tie site whose extra read has k = 2^20, half a unit off at b = 19."""
    job = bs.family_c_job(orc, params)
    off, bases, recs = job.ordered(0)
    first = recs["ref_start"].astype(np.int64) // ks.WIN
    span = np.array([sum(c >> 4 for c in recs["cigar"][o:o + n] if (c & 15) in (0, 2)) for o, n in zip(recs["cig_off"], recs["n_cig"])])
    last = (recs["ref_start"].astype(np.int64) + span - 1) // ks.WIN
    assert (first == last).all(), "no read reaches into the next window"
    per = np.bincount(first, minlength=bs.C_WINDOWS)
    assert per[bs.W_2047] == 2047 and per[bs.W_2048] == 2048 and per[bs.W_HEAVY] >= 32768, per
    assert (recs["n_cig"][(first == bs.W_2047) | (first == bs.W_2048)] == 1).all()
    assert list(job.items_per_window()[[bs.W_2047, bs.W_2048]]) == [2047, 2048]
    assert [bs.win_fx_bits(n) for n in job.items_per_window()[1:4]] == [20, 19, 15]
    assert len(recs["contig"]) <= 45_000 and per[bs.W_HEAVY] >= max(3072, 1.5 * len(recs["contig"]) / bs.C_WINDOWS)
    half = [s for g, s in job.contested() if g // ks.WIN == bs.W_2048 and s.get("extra") == 1 << 20]
    assert half and bs.share_units(1 << 20, 19) == 1   # (the share 2^-20 is half a unit of 2^-19: rounded up to a whole one)
    for w in (bs.W_2047, bs.W_2048):
        lone = [s for g, s in job.sites if g // ks.WIN == w and s["family"] == "lone"]
        assert len(lone) == 1 and lone[0]["k"] == [3]
    in_heavy = Counter(s["family"] for g, s in job.contested() if g // ks.WIN == bs.W_HEAVY)
    assert in_heavy["A"] >= 3 and in_heavy["B"] >= 3 and in_heavy["C"] >= 5, in_heavy
    for w in (bs.W_2047, bs.W_2048):
        fam = Counter(s["family"] for g, s in job.contested() if g // ks.WIN == w)
        assert fam["A"] >= 5 and fam["B"] >= 5, (w, fam)


@pytest.mark.parametrize("ntot", bs.D_DEPTHS)
def test_family_d_stacks_sit_on_and_below_both_thresholds(orc, ntot):
    job = bs.family_d_job(orc, ntot)
    p = bs.expected(orc, job, 0)["positions"]
    assert len(job.sites) == 4 and len(job.reads) == 4 * ntot <= 45_000 and {g // ks.WIN for g, _ in job.sites} == {1}
    got = []
    for g, s in job.sites:
        assert p["depth"][g] == float(ntot)
        sub = _tallies(p, g, job.raw[g])["sub%d" % (job.sites.index((g, s)) % 3)]
        got.append((sub - int(p["valid_thr"][g]), sub - int(p["invalid_thr"][g])))
    assert [a for a, _ in got[:2]] == [0, -1] and [b for _, b in got[2:]] == [0, -1], got
    assert len(set(p["status"][[g for g, _ in job.sites]].tolist())) >= 2


def test_sites_of_a_job_do_not_overlap(orc):
    """Job.site refuses a site on another one's reads; and independently: the sites of every job are at least 64 apart under
    reads that reach 20 in front and at most 20 behind."""
    job = bs.BaseJob((400,), 1)
    job.place(100, bs.spec(["own", "del", "sub1"], [1, 3, 5]))
    for g in (120, 139, 61, 390):
        with pytest.raises(AssertionError):
            job.place(g, bs.spec(["own"], [1]))
    job.place(141, bs.spec(["own"], [1]))
    assert len(job.sites) == 2 and len(job.reads) == 4
    for params in bs.OPTION_SETS:
        for _, make in FAMILIES + (("S", bs.shortcut_job),):
            g = np.sort([g for g, _ in make(orc, params).sites])
            assert (np.diff(g) >= 64).all()
    for ntot in bs.D_DEPTHS:
        assert (np.diff(np.sort([g for g, _ in bs.family_d_job(orc, ntot).sites])) >= 64).all()


@pytest.mark.parametrize("params", bs.OPTION_SETS, ids=bs.IDS)
def test_the_jobs_reach_every_branch_of_the_interval_rule(orc, params):
    """The interval rule in numpy (share_units, win_fx_bits and eps as test_interval_vote_cpu.py has them) over the site
    positions of families A to C: at least 5 where all three step functions agree at both ends of the interval, 5 where one
    differs by a step and both votes agree, 5 where one differs and the votes differ, 5 where two or three differ (or one by
    more than a step) -- and 5 whose shares are all multiples of the unit.  The shortcut job has sites of the second class only."""
    cls = Counter()
    per_family = {}
    for name, make in FAMILIES:
        c = Counter(bs.classify(make(orc, params)).values())
        per_family[name] = {CLASS_NAMES[k]: v for k, v in c.items()}
        cls.update(c)
    print(f"\noptions {params}: site positions per class {per_family}")
    for k in CLASS_NAMES:
        assert cls[k] >= 5, (params, CLASS_NAMES[k], per_family)
    short = bs.classify(bs.shortcut_job(orc, params))
    assert len(short) >= 20 and set(short.values()) == {1}, Counter(short.values())


def test_the_interval_model_holds_the_depth_of_both_file_orders(orc):
    """The model's interval is the kernel's bound: the oracle's depth at a site lies inside it in both file orders."""
    for params in bs.OPTION_SETS:
        for _, make in FAMILIES:
            job = make(orc, params)
            bits = [bs.win_fx_bits(n) for n in job.items_per_window()]
            for which in (0, 1):
                depth = bs.expected(orc, job, which)["positions"]["depth"]
                for g, s in job.contested():
                    b = bits[g // ks.WIN]
                    D = sum(bs.share_units(k, b) for k in s["k"]) / float(1 << b)
                    eps = len(s["k"]) * (0.5 / float(1 << b)) + 1e-9
                    assert D - eps <= depth[g] <= D + eps, (params, g, b, D, eps, depth[g])


def test_the_generator_is_deterministic(orc):
    def same(a, b):
        (o1, b1, r1), (o2, b2, r2) = a, b
        return np.array_equal(o1, o2) and np.array_equal(b1, b2) and all(np.array_equal(r1[k], r2[k]) for k in r1)
    for make in (bs.family_a_job, bs.family_b_job, bs.family_c_job):
        one, two = make(orc, bs.OPTION_SETS[2]), make.__wrapped__(orc, bs.OPTION_SETS[2])
        assert one is not two and same(one.ordered(0), two.ordered(0)) and same(one.ordered(1), two.ordered(1))
        assert not same(one.ordered(0), one.ordered(1))
