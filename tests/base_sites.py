"""Jobs made of sites where the A, C, G, T or "-" tally sits on a threshold that the FILE ORDER of the depth sum decides.

The reference adds a position's depth up as depth += 1.0 / k in file order (pileup.rs:64) and looks at it through three step
functions: bankers(depth * fraction_valid), bankers(depth * fraction_invalid) and depth < min_depth (pileup.rs:70-72,114).
Shares like 1/3 put the sum within an ulp of a step, and two orders of the same reads on either side of it.  A site here is a
position g under reads of 40 bases (key_sites.Job), each with its own k and one of three kinds: the assembly's own base, one
of the three other bases (a tally in another of the A/C/G/T rows), or a deleted base (a tally for "-").  A site is first a
SPEC -- the reads in file order 0, a permutation for file order 1, rows still abstract ("own", "sub0".."sub2", "del") -- and
becomes reads when it is placed on an assembly.  Four families:

  A  order-decided sites: a seeded search for multisets of k whose ordered f64 sum steps over one of the three in two orders
  B  m reads of k = 1 with m * fraction on an exact .5 tie plus one or two reads of a tiny or odd share; dyadic shares only
  C  the sites of A and B in windows of exactly 2047 and 2048 work items and in one of 36,000 (the window's unit 2^-b)
  D  stacks of 4095, 4096 and 4097 reads of k = 1: the end of the table of thresholds per integer depth

Everything is seeded and runs without a GPU.  Thresholds come from the oracle (`orc`), never from the code under test.  The
numpy model of the kernel's interval rule at the end only says which branch a site reaches; no expected result comes from it."""
import functools
from fractions import Fraction

import numpy as np

import key_sites as ks

OPTION_SETS = ks.OPTION_SETS + ((2, 0.5, 0.25),)   # 0.25: depth * fi is on a .5 tie at depths 2, 6, 10, ...
BYTE_SETS = ((5, 0.5, 0.2), (8, 0.7, 0.3), (2, 0.5, 0.25))
IDS = [f"{p[0]}-{p[1]}-{p[2]}" for p in OPTION_SETS]
A_KS = (1, 3, 5, 6, 7)
EXTRA_KS = (2, 1 << 19, 1 << 20, 1 << 21, 3, 236, 237, 1000, 1 << 31)   # the seams of kclass_of and share_deficit
STEPS = ("valid", "invalid", "min_depth")
ROWS = ("own", "sub0", "sub1", "sub2", "del")
VOTE_TAB_N = 4096
DEEP = (6, 80)   # reads per site of the deeper search for (1, 0.6, 0.05)


def ordered_sum(kseq):
    depth = 0.0
    for k in kseq:
        depth += 1.0 / float(k)
    return depth


def steps(orc, depth, params):
    """The three step functions of the vote at a depth."""
    md, fv, fi = params
    return orc.bankers_rounding(depth * fv), orc.bankers_rounding(depth * fi), depth < md


def spec(rows, kseq, perm=None, **tag):
    """rows[i], kseq[i]: row and k of read i in file order 0; perm: the reads' indices in file order 1 (default: reversed)."""
    assert len(rows) == len(kseq) and all(r in ROWS for r in rows)
    perm = list(range(len(rows)))[::-1] if perm is None else [int(i) for i in perm]
    assert sorted(perm) == list(range(len(rows)))
    return dict(rows=list(rows), k=[int(k) for k in kseq], perm=perm, **tag)


def counts_of(s):
    return {r: s["rows"].count(r) for r in ROWS}


def tally_rows(n, row, t, rest):
    """t reads for `row`, the other n - t for `rest` -- spread evenly over the file order, so that no row's reads share a k."""
    assert 0 <= t <= n and row != rest
    rows = [rest] * n
    for j in range(t):
        rows[(j * n) // max(t, 1)] = row
    assert rows.count(row) == t
    return rows


# ---- A. order-decided sites -----------------------------------------------------------------------------------------------

def _targets(params, which, n_max):
    """The rational depths on a step: depth * fraction = j + 1/2, or depth = min_depth."""
    md, fv, fi = params
    if which == 2:
        return [Fraction(md)]
    f = Fraction(str((fv, fi)[which]))
    return [d for d in (Fraction(2 * j + 1, 2) / f for j in range(n_max)) if d <= n_max]


def order_decided_multisets(orc, params, seed, want, n_lo=6, n_hi=60, max_shared=24, tries=20000, perms=48):
    """Up to `want` of (k sequence, permutation, step that moved, steps in order 0, steps in order 1) per step function:
    multisets of k from A_KS with n_lo..n_hi reads whose ordered f64 sum gives another value of that step in two orders.  The
    draw is directed: the reads with k > 1 are drawn, and as many reads of k = 1 added as put the exact sum on a step."""
    rng = np.random.default_rng(seed)
    found = {0: [], 1: [], 2: []}
    seen = set()
    targets = {w: _targets(params, w, n_hi) for w in range(3)}
    for t in range(tries):
        which = t % 3
        if len(found[which]) >= want or not targets[which]:
            if all(len(found[w]) >= want or not targets[w] for w in range(3)):
                break
            continue
        shared = rng.choice(A_KS[1:], int(rng.integers(2, max_shared + 1)))
        frac = sum(Fraction(1, int(k)) for k in shared)
        ones = [d - frac for d in targets[which] if d >= frac and (d - frac).denominator == 1
                and n_lo <= len(shared) + int(d - frac) <= n_hi]
        if not ones:
            continue
        kseq = np.concatenate([shared, np.ones(int(ones[int(rng.integers(len(ones)))]), np.int64)]).astype(np.int64)
        key = tuple(sorted(kseq.tolist()))
        if key in seen:
            continue
        seen.add(key)
        orders = [np.argsort(kseq, kind="stable"), np.argsort(-kseq, kind="stable")] + [rng.permutation(len(kseq)) for _ in range(perms)]
        st = [steps(orc, ordered_sum(kseq[o]), params) for o in orders]
        pair = next(((a, b) for a in range(len(st)) for b in range(a + 1, len(st)) if st[a][which] != st[b][which]), None)
        if pair is None:
            continue
        a, b = pair
        if st[a][which] > st[b][which]:   # order 0 is the one with the lower threshold (or the depth that is not too low)
            a, b = b, a
        k0 = kseq[orders[a]]
        inv = np.empty(len(kseq), np.int64)
        inv[orders[a]] = np.arange(len(kseq))
        found[which].append(dict(k=k0.tolist(), perm=inv[orders[b]].tolist(), moved=which, st0=st[a], st1=st[b]))
    return found


# which row gets the contested tally and which the rest, by the step that moved: the first pair of each is the one where the
# polished byte can differ (own base on the invalid threshold under a substituted base; a substituted base on the valid one)
PAIRS = {0: (("sub0", "own"), ("del", "own"), ("own", "sub1"), ("sub2", "del")),
         1: (("own", "sub0"), ("own", "del"), ("sub1", "own"), ("del", "sub2"), ("own", "sub2")),
         2: (("sub0", "own"), ("own", "sub1"), ("del", "own"))}


def order_decided_specs(orc, params, seed=0, want=10, rows_ok=ROWS, **search):
    """Three sites per multiset: one row's tally on the lower of the moved threshold's two values, one below it, one above the
    higher (where the depth test moved: around the valid threshold), the rest of the reads in one other row."""
    md = params[0]
    out = []
    found = order_decided_multisets(orc, params, 7000 + 10 * OPTION_SETS.index(params) + seed, want, **search)
    for which in range(3):
        pairs = [p for p in PAIRS[which] if p[0] in rows_ok and p[1] in rows_ok]
        for j, m in enumerate(found[which]):
            n = len(m["k"])
            if which == 2:
                lo = hi = max(md, m["st1"][0])
            else:
                lo, hi = sorted((m["st0"][which], m["st1"][which]))
                if which == 0:
                    lo, hi = max(md, lo), max(md, hi)
            for i, t in enumerate((lo, lo - 1, hi + 1)):
                if not 0 <= t <= n:
                    continue
                row, rest = pairs[0] if i == 0 and j % 2 == 0 else pairs[(j + i) % len(pairs)]
                out.append(spec(tally_rows(n, row, t, rest), m["k"], m["perm"], family="A", moved=STEPS[which], tally=t))
    return out


# ---- B. tie-tipping and share classes --------------------------------------------------------------------------------------

def tie_depths(params, which, m_max=100, count=3):
    """The first `count` integer depths m >= 2 at which m * fraction is an exact .5 in f64 that rounds DOWN to an even number --
    anything more tips it up --, and, for the valid threshold, to no less than min_depth (below it min_depth is the threshold)."""
    md, f = params[0], params[1 + which]
    return [m for m in range(2, m_max) if (m * f) % 1.0 == 0.5 and int(m * f) % 2 == 0 and (which or int(m * f) >= md)][:count]


def tie_specs(orc, params, rows_ok=ROWS, extra_ks=EXTRA_KS, count=3):
    """m reads of k = 1 on a tie of the valid or the invalid threshold and one or two reads of another share: the exact depth
    is m + 2^-20, say, and rounds differently from m.  One row's tally sits on each of the two candidate thresholds."""
    md = params[0]
    out = []
    for which in (0, 1):
        pairs = [p for p in PAIRS[which] if p[0] in rows_ok and p[1] in rows_ok]
        for m in tie_depths(params, which, count=count):
            for j, k in enumerate(extra_ks):
                extra = [k] * (1 + (j + m) % 2)
                kseq = [1] * (m // 2) + extra + [1] * (m - m // 2)
                cand = sorted({steps(orc, float(m), params)[which], steps(orc, ordered_sum(kseq), params)[which]})
                if which == 0:
                    cand = sorted({max(md, c) for c in cand})
                for i, t in enumerate(cand):
                    if 0 <= t <= len(kseq):
                        row, rest = pairs[(j + i) % len(pairs)]
                        out.append(spec(tally_rows(len(kseq), row, t, rest), kseq, family="B", moved=STEPS[which], tally=t, extra=k))
    return out


def dyadic_specs(orc, params, seed=0, count=12, rows_ok=ROWS):
    """Shares 1, 1/2, 1/4, 1/8 only: the depth is x.5, x.25, ... and exact in any order, but no integer -- the thresholds are
    neither replayed nor read from the table.  A substituted base on, or one below, the valid or the invalid threshold."""
    rng = np.random.default_rng(7500 + OPTION_SETS.index(params) + 10 * seed)
    out = []
    while len(out) < count:
        n = int(rng.integers(6, 24))
        kseq = rng.choice((1, 1, 2, 4, 8), n)
        depth = ordered_sum(kseq)
        if depth == int(depth):
            continue
        vthr, ithr = ks.thresholds(orc, depth, params)
        t = (vthr, vthr - 1, ithr, ithr - 1)[len(out) % 4]
        if not 0 <= t <= n:
            continue
        row, rest = [p for p in PAIRS[len(out) % 2] if p[0] in rows_ok and p[1] in rows_ok][len(out) % 2]
        out.append(spec(tally_rows(n, row, t, rest), kseq, family="B", moved="dyadic", tally=t))
    return out


# ---- placing specs ------------------------------------------------------------------------------------------------------------

class BaseJob(ks.Job):
    """key_sites.Job whose sites remember both file orders of their reads."""

    def __init__(self, contig_lens, seed, params=ks.DEFAULT):
        super().__init__(contig_lens, seed)
        self.params = params
        self.groups = []   # (first read, reads, permutation for file order 1) per site

    def place(self, g, s):
        ref = self.raw[g]
        arg = {"own": ("plain", None), "del": ("del", 1), "sub0": ("sub", bytes([ks.other_base(ref, 0)])),
               "sub1": ("sub", bytes([ks.other_base(ref, 1)])), "sub2": ("sub", bytes([ks.other_base(ref, 2)]))}
        first = len(self.reads)
        self.site(g, [arg[r] + (k,) for r, k in zip(s["rows"], s["k"])], plan=s)
        self.groups.append((first, len(s["rows"]), s["perm"]))
        return g

    def filler(self, g, n):
        """n plain reads of k = 1 stacked over g: nothing contested, only items of the window."""
        return self.place(g, spec(["own"] * n, [1] * n, family="filler"))

    def ordered(self, which, seed=0):
        """(contig_off, bases, recs) with the reads in file order `which` (0 or 1): the sites' reads are scattered over the file
        by one seeded shuffle -- the same for both orders --, and within a site they stand in its order 0 or its order 1."""
        n = len(self.reads)
        assert sum(g[1] for g in self.groups) == n, "every read belongs to a placed site"
        slot_of = np.random.default_rng(seed).permutation(n)   # read i of order 0 goes to slot slot_of[i]
        at = np.empty(n, np.int64)
        for first, m, perm in self.groups:
            slots = np.sort(slot_of[first:first + m])
            at[slots] = first + (np.asarray(perm) if which else np.arange(m))
        ent = [self.reads[i] for i in at]
        n_cig = np.array([len(e[4]) for e in ent], np.uint32)
        seq_len = np.array([len(e[3]) for e in ent], np.uint32)
        cig = np.array([(l << 4) | ks.OPS.index(o) for e in ent for l, o in e[4]], np.uint32)
        recs = {"contig": np.array([e[0] for e in ent], np.uint32), "ref_start": np.array([e[1] for e in ent], np.uint32),
                "k": np.array([e[2] for e in ent], np.uint32),
                "seq_off": (np.cumsum(seq_len, dtype=np.uint64) - seq_len).astype(np.uint64), "seq_len": seq_len,
                "cig_off": (np.cumsum(n_cig, dtype=np.uint64) - n_cig).astype(np.uint64), "n_cig": n_cig,
                "seq": np.frombuffer(b"".join(e[3] for e in ent), np.uint8), "cigar": cig}
        return self.off, self.bases, recs

    def contested(self):
        """(position, spec) of the sites proper (no fillers)."""
        return [(g, s) for g, s in self.sites if s["family"] != "filler"]

    def items_per_window(self):
        """Work items per window: a read of one M run is one item, a read with a deleted base is cut into three."""
        n = np.zeros((int(self.off[-1]) + ks.WIN - 1) // ks.WIN, np.int64)
        for g, s in self.sites:
            n[g // ks.WIN] += len(s["rows"]) + 2 * s["rows"].count("del")
        return n


APART = 128   # positions between the sites of a small job: at most 16 sites and far fewer than 2047 items in a window


def small_job(specs, seed, params, contig_lens=None):
    """The specs 128 positions apart on two contigs, in a seeded order."""
    need = (len(specs) + 2) * APART
    lens = contig_lens or (need - need // 3, need // 3 + 2 * APART)
    job = BaseJob(lens, seed, params)
    grid = [g for c in range(len(job.off) - 1) for g in range(int(job.off[c]) + 40, int(job.off[c + 1]) - 64, APART)]
    assert len(grid) >= len(specs), (len(grid), len(specs))
    for g, i in zip(grid, job.rng.permutation(len(specs))):
        job.place(g, specs[int(i)])
    return job


@functools.lru_cache(maxsize=None)
def family_a_job(orc, params, seed=0):
    specs = order_decided_specs(orc, params, seed)
    if params == OPTION_SETS[1]:   # the invalid tie at depths of 10, 30, ...: deeper sites, mostly k = 1
        specs += deep_invalid_specs(orc, params, seed)
    return small_job(specs, 8000 + 10 * OPTION_SETS.index(params) + seed, params)


def deep_invalid_specs(orc, params, seed=0, want=6):
    """(1, 0.6, 0.05): sites of up to 80 reads, at most 12 of them shared, whose depth of 10, 30 or 50 steps over the invalid tie."""
    found = order_decided_multisets(orc, params, 7700 + seed, want, n_lo=DEEP[0], n_hi=DEEP[1], max_shared=12, tries=6000)
    out = []
    for j, m in enumerate(found[1]):
        n = len(m["k"])
        lo, hi = sorted((m["st0"][1], m["st1"][1]))
        for t in (lo, hi + 1):
            if 0 <= t <= n:
                out.append(spec(tally_rows(n, "own", t, "sub%d" % (j % 3)), m["k"], m["perm"], family="A", moved="invalid", tally=t, deep=True))
    return out


@functools.lru_cache(maxsize=None)
def family_b_job(orc, params, seed=0):
    return small_job(tie_specs(orc, params) + dyadic_specs(orc, params, seed), 8100 + 10 * OPTION_SETS.index(params) + seed, params)


# ---- C. the window's unit ------------------------------------------------------------------------------------------------------

C_WINDOWS = 5
W_2047, W_2048, W_HEAVY = 1, 2, 3
HEAVY_ITEMS = 36_000   # (32,768 and more: b = 15)
LONE_SLOT = 31   # the window's last slot: one lone read of k = 3, which locates the seam of the unit
ONE_RUN = ("own", "sub0", "sub1", "sub2")   # rows whose reads are one M run: one work item on every path


def wide_specs(params, n_sites=6):
    """Sites for the 36,000-item window (b = 15) whose interval is wide enough to hold two steps at once: eleven reads of
    k = 12 and ~5,500 of k = 2^31, whose shares round to nothing -- the fixed-point depth is 11/12 and the bound a twelfth
    and more either side, from below 5/6 to 1.0.  (Which steps lie in it depends on the options; the model tells.)"""
    out = []
    for i in range(n_sites):
        n_big = 5489 + 3 * i
        kseq = [12] * 11 + [1 << 31] * n_big
        out.append(spec(tally_rows(len(kseq), "sub%d" % (i % 3), 3 + i, "own"), kseq, family="C", moved="wide", tally=3 + i))
    return out


def _slots(window):
    return [window * ks.WIN + 32 + 64 * s for s in range(ks.WIN // 64)]


def _fill(job, window, specs, n_items, n_fill_slots=6):
    """The specs on the window's first slots, the lone k = 3 read on its last, and plain k = 1 reads stacked on n_fill_slots
    others until the window holds exactly n_items reads."""
    slots = _slots(window)
    assert len(specs) <= len(slots) - 1 - n_fill_slots, (len(specs), len(slots))
    for g, s in zip(slots, specs):
        job.place(g, s)
    job.place(slots[LONE_SLOT], spec(["own"], [3], family="lone"))
    left = n_items - int(job.items_per_window()[window])
    assert left >= n_fill_slots, (window, left)
    for j, g in enumerate(slots[LONE_SLOT - n_fill_slots:LONE_SLOT]):
        job.filler(g, left // n_fill_slots + (j < left % n_fill_slots))
    assert int(job.items_per_window()[window]) == n_items


@functools.lru_cache(maxsize=None)
def family_c_job(orc, params, seed=0):
    """One contig of five windows: window 1 holds exactly 2047 reads (b = 20), window 2 exactly 2048 (b = 19), window 3
    32,768 and more (b = 15; a heavy window: its items are split over helper blocks whose partial deficits add up).  Every
    read of windows 1 and 2 lies inside its window and is one M run.  The 2048-item window has the tie sites whose extra
    read has k = 2^20: at b = 19 that share is off by exactly half a unit, the edge of the interval's bound."""
    job = BaseJob((C_WINDOWS * ks.WIN,), 8200 + 10 * OPTION_SETS.index(params) + seed, params)
    a = order_decided_specs(orc, params, seed + 1, want=4, rows_ok=ONE_RUN)
    b = tie_specs(orc, params, rows_ok=ONE_RUN, count=1)
    half = [s for s in b if s["extra"] == 1 << 20]
    rest = [s for s in b if s["extra"] != 1 << 20] + dyadic_specs(orc, params, seed + 1, 4, ONE_RUN)
    assert half, "the 2048-item window needs a site with a read of k = 2^20"
    room = ks.WIN // 64 - 1 - 6
    for window, lead, n_items in ((W_2047, half[:1], 2047), (W_2048, half[:2], 2048)):   # every other spec of A and of B each
        mixed = [x for pair in zip(a[window - W_2047::2], rest[window - W_2047::2]) for x in pair]
        _fill(job, window, (lead + mixed)[:room], n_items)
    heavy = wide_specs(params) + order_decided_specs(orc, params, seed + 2, want=1) + tie_specs(orc, params, count=1)[:8]
    _fill(job, W_HEAVY, heavy[:room], HEAVY_ITEMS)
    return job


# ---- D. the table's end ----------------------------------------------------------------------------------------------------------

D_DEPTHS = (VOTE_TAB_N - 1, VOTE_TAB_N, VOTE_TAB_N + 1)


@functools.lru_cache(maxsize=None)
def family_d_job(orc, ntot, params=ks.DEFAULT):
    """Four stacks of ntot reads of k = 1 in one window: a substituted base on and one below the valid and the invalid threshold.
    Depths below 4096 read both thresholds from the job's table, 4096 and 4097 compute them."""
    job = BaseJob((2 * ks.WIN,), 8300 + ntot, params)
    vthr, ithr = ks.thresholds(orc, float(ntot), params)
    for j, t in enumerate((vthr, vthr - 1, ithr, ithr - 1)):
        job.place(ks.WIN + 100 + 256 * j, spec(tally_rows(ntot, "sub%d" % (j % 3), t, "own"), [1] * ntot, family="D", moved=STEPS[j // 2], tally=t))
    return job


# ---- the interval rule, in numpy: which branch a site reaches -------------------------------------------------------------------

def bankers(x):   # misc.rs:208-215 for x >= 0
    r = int(np.floor(x))
    f = x - np.floor(x)
    return r if f < 0.5 else (r + 1 if f > 0.5 else r + (r & 1))


def share_units(k, b):
    return ((1 << b) + (k >> 1)) // k


def win_fx_bits(n_items):
    return min(20, 31 - max(int(n_items), 1).bit_length())


def vote_model(c, vthr, ithr, low):
    """(status, winning row) of the vote over the five rows with given thresholds (pileup.rs:67-134, no string keys)."""
    if low:
        return 2, "own"
    tallies = [(r, c[r]) for r in ROWS if r != "del" or c[r] > 0]
    valid = [r for r, t in tallies if t >= vthr]
    mid = [r for r, t in tallies if ithr <= t < vthr]
    if len(valid) == 1:
        return (5, "own") if mid else ((1 if valid[0] != "own" else 0), valid[0])
    return (3 if not valid else 4), "own"


def interval_class(s, b, params):
    """0: all three step functions agree at both ends of the interval (or every share is a multiple of the unit: "exact") |
    1: one differs by a step and the two votes agree | 2: one differs and the votes differ | 3: two or three differ."""
    md, fv, fi = params
    kk = np.asarray(s["k"], np.int64)
    units = np.array([share_units(int(k), b) for k in kk], np.int64)
    if (units * kk == (1 << b)).all():
        return "exact"
    n = len(kk)
    D = float(units.sum()) / float(1 << b)
    eps = n * (0.5 / float(1 << b)) + 1e-9
    lo, hi = max(D - eps, 0.0), D + eps
    v0, v1, i0, i1 = bankers(lo * fv), bankers(hi * fv), bankers(lo * fi), bankers(hi * fi)
    l0, l1 = lo < md, hi < md
    ndiff = (v0 != v1) + (i0 != i1) + (l0 != l1)
    if ndiff != 1 or v1 - v0 > 1 or i1 - i0 > 1:
        return 0 if ndiff == 0 else 3
    c = counts_of(s)
    return 1 if vote_model(c, max(md, v0), i0, l0) == vote_model(c, max(md, v1), i1, l1) else 2


def classify(job):
    """{position: interval_class} of the job's contested sites, each with the unit of its window."""
    b = [win_fx_bits(n) for n in job.items_per_window()]
    return {g: interval_class(s, b[g // ks.WIN], job.params) for g, s in job.contested()}


@functools.lru_cache(maxsize=None)
def shortcut_job(orc, params, seed=0):
    """Family-A sites of the class "one step differs, both votes agree" only (at b = 20): what the shortcut decides by itself."""
    specs = [s for s in order_decided_specs(orc, params, seed, want=14) if interval_class(s, 20, params) == 1]
    return small_job(specs, 8400 + OPTION_SETS.index(params), params)


# ---- the oracle's results, made once and shared -----------------------------------------------------------------------------------

def kw(params):
    return dict(min_depth=params[0], fraction_valid=params[1], fraction_invalid=params[2])


@functools.lru_cache(maxsize=None)
def expected(orc, job, which):
    """The oracle on the job's records in file order `which`: bytes, offsets, changed / zero_depth per contig, the per-position
    records, and the records themselves ("job")."""
    off, bases, recs = job.ordered(which)
    w = orc.polish_records(off, bases, recs, positions=True, **kw(job.params))
    o = [int(x) for x in off]
    st, depth = w["positions"]["status"], w["positions"]["depth"]
    return {"job": (off, bases, recs), "polished": w["polished"], "offsets": w["offsets"],
            "changed": [int((st[o[c]:o[c + 1]] == 1).sum()) for c in range(len(o) - 1)],
            "zero_depth": [int((depth[o[c]:o[c + 1]] == 0.0).sum()) for c in range(len(o) - 1)],
            "positions": w["positions"]}


def bytes_at(want, positions):
    """What each of the positions left in the polished assembly (b"" where it was deleted)."""
    n = want["positions"]["emit_len"].astype(np.int64)
    start = np.cumsum(n) - n
    return [want["polished"][int(start[g]):int(start[g] + n[g])] for g in positions]


def order_differences(orc, job):
    """(sites whose status, sites whose polished byte) the oracle gives differently for the two file orders of the job."""
    w0, w1 = expected(orc, job, 0), expected(orc, job, 1)
    sites = [g for g, _ in job.contested()]
    st = [g for g in sites if w0["positions"]["status"][g] != w1["positions"]["status"][g]]
    by = [g for g, a, b in zip(sites, bytes_at(w0, sites), bytes_at(w1, sites)) if a != b]
    return st, by
