"""Jobs made of SITES: positions of a random assembly where a chosen multiset of reads votes for string keys.

Where the assembly lacks a base every read over the spot votes for a string key (alignment.rs:175-201, pileup.rs:56-63), where
it has one too many for "-".  A site is a position p covered by reads that start at p - 20 and (by default) are 40 bases
of the assembly long, each of one kind:

  plain        40M                    the assembly's own base
  ins b        21M jI 19M             the key ref[p] + b: two bytes for one inserted byte (b may be "-"), longer ones else
  del j        20M jD 19M             "-" at p .. p + j - 1
  sub b        40M                    the byte b (N, say) in place of ref[p]
  slow b       10M 1D 10M 1I 19M      the key ref[p] + b from a read with two indels (and a "-" at p - 10)

The assembly has no homopolymer longer than 3, so the tail trim (alignment.rs:364-378) takes at most four positions off a
read and never reaches p; no two sites' reads overlap (Job.site checks it), so the depth at p is that of the site's own
reads.  Everything is seeded; nothing here needs a GPU.  The oracle (`orc`) is passed in where thresholds are needed: they
are the reference's own, max(min_depth, bankers(depth * fv)) and bankers(depth * fi), never the code's under test."""
import numpy as np

LEAD, TAIL = 20, 19
WIN = 2048           # positions per window of the pileup kernel, counted over the whole assembly
DEFAULT = (5, 0.5, 0.2)  # min_depth, fraction_valid, fraction_invalid
OPTION_SETS = (DEFAULT, (1, 0.6, 0.05), (8, 0.7, 0.3))
KEY2_VARIANTS = ("two_byte", "slow_read", "three_byte", "n_sub")
OPS = "MIDNSHP=X"
_ACGT = np.frombuffer(b"ACGT", np.uint8)


def assembly(rng, n):
    """n random bases without a homopolymer longer than 3 (a base repeats the one before it at most twice in a row)."""
    step = rng.integers(0, 4, n)
    z = step == 0
    third = z.copy()
    third[:2] = False
    third[2:] &= z[1:-1] & z[:-2]
    step[third] = 1 + (np.arange(n)[third] % 3)
    return _ACGT[np.cumsum(step) % 4]


def other_base(b, i=0):
    """One of the three bases that are not b."""
    return [x for x in b"ACGT" if x != b][i % 3]


class Job:
    """An assembly and the reads of its sites.  Positions are counted over the whole assembly (a window is WIN of them)."""

    def __init__(self, contig_lens, seed):
        self.rng = np.random.default_rng(seed)
        self.off = np.concatenate([[0], np.cumsum(contig_lens)]).astype(np.uint64)
        self.bases = assembly(self.rng, int(self.off[-1]))
        for e in self.off[1:]:  # a contig ends in two different bases: its last coverable position is end - 3 (end_site)
            e = int(e)
            if e >= 2 and self.bases[e - 1] == self.bases[e - 2]:
                self.bases[e - 1] = other_base(int(self.bases[e - 2]))
        self.raw = self.bases.tobytes()
        self.taken = np.zeros(len(self.raw), bool)
        self.reads = []   # (contig, start in the contig, k, seq, [(len, op)])
        self.sites = []   # (position, {"n": reads, "keys": {name: count}}) as planned

    def read(self, g, kind, arg=None, lead=LEAD, tail=TAIL):
        """(first position, seq, cigar) of one read over the site g."""
        r, s = self.raw, g - lead
        if kind == "plain":
            return s, r[s:g + 1 + tail], [(lead + 1 + tail, "M")]
        if kind == "ins":
            return s, r[s:g + 1] + arg + r[g + 1:g + 1 + tail], [(lead + 1, "M"), (len(arg), "I"), (tail, "M")]
        if kind == "del":
            return s, r[s:g] + r[g + arg:g + arg + tail], [(lead, "M"), (arg, "D"), (tail, "M")]
        if kind == "sub":
            return s, r[s:g] + arg + r[g + 1:g + 1 + tail], [(lead + 1 + tail, "M")]
        assert kind == "slow" and lead >= 4, kind
        h = lead // 2
        return (s, r[s:s + h] + r[s + h + 1:g + 1] + arg + r[g + 1:g + 1 + tail],
                [(h, "M"), (1, "D"), (lead - h, "M"), (1, "I"), (tail, "M")])

    def site(self, g, reads, lead=LEAD, tail=TAIL, plan=None):
        """reads: (kind, arg, k) each.  The reads' span must lie in one contig and touch no other site's."""
        c = int(np.searchsorted(self.off, g, side="right")) - 1
        lo, hi = int(self.off[c]), int(self.off[c + 1])
        span = max([tail] + [tail + a - 1 for kd, a, _ in reads if kd == "del"])
        assert lo <= g - lead and g + 1 + span <= hi, (g, lead, span, lo, hi)
        assert not self.taken[g - lead:g + 1 + span].any(), ("sites overlap", g)
        self.taken[g - lead:g + 1 + span] = True
        for kind, arg, k in reads:
            s, seq, cig = self.read(g, kind, arg, lead, tail)
            assert len(seq) == sum(l for l, o in cig if o in "MI"), (kind, len(seq), cig)
            self.reads.append((c, s - lo, k, seq, cig))
        self.sites.append((g, plan if plan is not None else {"n": len(reads)}))

    def end_site(self, contig, reads, plan=None):
        """The last position a read can cover in front of the contig's end: the contig ends in two different bases, the
        trim takes both, so it is end - 3, under reads that run to the end."""
        e = int(self.off[contig + 1])
        assert self.raw[e - 1] != self.raw[e - 2]
        self.site(e - 3, reads, lead=min(LEAD, e - 3 - int(self.off[contig])), tail=2, plan=plan)
        return e - 3

    def records(self, seed=0):
        """(contig_off, bases, recs): the reads in a random file order, as the C ABI's arrays."""
        order = np.random.default_rng(seed).permutation(len(self.reads))
        ent = [self.reads[i] for i in order]
        n_cig = np.array([len(e[4]) for e in ent], np.uint32)
        seq_len = np.array([len(e[3]) for e in ent], np.uint32)
        cig = np.array([(l << 4) | OPS.index(o) for e in ent for l, o in e[4]], np.uint32)
        recs = {"contig": np.array([e[0] for e in ent], np.uint32), "ref_start": np.array([e[1] for e in ent], np.uint32),
                "k": np.array([e[2] for e in ent], np.uint32),
                "seq_off": (np.cumsum(seq_len, dtype=np.uint64) - seq_len).astype(np.uint64), "seq_len": seq_len,
                "cig_off": (np.cumsum(n_cig, dtype=np.uint64) - n_cig).astype(np.uint64), "n_cig": n_cig,
                "seq": np.frombuffer(b"".join(e[3] for e in ent), np.uint8), "cigar": cig}
        return self.off, self.bases, recs

    def random_insert(self, j):
        return _ACGT[self.rng.integers(0, 4, j)].tobytes()


# ---- A. thresholds and competition ----------------------------------------------------------------------------------------

def thresholds(orc, depth, params):
    md, fv, fi = params
    return max(md, orc.bankers_rounding(depth * fv)), orc.bankers_rounding(depth * fi)


def compositions(orc, params):
    """(n, key 1, key 2, "-") counts: for every depth n of 5..24, key 1 one below or on the valid threshold, key 2 and "-"
    absent, one below or on the invalid threshold, or on the valid one, whatever fits in n; the assembly's own base gets
    the rest.  With key 1 that near the valid threshold the base is at least intermediate at most depths, so nothing is
    simply kept and little changed.  Two additions to that family: key 1 one below the invalid threshold at depths of
    5..44, alone or with a key 2 or a "-" as rare (kept); and key 1 with the REST, where the assembly's own base is
    absent, one below or on the invalid threshold and key 2 and "-" are absent or one below it (changed, too close)."""
    out = []
    for n in range(5, 25):
        vthr, ithr = thresholds(orc, float(n), params)
        side = sorted({c for c in (0, ithr - 1, ithr, vthr) if c >= 0})
        for c1 in sorted({vthr - 1, vthr}):
            out += [(n, c1, c2, cd) for c2 in side for cd in side if c1 + c2 + cd <= n and c1 + c2 + cd > 0]
        rare = sorted({c for c in (0, ithr - 1) if c >= 0})
        out += [(n, n - own - c2 - cd, c2, cd) for own in sorted({c for c in (0, ithr - 1, ithr) if c >= 0}) for c2 in rare
                for cd in rare if n - own - c2 - cd >= vthr]
    for n in range(5, 45):
        vthr, ithr = thresholds(orc, float(n), params)
        if ithr >= 2:
            out += [(n, ithr - 1, c2, cd) for c2 in (0, ithr - 1) for cd in (0, ithr - 1)]
    return out


def site_reads(job, g, c1, c2, cd, n, variant, ks=None):
    """The reads of one composition.  Key 1 is ref[g] + b1.  Key 2 by variant: a second two-byte key; the SAME key as key 1
    from a slow-class read (then c2 of key 1's c1 reads come that way, c1 stays the key's count); a three-byte key; N in
    place of ref[g].  Returns (reads, planned string-key counts)."""
    ref = job.raw[g]
    b1, b2 = bytes([other_base(ref, g)]), bytes([other_base(ref, g + 1)])
    if variant == "slow_read":
        slow = min(c1, c2)
        kinds = [("ins", b1)] * (c1 - slow) + [("slow", b1)] * slow
        keys = {"key1": c1}
    else:
        second = {"two_byte": ("ins", b2), "three_byte": ("ins", b2 + b1), "n_sub": ("sub", b"N")}[variant]
        kinds = [("ins", b1)] * c1 + [second] * c2
        keys = {"key1": c1, "key2": c2}
    kinds += [("del", 1)] * cd
    keys["-"] = cd
    assert len(kinds) <= n, (n, c1, c2, cd)
    kinds += [("plain", None)] * (n - len(kinds))
    ks = [1] * n if ks is None else ks
    return [(kd, a, int(k)) for (kd, a), k in zip(kinds, ks)], {k: v for k, v in keys.items() if v}


A_CONTIGS = (6144, 2500)
A_SEAMS = (2048, 4096, 8192)   # window starts inside a contig


def _a_places(job, variant_index):
    """Where the sites of an A job go: around the three window seams at window positions 2046, 2047, 0 and 1 (which seam
    gets which turns with the variant: sites are 64 apart, one per seam) -- an insertion after 2047 and a deletion of 2048
    come from reads that start in the window in front --, and every 64 positions elsewhere.  The two contig ends come on
    top (end_site)."""
    special = [s + (-2, -1, 0, 1)[(i + variant_index) % 4] for i, s in enumerate(A_SEAMS)]
    ends = [int(e) - 3 for e in job.off[1:]]
    grid = [g for c in range(len(job.off) - 1) for g in range(int(job.off[c]) + 32, int(job.off[c + 1]) - 64, 64)]
    return special, [g for g in grid if all(abs(g - s) >= 64 for s in special + ends)]


PT_SLOTS = 10   # what k_tile's table of two-byte keys holds per window
SEEDS = {False: (0,), True: (0, 1, 2)}   # the seeds of the dense and of the sparse jobs


class _Table:
    """The (position, two-byte key) pairs per window.  A job that is not sparse has 32 sites in a full window: the table
    overflows and k_exact groups and votes every key.  A sparse job leaves out the sites that no longer fit the table of
    their window, so that k_tile itself votes them (without per-position records)."""

    def __init__(self, sparse):
        self.sparse, self.used = sparse, {}

    def take(self, g, keys, variant):
        n = ("key1" in keys) + ("key2" in keys and variant == "two_byte")
        if self.sparse and self.used.get(g // WIN, 0) + n > PT_SLOTS:
            return False
        self.used[g // WIN] = self.used.get(g // WIN, 0) + n
        return True


def threshold_job(orc, params, variant, seed=0, sparse=False):
    """The composition family at depth shares 1, key 2 of one variant; sparse: see _Table.  Which compositions: a seeded draw without
    replacement; the sites at the window seams and the contig ends have 12 reads: all for key 1 or all for "-" (the
    length changes there), or key 1 on the valid threshold beside a key 2 on the invalid one, or alone one below it, or
    with the rest beside a "-" one below the invalid threshold."""
    vi = KEY2_VARIANTS.index(variant)
    job = Job(A_CONTIGS, 1000 + 100 * seed + 10 * OPTION_SETS.index(params) + vi)
    table = _Table(sparse)
    special, grid = _a_places(job, vi)
    if sparse:
        grid = [grid[i] for i in job.rng.permutation(len(grid))]
    fam = compositions(orc, params)
    fam = [fam[i] for i in job.rng.permutation(len(fam))]
    v12, i12 = thresholds(orc, 12.0, params)
    seam = [(12, 12, 0, 0), (12, 0, 0, 12), (12, v12, i12, 0), (12, v12 - 1, 0, 0), (12, 12 - max(i12 - 1, 0), 0, max(i12 - 1, 0))]
    for j, g in enumerate(special):
        n, c1, c2, cd = seam[(j + vi) % len(seam)]
        reads, keys = site_reads(job, g, c1, c2, cd, n, variant)
        table.take(g, keys, variant)
        job.site(g, reads, plan={"n": n, "keys": keys})
    for c in range(len(job.off) - 1):
        n, c1, c2, cd = seam[(c + vi) % 2]
        reads, keys = site_reads(job, int(job.off[c + 1]) - 3, c1, c2, cd, n, variant)
        table.take(int(job.off[c + 1]) - 3, keys, variant)
        job.end_site(c, reads, plan={"n": n, "keys": keys})
    for g, (n, c1, c2, cd) in zip(grid, fam):
        reads, keys = site_reads(job, g, c1, c2, cd, n, variant)
        if table.take(g, keys, variant):
            job.site(g, reads, plan={"n": n, "keys": keys})
    job.pairs = table.used
    return job


def shares_job(orc, params, seed=0, sparse=False):
    """Every read has k drawn from (1, 2, 3): the depth is a sum of shares in file order.  Both thresholds come from the
    sum in the order of the draw (the file order is another: where they differ the oracle decides, as everywhere).  Every
    eighth site has k = 3 for all of its 15, 30 or 45 reads: 15 thirds add up to 4.999999999999999.  Every sixteenth has two
    reads of k = 3 and nothing else, both for key 1: a depth below 1, too low whatever min_depth is.  sparse: see _Table."""
    job = Job(A_CONTIGS, 2000 + 100 * seed + OPTION_SETS.index(params))
    table = _Table(sparse)
    special, grid = _a_places(job, 0)
    rng = job.rng
    if sparse:
        grid = [grid[i] for i in rng.permutation(len(grid))]
    for j, g in enumerate(special + grid):
        if j % 16 == 4:
            reads, keys = site_reads(job, g, 2, 0, 0, 2, "two_byte", (3, 3))
            if table.take(g, keys, "two_byte"):
                job.site(g, reads, plan={"n": 2, "keys": keys, "k": [3, 3]})
            continue
        if j % 8 == 0:
            n = (15, 30, 45)[(j // 8) % 3]
            ks = np.full(n, 3)
        else:
            n = int(rng.integers(5, 25))
            ks = rng.choice((1, 2, 3), n)
        depth = 0.0
        for k in ks:
            depth += 1.0 / float(k)
        vthr, ithr = thresholds(orc, depth, params)
        side = [c for c in (0, ithr - 1, ithr, vthr) if c >= 0]
        for _ in range(50):
            c1, c2, cd = int(rng.choice((vthr - 1, vthr))), int(rng.choice(side)), int(rng.choice(side))
            if 0 < c1 + c2 + cd <= n:
                break
        else:
            c1, c2, cd = min(n, vthr), 0, 0
        reads, keys = site_reads(job, g, c1, c2, cd, n, "two_byte", ks)
        if table.take(g, keys, "two_byte"):
            job.site(g, reads, plan={"n": n, "keys": keys, "k": [int(k) for k in ks]})
    job.pairs = table.used
    return job


# ---- B. the table's capacity -----------------------------------------------------------------------------------------------

def capacity_job(n_pairs):
    """n_pairs distinct (position, two-byte key) pairs in window 1 of a three-window contig: sites of 16 reads with two keys
    each (the last site has one when n_pairs is odd) at default options -- thresholds 8 and 3.  Key 2 has 2 or 3 reads; key 1
    has 12 at the even sites (it wins where key 2 has 2: the assembly's own base is left with 2; too close where it has 3),
    7 at the odd ones (nothing valid)."""
    job = Job((3 * WIN,), 3000 + n_pairs)
    left, i = n_pairs, 0
    while left:
        g = WIN + 100 + 192 * i
        ref = job.raw[g]
        b1, b2 = bytes([other_base(ref, 0)]), bytes([other_base(ref, 1)])
        c1 = 12 if i % 2 == 0 else 7
        c2 = 0 if left == 1 else (2, 3)[(i // 2) % 2]
        kinds = [("ins", b1)] * c1 + [("ins", b2)] * c2
        kinds += [("plain", None)] * (16 - len(kinds))
        job.site(g, [(kd, a, 1) for kd, a in kinds], plan={"n": 16, "keys": {"key1": c1, "key2": c2}})
        left -= 1 + (c2 > 0)
        i += 1
    return job


def one_position_job():
    """Twelve different inserted bytes, one read each, and 8 plain reads at ONE position: 12 keys where the table has 10
    slots; depth 20, thresholds 10 and 4: nothing is valid."""
    job = Job((3 * WIN,), 3100)
    g = WIN + 700
    kinds = [("ins", bytes([b])) for b in b"ACGTNRYKMSWB"] + [("plain", None)] * 8
    job.site(g, [(kd, a, 1) for kd, a in kinds], plan={"n": 20, "keys": {f"key{i}": 1 for i in range(12)}})
    return job


# ---- C. multi-byte winners and deletions at the emission's seams -----------------------------------------------------------
# Each site: 12 identical reads at default options (thresholds 6 and 2): whatever they say wins.

def winner_reads(job, kind, g):
    ref = job.raw[g]
    what = {"two": lambda: ("ins", bytes([other_base(ref, g)])),   # a two-byte winner: code 0x82
            "del": lambda: ("del", 1),                             # "-" wins: nothing emitted
            "del16": lambda: ("del", 16),                          # ... at sixteen positions in a row
            "ins2": lambda: ("ins", job.random_insert(2)),         # eff 3
            "ins125": lambda: ("ins", job.random_insert(125)),     # eff 126: code 0xFE, the last length a code holds
            "ins126": lambda: ("ins", job.random_insert(126)),     # eff 127: code 0xFF, the length looked up
            "dash": lambda: ("ins", b"-"),                         # the key ref + "-": one byte left, status changed
            }[kind]()
    return [(what[0], what[1], 1)] * 12


def place(job, window, wpos, kind, lead=LEAD, tail=TAIL):
    g = window * WIN + wpos
    job.site(g, winner_reads(job, kind, g), lead=lead, tail=tail, plan={"n": 12, "kind": kind})


def place_end(job, contig, kind):
    job.end_site(contig, winner_reads(job, kind, int(job.off[contig + 1]) - 3), plan={"n": 12, "kind": kind})


def all_deleted_contig(job, contig):
    """A 30-base contig under 12 reads 2M22D6M: every position they cover behind their first two is deleted (a read has to
    begin and end with a match; the trim takes the end)."""
    lo = int(job.off[contig])
    assert int(job.off[contig + 1]) - lo == 30
    s = job.raw[lo:lo + 2] + job.raw[lo + 24:lo + 30]
    job.reads += [(contig, 0, 1, s, [(2, "M"), (22, "D"), (6, "M")])] * 12
    job.taken[lo:lo + 30] = True
    job.sites.append((lo + 2, {"n": 12, "kind": "del22"}))


def seam_job_small():
    """Three windows.  Window positions 0 and 2047, 15 / 16 (a thread of k_emit has 16 positions), 1023 / 1024 (its two waves
    meet there), each under a length-changing winner; every kind of winner; sixteen deleted positions that are one thread's;
    contig 1 (30 bases, all deleted) starts at position 300 of window 2, behind two winners and a deletion of that window;
    contig 2 behind it.  Sites closer than 64 to a neighbour or a contig start have shorter reads."""
    job = Job((2 * WIN + 300, 30, WIN - 330), 4000)
    for w, p, kind, lead, tail in ((0, 16, "ins2", 12, TAIL), (0, 1023, "two", LEAD, TAIL), (0, 1104, "del16", LEAD, TAIL),
                                   (0, 1300, "ins125", LEAD, TAIL), (0, 1500, "dash", LEAD, TAIL), (0, 1700, "ins126", LEAD, TAIL),
                                   (0, 2047, "two", LEAD, 8), (1, 15, "del", 5, TAIL), (1, 1024, "del", LEAD, TAIL),
                                   (1, 1200, "ins2", LEAD, TAIL), (1, 1424, "del16", LEAD, TAIL), (1, 2047, "del", LEAD, 8),
                                   (2, 16, "two", 6, TAIL), (2, 100, "ins2", LEAD, TAIL), (2, 200, "del", LEAD, TAIL),
                                   (2, 1023, "ins126", LEAD, TAIL), (2, 1500, "two", LEAD, TAIL)):
        place(job, w, p, kind, lead, tail)
    all_deleted_contig(job, 1)
    place_end(job, 0, "two")
    place_end(job, 2, "del")
    return job


KINDS = ("two", "del", "ins2", "ins125", "ins126", "dash")


def _seam_windows(job, windows):
    """A length-changing site or three in each of `windows`, at window positions that turn through the seams of k_emit."""
    spots = ((0, 1023, 2047), (15, 1024, 1600), (16, 1023, 2047), (0, 1024, 1700), (15, 900, 2047), (16, 1024, 1800))
    for i, w in enumerate(windows):
        for j, p in enumerate(spots[i % len(spots)]):
            g = w * WIN + p
            c = int(np.searchsorted(job.off, g, side="right")) - 1
            lead = 5 if p in (15, 16) else LEAD
            tail = 8 if p == 2047 else TAIL
            if g - lead < int(job.off[c]) or g + 1 + tail > int(job.off[c + 1]) or job.taken[g - lead:g + 1 + tail].any():
                continue  # (no room between a contig's start or end and the seam: the sites around it stay)
            place(job, w, p, KINDS[(i + j + i // len(spots)) % len(KINDS)], lead, tail)


def seam_job_coarse():
    """66 windows: the sums in front of a window change level at window 64.  Contigs start at position 5 of window 63 and
    position 10 of window 64; contig 0 ends under a two-byte winner at position 2 of window 63 -- in front of contig 1's
    start in that window; length-changing sites in windows 0, 62, 63, 64 and 65, and windows 1..43 hold every kind of
    winner at every seam position."""
    job = Job((63 * WIN + 5, WIN + 5, 2 * WIN - 10), 4100)
    place_end(job, 0, "two")
    place_end(job, 1, "del")
    _seam_windows(job, (0, 62, 63, 64, 65) + tuple(range(1, 44)))
    return job


BIG_CONTIGS = (63 * WIN + 5, WIN + 5, 4031 * WIN - 7, 3 * WIN - 3)


def seam_job_big():
    """4,098 windows: the second level of sums (4,096 windows each) has one full group in front of windows 4096 and 4097.
    Contig starts inside windows 63, 64 and 4095; sites in windows 0, 62..65 and 4094..4097."""
    job = Job(BIG_CONTIGS, 4200)
    for c, kind in ((0, "two"), (1, "del"), (2, "ins2")):
        place_end(job, c, kind)
    _seam_windows(job, (0, 62, 63, 64, 65, 4094, 4095, 4096, 4097))
    return job


# ---- D. more two-byte winners than a fresh context has room for ---------------------------------------------------------------

def many_winners_job(n_sites=65_600, apart=48):
    """n_sites sites `apart` positions apart, three reads each with the same inserted base: at min_depth 1 the depth is 3, the
    thresholds 2 and 1, every site a two-byte winner."""
    job = Job((n_sites * apart + 64,), 5000)
    raw = job.raw
    for i in range(n_sites):
        g = 24 + i * apart
        ref = raw[g]
        b = bytes([ref ^ 6 if ref in b"AG" else ref ^ 23])  # A <-> G, C <-> T: another base
        seq = raw[g - LEAD:g + 1] + b + raw[g + 1:g + 1 + TAIL]
        job.reads += [(0, g - LEAD, 1, seq, [(LEAD + 1, "M"), (1, "I"), (TAIL, "M")])] * 3
    job.sites = [(24 + i * apart, {"n": 3}) for i in range(n_sites)]
    return job
