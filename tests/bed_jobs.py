"""Hand-built polish jobs for the BED and soft-mask tests, on top of vcf_jobs.reads: a job is made of up to five record SETS, each the
reads of vcf_jobs.reads with copies=1 over the same stretches, concatenated.  A position names a MIX of keys, one per set, so that with
min_depth 1 its status is fixed by construction (pileup.rs:67-134; the tiles of a set overlap by half a read, so every count below is
the same small multiple of the mix -- thresholds are fractions of the depth, only the ratios matter):
    all sets alike             kept (the assembly's base) or changed (another base, b"-", an insertion); three sets at least: at a
                               depth of 3 and more the invalid threshold is at least 1, so a base no read carries is not "too close"
    2 + 2 sets of two bases    multiple      (a stretch covered by four sets)
    1 + 1 + 1 of three bases   none          (three sets)
    4 + 1 of two bases         too_close     (five sets)
    an uncovered stretch       low_depth     (`cover`; also what the homopolymer trim leaves behind a stretch's last read, and a contig
                                             too short for a read)
A stretch is covered by the first n sets over the very same interval, so their tiles coincide.  Positions with a mix keep clear of the
tiles' ends (place() asserts it): a read whose last bases differ between the sets would be trimmed differently.
job(T) lays three contigs of T + 37, 1 and 2T - 5 positions out around the boundaries of the position passes' workgroups (T positions);
`which` chooses the three statuses whose runs cross them.  check_oracle_made() asserts that the oracle reports exactly the built
statuses."""
import numpy as np

import vcf_jobs as vj

KEPT, CHANGED, LOW_DEPTH, NONE, MULTIPLE, TOO_CLOSE = range(6)
READ, STEP = 100, 50  # vcf_jobs.reads: read length and the tiles' step
N_SETS = {KEPT: 3, CHANGED: 3, MULTIPLE: 4, NONE: 3, TOO_CLOSE: 5}  # (a depth of 3 and more: the invalid threshold is at least 1)


def mix(status, base):
    """the key each of the stretch's sets carries at a position of this status"""
    o1, o2 = vj.other(base, 1), vj.other(base, 2)
    return {MULTIPLE: [o1, o1, o2, o2], NONE: [bytes([base]), o1, o2], TOO_CLOSE: [o1, o1, o1, o1, o2]}[status]


class Layout:
    def __init__(self, lens, seed):
        self.off, self.bases = vj.assembly(lens, seed)
        self.G = int(self.off[-1])
        self.cover = [[] for _ in range(5)]  # per set: the stretches it tiles
        self.spec = [dict() for _ in range(5)]
        self.want = {}  # position -> the status it is built to have (covered positions without an entry: kept)

    def stretch(self, lo, hi, n):
        """[lo, hi), inside one contig, tiled by the first n sets"""
        for k in range(n):
            self.cover[k].append((lo, hi))
        return lo

    def place(self, lo, hi, status, stretch_lo, n, key=None):
        """positions [lo, hi) get `status` inside the stretch that begins at stretch_lo and is tiled by n sets"""
        for p in range(lo, hi):
            assert 2 <= (p - stretch_lo) % STEP <= STEP - 6, ("a mix next to a tile's end", p, stretch_lo)
            b = int(self.bases[p])
            keys = [key(b)] * n if status == CHANGED else mix(status, b)
            assert len(keys) == n or status == CHANGED
            for k in range(n):
                self.spec[k][p] = keys[k]
            self.want[p] = status

    def records(self):
        sets = [vj.reads(self.off, self.bases, self.spec[k], read_len=READ, copies=1, cover=sorted(self.cover[k])) for k in range(5) if self.cover[k]]
        out = {}
        seq_at = np.cumsum([0] + [len(s["seq"]) for s in sets])
        cig_at = np.cumsum([0] + [len(s["cigar"]) for s in sets])
        for f in ("contig", "ref_start", "seq_len", "n_cig", "k", "seq", "cigar"):
            out[f] = np.concatenate([s[f] for s in sets])
        out["seq_off"] = np.concatenate([s["seq_off"] + np.uint64(seq_at[i]) for i, s in enumerate(sets)])
        out["cig_off"] = np.concatenate([s["cig_off"] + np.uint64(cig_at[i]) for i, s in enumerate(sets)])
        return out, sets[0]

    def status(self, set0):
        """the built statuses: low_depth where set 0 (it tiles every stretch) leaves a position uncovered -- a read covers its
        reference span but for its trailing homopolymer and one base more (alignment.rs:364-378; every read here ends in plain bases)"""
        depth = np.zeros(self.G, np.int64)
        for i in range(len(set0["contig"])):
            s = set0["seq"][int(set0["seq_off"][i]):int(set0["seq_off"][i]) + int(set0["seq_len"][i])]
            run = 1
            while run < len(s) and s[-1 - run] == s[-1]:
                run += 1
            cig = set0["cigar"][int(set0["cig_off"][i]):int(set0["cig_off"][i]) + int(set0["n_cig"][i])]
            assert int(cig[-1]) & 15 == vj.OP_M and int(cig[-1]) >> 4 > run + 1
            span = sum(int(c) >> 4 for c in cig if int(c) & 15 in (vj.OP_M, vj.OP_D))
            a = int(self.off[int(set0["contig"][i])]) + int(set0["ref_start"][i])
            depth[a:a + span - (run + 1)] += 1
        st = np.full(self.G, KEPT, np.uint8)
        st[depth == 0] = LOW_DEPTH
        for p, s in self.want.items():
            assert depth[p] > 0, ("a placed position is covered", p)
            st[p] = s
        return st


def job(T, which=0, seed=31):
    """{"off", "bases", "recs", "status", "names"}: three contigs of T + 37, 1 and 2T - 5 positions.  The runs that cross the workgroup
    boundaries T, 2T and 3T: which=0 multiple, none, too_close; which=1 low_depth, changed, kept"""
    assert T >= 2048, "the stretches below are laid out for workgroups of 2048 positions and more"
    L = Layout([T + 37, 1, 2 * T - 5], seed)
    c2 = T + 38  # contig 3 begins here
    sub = lambda b: vj.other(b, 3)  # noqa: E731
    ins = lambda b: bytes([b]) + vj.other(b, 2)  # noqa: E731
    dele = lambda b: b"-"  # noqa: E731
    # insertions and deletions in front of everything else, so that output offsets differ from positions at every boundary
    s = L.stretch(40, 400, 3)
    L.place(s + 60, s + 63, CHANGED, s, 3, ins)    # +3 bytes
    L.place(s + 110, s + 111, CHANGED, s, 3, dele)  # -1
    L.place(s + 160, s + 162, CHANGED, s, 3, sub)
    s = L.stretch(c2 + 12, c2 + 412, 3)
    L.place(s + 55, s + 60, CHANGED, s, 3, dele)   # -5
    L.place(s + 105, s + 106, CHANGED, s, 3, ins)
    if which == 0:
        s = L.stretch(T - 125, T + 37, 4)            # ... to the contig's end: its last positions are low_depth
        L.place(T - 10, T + 10, MULTIPLE, s, 4)
        L.place(T - 19, T - 10, CHANGED, s, 4, sub)  # two different statuses side by side
        L.place(T - 70, T - 69, CHANGED, s, 4, ins)
        s = L.stretch(2 * T - 125, 2 * T + 125, 3)
        L.place(2 * T - 8, 2 * T + 15, NONE, s, 3)
        L.place(2 * T - 70, 2 * T - 68, CHANGED, s, 3, dele)
        s = L.stretch(3 * T - 125, 3 * T + 33, 5)
        L.place(3 * T - 1, 3 * T + 1, TOO_CLOSE, s, 5)
        L.place(3 * T - 18, 3 * T - 12, TOO_CLOSE, s, 5)
        L.place(3 * T - 12, 3 * T - 9, CHANGED, s, 5, sub)
        # one more of each away from the boundaries, a run of one position among them
        s = L.stretch(c2 + 600, c2 + 900, 5)
        L.place(s + 105, s + 106, TOO_CLOSE, s, 5)
        s = L.stretch(c2 + 1000, c2 + 1300, 3)
        L.place(s + 152, s + 190, NONE, s, 3)
        L.place(s + 210, s + 211, CHANGED, s, 3, ins)
    else:
        L.stretch(T - 300, T - 12, 3)                # low_depth from its trimmed end across T ...
        L.stretch(T + 6, T + 37, 3)                  # ... to here
        s = L.stretch(2 * T - 125, 2 * T + 125, 3)
        L.place(2 * T - 15, 2 * T + 15, CHANGED, s, 3, sub)
        L.stretch(3 * T - 125, 3 * T + 33, 3)        # kept across 3T
        s = L.stretch(c2 + 600, c2 + 900, 4)
        L.place(s + 104, s + 130, MULTIPLE, s, 4)
        L.place(s + 130, s + 140, CHANGED, s, 4, dele)
        s = L.stretch(c2 + 1000, c2 + 1300, 5)
        L.place(s + 152, s + 190, TOO_CLOSE, s, 5)
        s = L.stretch(c2 + 1400, c2 + 1700, 3)
        L.place(s + 60, s + 61, NONE, s, 3)
    recs, set0 = L.records()
    return {"off": L.off, "bases": L.bases, "recs": recs, "status": L.status(set0), "names": [b"contig_1", b"one", b"the third contig"]}


def check_oracle_made(job, res):
    """the job is what it was built to be: the oracle reports exactly the built statuses"""
    got, want = res["positions"]["status"], job["status"]
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, [(int(p), int(got[p]), int(want[p])) for p in bad[:12]]
