"""A plain model of the paired-read filter between loading and writing, on the arrays of pp_filter_input (seam A of
include/polypolish_hip.h), for tests: Python ints in plain loops, no wrap-around except where the reference has one.
Written from the reference's behaviour (src/filter.rs, src/alignment.rs; file:line cited at each step) and pinned to the
oracle by tests/test_filter_model_cpu.py.  Also here: a seeded input generator with explicit knobs, a writer that turns an
input into two SAM texts, and the ONE table of generator configurations (SEAM_CASES, TEXT_CASES) that the CPU pin and the GPU tests share.

An input is a dict: n_reads, files = [f1, f2]; a file is a dict of numpy arrays named as pp_filter_file names them
(ref_id, ref_start, flags, cig_off, n_cig, cigar, read, grp_off, grp_idx).  The alignments of read r in file f are
grp_idx[grp_off[r] : grp_off[r + 1]], in file order (the order of the reference's Vec, src/filter.rs:136)."""
import numpy as np

OPS = "MIDNSHP=X"                       # PP_OP_M .. PP_OP_X = 0 .. 8
CONSUMES_REF = (0, 2, 3, 7, 8)          # M D N = X (src/alignment.rs:144)
OP_UNPARSEABLE = 15                     # PP_OP_UNPARSEABLE: a run length that does not fit 64 bits
END_UNPARSEABLE = 0xFFFFFFFFFFFFFFFF    # PP_REF_END_UNPARSEABLE
UNPARSEABLE_TEXT = "99999999999999999999M"  # 20 digits: above 2^64 - 1, `parse::<usize>().unwrap()` panics (alignment.rs:141)
ORIENTATIONS = ("fr", "rf", "ff", "rr")
NOT_SAMPLED = 255
MAX_RUN = (1 << 28) - 1                 # a packed run holds 28 bits of length

MSG_NO_PAIRS = "no one-alignment-per-read pairs available to determine orientation and insert size thresholds"
MSG_TIE = "could not automatically determine read pair orientation"
MSG_NO_SIZES = "no read pairs available to determine insert size thresholds"
MSG_LOW = "--low must be greater than 0 and less than 50"
MSG_HIGH = "--high must be greater than 50 and less than 100"


class Panic(Exception):
    """The reference would panic (exit code 101)."""


class Quit(Exception):
    """The reference would quit_with_error (exit code 1) with this message."""

    def __init__(self, msg):
        super().__init__(msg)
        self.msg = msg


# ---- the reference's functions ------------------------------------------------------------------------------------------

def ref_end_of(start, runs):
    """Alignment::get_ref_end (src/alignment.rs:138-149): None where a run length cannot be parsed."""
    end = int(start)
    for op in runs:
        o = int(op) & 15
        if o == OP_UNPARSEABLE:
            return None
        if o in CONSUMES_REF:
            end += int(op) >> 4
    return end


def ends_of(f):
    """get_ref_end of every alignment of a file, as a list of Python ints (None: unparseable).  A file that brings a
    precomputed `ref_end` array is taken at its word."""
    if "ref_end" in f and "cigar" not in f:
        return [None if e == END_UNPARSEABLE else e for e in f["ref_end"].tolist()]
    start, off, cnt, runs = f["ref_start"].tolist(), f["cig_off"].tolist(), f["n_cig"].tolist(), f["cigar"].tolist()
    return [ref_end_of(start[a], runs[off[a]:off[a] + cnt[a]]) for a in range(len(start))]


def ends_array(f):
    """ends_of as the uint64 array of pp_filter_file.ref_end."""
    return np.array([END_UNPARSEABLE if e is None else e for e in ends_of(f)], dtype=np.uint64)


def orientation_of(fl1, s1, e1, fl2, s2, e2):
    """get_orientation (src/filter.rs:189-209) -> 0 fr, 1 rf, 2 ff, 3 rr.  Not symmetric in its arguments."""
    f1, f2 = (fl1 & 16) == 0, (fl2 & 16) == 0
    p1 = s1 if f1 else e1                      # the read's start: the alignment's end on the reverse strand
    p2 = s2 if f2 else e2
    if f1 != f2:
        first_is_forward = f1 if p1 < p2 else f2   # "{s1}{s2}" if p1 < p2, else "{s2}{s1}"
        return 0 if first_is_forward else 1
    if f1:
        return 2 if p1 < p2 else 3
    return 2 if p2 < p1 else 3


def insert_of(s1, e1, s2, e2):
    """get_insert_size (src/filter.rs:212-218): usize difference, then `as u32`."""
    return (max(s1, e1, s2, e2) - min(s1, e1, s2, e2)) & 0xFFFFFFFF


def percentile(sorted_list, p):
    """get_percentile (src/filter.rs:249-259), nearest rank."""
    if not sorted_list:
        return 0
    rank = max(int(np.ceil(np.float64(p) / np.float64(100.0) * np.float64(len(sorted_list)))), 1)
    return sorted_list[rank - 1] if rank - 1 < len(sorted_list) else 0


def _groups(f, n_reads):
    off, idx = f["grp_off"].tolist(), f["grp_idx"].tolist()
    return [idx[off[r]:off[r + 1]] for r in range(n_reads)]


class _View:
    """A file's fields as Python lists."""

    def __init__(self, f, n_reads):
        self.ref, self.start, self.flags = f["ref_id"].tolist(), f["ref_start"].tolist(), f["flags"].tolist()
        self.end = ends_of(f)
        self.groups = _groups(f, n_reads)
        self.n = len(self.ref)


def samples(inp):
    """The sampling loop of get_insert_size_thresholds (src/filter.rs:155-167): for every read with exactly one alignment in
    each file on the same reference, orientation and insert size; 255 / 0 for every other read.  Returns (orient uint8,
    insert uint32, panicked): panicked = the loop needs an end that cannot be parsed (the values are then void)."""
    n = inp["n_reads"]
    v1, v2 = _View(inp["files"][0], n), _View(inp["files"][1], n)
    orient, insert, panicked = np.full(n, NOT_SAMPLED, np.uint8), np.zeros(n, np.uint32), False
    for r in range(n):
        g1, g2 = v1.groups[r], v2.groups[r]
        if len(g1) != 1 or len(g2) != 1:
            continue
        a, b = g1[0], g2[0]
        if v1.ref[a] != v2.ref[b]:
            continue
        if v1.end[a] is None or v2.end[b] is None:   # get_insert_size parses both ends
            panicked = True
            continue
        orient[r] = orientation_of(v1.flags[a], v1.start[a], v1.end[a], v2.flags[b], v2.start[b], v2.end[b])
        insert[r] = insert_of(v1.start[a], v1.end[a], v2.start[b], v2.end[b])
    return orient, insert, panicked


def _pass_qc(me, a, n_this, other, mates, low, high, correct):
    """alignment_pass_qc (src/filter.rs:352-377) -> (verdict, panicked)."""
    if not mates or n_this == 1:
        return 1, False
    for b in mates:
        # get_insert_size comes first in the loop body and parses both ends, whatever the references are
        if me.end[a] is None or other.end[b] is None:
            return 0, True
        ins = insert_of(me.start[a], me.end[a], other.start[b], other.end[b])
        o = orientation_of(me.flags[a], me.start[a], me.end[a], other.flags[b], other.start[b], other.end[b])
        if me.ref[a] == other.ref[b] and low <= ins <= high and o == correct:
            return 1, False          # the mates behind this one are not looked at
    return 0, False


def verdicts(inp, low, high, correct):
    """alignment_pass_qc for every alignment of both files -> (pass1, pass2, panicked).  An alignment that is in no read's
    group passes, as one without mates does."""
    n = inp["n_reads"]
    v = [_View(inp["files"][0], n), _View(inp["files"][1], n)]
    out, panicked = [np.ones(v[0].n, np.uint8), np.ones(v[1].n, np.uint8)], False
    for f in range(2):
        me, other = v[f], v[1 - f]
        for r in range(n):
            mine, mates = me.groups[r], other.groups[r]
            if len(mine) <= 1 or not mates:
                continue
            for a in mine:
                ok, p = _pass_qc(me, a, len(mine), other, mates, low, high, correct)
                out[f][a] = ok
                panicked = panicked or p
    return out[0], out[1], panicked


def listed_reads(inp):
    """The reads whose verdicts need the thresholds: several alignments in one file and at least one in the other."""
    n1, n2 = np.diff(inp["files"][0]["grp_off"].astype(np.int64)), np.diff(inp["files"][1]["grp_off"].astype(np.int64))
    return ((n1 > 1) & (n2 > 0)) | ((n2 > 1) & (n1 > 0))


def thresholds(orient, insert, orientation, low_p, high_p):
    """The rest of get_insert_size_thresholds (src/filter.rs:168-186) with determine_correct_orientation and
    auto_determine_orientation (src/filter.rs:221-246) -> (counts, correct, low, high), or Quit."""
    counts = [int((orient == o).sum()) for o in range(4)]
    if sum(counts) == 0:
        raise Quit(MSG_NO_PAIRS)
    if orientation == "auto":
        best = [o for o in range(4) if counts[o] == max(counts)]
        if len(best) != 1:
            raise Quit(MSG_TIE)
        correct = best[0]
    else:
        correct = ORIENTATIONS.index(orientation)
    sizes = sorted(insert[orient == correct].tolist())
    if not sizes:
        raise Quit(MSG_NO_SIZES)
    return counts, correct, percentile(sizes, low_p), percentile(sizes, high_p)


def command(inp, orientation="auto", low_p=0.1, high_p=99.9):
    """filter::filter (src/filter.rs:26-37) on a loaded input: a dict with the report's figures and both verdict arrays,
    or Quit / Panic as the reference would end."""
    if low_p <= 0.0 or low_p >= 50.0:
        raise Quit(MSG_LOW)
    if high_p <= 50.0 or high_p >= 100.0:
        raise Quit(MSG_HIGH)
    n_aln = [len(f["ref_id"]) for f in inp["files"]]
    if n_aln[0] == 0:                       # load_alignments_one_file, src/filter.rs:141-143: the map is still empty
        raise Quit("no alignments found in file 1")
    orient, insert, panicked = samples(inp)
    if panicked:
        raise Panic("sampling loop")
    counts, correct, low, high = thresholds(orient, insert, orientation, low_p, high_p)
    p1, p2, panicked = verdicts(inp, low, high, correct)
    if panicked:
        raise Panic("pair comparison")
    return {"before": n_aln[0] + n_aln[1], "after": int(p1.sum()) + int(p2.sum()), "low": low, "high": high,
            "orientation": ORIENTATIONS[correct], "counts": counts, "pass": (p1, p2)}


# ---- inputs -------------------------------------------------------------------------------------------------------------

def file_from_groups(read, ref_id, ref_start, flags, runs, n_reads):
    """A file from per-alignment lists in file order; `runs` is a list of run lists (packed length << 4 | op)."""
    n = len(read)
    read = np.asarray(read, dtype=np.uint32).reshape(n)
    cnt = np.bincount(read, minlength=n_reads) if n else np.zeros(n_reads, np.int64)
    n_cig = np.array([len(x) for x in runs], dtype=np.uint32).reshape(n)
    return {
        "ref_id": np.asarray(ref_id, dtype=np.uint32).reshape(n), "ref_start": np.asarray(ref_start, dtype=np.uint32).reshape(n),
        "flags": np.asarray(flags, dtype=np.uint32).reshape(n),
        "cig_off": np.concatenate([[0], np.cumsum(n_cig)[:-1]]).astype(np.uint64) if n else np.zeros(0, np.uint64),
        "n_cig": n_cig, "cigar": np.array([x for rr in runs for x in rr], dtype=np.uint32), "read": read,
        "grp_off": np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32),
        "grp_idx": np.argsort(read, kind="stable").astype(np.uint32)}


# where the listed reads sit, by read number (the kernel's constants: 64 lanes, 256 threads, two reads a lane, 512 reads a
# workgroup -- a lane's first read is r % 512 < 256, its second r % 512 >= 256)
def _listed_mask(where, n):
    r = np.arange(n)
    return {"none": r < 0, "all": r >= 0, "last": r == n - 1, "lane0": r % 64 == 0, "lane63": r % 64 == 63,
            "first_half": r % 512 < 256, "second_half": r % 512 >= 256,
            "one_in_last_wg": r == (n - 1) // 512 * 512 + ((n - 1) % 512) // 2}[where]


LISTED_COUNTS = ((2, 1), (1, 2), (2, 2), (3, 1), (1, 3), (2, 3))
UNLISTED_COUNTS = ((1, 1), (1, 1), (1, 1), (1, 0), (0, 1), (0, 0), (3, 0), (0, 2))


def generate(seed, n_reads, cnt=((0, 1, 1, 1, 2, 3), (0, 1, 1, 1, 2, 3)), listed=None, n_contigs=2, p_reverse=0.5,
             pos_range=5000, max_runs=3, max_len=120, ops=(0, 0, 1, 2, 4, 7, 8), p_norun=0.0, unparseable=None,
             p_unparseable=0.02, extra_flags=True, shuffle=True):
    """A seeded input.  Knobs:
    cnt          per file, the values a read's alignment count is drawn from (ignored when `listed` is given)
    listed       None, or where the reads with several alignments here and some there sit (_listed_mask); every other read
                 then gets counts that need no thresholds
    n_contigs, p_reverse, pos_range      references, strands, start positions (a small range makes equal positions common)
    max_runs, max_len, ops, p_norun      run shapes: 1..max_runs runs of 1..max_len, op codes drawn from `ops`; an alignment
                                         has no run at all with probability p_norun
    unparseable  None; "safe": op 15 only in alignments nobody compares; "any": anywhere (the model says what happens)
    shuffle      file order differs from group order (the reads' alignments are spread over the file)"""
    rng = np.random.default_rng(seed)
    if listed is None:
        c = [rng.choice(np.asarray(cnt[f]), n_reads) if n_reads else np.zeros(0, np.int64) for f in range(2)]
    else:
        m = _listed_mask(listed, n_reads)
        lc, uc = np.asarray(LISTED_COUNTS), np.asarray(UNLISTED_COUNTS)
        pick = np.where(m[:, None], lc[rng.integers(0, len(lc), n_reads)], uc[rng.integers(0, len(uc), n_reads)])
        c = [pick[:, 0], pick[:, 1]]
    files = []
    for f in range(2):
        n = int(c[f].sum())
        read = np.repeat(np.arange(n_reads, dtype=np.uint32), c[f])
        if shuffle:
            read = rng.permutation(read)
        n_cig = rng.integers(1, max_runs + 1, n)
        n_cig[rng.random(n) < p_norun] = 0
        total = int(n_cig.sum())
        cigar = (rng.integers(1, max_len + 1, total).astype(np.uint32) << 4) | rng.choice(np.asarray(ops, np.uint32), total)
        flags = np.where(rng.random(n) < p_reverse, 16, 0).astype(np.uint32)
        if extra_flags:  # bits that must not matter: paired, first/second in pair, secondary, supplementary
            flags |= rng.choice(np.asarray([0, 0, 1, 65, 129, 256, 2048], np.uint32), n)
        files.append({
            "ref_id": rng.integers(0, n_contigs, n).astype(np.uint32), "ref_start": rng.integers(0, pos_range, n).astype(np.uint32),
            "flags": flags, "cig_off": (np.cumsum(n_cig) - n_cig).astype(np.uint64), "n_cig": n_cig.astype(np.uint32),
            "cigar": cigar.astype(np.uint32), "read": read.astype(np.uint32),
            "grp_off": np.concatenate([[0], np.cumsum(c[f])]).astype(np.uint32),
            "grp_idx": np.argsort(read, kind="stable").astype(np.uint32)})
    inp = {"n_reads": int(n_reads), "files": files}
    if unparseable:
        _plant_unparseable(inp, rng, unparseable, p_unparseable)
    return inp


def compared(inp):
    """Per file, which alignments take part in some comparison whatever the thresholds are (as `a` of alignment_pass_qc, as
    the first mate of one, or in the sampling loop); the mates behind the first may or may not be reached."""
    n = inp["n_reads"]
    g = [_groups(inp["files"][0], n), _groups(inp["files"][1], n)]
    ref = [inp["files"][0]["ref_id"].tolist(), inp["files"][1]["ref_id"].tolist()]
    out = [np.zeros(len(ref[0]), bool), np.zeros(len(ref[1]), bool)]
    for r in range(n):
        a, b = g[0][r], g[1][r]
        if len(a) == 1 and len(b) == 1:
            if ref[0][a[0]] == ref[1][b[0]]:
                out[0][a[0]] = out[1][b[0]] = True
        elif a and b:               # one side has several: all of them are `a`, all of the other side may be mates
            out[0][a] = True
            out[1][b] = True
    return out


def _plant_unparseable(inp, rng, mode, p):
    cmp_ = compared(inp)
    for f in range(2):
        d = inp["files"][f]
        n = len(d["ref_id"])
        hit = (rng.random(n) < p) & (d["n_cig"] > 0)
        if mode == "safe":
            hit &= ~cmp_[f]
        for a in np.flatnonzero(hit):
            d["cigar"][int(d["cig_off"][a]) + int(rng.integers(0, d["n_cig"][a]))] = OP_UNPARSEABLE
    return inp


def with_ref_end(inp):
    """The same input in its precomputed-ends form (what the device loader hands over): no CIGAR arrays."""
    files = []
    for f in inp["files"]:
        g = {k: v for k, v in f.items() if k not in ("cig_off", "n_cig", "cigar")}
        g["ref_end"] = ends_array(f)
        files.append(g)
    return {"n_reads": inp["n_reads"], "files": files}


def concat(inputs):
    """Several inputs as one: the reads of each follow those of the one before, each file's alignments likewise."""
    n_reads, files = 0, []
    for f in range(2):
        parts = [i["files"][f] for i in inputs]
        n_run = np.cumsum([0] + [len(p["cigar"]) for p in parts])
        n_rd = np.cumsum([0] + [i["n_reads"] for i in inputs])
        cat = lambda k, dt, add=None: np.concatenate(  # noqa: E731
            [p[k].astype(np.int64) + (0 if add is None else int(add[j])) for j, p in enumerate(parts)]).astype(dt)
        read = cat("read", np.uint32, n_rd)
        cnt = np.bincount(read, minlength=int(n_rd[-1])) if len(read) else np.zeros(int(n_rd[-1]), np.int64)
        files.append({"ref_id": cat("ref_id", np.uint32), "ref_start": cat("ref_start", np.uint32), "flags": cat("flags", np.uint32),
                      "cig_off": cat("cig_off", np.uint64, n_run), "n_cig": cat("n_cig", np.uint32), "cigar": cat("cigar", np.uint32),
                      "read": read, "grp_off": np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32),
                      "grp_idx": np.argsort(read, kind="stable").astype(np.uint32)})
        n_reads = int(n_rd[-1])
    return {"n_reads": n_reads, "files": files}


def hand_built(reads):
    """An input from a list of reads, each a pair (alignments in file 1, alignments in file 2); an alignment is
    (ref_id, ref_start, flags, [(length, op), ...])."""
    files = []
    for f in range(2):
        rows = [(r, al) for r, rd in enumerate(reads) for al in rd[f]]
        files.append(file_from_groups([r for r, _ in rows], [al[0] for _, al in rows], [al[1] for _, al in rows],
                                      [al[2] for _, al in rows],
                                      [[(OP_UNPARSEABLE if o == OP_UNPARSEABLE else (ln << 4) | o) for ln, o in al[3]] for _, al in rows],
                                      len(reads)))
    return {"n_reads": len(reads), "files": files}


def canonical(inp):
    """The same alignments with the reads numbered as a loader numbers them: by first appearance, file 1 then file 2; reads
    without any alignment do not exist.  (Verdicts are per alignment, in file order: they do not change.)"""
    seen = np.concatenate([inp["files"][0]["read"], inp["files"][1]["read"]]).astype(np.int64)
    uniq, first = np.unique(seen, return_index=True)
    new = np.full(inp["n_reads"] + 1, -1, np.int64)
    new[uniq[np.argsort(first)]] = np.arange(len(uniq))
    files = []
    for f in inp["files"]:
        g = dict(f)
        g["read"] = new[f["read"].astype(np.int64)].astype(np.uint32)
        cnt = np.bincount(g["read"], minlength=len(uniq)) if len(g["read"]) else np.zeros(len(uniq), np.int64)
        g["grp_off"] = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
        g["grp_idx"] = np.argsort(g["read"], kind="stable").astype(np.uint32)
        files.append(g)
    return {"n_reads": int(len(uniq)), "files": files}


# ---- SAM text -----------------------------------------------------------------------------------------------------------

def cigar_text(runs):
    if not len(runs):
        return "*"
    out = []
    for op in runs:
        op = int(op)
        if op & 15 == OP_UNPARSEABLE:
            return UNPARSEABLE_TEXT   # (the loader marks the whole alignment; the reference panics at this run)
        out.append(f"{op >> 4}{OPS[op & 15]}")
    return "".join(out)


def default_read_name(r):
    return f"read{r}"


def default_ref_name(c):
    return f"contig_{c}"


def sam_texts(inp, read_name=default_read_name, ref_name=default_ref_name, header=True):
    """Two SAM texts (bytes) of an input: 11 columns, POS = ref_start + 1, CIGAR from the runs."""
    texts = []
    refs = sorted({int(c) for f in inp["files"] for c in f["ref_id"]})
    for f in inp["files"]:
        lines = ["@HD\tVN:1.6"] + [f"@SQ\tSN:{ref_name(c)}\tLN:4000000000" for c in refs] if header else []
        rd, ref, start, flags = f["read"].tolist(), f["ref_id"].tolist(), f["ref_start"].tolist(), f["flags"].tolist()
        off, cnt, runs = f["cig_off"].tolist(), f["n_cig"].tolist(), f["cigar"].tolist()
        for a in range(len(rd)):
            lines.append(f"{read_name(rd[a])}\t{flags[a]}\t{ref_name(ref[a])}\t{start[a] + 1}\t60\t"
                         f"{cigar_text(runs[off[a]:off[a] + cnt[a]])}\t*\t0\t0\t*\t*")
        texts.append(("\n".join(lines) + "\n").encode() if lines else b"")
    return texts


def write_sams(inp, directory, **kw):
    import os
    paths = [os.path.join(str(directory), n) for n in ("in_1.sam", "in_2.sam")]
    for p, t in zip(paths, sam_texts(inp, **kw)):
        with open(p, "wb") as fh:
            fh.write(t)
    return paths


def failed_lines(text):
    """Per aligned record of a filtered SAM text (bytes), in file order: 0 where the line ends in the ZP:Z:fail tag."""
    out = []
    for line in text.split(b"\n"):
        if not line or line.startswith(b"@"):
            continue
        col = line.split(b"\t")
        if int(col[1]) & 4:
            continue
        out.append(0 if col[-1] == b"ZP:Z:fail" and len(col) > 11 else 1)
    return np.array(out, dtype=np.uint8)


def make_pairs(seed, n, orientation, insert_lo, insert_hi, read_len=100, n_contigs=1, pos_range=1_000_000):
    """n reads with one alignment in each file on the same reference, built to have the given orientation (0..3) and an
    insert size drawn from [insert_lo, insert_hi) (at least 3 * read_len)."""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, pos_range, n)
    ins = rng.integers(insert_lo, insert_hi, n)
    far = s + ins - read_len
    # (file 1 start, file 1 flags, file 2 start, file 2 flags); the read start of a reverse alignment is its end
    s1, f1, s2, f2 = {0: (s, 0, far, 16), 1: (s, 16, far, 0), 2: (s, 0, far, 0), 3: (far, 0, s, 0)}[orientation]
    ref = rng.integers(0, n_contigs, n)
    order = [rng.permutation(n), rng.permutation(n)]
    files = []
    for f, (st, fl) in enumerate(((s1, f1), (s2, f2))):
        o = order[f]
        files.append(file_from_groups(o, ref[o], st[o], np.full(n, fl), [[(read_len << 4) | 0]] * n, n))
    return {"n_reads": int(n), "files": files}


# ---- the table of configurations: the CPU pin and the GPU tests import the same one --------------------------------------------

U32_MAX = 0xFFFFFFFF
ALL_CORRECT = tuple((0, U32_MAX, c) for c in range(4))


def occurring_insert(inp):
    """low == high == an insert size that occurs among the sampled pairs (the median one), for every orientation."""
    orient, insert, _ = samples(inp)
    seen = sorted(insert[orient != NOT_SAMPLED].tolist())
    v = seen[len(seen) // 2]
    return tuple((v, v, c) for c in range(4))


def _norm(n=5, seed=900):
    """a few ordinary reads around a hand-built one"""
    return generate(seed, n, extra_flags=False)


M100 = [(100, 0)]
BAD = [(1, OP_UNPARSEABLE)]


def _hand(reads, pad=40):
    return concat([_norm(pad, 901), hand_built(reads), _norm(pad, 902)])


# name -> (builder of the input, thresholds: a tuple of (low, high, correct) or a function of the input)
SEAM_CASES = {}


def _add(name, build, thr=((100, 900, 0), (300, 4000, 3))):
    assert name not in SEAM_CASES
    SEAM_CASES[name] = (build, thr)


def knobs(name):
    """The seed and the knobs of a configuration, as the table states them (for a failure's message)."""
    import inspect
    table = SEAM_CASES if name in SEAM_CASES else TEXT_CASES
    try:
        return " ".join(inspect.getsource(table[name][0]).split())
    except (OSError, TypeError):
        return name


for _n in (0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1025):
    _add(f"reads_{_n}", lambda n=_n: generate(1000 + n, n), ((100, 900, 0), (0, U32_MAX, 1)))
_add("reads_300k", lambda: generate(7, 300_000, pos_range=200_000), ((100, 900, 0),))
for _w in ("none", "all", "last", "lane0", "lane63", "first_half", "second_half", "one_in_last_wg"):
    _add(f"listed_{_w}_1300", lambda w=_w: generate(2000 + len(w), 1300, listed=w))
_add("listed_all_1024", lambda: generate(2100, 1024, listed="all"))
_add("listed_second_half_700", lambda: generate(2101, 700, listed="second_half"))
_add("listed_last_513", lambda: generate(2102, 513, listed="last"))
_add("group_1_vs_40", lambda: generate(2200, 70, cnt=((1,), (40,)), pos_range=600))
_add("group_40_vs_1", lambda: generate(2201, 70, cnt=((40,), (1,)), pos_range=600))
_add("group_40_vs_40", lambda: generate(2202, 40, cnt=((40,), (40,)), pos_range=600))
_add("several_vs_none", lambda: generate(2203, 600, cnt=((2, 3), (0,))))
_add("one_file_only_reads", lambda: generate(2204, 600, cnt=((0, 0, 1, 2), (0, 0, 1, 2))))
_add("file1_empty", lambda: generate(2205, 600, cnt=((0,), (1, 2))))
_add("file2_empty", lambda: generate(2206, 600, cnt=((1, 2), (0,))))
_add("both_empty", lambda: generate(2207, 600, cnt=((0,), (0,))))
_add("pairs_on_other_references", lambda: generate(2208, 700, cnt=((1,), (1,)), n_contigs=50))
_add("equal_positions", lambda: generate(2209, 3000, cnt=((1, 1, 2), (1, 1, 2)), pos_range=6, max_len=4, max_runs=2, n_contigs=1),
     ALL_CORRECT + ((0, 3, 0), (2, 2, 2), (1, 8, 3)))
_add("equal_positions_pairs", lambda: generate(2210, 3000, cnt=((1,), (1,)), pos_range=5, max_len=3, max_runs=1, n_contigs=1, ops=(0, 1)),
     ALL_CORRECT)
_add("threshold_on_an_insert", lambda: generate(2211, 2000, pos_range=300, n_contigs=1), occurring_insert)
_add("low_above_high", lambda: generate(2212, 2000), ((900, 100, 0), (1, 0, 2)))
_add("every_orientation_all_sizes", lambda: generate(2213, 2000), ALL_CORRECT + ((0, 0, 0), (U32_MAX, U32_MAX, 1)))
_add("every_op_many_runs", lambda: generate(2214, 1500, ops=tuple(range(9)), max_runs=40, p_norun=0.15, max_len=60), ALL_CORRECT + ((100, 900, 0),))
_add("no_runs_at_all", lambda: generate(2215, 800, p_norun=1.0, pos_range=1000), ((0, 500, 2), (0, 500, 3), (1, U32_MAX, 2)))
_add("ends_past_2_32", lambda: generate(2216, 1500, max_runs=40, max_len=MAX_RUN, pos_range=U32_MAX, ops=(0, 0, 2, 3, 7, 8, 1, 4), n_contigs=1),
     ALL_CORRECT + ((0, 1 << 31, 0), (1 << 31, U32_MAX, 3), (0, 1 << 30, 2)))
_add("unparseable_where_nobody_looks", lambda: generate(2217, 2500, unparseable="safe", p_unparseable=0.3), ((100, 900, 0), (0, U32_MAX, 2)))
_add("unparseable_anywhere", lambda: generate(2218, 2500, unparseable="any", p_unparseable=0.01))
_add("unparseable_only_alignment_of_a_read_without_mates", lambda: _hand([([(0, 10, 0, BAD)], []), ([], [(0, 10, 16, BAD)])]))
_add("unparseable_several_here_none_there", lambda: _hand([([(0, 10, 0, BAD), (0, 50, 0, M100), (1, 9, 16, BAD)], [])]))
_add("unparseable_pair_on_different_references", lambda: _hand([([(0, 10, 0, BAD)], [(1, 200, 16, M100)]),
                                                                ([(0, 10, 0, M100)], [(1, 200, 16, BAD)])]))
_add("unparseable_in_a_sampled_pair", lambda: _hand([([(0, 10, 0, M100)], [(0, 200, 16, BAD)])]))
_add("unparseable_single_mate_of_several", lambda: _hand([([(0, 10, 0, M100), (0, 700, 0, M100)], [(0, 200, 16, BAD)])]))
_add("unparseable_one_of_several_single_mate", lambda: _hand([([(0, 10, 0, M100), (0, 700, 0, BAD)], [(0, 200, 16, M100)])]))
# The mate behind the first good pair: file 1's alignments both make a good pair with file 2's FIRST alignment and never look
# at the second -- but file 2 has two alignments of this read and one mate at least, so the second is itself the `a` of
# alignment_pass_qc when file 2 is filtered, and its end is parsed there (src/filter.rs:367): the reference panics.
_add("unparseable_mate_behind_the_first_good_pair",
     lambda: _hand([([(0, 10, 0, M100), (0, 20, 0, M100)], [(0, 200, 16, M100), (0, 300, 16, BAD)])]), ((100, 900, 0),))
# ... and with thresholds under which the first mate is NOT a good pair, file 1's own loop reaches it as well
_add("unparseable_mate_reached_from_both_sides",
     lambda: _hand([([(0, 10, 0, M100), (0, 20, 0, M100)], [(0, 200, 16, M100), (0, 300, 16, BAD)])]), ((5000, 9000, 0),))
# listed reads whose verdict differs between the two files' views: both reverse, file 1's read starts later -> file 1 sees
# ff (p2 < p1), file 2 sees rr
_add("argument_order_both_reverse", lambda: _hand([([(0, 500, 16, M100), (0, 520, 16, M100)], [(0, 100, 16, M100), (0, 120, 16, M100)]),
                                                   ([(0, 100, 16, M100), (0, 120, 16, M100)], [(0, 500, 16, M100), (0, 520, 16, M100)]),
                                                   ([(0, 100, 0, M100), (0, 120, 0, M100)], [(0, 500, 0, M100), (0, 520, 0, M100)]),
                                                   ([(0, 100, 16, M100), (0, 100, 16, M100)], [(0, 100, 16, M100), (0, 100, 16, M100)]),
                                                   ([(0, 100, 0, M100), (0, 100, 0, M100)], [(0, 100, 0, M100), (0, 100, 0, M100)]),
                                                   ([(0, 100, 0, M100)], [(0, 100, 0, M100)]), ([(0, 100, 16, M100)], [(0, 100, 16, M100)]),
                                                   ([(0, 100, 0, M100)], [(0, 0, 16, M100)]), ([(0, 0, 16, M100)], [(0, 100, 0, M100)])]),
     ALL_CORRECT)


# ---- the command from text: (builder, naming, [(orientation, low percentile, high percentile), ...]) -------------------------

def stress_name(r):
    """QNAMEs of 1 and of several hundred bytes, names that differ only in their last byte or only in length."""
    return {0: "x", 1: "y", 2: "x" * 300, 3: "x" * 299 + "y", 4: "x" * 301, 5: "xx", 6: "read", 7: "read7 "[:5]}.get(r, f"read{r}")


def many_ref_name(c):
    return f"scaffold{c}|len{c % 97}"


DEFAULT_RUNS = (("auto", 0.1, 99.9),)


def _big_uneven():
    # four slices of 65,536 reads and more for the reduction threads: fr pairs nearly all in the first quarter, rf in the
    # last, multi-mapped and unpaired reads in between
    return concat([make_pairs(31, 70_000, 0, 300, 700), generate(32, 60_000, pos_range=500_000), make_pairs(33, 2_000, 0, 5_000, 9_000),
                   generate(34, 50_000, listed="lane63"), make_pairs(35, 30_000, 1, 300, 50_000), make_pairs(36, 37, 0, 100_000, 300_000)])


def _sizes(frac_big, n=20_000, seed=40):
    k = int(round(n * frac_big))
    parts = [make_pairs(seed, n - k, 0, 300, 900)] if n - k else []
    if k:
        parts.append(make_pairs(seed + 1, k, 0, 1 << 16, 1 << 20))
    parts.append(generate(seed + 2, 3000, pos_range=3000, n_contigs=1))
    return concat(parts)


TEXT_CASES = {
    "big_uneven_slices": (_big_uneven, default_read_name, default_ref_name, DEFAULT_RUNS + (("fr", 2.0, 99.99), ("rf", 40.0, 60.0))),
    "sizes_none_big": (lambda: _sizes(0.0), default_read_name, default_ref_name, DEFAULT_RUNS),
    "sizes_few_big_above_high": (lambda: _sizes(0.0004), default_read_name, default_ref_name, DEFAULT_RUNS + (("fr", 1.0, 99.0),)),
    "sizes_percentile_among_big": (lambda: _sizes(0.05), default_read_name, default_ref_name, DEFAULT_RUNS + (("fr", 49.0, 97.0),)),
    "sizes_all_big": (lambda: concat([make_pairs(50, 5000, 0, 1 << 16, 1 << 22), generate(51, 500)]), default_read_name, default_ref_name,
                      DEFAULT_RUNS + (("fr", 49.9, 50.1),)),
    # ceil(p / 100 * n) on 1 and on n; percentiles 0 and 100 are refused (src/filter.rs:47-52)
    "percentile_ranks": (lambda: concat([make_pairs(52, 1000, 0, 300, 5000), generate(53, 400, pos_range=3000)]), default_read_name,
                         default_ref_name, (("fr", 0.0001, 99.9999), ("fr", 0.1, 99.91), ("fr", 0.0, 99.0), ("fr", 1.0, 100.0),
                                            ("auto", 50.0, 60.0), ("auto", 10.0, 50.0), ("rr", 1.0, 99.0))),
    "no_pairs_of_that_orientation": (lambda: make_pairs(54, 300, 0, 300, 900), default_read_name, default_ref_name,
                                     (("rf", 1.0, 99.0), ("ff", 1.0, 99.0), ("rr", 1.0, 99.0), ("fr", 1.0, 99.0))),
    "auto_tie": (lambda: concat([make_pairs(55, 200, 0, 300, 900), make_pairs(56, 200, 2, 300, 900), make_pairs(57, 150, 1, 300, 900)]),
                 default_read_name, default_ref_name, DEFAULT_RUNS + (("ff", 1.0, 99.0),)),
    "no_one_and_one_pair": (lambda: generate(58, 500, cnt=((2, 3), (0, 2))), default_read_name, default_ref_name, DEFAULT_RUNS),
    "one_name_thousands_of_alignments": (lambda: concat([make_pairs(59, 500, 0, 300, 900),
                                                         generate(60, 1, cnt=((3000,), (2,)), pos_range=2000, n_contigs=1, extra_flags=False),
                                                         generate(61, 1, cnt=((2,), (2500,)), pos_range=2000, n_contigs=1, extra_flags=False),
                                                         generate(62, 300)]), default_read_name, default_ref_name, DEFAULT_RUNS),
    "tens_of_thousands_of_references": (lambda: concat([generate(63, 40_000, n_contigs=30_000), make_pairs(64, 3000, 0, 300, 900, n_contigs=30_000)]),
                                        default_read_name, many_ref_name, DEFAULT_RUNS),
    "names_1_byte_to_hundreds": (lambda: generate(65, 4000), stress_name, default_ref_name, DEFAULT_RUNS + (("fr", 5.0, 95.0),)),
}
