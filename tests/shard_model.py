"""A plain model of pp_shard_split / pp_shard_count, written from the contract in include/polypolish_hip.h (the comments on
pp_shard_split and pp_shard_count, pp_aln_batch, pp_wo_rec, PP_SEQ_ALIGN, PP_SEQ4_*) in Python integers, so nothing can wrap.
tests/test_shard_model_cpu.py pins the host loop to it and it to hand-computed answers; tests/test_shard_split_gpu.py holds the
kernels of polypolish_amd/csrc/pp_shard_dev.hip to it.  It never calls the library.

A batch is a dict of numpy arrays (contig ref_start k seq_off seq_len cig_off n_cig seq cigar, optionally "wo": WO_DTYPE
entries, and "wo_runs": the ends of the mirror's runs).  A plan is anything with unit_contig / unit_lo / unit_hi / unit_rank
(per unit, contig by contig, windows in position order) and n_contigs.

Also here: the builders of the cases both tests run (the seam batch, random short reads, the seq layouts, mirrors)."""
import numpy as np

SEQ_ALIGN = 32      # PP_SEQ_ALIGN
WO_MAX_RUNS = 16    # PP_WO_MAX_RUNS
WO_MULTI_RUN = 0xFFFFFFFF
WINDOW = 2048
M, I, D, N, S, H, P, EQ, X = range(9)   # the packed CIGAR codes (op & 15), BAM's
REF_CODES = (M, EQ, X, D, N)
SEQ4 = {ord("A"): 0, ord("C"): 1, ord("T"): 2, ord("G"): 3, ord("N"): 4, ord("-"): 5}   # PP_SEQ4_*: anything else is 15
SEQ4_OTHER = 15
WO_DTYPE = np.dtype([("contig", np.uint32), ("ref_start", np.uint32), ("k", np.uint32), ("seq_len", np.uint32),
                     ("seq_off", np.uint64), ("op0", np.uint32), ("file_idx", np.uint32)])
FIELDS = (("contig", np.uint32), ("ref_start", np.uint32), ("k", np.uint32), ("seq_off", np.uint64), ("seq_len", np.uint32),
          ("cig_off", np.uint64), ("n_cig", np.uint32), ("seq", np.uint8), ("cigar", np.uint32))


# ---- the model ------------------------------------------------------------------------------------------------------------------

def span(recs, i):
    """reference positions record i can touch: the lengths of its M / = / X / D / N runs, at least 1"""
    co, nc = int(recs["cig_off"][i]), int(recs["n_cig"][i])
    return max(1, sum(int(o) >> 4 for o in recs["cigar"][co:co + nc] if (int(o) & 15) in REF_CODES))


def owners(plan, c, rs, sp):
    """the ranks a record of contig c over [rs, rs + sp) goes to: every unit it touches; none -> the contig's last unit;
    no such contig -> the plan's last unit"""
    if c >= plan.n_contigs:
        return {int(plan.unit_rank[-1])}
    us = [u for u in range(len(plan.unit_contig)) if int(plan.unit_contig[u]) == c]
    hit = {int(plan.unit_rank[u]) for u in us if rs < int(plan.unit_hi[u]) and rs + sp > int(plan.unit_lo[u])}
    return hit or {int(plan.unit_rank[us[-1]])}


def selected(plan, dest, recs):
    """indices of the records rank `dest` is handed, in file order"""
    return [i for i in range(len(recs["contig"]))
            if dest in owners(plan, int(recs["contig"][i]), int(recs["ref_start"][i]), span(recs, i))]


# the two functions tests/test_distributed_cpu.py had of its own
_ref_span = span


def _split_reference(plan, dest, contig_off, recs):
    """The routing rule in plain Python: a record goes to the rank of every unit its [ref_start, ref_start + span) touches."""
    assert plan.n_contigs == len(contig_off) - 1
    return np.array(selected(plan, dest, recs), dtype=np.int64)


def room(n):
    return (n + SEQ_ALIGN - 1) // SEQ_ALIGN * SEQ_ALIGN


def seq4_of(seq):
    """the 4-bit mirror of a seq array of even length: base i in bits 4 * (i & 1) of byte i >> 1"""
    lut = np.full(256, SEQ4_OTHER, dtype=np.uint8)
    for byte, code in SEQ4.items():
        lut[byte] = code
    codes = lut[np.asarray(seq, dtype=np.uint8)]
    assert len(codes) % 2 == 0
    return (codes[0::2] | (codes[1::2] << 4)).astype(np.uint8)


def runs_usable(recs):
    runs = recs.get("wo_runs")
    if recs.get("wo") is None or runs is None or not 1 <= len(runs) <= WO_MAX_RUNS:
        return False
    ends = [int(e) for e in runs]
    return all(a <= b for a, b in zip([0] + ends[:-1], ends)) and ends[-1] == len(recs["contig"])


def split(plan, dest, recs, wo_idx_base=0):
    """-> (part, orig): the part as a batch dict (plus "seq4"; "wo" / "wo_runs" only when the part has them), orig = the index
    of every record of the part in `recs`.

    The part's seq array: a room of room(seq_len) bytes per record, the rooms tiling the array, zeros behind the read.  The rooms
    follow the SOURCE's seq array -- slot by slot of SEQ_ALIGN bytes -- when every selected record that has SEQ bytes starts on
    a slot of its own inside that array, otherwise the records.  A record without SEQ bytes takes no room and claims no slot; it
    sits in front of the room of a record that starts in its slot.  wo_idx_base: what the file_idx of recs["wo"] count from."""
    n = len(recs["contig"])
    pick = selected(plan, dest, recs)
    cnt = len(pick)
    so = [int(recs["seq_off"][i]) for i in pick]
    sl = [int(recs["seq_len"][i]) for i in pick]
    n_slots = (len(recs["seq"]) + SEQ_ALIGN - 1) // SEQ_ALIGN
    first = [o // SEQ_ALIGN for o, l in zip(so, sl) if l]
    own_slots = all(o % SEQ_ALIGN == 0 and o // SEQ_ALIGN < n_slots for o, l in zip(so, sl) if l) and len(set(first)) == len(first)
    order = sorted(range(cnt), key=lambda j: (so[j] // SEQ_ALIGN, sl[j] != 0, j)) if own_slots else list(range(cnt))
    place, at = [0] * cnt, 0
    for j in order:
        place[j] = at
        at += room(sl[j])
    seq = np.zeros(at, dtype=np.uint8)
    for j in range(cnt):
        seq[place[j]:place[j] + sl[j]] = recs["seq"][so[j]:so[j] + sl[j]]
    nc = [int(recs["n_cig"][i]) for i in pick]
    cig_off = [sum(nc[:j]) for j in range(cnt)] if cnt < 64 else np.concatenate([[0], np.cumsum(nc)[:-1]]).tolist()
    runs = [recs["cigar"][int(recs["cig_off"][i]):int(recs["cig_off"][i]) + m] for i, m in zip(pick, nc)]
    part = {k: np.asarray(recs[k])[pick].astype(dt) if cnt else np.zeros(0, dt)
            for k, dt in FIELDS if k in ("contig", "ref_start", "k", "seq_len", "n_cig")}
    part["seq_off"] = np.array(place, dtype=np.uint64)
    part["cig_off"] = np.array(cig_off, dtype=np.uint64)
    part["seq"] = seq
    part["cigar"] = np.concatenate(runs).astype(np.uint32) if cnt else np.zeros(0, np.uint32)
    part["seq4"] = seq4_of(seq)
    orig = np.array(pick, dtype=np.uint32)
    if recs.get("wo") is None or not cnt:
        return part, orig
    # the mirror: the source's entries of the part's records, in the source's order.  A mirror has one entry per record
    # (pp_aln_batch.wo: n_aln entries): a selection that does not come to that is no mirror of the part.
    new_idx = {i: j for j, i in enumerate(pick)}
    keep, before = [], []
    for j in range(n):
        fi = int(recs["wo"]["file_idx"][j]) - wo_idx_base
        if not 0 <= fi < n:
            return part, orig
        before.append(len(keep))
        if fi in new_idx:
            keep.append((j, new_idx[fi]))
    before.append(len(keep))
    if len(keep) != cnt:
        return part, orig
    wo = recs["wo"][[j for j, _ in keep]].copy()
    wo["seq_off"] = [place[p] for _, p in keep]
    wo["file_idx"] = [p for _, p in keep]
    part["wo"] = wo
    if runs_usable(recs):
        part["wo_runs"] = np.array([before[int(e)] for e in recs["wo_runs"]], dtype=np.uint64)
    return part, orig


def count(contig, n_contigs, into):
    """pp_shard_count: ADDS one per record with contig < n_contigs to `into` (a list of Python integers)"""
    for c in contig:
        if int(c) < n_contigs:
            into[int(c)] += 1
    return into


class PlanModel:
    """a plan given by hand: units as (contig, lo, hi, rank)"""

    def __init__(self, n_contigs, units):
        self.n_contigs = n_contigs
        self.unit_contig, self.unit_lo, self.unit_hi, self.unit_rank = (list(x) for x in zip(*units))


# ---- builders -------------------------------------------------------------------------------------------------------------------

LENS = (6144, 300, 2048, 5000)     # the assembly of every case; contig 0 is cut into [0,2048) [2048,4096) [4096,6144)
CONTIG_OFF = np.array([0, 6144, 6444, 8492, 13492], dtype=np.uint64)
WORLD, MIN_WINDOW = 3, 2048
ALPHABET = np.frombuffer(b"ACGTN-acgt*\x00\xff", dtype=np.uint8)


def op(length, code):
    return (length << 4) | code


def batch(rows, layout="rooms", order=None, lead=0):
    """rows of (contig, ref_start, k, seq bytes, [packed runs]) -> a batch dict.  layout: "rooms" = every record in a room of
    room(seq_len) bytes, "tight" = the reads one behind the other; order: the records' order in the seq array (default: the
    records'); lead: bytes in front of the first read."""
    n = len(rows)
    order = list(range(n)) if order is None else [int(j) for j in order]
    sl = [len(r[3]) for r in rows]
    off, at = [0] * n, lead
    for j in order:
        off[j] = at
        at += room(sl[j]) if layout == "rooms" else sl[j]
    seq = np.zeros(at, dtype=np.uint8)
    for j, r in enumerate(rows):
        seq[off[j]:off[j] + sl[j]] = np.frombuffer(bytes(r[3]), dtype=np.uint8)
    nc = [len(r[4]) for r in rows]
    return {"contig": np.array([r[0] for r in rows], dtype=np.uint32), "ref_start": np.array([r[1] for r in rows], dtype=np.uint32),
            "k": np.array([r[2] for r in rows], dtype=np.uint32), "seq_off": np.array(off, dtype=np.uint64),
            "seq_len": np.array(sl, dtype=np.uint32),
            "cig_off": np.concatenate([[0], np.cumsum(nc)[:-1]]).astype(np.uint64) if n else np.zeros(0, np.uint64),
            "n_cig": np.array(nc, dtype=np.uint32), "seq": seq,
            "cigar": np.array([x for r in rows for x in r[4]], dtype=np.uint32)}


BIG = (1 << 28) - 1   # the largest run length the packed form holds
SEAM_SEQ_LENS = (0, 1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 255, 256, 257, 300)


def seam_rows():
    """The seam batch: -> (rows, where): where[i] = the units record i must reach, worked out by hand, as (contig, window of
    the contig) pairs -- ("last", c) = touches none, goes to contig c's last unit; "fallback" = the plan's last unit."""
    rng = np.random.default_rng(77)
    w0, w1, w2 = (0, 0), (0, 1), (0, 2)
    rows, where = [], []

    def add(contig, rs, runs, units, seq=b"ACGT", k=1):
        rows.append((contig, rs, k, seq, runs))
        where.append(units)
    add(0, 2047, [op(1, M)], [w0])
    add(0, 2047, [op(2, M)], [w0, w1])
    add(0, 2048, [op(1, M)], [w1])
    add(0, 2040, [op(8, M)], [w0])                                            # ends exactly at 2048
    add(0, 100, [op(10, M), op(3000, D), op(10, M)], [w0, w1])                  # [100, 3120): two windows, 3120 < 4096
    add(0, 100, [op(10, M), op(3000, N), op(10, M)], [w0, w1], k=2)
    add(0, 1100, [op(10, M), op(3000, D), op(10, M)], [w0, w1, w2])             # [1100, 4120): all three
    add(0, 1100, [op(10, M), op(3000, N), op(10, M)], [w0, w1, w2], k=2)
    add(0, 2048, [op(5, S), op(7, I), op(3, S)], [w1])                          # span 0 -> 1
    add(0, 6144, [op(5, S), op(7, I), op(3, S)], [("last", 0)])                 # past the end
    add(0, 4095, [], [w1])                                                      # n_cig = 0: span 1
    add(0, 2040, [op(4, M), op(50, H), op(50, P)] + [op(50, c) for c in range(9, 16)] + [op(4, M)], [w0])   # span 8, not 458
    add(3, 0, [op(BIG, M)] * 32, [(3, 0)], k=3)                                 # span 2^33 - 32
    add(0, 0, [op(BIG, M)] * 32, [w0, w1, w2])
    add(0, 0, [op(BIG, EQ)] * 16 + [op(16, X)], [w0, w1, w2])                   # span 2^32 exactly: 0 in 32 bits
    add(0, 0xFFFFFFFF, [op(4, M)], [("last", 0)])
    add(4, 10, [op(4, M)], ["fallback"])
    add(0xFFFFFFFF, 10, [op(4, M)], ["fallback"])
    add(1, 0, [op(300, M)], [(1, 0)])
    add(1, 300, [op(4, M)], [("last", 1)])
    add(2, 2047, [op(4, M)], [(2, 0)])
    for j, n in enumerate(SEAM_SEQ_LENS):
        seq = ALPHABET[rng.integers(0, len(ALPHABET), n)]
        if n == 300:
            seq[:len(ALPHABET)] = ALPHABET
        rs = 1990 + 1024 * (j % 4) + j                                          # [rs, rs + max(n, 1))
        lo, hi = rs // 2048, (rs + max(n, 1) - 1) // 2048
        add(0, rs, [op(n, M)] if n else [op(3, I)], [(0, w) for w in range(lo, min(hi, 2) + 1)], seq=bytes(seq), k=1 + j % 3)
    return rows, where


def random_rows(n, seed):
    """n short reads (1 to 40 bases) over the four contigs, most of them on contig 0 and many around its window edges"""
    rng = np.random.default_rng(seed)
    contig = rng.choice([0, 0, 0, 0, 0, 0, 0, 1, 2, 3], n)
    contig[rng.random(n) < 0.01] = 4 + int(seed)
    edge = rng.choice([2048, 4096, 6144], n) + rng.integers(-45, 5, n)
    rs = np.where(rng.random(n) < 0.4, edge, rng.integers(0, 6200, n))
    rs = np.where(contig == 0, rs, rs % (np.array(LENS + (1 << 20,) * 16)[np.minimum(contig, 4)] + 8))
    sl = rng.integers(1, 41, n)
    kind = rng.integers(0, 4, n)
    seqs = ALPHABET[rng.integers(0, len(ALPHABET), int(sl.sum()))]
    ends = np.cumsum(sl)
    rows = []
    for i in range(n):
        L, a = int(sl[i]), int(sl[i]) // 2
        if kind[i] == 1 and L > 2:
            runs = [op(a, M), op(1 + i % 60, D), op(L - a, M)]
        elif kind[i] == 2 and L > 2:
            runs = [op(a, M), op(1, I), op(L - a - 1, M)]
        else:
            runs = [op(L, M)]
        rows.append((int(contig[i]), int(rs[i]), 1 + i % 3, seqs[ends[i] - L:ends[i]].tobytes(), runs))
    return rows


def mirror(recs, per_file=None, order=None):
    """a window-order mirror of the batch: its records per file (per_file: records of every file; None = one), inside a file by
    the 2048-position window of the assembly they start in, file order inside a window -- or in the given order"""
    n = len(recs["contig"])
    if order is None:
        c = np.minimum(recs["contig"].astype(np.int64), len(LENS) - 1)
        win = np.minimum((CONTIG_OFF[c].astype(np.int64) + recs["ref_start"].astype(np.int64)) // WINDOW, int(CONTIG_OFF[-1]) // WINDOW)
        file_of = np.repeat(np.arange(len(per_file)), per_file) if per_file is not None else np.zeros(n, np.int64)
        order = np.argsort(file_of * (1 << 20) + win, kind="stable")
    order = np.asarray(order, dtype=np.int64)
    wo = np.zeros(n, dtype=WO_DTYPE)
    for k in ("contig", "ref_start", "k", "seq_len", "seq_off"):
        wo[k] = recs[k][order]
    for j, i in enumerate(order):
        wo["op0"][j] = recs["cigar"][int(recs["cig_off"][i])] if int(recs["n_cig"][i]) == 1 else WO_MULTI_RUN
    wo["file_idx"] = order
    return wo


def view(recs, lo, hi):
    """records [lo, hi) of a batch as the one-process multi-GPU driver hands them on: the per-record arrays and the mirror cut,
    seq / cigar whole (seq_off / cig_off stay absolute), the mirror's file_idx still counting from the batch's start"""
    v = {k: recs[k][lo:hi] for k in ("contig", "ref_start", "k", "seq_off", "seq_len", "cig_off", "n_cig")}
    v["seq"], v["cigar"] = recs["seq"], recs["cigar"]
    if "wo" in recs:
        v["wo"] = recs["wo"][lo:hi]
    return v


# ---- the cases (A to E) -----------------------------------------------------------------------------------------------------------

SIZES = (0, 1, 255, 256, 257, 8191, 8192, 8193, 16385)   # the block edges and the edges of the scan's 8192-element tiles


def seam_batch():
    """case A -> (batch, where)"""
    rows, where = seam_rows()
    return batch(rows), where


def size_batch(n):
    """case B"""
    return batch(random_rows(n, seed=n % 89))


def layout_cases(n=600, seed=3):
    """case C -> [(name, batch)]: the ways a source lays out its seq array"""
    rng = np.random.default_rng(seed)
    rows = random_rows(n, seed)
    perm = rng.permutation(n)
    out = [("rooms in record order", batch(rows)), ("rooms shuffled", batch(rows, order=perm)),
           ("tight in record order", batch(rows, "tight", lead=3)), ("tight out of record order", batch(rows, "tight", order=perm, lead=3))]
    empty = [r if i % 7 else r[:3] + (b"", [op(2, I)]) for i, r in enumerate(rows)]   # every seventh record without SEQ bytes
    out.append(("zero-length records at the next record's offset", batch(empty)))
    out.append(("zero-length records at the offset of a record elsewhere in the file", batch(empty, order=perm)))
    last = [j for j in perm if j != 7 * 40] + [7 * 40]                               # record 280 has none and comes last in the array
    b = batch(empty, order=last)
    assert int(b["seq_off"][280]) == len(b["seq"]) and len(b["seq"]) % SEQ_ALIGN == 0
    out.append(("a zero-length record at seq_bytes", b))
    b = batch(empty, order=perm)
    for i in range(0, n, 7):                                                          # ... and off the slot boundaries, inside the array
        b["seq_off"][i] = min(int(b["seq_off"][i]) + 1 + i % 31, len(b["seq"]))
    out.append(("zero-length records at unaligned offsets", b))
    b = batch(rows, order=perm)
    for a in range(5, n - 1, 50):                                                     # record a + 1 is record a once more
        for k in ("contig", "ref_start", "seq_off", "seq_len"):
            b[k][a + 1] = b[k][a]
    out.append(("two records sharing one room", b))
    return out


def mirror_cases(n=700, seed=5):
    """case D -> [(name, batch with "wo" and maybe "wo_runs", wo_idx_base)]"""
    rng = np.random.default_rng(seed)
    rows = random_rows(n, seed)
    base = batch(rows, order=rng.permutation(n))

    def with_mirror(per_file, runs="per_file"):
        b = dict(base)
        b["wo"] = mirror(base, per_file)
        if runs is not None:
            b["wo_runs"] = np.cumsum(per_file).astype(np.uint64) if isinstance(runs, str) else np.array(runs, dtype=np.uint64)
        return b
    third = n // 3
    out = [("empty runs", with_mirror([0, third, 0, n - third]), 0),
           ("no run table", with_mirror([third, n - third], None), 0),
           ("a table that does not end at n", with_mirror([third, n - third], [third, n - 1]), 0),
           ("a table that descends", with_mirror([third, n - third], [third, third - 1, n]), 0),
           ("seventeen runs", with_mirror([n // 17] * 16 + [n - 16 * (n // 17)]), 0),
           ("sixteen runs", with_mirror([n // 16] * 15 + [n - 15 * (n // 16)]), 0)]
    two = with_mirror([third, n - third])
    for name, lo, hi in (("the second file of two as a view", third, n), ("the first file of two as a view", 0, third)):
        v = view(two, lo, hi)
        v["wo_runs"] = np.array([hi - lo], dtype=np.uint64)
        out.append((name, v, lo))
    one = with_mirror([n])                                 # one file in window order: a stretch of its mirror names records anywhere
    v = view(one, third, n)
    v["wo_runs"] = np.array([n - third], dtype=np.uint64)
    assert (v["wo"]["file_idx"] < third).any()
    out.append(("a view whose mirror stretch names records outside it", v, third))
    return out


COUNT_CONTIGS = (1, 8192, 8193)             # the LDS histogram's last size and the first one beyond
COUNT_SIZES = (1, 1023, 1024, 1025, 1024 * 1024 + 7)   # one block, and more records than the grid has threads


def count_case(n, n_contigs, seed=0):
    """case E -> (contig array, the counts beforehand): values at and above n_contigs in the mix"""
    rng = np.random.default_rng(seed + n + n_contigs)
    contig = rng.integers(0, n_contigs + n_contigs // 8 + 2, n).astype(np.uint32)
    contig[rng.random(n) < 0.02] = 0xFFFFFFFF
    contig[rng.random(n) < 0.02] = n_contigs
    contig[rng.random(n) < 0.05] = n_contigs - 1
    return contig, rng.integers(0, 1 << 40, n_contigs).astype(np.uint64)


# ---- what both tests do with a case ---------------------------------------------------------------------------------------------

def seam_plan(pp):
    """the plan of every case, from the library (polypolish_amd as pp) and held to the cuts worked out by hand: the seam
    batch's own counts -- contig 0 carries more than two thirds of the records, so it is cut into one window per rank"""
    recs, _ = seam_batch()
    counts = count(recs["contig"], 4, [0, 0, 0, 0])
    assert 3 * counts[0] > 2 * sum(counts)
    plan = pp.Plan(CONTIG_OFF, counts, WORLD, MIN_WINDOW)
    units = list(zip(plan.unit_contig.tolist(), plan.unit_lo.tolist(), plan.unit_hi.tolist()))
    assert units == [(0, 0, 2048), (0, 2048, 4096), (0, 4096, 6144), (1, 0, 300), (2, 0, 2048), (3, 0, 5000)], units
    assert sorted(plan.unit_rank[:3].tolist()) == [0, 1, 2]
    return plan


def assert_part(got, got_orig, want, want_orig, what, seq4=False):
    """a part read back from the library against the model's: the nine arrays, orig, (seq4,) the mirror field by field, its
    runs, and whether there is a mirror and a run table at all -- exact equality throughout"""
    assert np.array_equal(got_orig, want_orig), (what, "orig")
    for name in [k for k, _ in FIELDS] + (["seq4"] if seq4 else []):
        assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), (what, name)
    assert ("wo" in got) == ("wo" in want), (what, "a mirror", "wo" in want)
    if "wo" in want:
        assert len(got["wo"]) == len(want["wo"]), what
        for f in WO_DTYPE.names:
            assert np.array_equal(got["wo"][f], want["wo"][f]), (what, "wo." + f)
    assert ("wo_runs" in got) == ("wo_runs" in want), (what, "a run table", "wo_runs" in want)
    if "wo_runs" in want:
        assert [int(x) for x in got["wo_runs"]] == [int(x) for x in want["wo_runs"]], (what, "wo_runs")
