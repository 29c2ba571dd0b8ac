"""A plain model of pp_filter_records (include/polypolish_hip.h): "the raw records of the two SAM files -> the filter's verdicts,
counts and report".  Test infrastructure, it does not call the library: the aligned records of either file are grouped into reads
by a Python dict on read_id (the reference's HashMap<String, Vec<Alignment>>, src/filter.rs:91-145), which gives the
pp_filter_input dict of tests/filter_model.py, and filter_model.command does the rest.  tests/test_filter_records_model_cpu.py
pins it to the oracle on the SAM text of the same records; tests/test_filter_records_gpu.py runs the device against it.

Also here: raw batches made from a filter_model input (ids chosen by a function of the read number, unaligned records in
between), their SAM texts (the QNAME derived from the id), and the ONE table of cases both test files run."""
import numpy as np

import filter_model as fm

RAW_FIELDS = (("flag", np.uint16), ("read_id", np.uint64), ("contig", np.uint32), ("ref_start", np.uint32), ("nm", np.uint32),
              ("seq_off", np.uint64), ("seq_len", np.uint32), ("cig_off", np.uint64), ("n_cig", np.uint32), ("seq", np.uint8),
              ("cigar", np.uint32))
U64_MAX = 0xFFFFFFFFFFFFFFFF
MSG_FILE1 = "no alignments found in file 1"


class ArgError(Exception):
    """PP_ERR_ARG: the CIGAR range of an aligned record does not lie inside the cigar array"""

    def __init__(self, file, record):
        super().__init__(f"file {file + 1} record {record}")
        self.file, self.record = file, record


def aligned(raw):
    """raw indices of the file's aligned records, in file order: their rank is the numbering of the verdicts"""
    return np.flatnonzero((np.asarray(raw["flag"]) & 4) == 0)


def to_input(raws):
    """-> (pp_filter_input dict of filter_model, [(aligned records, distinct ids)] per file).  Reads are numbered by the first
    appearance of their id, file 1 then file 2."""
    number = {}
    files, counts = [], []
    for raw in raws:
        idx = aligned(raw).tolist()
        ids = [int(raw["read_id"][r]) for r in idx]
        for i in ids:
            number.setdefault(i, len(number))
        counts.append((len(idx), len(set(ids))))
        files.append((idx, ids))
    out = []
    for raw, (idx, ids) in zip(raws, files):
        cig = np.asarray(raw["cigar"]).tolist()
        runs = [cig[int(raw["cig_off"][r]):int(raw["cig_off"][r]) + int(raw["n_cig"][r])] for r in idx]
        out.append(fm.file_from_groups([number[i] for i in ids], [int(raw["contig"][r]) for r in idx], [int(raw["ref_start"][r]) for r in idx],
                                       [int(raw["flag"][r]) for r in idx], runs, len(number)))
    return {"n_reads": len(number), "files": out}, counts


def command(raws, orientation="auto", low_p=0.1, high_p=99.9):
    """-> {"pass": (p1, p2), "counts": [(alignments, reads)] * 2, "report": filter_model.command's figures}, or raises
    filter_model.Quit / filter_model.Panic / ArgError in the order of pp_filter_records."""
    if low_p <= 0.0 or low_p >= 50.0:
        raise fm.Quit(fm.MSG_LOW)
    if high_p <= 50.0 or high_p >= 100.0:
        raise fm.Quit(fm.MSG_HIGH)
    for f, raw in enumerate(raws):
        total = len(raw["cigar"])
        for r in aligned(raw).tolist():
            if int(raw["n_cig"][r]) and int(raw["cig_off"][r]) + int(raw["n_cig"][r]) > total:
                raise ArgError(f, r)
    inp, counts = to_input(raws)
    res = fm.command(inp, orientation, low_p, high_p)
    return {"pass": res["pass"], "counts": counts, "report": {k: res[k] for k in ("before", "after", "low", "high", "orientation", "counts")}}


# ---- raw batches ------------------------------------------------------------------------------------------------------------

def pack(rows):
    """rows of (flag, read_id, contig, ref_start, runs) -> the arrays of pp_raw_batch (nm 0, no SEQ: the filter reads neither)"""
    n = len(rows)
    n_cig = np.array([len(r[4]) for r in rows], np.uint32).reshape(n)
    return {"flag": np.array([r[0] for r in rows], np.uint16).reshape(n), "read_id": np.array([r[1] for r in rows], np.uint64).reshape(n),
            "contig": np.array([r[2] for r in rows], np.uint32).reshape(n), "ref_start": np.array([r[3] for r in rows], np.uint32).reshape(n),
            "nm": np.zeros(n, np.uint32), "seq_off": np.zeros(n, np.uint64), "seq_len": np.zeros(n, np.uint32),
            "cig_off": (np.cumsum(n_cig, dtype=np.int64) - n_cig).astype(np.uint64), "n_cig": n_cig, "seq": np.zeros(0, np.uint8),
            "cigar": np.array([x for r in rows for x in r[4]], np.uint32)}


def raws_from_input(inp, id_of=lambda r: r, p_unaligned=0.0, seed=0):
    """The two raw batches of a filter_model input: alignment a of file f becomes a record with read_id = id_of(read[a]); with
    probability p_unaligned an UNALIGNED record (FLAG & 4) goes in front of it -- carrying the id of some aligned record, a
    reference and a position, which must all count for nothing -- and one more ends the file."""
    rng = np.random.default_rng(seed)
    raws = []
    for f in inp["files"]:
        rows = []
        n = len(f["read"])
        cig = f["cigar"].tolist()
        for a in range(n):
            if rng.random() < p_unaligned:
                rows.append((4 | (16 if rng.random() < 0.5 else 0), id_of(int(f["read"][rng.integers(0, n)])), int(f["ref_id"][a]),
                             int(f["ref_start"][a]), [(50 << 4)] if rng.random() < 0.5 else []))
            rows.append((int(f["flags"][a]) & ~4, id_of(int(f["read"][a])), int(f["ref_id"][a]), int(f["ref_start"][a]),
                         cig[int(f["cig_off"][a]):int(f["cig_off"][a]) + int(f["n_cig"][a])]))
        if p_unaligned and n:
            rows.append((4, id_of(int(f["read"][0])), 0, 0, []))
        raws.append(pack(rows))
    return raws


def table_capacity(n_aligned):
    """slots of the device's id table for n_aligned records in the two files together (pp_filter_rec.hip)"""
    cap = 1024
    while cap < 2 * n_aligned + 2:
        cap <<= 1
    return cap


# ---- SAM text ---------------------------------------------------------------------------------------------------------------

def qname(i):
    return f"q{int(i)}"


def sam_texts(raws):
    """the equivalent SAM texts (bytes): one line per record, unaligned ones included, QNAME derived from the id, RNAME from the
    contig id"""
    texts = []
    for raw in raws:
        lines = ["@HD\tVN:1.6"]
        cig = np.asarray(raw["cigar"]).tolist()
        for r in range(len(raw["flag"])):
            runs = cig[int(raw["cig_off"][r]):int(raw["cig_off"][r]) + int(raw["n_cig"][r])]
            lines.append(f"{qname(raw['read_id'][r])}\t{int(raw['flag'][r])}\tref{int(raw['contig'][r])}\t{int(raw['ref_start'][r]) + 1}\t60\t"
                         f"{fm.cigar_text(runs)}\t*\t0\t0\t*\t*")
        texts.append(("\n".join(lines) + "\n").encode())
    return texts


def write_sams(raws, directory):
    import os
    paths = [os.path.join(str(directory), n) for n in ("rec_1.sam", "rec_2.sam")]
    for p, t in zip(paths, sam_texts(raws)):
        with open(p, "wb") as fh:
            fh.write(t)
    return paths


# ---- the table of cases: name -> (builder of the two raw batches, [(orientation, low percentile, high percentile), ...]) -----------

M100 = [(100, 0)]
BAD = [(1, fm.OP_UNPARSEABLE)]
DEFAULT_RUNS = (("auto", 0.1, 99.9), ("fr", 10.0, 90.0))
CASES = {}


def _add(name, build, runs=DEFAULT_RUNS):
    assert name not in CASES
    CASES[name] = (build, runs)


def _mixed(seed, n_pairs=300, n_other=200, **kw):
    """fr pairs to take thresholds from, and reads with every count of alignments around them"""
    return fm.concat([fm.make_pairs(seed, n_pairs, 0, 300, 700, pos_range=50_000), fm.generate(seed + 1, n_other, pos_range=3000, n_contigs=1, **kw)])


def _ids_0_and_max(r):
    return {0: 0, 1: U64_MAX, 2: 1, 3: U64_MAX - 1, 4: 1 << 63, 5: 1 << 32}.get(r, r + 1000)


def _capacity_multiples():
    inp = _mixed(110)
    cap = table_capacity(len(inp["files"][0]["read"]) + len(inp["files"][1]["read"]))
    # every id a multiple of the capacity (and of 2^32 for every other one): a hash that only masks would chain them all
    return raws_from_input(inp, lambda r: (r * cap) if r % 2 else ((r * cap) << 32) & U64_MAX)


def _far_apart():
    # read 0's three records of file 1 are the first, the middle and the last of ~3000; its mate is the last record of file 2
    inp = fm.concat([fm.make_pairs(120, 1500, 0, 300, 700, pos_range=50_000), fm.generate(121, 400, pos_range=3000, n_contigs=1)])
    raws = raws_from_input(inp, lambda r: r + 1)
    far = [(0, 0, 0, 100, [(100 << 4)]), (0, 0, 0, 4000, [(100 << 4)]), (256, 0, 0, 150, [(100 << 4)])]
    mate = (16, 0, 0, 520, [(100 << 4)])

    def rows_of(raw):
        cig = raw["cigar"].tolist()
        return [(int(raw["flag"][r]), int(raw["read_id"][r]), int(raw["contig"][r]), int(raw["ref_start"][r]),
                 cig[int(raw["cig_off"][r]):int(raw["cig_off"][r]) + int(raw["n_cig"][r])]) for r in range(len(raw["flag"]))]
    r1, r2 = rows_of(raws[0]), rows_of(raws[1])
    half = len(r1) // 2
    return [pack([far[0]] + r1[:half] + [far[1]] + r1[half:] + [far[2]]), pack(r2 + [mate])]


def _group_300_vs_2():
    return raws_from_input(fm.concat([fm.make_pairs(130, 400, 0, 300, 700, pos_range=2000),
                                      fm.generate(131, 1, cnt=((300,), (2,)), pos_range=2000, n_contigs=1, extra_flags=False),
                                      fm.generate(132, 50, pos_range=2000, n_contigs=1)]), lambda r: r * 7 + 3, p_unaligned=0.05, seed=133)


def _unknown_references():
    # pairs whose two records sit on two DIFFERENT references outside the assembly (ids 1000 / 1001): not sampled, and a read with
    # several alignments here fails against a mate on the other one; reads on ONE unknown reference pair as on any other
    reads = [([(1000, 10, 0, M100)], [(1001, 200, 16, M100)]) for _ in range(20)]
    reads += [([(1000, 10 + i, 0, M100)], [(1000, 400 + i, 16, M100)]) for i in range(30)]
    reads += [([(1000, 10, 0, M100), (1001, 10, 0, M100)], [(1001, 400, 16, M100)]), ([(1001, 10, 0, M100), (1001, 30, 0, M100)], [(1000, 400, 16, M100)])]
    return raws_from_input(fm.concat([fm.make_pairs(140, 200, 0, 300, 700), fm.hand_built(reads)]))


def _pairs_exactly(n_aligned, seed):
    # n_aligned aligned records in either file, unaligned ones in between
    return raws_from_input(fm.make_pairs(seed, n_aligned, 0, 300, 900, pos_range=20_000), lambda r: r ^ 0x5555, p_unaligned=0.2, seed=seed + 1)


_add("ids_0_and_2_64_minus_1", lambda: raws_from_input(_mixed(100), _ids_0_and_max))
_add("ids_equal_in_the_low_32_bits", lambda: raws_from_input(_mixed(105), lambda r: (r << 32) | 0xDEADBEEF))
_add("ids_multiples_of_the_table_capacity", _capacity_multiples)
_add("a_read_far_apart_in_its_file", _far_apart)
_add("unaligned_records_interleaved", lambda: raws_from_input(_mixed(115), lambda r: r + 5, p_unaligned=0.35, seed=116))
_add("reads_only_in_file_2", lambda: raws_from_input(fm.concat([fm.make_pairs(117, 200, 0, 300, 700), fm.generate(118, 300, cnt=((0,), (1, 2, 3)))])))
_add("file_2_empty", lambda: raws_from_input(fm.generate(119, 300, cnt=((1, 2), (0,)))))
_add("file_2_only_unaligned", lambda: [raws_from_input(_mixed(122))[0], pack([(4, i, 0, 10, [(50 << 4)]) for i in range(70)])])
_add("file_1_empty", lambda: raws_from_input(fm.generate(123, 300, cnt=((0,), (1, 2)))))
_add("file_1_only_unaligned", lambda: [pack([(4 | 16, i, 0, 10, []) for i in range(70)]), raws_from_input(_mixed(124))[1]])
_add("one_read_300_here_2_there", _group_300_vs_2)
_add("no_runs_at_all", lambda: raws_from_input(fm.generate(134, 600, p_norun=1.0, pos_range=1000, n_contigs=1)), (("auto", 0.1, 99.9), ("rf", 10.0, 90.0)))
_add("some_records_without_runs", lambda: raws_from_input(_mixed(135, p_norun=0.3)))
_add("unparseable_where_nobody_compares", lambda: raws_from_input(fm.generate(136, 1500, unparseable="safe", p_unparseable=0.3)))
_add("unparseable_in_a_sampled_pair", lambda: raws_from_input(fm.concat([fm.make_pairs(137, 100, 0, 300, 700),
                                                                          fm.hand_built([([(0, 10, 0, M100)], [(0, 200, 16, BAD)])])])))
_add("unparseable_in_a_compared_mate", lambda: raws_from_input(fm.concat([fm.make_pairs(138, 100, 0, 300, 700),
                                                                           fm.hand_built([([(0, 10, 0, M100), (0, 700, 0, M100)], [(0, 200, 16, BAD)])])])))
_add("two_unknown_references", _unknown_references)
for _n in (255, 256, 257):
    _add(f"aligned_{_n}", lambda n=_n: _pairs_exactly(n, 150 + n))
_add("auto_tie", lambda: raws_from_input(fm.concat([fm.make_pairs(160, 120, 0, 300, 900), fm.make_pairs(161, 120, 2, 300, 900), fm.make_pairs(162, 70, 1, 300, 900)])),
     (("auto", 0.1, 99.9), ("ff", 1.0, 99.0), ("rr", 1.0, 99.0)))
_add("percentiles_out_of_range", lambda: raws_from_input(_mixed(163, 50, 20)), (("auto", 0.0, 99.9), ("auto", 50.0, 99.9), ("auto", 0.1, 50.0), ("auto", 0.1, 100.0)))
# the jobs of the "large -> tiny -> large on one context" test
_add("large_a", lambda: raws_from_input(_mixed(170, 6000, 3000), lambda r: r * 0x9E3779B97F4A7C15 & U64_MAX, p_unaligned=0.02, seed=171))
_add("tiny", lambda: raws_from_input(fm.make_pairs(172, 3, 0, 300, 700), lambda r: U64_MAX - r))
_add("large_b", lambda: raws_from_input(_mixed(173, 5000, 4000), lambda r: r, p_unaligned=0.01, seed=174))
