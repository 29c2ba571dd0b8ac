"""Polish jobs whose winners and --debug lines are LONG, for the three passes that turn a finished job into text on the device: the
--debug TSV (pp_k_debug.h), the VCF (pp_k_vcf.h) and the soft mask (k_bed_mask, pp_k_bed.h).  Each of them works out again how many
bytes a position emits and where they lie; a position that emits 127 bytes or more has the emit code 0xFF and its length comes from
the multi-byte winners' list.  Everything here is seeded plain Python: no GPU.  tests/test_long_sites_cpu.py proves with the oracle
that every job holds what it claims, tests/test_long_winner_outputs_gpu.py runs them on the device.

  L1  key_sites' emit-seam jobs as they are: winners of 0, 2, 3, 126 and 127 bytes at k_emit's seams (default options)
  L1d winners of 126, 127 and 202 emitted bytes with '-' bytes inside (dashed_job): the raw length differs from the emitted one
  L2  winners of 126, 127, 128, 201 and 301 bytes through vcf_jobs.reads (min_depth 1): side by side, two among one thread's
      positions, on both sides of a workgroup boundary, between two substitutions, in front of a deleted stretch, at the third-last
      position of the last contig, and one whose bytes are the neighbours of 'A'..'Z'
  L3  72 winners of 301 bytes: a VCF text longer than one text workgroup, under contig names of 1..16 bytes
  T1  a random dataset under contig names of 90, 97 and 103 bytes: every 256 TSV lines fill more than one staging window
  T2  a hand-built pair: one TSV line longer than a staging window (140 items with 127-byte keys), new_base of 126, 127, 128 and
      201 bytes, positions with exactly 12 and 13 items

A job is a dict: off, bases, recs (the C ABI's arrays), names (bytes), kw (the polish options), spec (L2, L3 and the small jobs: what
vcf_jobs.check_oracle_made checks)."""
import os

import numpy as np

import key_sites as ks
import synth
import vcf_jobs as vj
from debug_tsv_util import _write_job

WIN = 16384                            # DFMT_WIN (pp_k_debug.h): bytes of one staging window
BLOCK = 256                            # DFMT_THREADS: lines per workgroup
HEAVY = 12                             # DFMT_HEAVY: more items than this are placed by the workgroup
INSERTS = (125, 126, 127, 200, 300)    # inserted bytes: the winners emit one more
CASE_BYTES = b"@AZ[`az{N*"             # both neighbours of 'A'..'Z' and of 'a'..'z' (a '-' would be dropped by vcf_jobs.reads)
CASE_BYTES_UPPER = b"@AZ[`{N*"         # ... without the lower-case letters, which SAM text loses on its way in (write_files)
MIN1 = dict(min_depth=1, fraction_valid=0.5, fraction_invalid=0.2)
DEFAULT = dict(min_depth=5, fraction_valid=0.5, fraction_invalid=0.2)


def contig_names(n):
    return [b"contig_%d" % (i + 1) for i in range(n)]


def _job(off, bases, recs, kw, spec=None, names=None):
    return {"off": np.asarray(off, np.uint64), "bases": np.ascontiguousarray(bases, np.uint8), "recs": recs, "kw": kw, "spec": spec,
            "names": names or contig_names(len(off) - 1)}


# ---- L1 -----------------------------------------------------------------------------------------------------------------------------
def l1_job(which):
    off, bases, recs = {"small": ks.seam_job_small, "coarse": ks.seam_job_coarse}[which]().records()
    return _job(off, bases, recs, DEFAULT)


def dashed_job():
    """long winners with '-' bytes inside, which the polish drops: the raw length (what the TSV shows) is not the emitted one.  Twelve
    identical reads a site (default options): a winner of 128 raw bytes that emits 126 (the emit code still holds that), one of 129
    that emits 127 and one of 205 that emits 202 (code 0xFF: the length comes from the winners' list, whose entries hold both)"""
    job = ks.Job((1500,), 4300)
    for g, n, dashes in ((300, 127, (40, 90)), (301 + 64, 128, (0, 127)), (700, 204, (1, 100, 203)), (900, 2, ())):
        ins = bytearray(job.random_insert(n))
        for d in dashes:
            ins[d] = ord("-")
        job.site(g, [("ins", bytes(ins), 1)] * 12, plan={"n": 12, "kind": "dashed"})
    off, bases, recs = job.records()
    return _job(off, bases, recs, DEFAULT)


# ---- L2 -----------------------------------------------------------------------------------------------------------------------------
def _two_bases_at_the_end(off, bases):
    """every contig ends in two different bases: the homopolymer trim takes exactly these two off a read that runs to the end, so
    the third-last position is the last one a read covers"""
    for e in off[1:]:
        e = int(e)
        if bases[e - 1] == bases[e - 2]:
            bases[e - 1] = vj.other(int(bases[e - 2]))[0]


def _insert(rng, bases, p, n):
    return bytes(bases[p:p + 1]) + np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()


def l2_sites(tile, ppt):
    """{what: global positions} of l2_job(tile, ppt)"""
    c1 = 2 * tile + 600
    return {"adjacent": (300, 301), "one_thread": (50 * ppt + 1, 50 * ppt + ppt - 2), "tile_seam": (tile - 1, tile), "between_subs": (601,),
            "before_deletion": (700,), "code_fe": (800, c1 + 100), "case": (900,), "third_last": (c1 + 1200 - 3,), "contig_2": (c1 + 200,),
            "contig_1_start": c1}


def l2_job(tile, ppt, case_bytes=CASE_BYTES):
    """tile, ppt: VCF_TILE and VCF_PPT, the position passes' positions per workgroup and per thread"""
    s = l2_sites(tile, ppt)
    assert s["one_thread"][0] // ppt == s["one_thread"][1] // ppt and 301 < s["one_thread"][0] and s["one_thread"][1] < 600 < tile - 1
    off, bases = vj.assembly([s["contig_1_start"], 1200], 41)
    _two_bases_at_the_end(off, bases)
    rng = np.random.default_rng(42)
    spec = {}
    for ps, ns in ((s["adjacent"], (126, 127)), (s["one_thread"], (200, 300)), (s["tile_seam"], (126, 300)), (s["between_subs"], (127,)),
                   (s["before_deletion"], (200,)), (s["code_fe"], (125, 125)), (s["third_last"], (126,)), (s["contig_2"], (300,))):
        for p, n in zip(ps, ns):
            spec[p] = _insert(rng, bases, p, n)
    for p in (600, 602, 1000):
        spec[p] = vj.other(int(bases[p]))
    for p in list(range(701, 706)) + [1100]:
        spec[p] = b"-"
    spec[s["case"][0]] = bytes(bases[s["case"][0]:s["case"][0] + 1]) + case_bytes
    return _job(off, bases, vj.reads(off, bases, spec), MIN1, spec)


# ---- L3 -----------------------------------------------------------------------------------------------------------------------------
def l3_job():
    off, bases = vj.assembly([2000, 1200], 43)
    rng = np.random.default_rng(44)
    spec = {p: _insert(rng, bases, p, 300) for p in list(range(30, 30 + 40 * 45, 40)) + list(range(2030, 2030 + 40 * 27, 40))}
    return _job(off, bases, vj.reads(off, bases, spec), MIN1, spec)


def l3_names(n):
    return [b"a" * n, b"b" * n]


def alt_fields(vcf):
    """[(first byte, one past the last byte)] of the ALT fields of a VCF text"""
    out, at = [], 0
    for ln in vcf.split(b"\n")[:-1]:
        if ln[:1] != b"#":
            f = ln.split(b"\t")
            a = at + sum(len(x) + 1 for x in f[:4])
            out.append((a, a + len(f[4])))
        at += len(ln) + 1
    return out


def strictly_inside_a_long_alt(vcf, t, least=127):
    return any(a < t < b - 1 and b - a >= least for a, b in alt_fields(vcf))


# ---- small jobs for the job-after-job sequence ---------------------------------------------------------------------------------------
def no_multi_job():
    """substitutions and deletions alone: no position emits two bytes, the job has no multi-byte winner"""
    off, bases = vj.assembly([2600, 500], 45)
    spec = {p: (b"-" if i % 3 == 2 else vj.other(int(bases[p]), 1 + i % 2)) for i, p in enumerate(range(20, 2500, 61))}
    return _job(off, bases, vj.reads(off, bases, spec), MIN1, spec)


def one_contig_job():
    off, bases = vj.assembly([1500], 46)
    rng = np.random.default_rng(47)
    spec = {100: _insert(rng, bases, 100, 1), 200: _insert(rng, bases, 200, 126), 201: b"-", 640: vj.other(int(bases[640])),
            900: _insert(rng, bases, 900, 130), 901: _insert(rng, bases, 901, 3)}
    return _job(off, bases, vj.reads(off, bases, spec), MIN1, spec)


# ---- a records job as files: what the oracle's --debug TSV is made from ---------------------------------------------------------------
def write_files(tmp, job, name):
    """the job's assembly as FASTA and its records as SAM text, every record a read of its own (k = 1 throughout)"""
    off, bases, recs = job["off"], job["bases"], job["recs"]
    assert (np.asarray(recs["k"]) == 1).all()
    fa, sam = os.path.join(tmp, name + ".fasta"), os.path.join(tmp, name + ".sam")
    with open(fa, "wb") as f:
        for c, n in enumerate(job["names"]):
            f.write(b">" + n + b"\n" + bytes(bases[int(off[c]):int(off[c + 1])]) + b"\n")
    seq = np.asarray(recs["seq"], np.uint8).tobytes()
    with open(sam, "wb") as f:
        for c, n in enumerate(job["names"]):
            f.write(b"@SQ\tSN:%s\tLN:%d\n" % (n, int(off[c + 1]) - int(off[c])))
        for i in range(len(recs["contig"])):
            co, so = int(recs["cig_off"][i]), int(recs["seq_off"][i])
            cig = "".join("%d%s" % (int(x) >> 4, ks.OPS[int(x) & 15]) for x in recs["cigar"][co:co + int(recs["n_cig"][i])])
            f.write(b"r%d\t0\t%s\t%d\t60\t%s\t*\t0\t0\t%s\t*\tNM:i:0\n" % (i, job["names"][int(recs["contig"][i])], int(recs["ref_start"][i]) + 1,
                                                                        cig.encode(), seq[so:so + int(recs["seq_len"][i])]))
    return fa, sam


# ---- T1 -----------------------------------------------------------------------------------------------------------------------------
T1_NAMES = tuple(("chromosome_%d|a_long_name_as_assemblers_write_them|length=1600|coverage=40.0x|circular=false|" % (i + 1) + "x" * 40)[:n]
                 for i, n in enumerate((90, 97, 103)))


def t1_files(tmp):
    """(fasta, [sam1, sam2]) of a random dataset of three contigs whose names are T1_NAMES in the FASTA, the @SQ lines and the records"""
    ds = synth.rich_dataset(tmp, seed=31, contig_lens=(1600, 1000, 700), coverage=40)
    new = {"contig_%d" % (i + 1): n for i, n in enumerate(T1_NAMES)}
    out = []
    for key in ("fasta", "sam1", "sam2"):
        lines = open(ds[key]).read().split("\n")
        for i, ln in enumerate(lines):
            if ln[:1] == ">":
                word, _, rest = ln[1:].partition(" ")  # (a description behind the name stays)
                lines[i] = ">" + new[word] + (" " + rest if rest else "")
            elif ln.startswith("@SQ"):
                lines[i] = "\t".join("SN:" + new[f[3:]] if f.startswith("SN:") else f for f in ln.split("\t"))
            elif ln and ln[0] != "@" and key != "fasta":
                f = ln.split("\t")
                f[2], f[6] = new.get(f[2], f[2]), new.get(f[6], f[6])
                lines[i] = "\t".join(f)
        path = os.path.join(tmp, "long_" + os.path.basename(ds[key]))
        with open(path, "w") as fh:
            fh.write("\n".join(lines))
        out.append(path)
    return out[0], out[1:]


def blocks(body):
    """the bytes of every full block of BLOCK consecutive lines of a TSV body, from line 0 on"""
    ln = [len(x) + 1 for x in body.split(b"\n")[:-1]]
    return [sum(ln[i:i + BLOCK]) for i in range(0, len(ln) - BLOCK + 1, BLOCK)]


# ---- T2 -----------------------------------------------------------------------------------------------------------------------------
# 118 bytes: with a name of this length byte WIN of the TSV -- the first of the second staging window -- is a comma of the long line
T2_NAME = ("hand-built|" + "one_line_of_this_job_is_longer_than_a_staging_window|" * 3)[:118]
T2 = {"long": 0, "winners": {200: 125, 300: 126, 400: 127, 500: 200}, "items12": 600, "items13": 700, "n_long": 140}


def t2_files(tmp):
    """(fasta, sam): one contig of 1000 bases.  Position 0 lies under 140 reads with 140 different 126-base insertions (items with
    keys of 127 bytes, one read each: nothing wins) and three plain reads; 200, 300, 400 and 500 under 12 identical reads with an
    insertion of 125, 126, 127 and 200 bases (they win); 600 and 700 under reads that carry A, C, G, T and 8 / 9 other bytes there:
    12 and 13 items.  No two positions' reads overlap."""
    rng = np.random.default_rng(48)
    dna = lambda n: "".join("ACGT"[i] for i in rng.integers(0, 4, n))  # noqa: E731
    ref = dna(1000)
    alns = []

    def ins_read(p, ins, left=15, right=15):
        s = p - left + 1
        alns.append(("r%d" % len(alns), T2_NAME, s, "%dM%dI%dM" % (left, len(ins), right), ref[s:p + 1] + ins + ref[p + 1:p + 1 + right]))

    def sub_read(p, b, n=30):
        s = p - 12
        alns.append(("r%d" % len(alns), T2_NAME, s, "%dM" % n, ref[s:p] + b + ref[p + 1:s + n]))

    seen = set()
    while len(seen) < T2["n_long"]:
        seen.add(dna(126))
    for ins in sorted(seen):
        ins_read(T2["long"], ins, left=1)  # (position 0: the read begins with its one base there)
    for _ in range(3):
        alns.append(("r%d" % len(alns), T2_NAME, 0, "30M", ref[:30]))
    for p, n in T2["winners"].items():
        ins = dna(n)
        for _ in range(12):
            ins_read(p, ins)
    for p, extra in ((T2["items12"], "NRYKMSWB"), (T2["items13"], "NRYKMSWBD")):
        for b in "ACGT" + extra:
            sub_read(p, b)
        sub_read(p, ref[p])
    return _write_job(tmp, [(T2_NAME, ref)], alns, name="t2")


def tsv_lines(body):
    return body.split(b"\n")[:-1]


def comma_cut(body, long_line):
    """a first position lo <= long_line such that, in the TSV of the positions from lo on, the byte at WIN -- the first of the second
    staging window of the workgroup that begins with line lo -- is a comma of the long line; None if there is none"""
    lines = tsv_lines(body)
    for lo in range(long_line, max(long_line - BLOCK, -1), -1):
        before = sum(len(x) + 1 for x in lines[lo:long_line])
        k = WIN - before
        if 0 <= k < len(lines[long_line]) and lines[long_line][k:k + 1] == b",":
            return lo
    return None
