"""`polypolish polish / filter / filter-polish` on BAM files: the commands join the device links of the record chain themselves
(pp_aln_file_kind -> pp_bgzf_inflate -> pp_bam_header -> pp_bgzf_bam_walk -> pp_bam_records -> pp_names -> pp_filter_records ->
pp_batch_gate -> pp_polish_*, and pp_bam_tagged -> pp_bam_out_deflate on the write side), against the oracle on the SAM text.
The dataset is the chain tests' (tests/test_bgzf_chain_gpu.py): header in REVERSE FASTA order, blocks cut every 4,093 bytes and never
at a record boundary, a stored block, a Z_FIXED block and a mid-file EOF block mixed in.  The error and order cases are one small
hand-built file each.  Every test runs bin/polypolish as a child process.  Needs an MI355X: `-m gpu`."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import bam_model as bm
import bam_tag_model as tm
import bgzf_deflate_model as D
import bgzf_model as zm
from test_bgzf_chain_gpu import MAX_ERRORS, bgzf_file, cut_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "polypolish")
pytestmark = pytest.mark.gpu


def run(*argv, env=None):
    r = subprocess.run([EXE, *map(str, argv)], capture_output=True, env=dict(os.environ, **(env or {})), timeout=300)
    if r.returncode < 0 or r.returncode in (134, 139) or b"illegal memory access" in r.stderr:  # a crash is a finding: nothing more is started on the device
        pytest.exit(f"polypolish {' '.join(map(str, argv))} ended with {r.returncode}: {r.stderr.decode()[-600:]}", returncode=3)
    return r


def put(path, data):
    with open(path, "wb") as f:
        f.write(data)
    return str(path)


@pytest.fixture(scope="module")
def ds(tmp_path_factory, orc):
    import synth
    d = str(tmp_path_factory.mktemp("bam_cli"))
    s = synth.rich_dataset(d, seed=23, contig_lens=(4000, 2500), coverage=30, repeat_len=400, repeat_copies=3, zp_frac=0.02)
    contigs = [(c.name, c.assembly) for c in s["contigs"]]
    header_order = [name for name, _ in contigs][::-1]
    lens = [len(dict(contigs)[n]) for n in header_order]
    sams = [s["sam1"], s["sam2"]]
    outs = [os.path.join(d, f"oracle_filtered_{i}.sam") for i in (1, 2)]
    report = orc.filter_files(sams[0], sams[1], outs[0], outs[1])
    bams, raws, want_filtered, streams = [], [], [], []
    for f, path in enumerate(sams):
        text = open(path, "rb").read()
        enc = bm.encode(text, header_order, lens)
        data = enc["header"] + enc["records"]
        at = len(enc["header"])
        starts = set((enc["rec_off"] + np.uint64(at)).tolist())
        cuts = cut_points(len(data), starts)
        assert len(cuts) > 8 and not set(cuts[1:]) & starts, "records straddle the blocks"
        bams.append(put(os.path.join(d, f"reads_{f + 1}.bam"), bgzf_file(data, cuts)))
        raws.append(put(os.path.join(d, f"reads_{f + 1}.raw.bam"), data))
        verdict = tm.own_verdicts(text, open(outs[f], "rb").read())
        assert (verdict == 0).any()
        streams.append(tm.tagged(data, at, enc["rec_off"] + np.uint64(at), verdict))
        want_filtered.append(D.deflate_file(streams[-1])[0])
    return {"fasta": s["fasta"], "sams": sams, "bams": bams, "raws": raws, "outs": outs, "report": report, "want_filtered": want_filtered,
            "streams": streams,
            "polish": orc.polish_files(s["fasta"], sams, max_errors=MAX_ERRORS),
            "per_file": [orc.polish_files(s["fasta"], [p], max_errors=MAX_ERRORS)["counts"] for p in sams],
            "polish_filtered": orc.polish_files(s["fasta"], outs, max_errors=MAX_ERRORS)["fasta"], "dir": d}


def test_polish_on_the_bam_pair_is_the_oracle_s_fasta_and_counts(ds):
    r = run("polish", ds["fasta"], *ds["bams"])
    log = r.stderr.decode()
    assert r.returncode == 0 and r.stdout == ds["polish"]["fasta"], log[-800:]
    for path, (alignments, _, reads) in zip(ds["bams"], ds["per_file"]):
        assert f"{path}: {alignments:,} alignments from {reads:,} reads\n" in log
    total, used, _ = ds["polish"]["counts"]
    assert f"  {used:,} alignments kept\n  {total - used:,} alignments discarded\n" in log


@pytest.mark.parametrize("argv, kw", [(["--careful"], dict(careful=True)), (["--max_errors", "2"], dict(max_errors=2))])
def test_polish_on_the_bam_pair_with_options(ds, orc, argv, kw):
    want = orc.polish_files(ds["fasta"], ds["sams"], **kw)
    r = run("polish", *argv, ds["fasta"], *ds["bams"])
    assert r.returncode == 0 and r.stdout == want["fasta"], r.stderr.decode()[-800:]
    assert f"  {want['counts'][1]:,} alignments kept\n".encode() in r.stderr


def test_polish_debug_tsv_from_bam_is_the_oracle_s(ds, orc, tmp_path):
    want = orc.polish_files(ds["fasta"], ds["sams"], debug=True)
    tsv = str(tmp_path / "debug.tsv")
    r = run("polish", "--debug", tsv, ds["fasta"], *ds["bams"])
    assert r.returncode == 0 and r.stdout == want["fasta"], r.stderr.decode()[-800:]
    assert open(tsv, "rb").read() == want["debug"]


def test_polish_on_uncompressed_bam_and_with_the_prepared_route(ds):
    r = run("polish", ds["fasta"], *ds["raws"])
    assert r.returncode == 0 and r.stdout == ds["polish"]["fasta"], r.stderr.decode()[-800:]
    r = run("polish", ds["fasta"], *ds["bams"], env=dict(PP_BAM_PREPARE="1"))
    assert r.returncode == 0 and r.stdout == ds["polish"]["fasta"], r.stderr.decode()[-800:]


@pytest.fixture(scope="module")
def filtered(ds):
    """`polypolish filter` BAM -> BAM, once"""
    outs = [os.path.join(ds["dir"], f"filtered_{i}.bam") for i in (1, 2)]
    r = run("filter", "--in1", ds["bams"][0], "--in2", ds["bams"][1], "--out1", outs[0], "--out2", outs[1])
    assert r.returncode == 0 and r.stdout == b"", r.stderr.decode()[-800:]
    return outs, r.stderr.decode()


def test_filter_writes_the_model_s_compressed_bam_files_and_the_oracle_s_report(ds, filtered):
    outs, log = filtered
    for f in range(2):
        got = open(outs[f], "rb").read()
        assert got == ds["want_filtered"][f], f
        assert gzip.decompress(got) == ds["streams"][f], "gzip reads the file back to the tagged records"
    rep = ds["report"]
    for name, n in zip(("fr", "rf", "ff", "rr"), rep["counts"]):
        assert f"{name}: {n:,} pairs\n" in log
    assert f"Automatically determined correct orientation: {rep['orientation']}\n" in log
    assert re.search(rf"Low threshold:  {rep['low']} \(", log) and re.search(rf"High threshold: {rep['high']} \(", log)
    assert f"Alignments before filtering: {rep['before']:,}\nAlignments after filtering:  {rep['after']:,}\n" in log


def test_polish_on_the_filtered_bam_files_is_the_oracle_s_two_commands(ds, filtered):
    r = run("polish", ds["fasta"], *filtered[0])
    assert r.returncode == 0 and r.stdout == ds["polish_filtered"], r.stderr.decode()[-800:]


def test_filter_polish_on_the_bam_pair(ds, filtered, tmp_path):
    r = run("filter-polish", "--in1", ds["bams"][0], "--in2", ds["bams"][1], ds["fasta"])
    assert r.returncode == 0 and r.stdout == ds["polish_filtered"], r.stderr.decode()[-800:]
    outs = [str(tmp_path / f"fused_{i}.bam") for i in (1, 2)]
    r = run("filter-polish", "--in1", ds["bams"][0], "--in2", ds["bams"][1], "--out1", outs[0], "--out2", outs[1], ds["fasta"])
    assert r.returncode == 0 and r.stdout == ds["polish_filtered"], r.stderr.decode()[-800:]
    for f in range(2):
        assert open(outs[f], "rb").read() == open(filtered[0][f], "rb").read(), f


def test_the_python_face_inherits_bam(ds, tmp_path):
    import polypolish_amd as pp
    ctx = pp.Context(0)
    try:
        assert ctx.polish_files(ds["fasta"], ds["bams"]) == ds["polish"]["fasta"]
        outs = [str(tmp_path / f"py_{i}.bam") for i in (1, 2)]
        rep = ctx.filter_files(ds["bams"][0], ds["bams"][1], outs[0], outs[1])
        assert rep["after"] == ds["report"]["after"] and rep["low"] == ds["report"]["low"] and rep["high"] == ds["report"]["high"]
        for f in range(2):
            assert open(outs[f], "rb").read() == ds["want_filtered"][f], f
    finally:
        ctx.close()


# ---- errors and their order: small hand-built files ------------------------------------------------------------------------------
ASM = "".join("ACGT"[(i * 7 + i // 3 + i // 11) % 4] for i in range(400))
NM0 = bm.aux("NM", "C", 0)


def good(qname, pos, n=40, flag=0, aux=NM0, ref_id=0, seq=None, runs=None):
    return bm.record(qname, flag, ref_id, pos, [n << 4] if runs is None else runs, ASM[pos:pos + n] if seq is None else seq, aux)


def star(qname, pos, n=40, flag=256):
    """an aligned record without SEQ (l_seq 0)"""
    return bm.record(qname, flag, 0, pos, [n << 4], "", NM0)


def bam_file(path, records, refs=(("ctg", len(ASM)),), per_block=2):
    """header and records as BGZF, `per_block` records to a block"""
    head = bm.header_bytes(list(refs), "")
    pieces = [head] + [b"".join(records[i:i + per_block]) for i in range(0, len(records), per_block)]
    return put(path, b"".join(zm.block(p, 6) for p in pieces) + zm.EOF_BLOCK)


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    d = tmp_path_factory.mktemp("bam_cli_small")
    fasta = put(d / "asm.fasta", (">ctg\n" + ASM + "\n").encode())
    reads = [good(b"r%d" % i, 10 * i) for i in range(12)]
    return {"dir": d, "fasta": fasta, "reads": reads, "ok": bam_file(d / "ok.bam", reads)}


def refused(r, code, *words):
    err = r.stderr.decode()
    assert r.returncode == code and r.stdout == b"", (r.returncode, err[-600:])
    assert "Error: " in err
    for w in words:
        assert str(w) in err.split("Error: ")[-1], (w, err[-600:])


def test_the_small_good_file_polishes(small):
    r = run("polish", small["fasta"], small["ok"])
    assert r.returncode == 0 and r.stdout == (">ctg polypolish\n" + ASM + "\n").encode(), r.stderr.decode()[-600:]


def test_gzip_that_is_not_bgzf_and_bgzf_that_is_not_bam(small):
    d, reads = small["dir"], small["reads"]
    plain = put(d / "plain.bam.gz", gzip.compress(bm.header_bytes([("ctg", len(ASM))]) + b"".join(reads)))
    refused(run("polish", small["fasta"], plain), 1, plain, "is gzip-compressed but not BGZF")
    text = b"@SQ\tSN:ctg\tLN:400\nr1\t0\tctg\t1\t60\t40M\t*\t0\t0\t" + ASM[:40].encode() + b"\t*\tNM:i:0\n"
    bgz = put(d / "text.sam.gz", zm.block(text, 6) + zm.EOF_BLOCK)
    refused(run("polish", small["fasta"], bgz), 1, bgz, "is BGZF-compressed but does not hold BAM")
    refused(run("filter", "--in1", bgz, "--in2", small["ok"], "--out1", d / "x1.bam", "--out2", d / "x2.bam"), 1, bgz, "does not hold BAM")


def test_bgzf_defects_name_the_path_and_the_block(small):
    d = small["dir"]
    whole = open(small["ok"], "rb").read()
    off, _, end, ok = zm.walk(whole)
    assert ok and len(off) >= 5
    crc_at = int(off[3]) - 8                                   # the CRC32 of the third block
    flipped = put(d / "crc.bam", whole[:crc_at] + bytes([whole[crc_at] ^ 0x10]) + whole[crc_at + 1:])
    refused(run("polish", small["fasta"], flipped), 1, flipped, "(block 3)", "CRC")
    cut = put(d / "cut.bam", whole[:int(off[2]) + 25])         # the file ends inside its third block
    refused(run("polish", small["fasta"], cut), 1, cut, "(block 3)")


def test_a_block_size_chain_break_names_the_record(small):
    d, reads = small["dir"], small["reads"]
    long_one = bm.record(b"far", 0, 0, 0, [40 << 4], ASM[:40], NM0, block_size=100000)
    broken = bam_file(d / "chain.bam", reads[:5] + [long_one])
    refused(run("polish", small["fasta"], broken), 1, broken, "(record 6)")


def test_nm_defects(small):
    d, reads = small["dir"], small["reads"]
    no_nm = bam_file(d / "no_nm.bam", reads[:4] + [good(b"bare", 50, aux=b"")] + reads[5:])
    refused(run("polish", small["fasta"], no_nm), 1, no_nm, "missing NM tag", "(record 5)")
    refused(run("filter", "--in1", no_nm, "--in2", small["ok"], "--out1", d / "y1.bam", "--out2", d / "y2.bam"), 1, no_nm, "missing NM tag", "(record 5)")
    negative = bam_file(d / "neg_nm.bam", reads[:2] + [good(b"neg", 20, aux=bm.aux("NM", "i", -1))] + reads[3:])
    refused(run("polish", small["fasta"], negative), 101, negative, "(record 3)")


def test_files_without_usable_alignments(small):
    d = small["dir"]
    unaligned = bam_file(d / "unaligned.bam", [bm.record(b"u%d" % i, 4, -1, -1, [], ASM[:30], b"") for i in range(5)])
    refused(run("polish", small["fasta"], unaligned), 1, f'no alignments in "{unaligned}"')
    stars = bam_file(d / "stars.bam", small["reads"][:3] + [star(b"hollow", 100, flag=0), star(b"hollow", 200)] + small["reads"][3:])
    refused(run("polish", small["fasta"], stars), 1, "no alignments for read hollow contain sequence", stars, "(record 4)")


def test_a_reference_the_assembly_lacks(small):
    d = small["dir"]
    refs = (("ghost", 1000), ("ctg", len(ASM)))
    recs = [good(b"r%d" % i, 10 * i, ref_id=1) for i in range(4)] + [good(b"lost", 30, ref_id=0)] + [good(b"s", 90, ref_id=1)]
    f = bam_file(d / "ghost.bam", recs, refs=refs)
    refused(run("polish", small["fasta"], f), 1, "query name ghost in SAM but not in assembly", f, "(record 5)")


def test_mixed_kinds_and_several_gpus_are_refused(small):
    d = small["dir"]
    text = b"@SQ\tSN:ctg\tLN:400\nr1\t0\tctg\t1\t60\t40M\t*\t0\t0\t" + ASM[:40].encode() + b"\t*\tNM:i:0\n"
    sam = put(d / "one.sam", text)
    refused(run("polish", small["fasta"], sam, small["ok"]), 1, sam, small["ok"], "SAM text", "BAM")
    refused(run("filter", "--in1", small["ok"], "--in2", sam, "--out1", d / "z1", "--out2", d / "z2"), 1, sam, small["ok"], "both")
    refused(run("polish", small["fasta"], small["ok"], env=dict(PP_GPUS="2")), 1, small["ok"], "one GPU")


def test_the_first_error_in_streaming_order_stands(small):
    """the reference streams: what it meets first is what it reports"""
    d, reads = small["dir"], small["reads"]
    hollow = [star(b"hollow", 100, flag=0), star(b"hollow", 200)]
    bare = good(b"bare", 50, aux=b"")
    # an all-* group two groups ahead of the missing NM: the gate's sentence
    f = bam_file(d / "order_a.bam", reads[:3] + hollow + reads[3:5] + [bare] + reads[5:])
    refused(run("polish", small["fasta"], small["ok"], f, small["ok"]), 1, "no alignments for read hollow contain sequence", f, "(record 4)")
    # the two swapped: the decode's
    f = bam_file(d / "order_b.bam", reads[:3] + [bare] + reads[3:5] + hollow + reads[5:])
    refused(run("polish", small["fasta"], small["ok"], f, small["ok"]), 1, "missing NM tag", f, "(record 4)")
    # the all-* group still pending at the missing NM is never processed
    f = bam_file(d / "order_c.bam", reads[:3] + hollow + [bare] + reads[3:])
    refused(run("polish", small["fasta"], f), 1, "missing NM tag", f, "(record 6)")
    # a CIGAR / SEQ length mismatch that only the walk rejects, in the file before the one with the missing NM: the walk's
    short = good(b"short", 60, runs=[39 << 4])
    f1 = bam_file(d / "order_d1.bam", reads[:6] + [short] + reads[6:])
    f2 = bam_file(d / "order_d2.bam", reads[:3] + [bare] + reads[3:])
    refused(run("polish", small["fasta"], f1, f2, small["ok"]), 1, "does not match read sequence", f1, "(record 7)")
