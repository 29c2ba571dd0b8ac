"""`polypolish filter / filter-polish --out_sam`: BAM in, SAM text out through pp_bam_sam -> pp_sam_out_write, against the oracle: the
files are, byte for byte, the oracle's filtered SAM files of the text the BAM inputs were made from.  That text is the canonical form
of the dataset of tests/test_out_bam_cli_gpu.py (QUAL as long as SEQ, SEQ upper-cased); the BAM inputs are sam_bam_model.encode(text)
framed as BGZF, so that l_text carries the SAM's own header.  Every test runs bin/polypolish as a child process.
Needs an MI355X: `-m gpu`."""
import os
import re

import pytest

import sam_bam_model as sb
from test_bam_cli_gpu import put, run
from test_bam_sam_chain_gpu import canonical_texts
from test_bgzf_chain_gpu import MAX_ERRORS, bgzf_file, cut_points

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ds(tmp_path_factory, orc):
    import synth
    d = str(tmp_path_factory.mktemp("out_sam_cli"))
    s = synth.rich_dataset(d, seed=23, contig_lens=(4000, 2500), coverage=30, repeat_len=400, repeat_copies=3, zp_frac=0.02)
    texts = canonical_texts(s)
    sams = [put(os.path.join(d, f"canonical_{f + 1}.sam"), t) for f, t in enumerate(texts)]
    outs = [os.path.join(d, f"oracle_filtered_{i}.sam") for i in (1, 2)]
    report = orc.filter_files(sams[0], sams[1], outs[0], outs[1])
    bams, encs = [], []
    for f, text in enumerate(texts):
        enc = sb.encode(text)
        encs.append(enc)
        bams.append(put(os.path.join(d, f"reads_{f + 1}.bam"), bgzf_file(enc["bytes"], cut_points(len(enc["bytes"]), set(enc["rec_off"].tolist())))))
    want = [open(p, "rb").read() for p in outs]
    assert all(b"\tZP:Z:fail\n" in w for w in want)
    return {"fasta": s["fasta"], "sams": sams, "texts": texts, "outs": outs, "report": report, "want": want, "bams": bams, "encs": encs,
            "polish_filtered": orc.polish_files(s["fasta"], outs, max_errors=MAX_ERRORS)["fasta"], "dir": d}


def io(ins, outs):
    return ["--in1", ins[0], "--in2", ins[1], "--out1", outs[0], "--out2", outs[1]]


def the_log(r, outs):
    """a filter run's log without what differs between two runs by design: the outputs' names, the time and the lap's word"""
    log = r.stderr.decode()
    for k, p in enumerate(outs):
        log = log.replace(p, f"<out{k + 1}>")
    return re.sub(r"Time to run: .*\n", "", log).replace("filtered BAMs written", "filtered <kind> written").replace("filtered SAMs written", "filtered <kind> written")


@pytest.fixture(scope="module")
def filtered(ds):
    """`polypolish filter --out_sam` on the BAM pair, once, and the BAM -> BAM run next to it"""
    outs = [os.path.join(ds["dir"], f"filtered_{i}.sam") for i in (1, 2)]
    plain = [os.path.join(ds["dir"], f"filtered_{i}.bam") for i in (1, 2)]
    r = run("filter", "--out_sam", *io(ds["bams"], outs))
    assert r.returncode == 0 and r.stdout == b"", r.stderr.decode()[-800:]
    p = run("filter", *io(ds["bams"], plain))
    assert p.returncode == 0, p.stderr.decode()[-800:]
    return outs, plain, the_log(r, outs), the_log(p, plain)


def test_filter_out_sam_writes_the_oracle_s_filtered_files(ds, filtered):
    outs, plain, log, plain_log = filtered
    for f in range(2):
        got = open(outs[f], "rb").read()
        assert got == ds["want"][f], f
        assert open(plain[f], "rb").read()[:4] == b"\x1f\x8b\x08\x04", "without the flag: BAM files as before"
    assert log == plain_log, "the counts and the log are the BAM -> BAM run's"
    rep = ds["report"]
    assert f"Alignments before filtering: {rep['before']:,}\nAlignments after filtering:  {rep['after']:,}\n" in log
    assert log.count(" pass\n") == 2 and log.count(" fail\n") == 2


def test_polish_on_the_written_files_is_the_oracle_s_two_commands(ds, filtered):
    r = run("polish", ds["fasta"], *filtered[0])
    assert r.returncode == 0 and r.stdout == ds["polish_filtered"], r.stderr.decode()[-800:]


def test_filter_polish_out_sam_with_and_without_outputs(ds, filtered, tmp_path):
    outs = [str(tmp_path / f"fused_{i}.sam") for i in (1, 2)]
    r = run("filter-polish", "--out_sam", *io(ds["bams"], outs), ds["fasta"])
    assert r.returncode == 0 and r.stdout == ds["polish_filtered"], r.stderr.decode()[-800:]
    for f in range(2):
        assert open(outs[f], "rb").read() == ds["want"][f], f
    r = run("filter-polish", "--out_sam", "--in1", ds["bams"][0], "--in2", ds["bams"][1], ds["fasta"])      # no outputs: the plain FASTA
    assert r.returncode == 0 and r.stdout == ds["polish_filtered"], r.stderr.decode()[-800:]


def test_sam_text_inputs_with_the_flag_write_what_they_write_without_it(ds, tmp_path):
    a = [str(tmp_path / f"with_{i}.sam") for i in (1, 2)]
    assert run("filter", "--out_sam", *io(ds["sams"], a)).returncode == 0
    for f in range(2):
        assert open(a[f], "rb").read() == ds["want"][f], f


def test_both_flags_on_bam_inputs_write_text(ds, tmp_path):
    a = [str(tmp_path / f"both_{i}.sam") for i in (1, 2)]
    assert run("filter", "--out_bam", "--out_sam", *io(ds["bams"], a)).returncode == 0
    for f in range(2):
        assert open(a[f], "rb").read() == ds["want"][f], f


def test_a_refused_record_ends_the_command_and_leaves_nothing_behind(ds, tmp_path):
    enc = ds["encs"][1]
    b, off = bytearray(enc["bytes"]), enc["rec_off"]
    k = 40
    at = int(off[k]) + 36
    assert 0x21 <= b[at + 1] <= 0x7E and b[at + 2] != 0
    b[at + 1] = 9                                   # a tab inside the QNAME of record k
    bad = put(tmp_path / "tab_2.bam", bgzf_file(bytes(b), cut_points(len(b), set(off.tolist()))))
    outs = [str(tmp_path / f"never_{i}.sam") for i in (1, 2)]
    r = run("filter", "--out_sam", *io([ds["bams"][0], bad], outs))
    msg = r.stderr.decode()
    assert r.returncode == 1, msg[-800:]
    assert f'"{bad}"' in msg and f"record {k + 1})" in msg and "--out_sam" in msg and "QNAME" in msg, msg[-800:]
    assert not os.path.exists(outs[0]) and not os.path.exists(outs[1])
    plain = [str(tmp_path / f"plain_{i}.bam") for i in (1, 2)]
    assert run("filter", *io([ds["bams"][0], bad], plain)).returncode == 0, "without the flag the record is copied like any other"


def test_the_flag_takes_no_value():
    r = run("filter", "--out_sam=1", "--in1", "a", "--in2", "b", "--out1", "c", "--out2", "d")
    assert r.returncode == 2 and b"unexpected value '1' for '--out_sam' found; no more were expected" in r.stderr
    assert b"--out_sam" in run("filter", "--help").stdout and b"--out_sam" in run("filter-polish", "--help").stdout


def test_the_python_face(ds, tmp_path):
    import polypolish_amd as pp
    ctx = pp.Context(0)
    try:
        outs = [str(tmp_path / f"py_{i}.sam") for i in (1, 2)]
        rep = ctx.filter_files(ds["bams"][0], ds["bams"][1], outs[0], outs[1], out_sam=True)
        assert rep["after"] == ds["report"]["after"] and [open(p, "rb").read() for p in outs] == ds["want"]
        again = [str(tmp_path / f"py_{i}.bam") for i in (1, 2)]
        ctx.filter_files(ds["bams"][0], ds["bams"][1], again[0], again[1])
        assert open(again[0], "rb").read()[:4] == b"\x1f\x8b\x08\x04", "the flag held for one call"
        fasta, _ = ctx.filter_polish_files(ds["fasta"], ds["bams"][0], ds["bams"][1], outs[0], outs[1], out_sam=True, max_errors=MAX_ERRORS)
        assert fasta == ds["polish_filtered"] and [open(p, "rb").read() for p in outs] == ds["want"]
    finally:
        ctx.close()
