"""`polypolish filter / filter-polish --out_bam`: SAM text in, compressed BAM out through pp_sam_bam -> pp_bam_tagged ->
pp_bam_out_deflate -> pp_bgzf_out_write, against the models (the files byte for byte) and the oracle (verdicts, report, FASTA).  The
dataset is that of tests/test_bam_cli_gpu.py with its QUAL columns made as long as their SEQ (sam_bam_model.with_fitting_qual: the
dataset's own lines with an indel are no valid SAM and the encoder refuses them).  Every test runs bin/polypolish as a child process.
Needs an MI355X: `-m gpu`."""
import gzip
import os
import re

import numpy as np
import pytest

import bam_model as bm
import bam_tag_model as tm
import bgzf_deflate_model as D
import sam_bam_model as sb
from test_bam_cli_gpu import put, run
from test_bgzf_chain_gpu import MAX_ERRORS, bgzf_file, cut_points

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ds(tmp_path_factory, orc):
    import synth
    d = str(tmp_path_factory.mktemp("out_bam_cli"))
    s = synth.rich_dataset(d, seed=23, contig_lens=(4000, 2500), coverage=30, repeat_len=400, repeat_copies=3, zp_frac=0.02)
    names, lens = [c.name for c in s["contigs"]], [len(c.assembly) for c in s["contigs"]]
    texts = [sb.with_fitting_qual(open(p, "rb").read()) for p in (s["sam1"], s["sam2"])]
    sams = [put(os.path.join(d, f"fitting_{f + 1}.sam"), t) for f, t in enumerate(texts)]
    outs = [os.path.join(d, f"oracle_filtered_{i}.sam") for i in (1, 2)]
    report = orc.filter_files(sams[0], sams[1], outs[0], outs[1])
    want, streams, bams = [], [], []
    for f, text in enumerate(texts):
        verdict = tm.own_verdicts(text, open(outs[f], "rb").read())
        assert (verdict == 0).any()
        model = sb.encode(text)
        streams.append(tm.tagged(model["bytes"], model["records_at"], model["rec_off"], verdict))
        want.append(D.deflate_file(streams[-1])[0])
        enc = bm.encode(text, names, lens)
        data = enc["header"] + enc["records"]
        bams.append(put(os.path.join(d, f"reads_{f + 1}.bam"), bgzf_file(data, cut_points(len(data), set()))))
    return {"fasta": s["fasta"], "sams": sams, "texts": texts, "outs": outs, "report": report, "want": want, "streams": streams, "bams": bams,
            "polish_filtered": orc.polish_files(s["fasta"], outs, max_errors=MAX_ERRORS)["fasta"], "dir": d}


def io(ins, outs):
    return ["--in1", ins[0], "--in2", ins[1], "--out1", outs[0], "--out2", outs[1]]


def the_log(r, outs):
    """a filter run's log without what differs between two runs by design: the outputs' names and the time"""
    log = r.stderr.decode()
    for k, p in enumerate(outs):
        log = log.replace(p, f"<out{k + 1}>")
    return re.sub(r"Time to run: .*\n", "", log)


@pytest.fixture(scope="module")
def filtered(ds):
    """`polypolish filter --out_bam` on the SAM pair, once, and the plain run next to it"""
    outs = [os.path.join(ds["dir"], f"filtered_{i}.bam") for i in (1, 2)]
    plain = [os.path.join(ds["dir"], f"filtered_{i}.sam") for i in (1, 2)]
    r = run("filter", "--out_bam", *io(ds["sams"], outs))
    assert r.returncode == 0 and r.stdout == b"", r.stderr.decode()[-800:]
    p = run("filter", *io(ds["sams"], plain))
    assert p.returncode == 0, p.stderr.decode()[-800:]
    return outs, plain, the_log(r, outs), the_log(p, plain)


def test_filter_out_bam_writes_the_models_files_with_the_oracle_s_verdicts(ds, filtered):
    outs, plain, log, plain_log = filtered
    for f in range(2):
        got = open(outs[f], "rb").read()
        assert got == ds["want"][f], f
        assert gzip.decompress(got) == ds["streams"][f] and len(got) < len(ds["texts"][f]) // 3
        assert open(plain[f], "rb").read() == open(ds["outs"][f], "rb").read(), "without the flag: the text files as before"
    assert log == plain_log, "the counts and the log are the plain run's"
    rep = ds["report"]
    assert f"Alignments before filtering: {rep['before']:,}\nAlignments after filtering:  {rep['after']:,}\n" in log
    assert log.count(" pass\n") == 2 and log.count(" fail\n") == 2


def test_polish_on_the_written_files_is_the_oracle_s_two_commands(ds, filtered):
    r = run("polish", ds["fasta"], *filtered[0])
    assert r.returncode == 0 and r.stdout == ds["polish_filtered"], r.stderr.decode()[-800:]


def test_filter_polish_out_bam(ds, filtered, tmp_path):
    outs = [str(tmp_path / f"fused_{i}.bam") for i in (1, 2)]
    r = run("filter-polish", "--out_bam", *io(ds["sams"], outs), ds["fasta"])
    assert r.returncode == 0 and r.stdout == ds["polish_filtered"], r.stderr.decode()[-800:]
    for f in range(2):
        assert open(outs[f], "rb").read() == ds["want"][f], f
    r = run("filter-polish", "--out_bam", "--in1", ds["sams"][0], "--in2", ds["sams"][1], ds["fasta"])      # no outputs: the plain FASTA
    assert r.returncode == 0 and r.stdout == ds["polish_filtered"], r.stderr.decode()[-800:]


def test_bam_inputs_with_the_flag_write_what_they_write_without_it(ds, tmp_path):
    a = [str(tmp_path / f"with_{i}.bam") for i in (1, 2)]
    b = [str(tmp_path / f"without_{i}.bam") for i in (1, 2)]
    assert run("filter", "--out_bam", *io(ds["bams"], a)).returncode == 0 and run("filter", *io(ds["bams"], b)).returncode == 0
    for f in range(2):
        assert open(a[f], "rb").read() == open(b[f], "rb").read() and len(open(a[f], "rb").read()) > 1000, f


def test_a_refused_line_ends_the_command_and_leaves_nothing_behind(ds, tmp_path):
    lines = ds["texts"][1].split(b"\n")
    k = next(i for i, ln in enumerate(lines) if ln and ln[:1] != b"@") + 40
    lines[k] += b"\tde:f:nan"
    bad = put(tmp_path / "nan_2.sam", b"\n".join(lines))
    outs = [str(tmp_path / f"never_{i}.bam") for i in (1, 2)]
    r = run("filter", "--out_bam", *io([ds["sams"][0], bad], outs))
    msg = r.stderr.decode()
    assert r.returncode == 1, msg[-800:]
    assert f'"{bad}"' in msg and f"line {k + 1})" in msg and "--out_bam" in msg and "de" in msg, msg[-800:]
    assert not os.path.exists(outs[0]) and not os.path.exists(outs[1])
    plain = [str(tmp_path / f"plain_{i}.sam") for i in (1, 2)]
    assert run("filter", *io([ds["sams"][0], bad], plain)).returncode == 0, "without the flag the line is copied like any other"
    assert b"\tde:f:nan\n" in open(plain[1], "rb").read()


def test_the_python_face(ds, tmp_path):
    import polypolish_amd as pp
    ctx = pp.Context(0)
    try:
        outs = [str(tmp_path / f"py_{i}.bam") for i in (1, 2)]
        rep = ctx.filter_files(ds["sams"][0], ds["sams"][1], outs[0], outs[1], out_bam=True)
        assert rep["after"] == ds["report"]["after"] and [open(p, "rb").read() for p in outs] == ds["want"]
        texts = [str(tmp_path / f"py_{i}.sam") for i in (1, 2)]
        ctx.filter_files(ds["sams"][0], ds["sams"][1], texts[0], texts[1])
        assert open(texts[0], "rb").read() == open(ds["outs"][0], "rb").read(), "the flag held for one call"
        fasta, _ = ctx.filter_polish_files(ds["fasta"], ds["sams"][0], ds["sams"][1], outs[0], outs[1], out_bam=True, max_errors=MAX_ERRORS)
        assert fasta == ds["polish_filtered"] and [open(p, "rb").read() for p in outs] == ds["want"]
    finally:
        ctx.close()
