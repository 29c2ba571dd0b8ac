"""`polypolish polish` and `filter-polish` with --bed, --bed_bgzf, --soft_mask and --bed_status (pp_ctx_set_bed, pp_ctx_set_soft_mask:
pp_polish_bed and pp_polish_masked behind the drivers' polish) on the golden pair (tests/golden/derived_e2e), from SAM text and from
BAM: the BED is the model's text (tests/bed_model.py) of the ORACLE's per-position statuses, plain and bgzipped; stdout and the log are
the plain run's, but for the FASTA's case under --soft_mask, which is the model's on the oracle's output; a --vcf alongside is the plain
run's file; the usage errors, the refusal of several contexts and an unwritable path leave nothing behind; the same through Python.
Every command test runs bin/polypolish as a child process.  Needs an MI355X: `-m gpu`."""
import ctypes as C
import gzip
import os
import re
import zlib

import numpy as np
import pytest

import bam_model
import bed_model as bm
import fasta_model as fm
import fasta_text_model as tm
import sam_bam_model as sb
from test_bam_cli_gpu import put, run
from test_bgzf_chain_gpu import bgzf_file, cut_points

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "derived_e2e")
MIXED = "changed,too_close,low_depth"


def log_of(r):
    """stderr without what differs from run to run: the durations"""
    return re.sub(rb"(Time to run: )[^\n]*", rb"\1-", r.stderr)


@pytest.fixture(scope="module")
def pp():
    import polypolish_amd
    return polypolish_amd


@pytest.fixture(scope="module")
def ds(tmp_path_factory, orc):
    d = str(tmp_path_factory.mktemp("bed_cli"))
    fa = os.path.join(GOLDEN, "case.fasta")
    names, _, off, bases = fm.parse(open(fa, "rb").read())
    lens = {n.decode(): int(off[i + 1] - off[i]) for i, n in enumerate(names)}
    texts = [sb.with_fitting_qual(open(os.path.join(GOLDEN, f"case_{f}.sam"), "rb").read()) for f in (1, 2)]
    sams = [put(os.path.join(d, f"case_{f + 1}.sam"), t) for f, t in enumerate(texts)]
    bams = []
    for f, text in enumerate(texts):
        order = [ln.split("\t")[1][3:] for ln in text.decode().split("\n") if ln.startswith("@SQ")]
        enc = bam_model.encode(text, order, [lens[n] for n in order])
        b = enc["header"] + enc["records"]
        bams.append(put(os.path.join(d, f"case_{f + 1}.bam"), bgzf_file(b, cut_points(len(b), set()))))
    outs = [os.path.join(d, f"oracle_filtered_{i}.sam") for i in (1, 2)]
    orc.filter_files(sams[0], sams[1], outs[0], outs[1])
    want = {}
    for cmd, files in (("polish", sams), ("filter-polish", outs)):
        res = orc.polish_files(fa, files, positions=True)
        pos = res["positions"]
        heads, seqs = tm.parse_headers(res["fasta"])
        polished = b"".join(seqs)
        w = {"fasta": res["fasta"], "heads": heads, "seq_lens": [len(s) for s in seqs]}
        for key, mask in (("default", bm.UNDECIDED), ("mixed", bm.parse_status_list(MIXED))):
            w["bed_" + key] = bm.bed(pos["status"], off, names, mask)
            assert len(bm.parse(w["bed_" + key])) >= 1
            m = bm.masked(polished, pos["emit_len"], pos["status"], mask)
            assert m != polished and m.upper() == polished.upper()
            at = np.concatenate([[0], np.cumsum(w["seq_lens"])])
            w["masked_" + key] = b"".join(b">" + h + b"\n" + m[int(at[i]):int(at[i + 1])] + b"\n" for i, h in enumerate(heads))
        assert b"".join(b">" + h + b"\n" + s + b"\n" for h, s in zip(heads, seqs)) == res["fasta"], "the headers as tm.parse_headers gives them"
        want[cmd] = w
    return {"dir": d, "fasta": fa, "sams": sams, "bams": bams, "want": want}


def _command(ds, cmd, kind, *flags):
    files = ds["sams"] if kind == "sam" else ds["bams"]
    return ("polish", *flags, ds["fasta"], *files) if cmd == "polish" else ("filter-polish", *flags, "--in1", files[0], "--in2", files[1], ds["fasta"])


@pytest.mark.parametrize("kind", ["sam", "bam"])
@pytest.mark.parametrize("cmd", ["polish", "filter-polish"])
def test_the_bed_is_the_models_and_the_run_is_the_plain_one(ds, tmp_path, cmd, kind):
    w = ds["want"][cmd]
    path, gz, vcf, vcf0 = (str(tmp_path / n) for n in ("u.bed", "u.bed.gz", "with.vcf", "plain.vcf"))
    plain = run(*_command(ds, cmd, kind, "--vcf", vcf0))
    assert plain.returncode == 0 and plain.stdout == w["fasta"], plain.stderr.decode()[-800:]
    r = run(*_command(ds, cmd, kind, "--bed", path, "--vcf", vcf))
    assert r.returncode == 0 and r.stdout == plain.stdout and log_of(r) == log_of(plain), r.stderr.decode()[-800:]
    assert open(path, "rb").read() == w["bed_default"]
    assert open(vcf, "rb").read() == open(vcf0, "rb").read(), "--vcf alongside gives the plain run's file"
    assert not os.path.exists(str(tmp_path / "debug.tsv")) and len(os.listdir(str(tmp_path))) == 3, "with --bed alone no TSV is written"
    r = run(*_command(ds, cmd, kind, "--bed", gz, "--bed_bgzf", "--bed_status", MIXED))
    assert r.returncode == 0 and r.stdout == plain.stdout and log_of(r) == log_of(plain), r.stderr.decode()[-800:]
    data = open(gz, "rb").read()
    assert data[:4] == b"\x1f\x8b\x08\x04" and data[12:16] == b"BC\x02\x00", "BGZF blocks"
    text, at = b"", data
    while at:  # read back through zlib, member by member
        z = zlib.decompressobj(31)
        text += z.decompress(at)
        at = z.unused_data
    assert text == w["bed_mixed"] == gzip.decompress(data)


@pytest.mark.parametrize("kind", ["sam", "bam"])
@pytest.mark.parametrize("cmd", ["polish", "filter-polish"])
def test_soft_mask_lower_cases_the_models_bytes(ds, tmp_path, cmd, kind):
    w = ds["want"][cmd]
    vcf, vcf0, bed = (str(tmp_path / n) for n in ("with.vcf", "plain.vcf", "u.bed"))
    plain = run(*_command(ds, cmd, kind, "--vcf", vcf0))
    r = run(*_command(ds, cmd, kind, "--soft_mask", "--vcf", vcf, "--bed", bed))
    assert plain.returncode == 0 and r.returncode == 0, r.stderr.decode()[-800:]
    assert r.stdout == w["masked_default"] and r.stdout.upper() == plain.stdout.upper() and r.stdout != plain.stdout
    assert [ln for ln in r.stdout.split(b"\n") if ln[:1] == b">"] == [ln for ln in plain.stdout.split(b"\n") if ln[:1] == b">"], "headers are unchanged"
    assert log_of(r) == log_of(plain)
    assert open(vcf, "rb").read() == open(vcf0, "rb").read() and open(bed, "rb").read() == w["bed_default"]
    r = run(*_command(ds, cmd, kind, "--soft_mask", "--bed_status", MIXED))
    assert r.returncode == 0 and r.stdout == w["masked_mixed"]
    # the same with --wrap 60 --out_bgzf: the device's FASTA text link takes the masked bytes
    p = run(*_command(ds, cmd, kind, "--wrap", "60", "--out_bgzf"))
    r = run(*_command(ds, cmd, kind, "--wrap", "60", "--out_bgzf", "--soft_mask"))
    assert p.returncode == 0 and r.returncode == 0, r.stderr.decode()[-800:]
    got, base = gzip.decompress(r.stdout), gzip.decompress(p.stdout)
    assert got.upper() == base.upper() and got != base and log_of(r) == log_of(p)
    heads, seqs = tm.parse_headers(w["masked_default"])
    assert got == b"".join(b">" + h + b"\n" + b"".join(s[i:i + 60] + b"\n" for i in range(0, len(s), 60)) for h, s in zip(heads, seqs))


def test_soft_mask_with_out_and_index(ds, tmp_path):
    w = ds["want"]["polish"]
    out = str(tmp_path / "o.fa")
    p = run(*_command(ds, "polish", "sam", "--out", out, "--wrap", "70", "--index"))
    fai = open(out + ".fai", "rb").read()
    r = run(*_command(ds, "polish", "bam", "--out", out, "--wrap", "70", "--index", "--soft_mask"))
    assert p.returncode == 0 and r.returncode == 0 and r.stdout == b"", r.stderr.decode()[-800:]
    assert open(out + ".fai", "rb").read() == fai
    heads, seqs = tm.parse_headers(w["masked_default"])
    assert open(out, "rb").read() == b"".join(b">" + h + b"\n" + b"".join(s[i:i + 70] + b"\n" for i in range(0, len(s), 70)) for h, s in zip(heads, seqs))


def test_a_debug_file_alongside(ds, tmp_path):
    w = ds["want"]["polish"]
    tsv, tsv0, bed = (str(tmp_path / n) for n in ("d.tsv", "d0.tsv", "u.bed"))
    p = run(*_command(ds, "polish", "sam", "--debug", tsv0))
    r = run(*_command(ds, "polish", "sam", "--debug", tsv, "--bed", bed, "--soft_mask"))
    assert p.returncode == 0 and r.returncode == 0, r.stderr.decode()[-800:]
    assert open(tsv, "rb").read() == open(tsv0, "rb").read() and open(bed, "rb").read() == w["bed_default"] and r.stdout == w["masked_default"]
    assert bm.bed(bm.status_of_debug_tsv(open(tsv, "rb").read()), *_table(ds)) == w["bed_default"]


def _table(ds):
    names, _, off, _ = fm.parse(open(ds["fasta"], "rb").read())
    return off, names


def test_usage_errors_leave_nothing_behind(ds, tmp_path):
    bed = str(tmp_path / "u.bed")
    for cmd in ("polish", "filter-polish"):
        for flags, words in ((["--bed_bgzf"], b"--bed_bgzf needs --bed"), (["--bed_status", "none"], b"--bed_status needs --bed"),
                             (["--bed", bed, "--bed_status", "none,maybe"], b"'maybe' is not one of"), (["--bed", bed, "--bed_status", ""], b"empty status list"),
                             (["--soft_mask", "--bed_status", "kept,"], b"is not one of"), (["--bed", bed, "--bed", bed], b"multiple times")):
            r = run(*_command(ds, cmd, "sam", *flags))
            assert r.returncode == 2 and r.stdout == b"" and words in r.stderr, (cmd, flags, r.stderr[-300:])
            assert os.listdir(str(tmp_path)) == []
    # a run that fails leaves no file behind
    r = run("polish", "--bed", bed, ds["fasta"], str(tmp_path / "missing.sam"))
    assert r.returncode == 1 and os.listdir(str(tmp_path)) == []
    r = run("polish", "--bed", bed, "--soft_mask", "--fraction_valid", "2", ds["fasta"], *ds["sams"])
    assert r.returncode == 1 and r.stdout == b"" and os.listdir(str(tmp_path)) == []


@pytest.mark.parametrize("env", [dict(PP_SHARE_GPU="2"), dict(PP_GPUS="2")], ids=["share_gpu", "gpus"])
def test_several_contexts_are_refused_and_leave_no_file(ds, tmp_path, env):
    bed = str(tmp_path / "u.bed")
    r = run(*_command(ds, "polish", "sam", "--bed", bed), env=env)
    assert r.returncode == 1 and r.stdout == b"" and b"--bed runs on one GPU" in r.stderr and os.listdir(str(tmp_path)) == []
    assert b"Loading" not in r.stderr, "refused before any file is opened"
    r = run(*_command(ds, "polish", "sam", "--soft_mask"), env=env)
    assert r.returncode == 1 and r.stdout == b"" and b"--soft_mask runs on one GPU" in r.stderr and b"Loading" not in r.stderr


def test_an_unwritable_path(ds, tmp_path):
    nowhere = str(tmp_path / "no" / "such" / "dir" / "u.bed")
    for cmd in ("polish", "filter-polish"):
        r = run(*_command(ds, cmd, "sam", "--bed", nowhere))
        assert r.returncode == 1 and r.stdout == b"" and b'unable to write the BED to "' + nowhere.encode() + b'"' in r.stderr


def test_the_distributed_launcher_refuses_by_name():
    from polypolish_amd import distributed
    for argv, flag in ((["polish", "--bed", "x.bed", "a.fasta"], "--bed"), (["polish", "--soft_mask", "a.fasta"], "--soft_mask"),
                       (["polish", "--bed_status", "none", "a.fasta"], "--bed_status")):
        with pytest.raises(SystemExit) as e:
            distributed.main(argv)
        assert f"{flag} runs on one GPU" in str(e.value)


def test_the_same_through_python(ds, pp, tmp_path):
    w, wf = ds["want"]["polish"], ds["want"]["filter-polish"]
    path, fa = str(tmp_path / "py.bed"), ds["fasta"]
    c = pp.Context(0)
    try:
        with pytest.raises(pp.PolypolishError) as e:
            c.bed()
        assert e.value.code == pp.ERR_ARG and "pp_ctx_set_bed" in e.value.msg
        fasta = c.polish_files(fa, ds["sams"], bed=path)
        assert fasta == w["fasta"] and open(path, "rb").read() == w["bed_default"] == c.bed()
        fasta = c.polish_files(fa, ds["bams"], bed=path, bed_status=MIXED, soft_mask=True)
        assert fasta == w["masked_mixed"] and open(path, "rb").read() == w["bed_mixed"]
        fasta, _ = c.filter_polish_files(fa, ds["bams"][0], ds["bams"][1], bed=path, bed_bgzf=True, soft_mask=True)
        assert fasta == wf["masked_default"] and gzip.decompress(open(path, "rb").read()) == wf["bed_default"]
        os.remove(path)
        assert c.polish_files(fa, ds["sams"], soft_mask=True, bed_status=["kept"]).upper() == w["fasta"].upper()
        assert c.polish_files(fa, ds["sams"]) == w["fasta"]  # off again behind the call ...
        with pytest.raises(pp.PolypolishError):
            c.bed()  # ... and a run that begins drops the file of the run before
        for kw, words in ((dict(bed_bgzf=True), "bed_bgzf=True needs bed="), (dict(bed_status="none"), "bed_status= needs bed="),
                          (dict(bed=path, bed_status="none,maybe"), "'maybe' is not one of"), (dict(soft_mask=True, bed_status=""), "empty status list")):
            with pytest.raises(pp.PolypolishError) as e:
                c.polish_files(fa, ds["sams"], **kw)
            assert words in e.value.msg and not os.path.exists(path), kw
        with pytest.raises(pp.PolypolishError) as e:
            c.polish_files(fa, ds["sams"], bed=str(tmp_path / "no" / "dir" / "x.bed"))
        assert e.value.code == pp.ERR_QUIT and "unable to write the BED" in e.value.msg
        with pytest.raises(pp.PolypolishError) as e:
            c.set_bed(True, 0)
        assert e.value.code == pp.ERR_ARG and "mask of 0" in e.value.msg
        # pp_polish_files_multi: one context makes the file, two are refused by name before any input is looked at
        L = pp.lib()
        opt = pp.PolishOptions(0.2, 0.5, 10, 5, 0, None, 1)
        sams = (C.c_char_p * 2)(*[s.encode() for s in ds["sams"]])
        c.set_bed(True)
        c.set_soft_mask()
        one = (C.c_void_p * 1)(c._h)
        res = pp.Bytes()
        assert L.pp_polish_files_multi(one, 1, fa.encode(), sams, 2, C.byref(opt), C.byref(res)) == 0
        assert C.string_at(res.data, res.len) == w["masked_default"]
        L.pp_bytes_free(C.byref(res))
        assert c.bed() == w["bed_default"]
        c2 = pp.Context(0)
        try:
            two = (C.c_void_p * 2)(c._h, c2._h)
            rc = L.pp_polish_files_multi(two, 2, b"/no/such/assembly.fasta", sams, 2, C.byref(opt), C.byref(res))
            assert rc == pp.ERR_QUIT and b"--bed runs on one GPU" in L.pp_last_error(c._h)
            with pytest.raises(pp.PolypolishError):
                c.bed()
            c.set_bed(False)
            rc = L.pp_polish_files_multi(two, 2, b"/no/such/assembly.fasta", sams, 2, C.byref(opt), C.byref(res))
            assert rc == pp.ERR_QUIT and b"--soft_mask runs on one GPU" in L.pp_last_error(c._h)
        finally:
            c2.close()
        c.set_soft_mask(0)
    finally:
        c.close()
