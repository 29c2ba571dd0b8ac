"""`polypolish polish --vcf` and `filter-polish --vcf` (pp_ctx_set_vcf: pp_polish_vcf behind the drivers' polish) on a rich_dataset pair as
SAM text and as BAM, on every input route: the file is the model's text (tests/vcf_model.py) of the ORACLE's --debug TSV, apply() on it
gives the command's FASTA, and stdout and the log are the plain run's.  --vcf_bgzf, the refusals, and the same bytes through the Python
wrapper.  Every command runs bin/polypolish as a child process.  Needs an MI355X: `-m gpu`."""
import ctypes as C
import gzip
import os
import struct

import pytest

import fasta_text_model as tm
import vcf_model as vm
from test_bgzf_chain_gpu import MAX_ERRORS
from test_fasta_cli_gpu import ds, log_of, run  # noqa: F401 (ds: the module's dataset fixture -- SAM pair, BAM pair, the oracle's results)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pp():
    import polypolish_amd
    return polypolish_amd


@pytest.fixture(scope="module")
def want(ds, orc, pp):
    """the model's VCF of the two commands, from the oracle's TSVs"""
    names, _, off, bases = ds["parsed"]
    version = pp.lib().pp_version()
    outs = [os.path.join(ds["dir"], f"oracle_filtered_{i}.sam") for i in (1, 2)]
    filtered = orc.polish_files(ds["forms"]["lf60"], outs, max_errors=MAX_ERRORS, debug=True)
    assert filtered["fasta"] == ds["polish_filtered"]
    w = {"polish": vm.from_debug_tsv(names, off, bytes(bases), ds["polish"]["debug"], version),
         "filter-polish": vm.from_debug_tsv(names, off, bytes(bases), filtered["debug"], version)}
    assert len(vm.parse(w["polish"])[1]) > 5 and len(vm.parse(w["filter-polish"])[1]) > 5
    return w


def _command(ds, cmd, kind, *flags):
    files = ds["sams"] if kind == "sam" else ds["bams"]
    fa = ds["forms"]["lf60"]
    return ("polish", *flags, fa, *files) if cmd == "polish" else ("filter-polish", *flags, "--in1", files[0], "--in2", files[1], fa)


def _applies(ds, vcf, fasta):
    names, _, off, bases = ds["parsed"]
    contigs = [(n, bytes(bases[off[i]:off[i + 1]])) for i, n in enumerate(names)]
    assert [s for _, s in vm.apply(contigs, vcf)] == tm.parse_headers(fasta)[1]


@pytest.mark.parametrize("kind", ["sam", "bam"])
@pytest.mark.parametrize("cmd", ["polish", "filter-polish"])
def test_the_file_is_the_models_and_the_run_is_the_plain_one(ds, want, tmp_path, cmd, kind):
    path = str(tmp_path / "edits.vcf")
    plain = run(*_command(ds, cmd, kind))
    r = run(*_command(ds, cmd, kind, "--vcf", path))
    assert plain.returncode == 0 and r.returncode == 0, r.stderr.decode()[-800:]
    assert r.stdout == plain.stdout and log_of(r) == log_of(plain)
    assert r.stdout == (ds["polish"]["fasta"] if cmd == "polish" else ds["polish_filtered"])
    vcf = open(path, "rb").read()
    assert vcf == want[cmd]
    _applies(ds, vcf, r.stdout)


def _bgzf_blocks(data):
    """the uncompressed sizes of the BGZF blocks a file is made of (asserts that every gzip member is one, the EOF block last)"""
    sizes, at = [], 0
    while at < len(data):
        assert data[at:at + 4] == b"\x1f\x8b\x08\x04" and data[at + 10:at + 16] == b"\x06\x00BC\x02\x00", at
        (bsize,) = struct.unpack_from("<H", data, at + 16)
        sizes.append(struct.unpack_from("<I", data, at + bsize + 1 - 4)[0])
        at += bsize + 1
    assert at == len(data) and sizes[-1] == 0 and len(data) - 28 >= 0
    return sizes


@pytest.mark.parametrize("cmd, kind", [("polish", "sam"), ("filter-polish", "bam")])
def test_vcf_bgzf_decompresses_to_the_same_bytes(ds, want, tmp_path, cmd, kind):
    path = str(tmp_path / "edits.vcf.gz")
    plain = run(*_command(ds, cmd, kind))
    r = run(*_command(ds, cmd, kind, "--vcf", path, "--vcf_bgzf"))
    assert r.returncode == 0 and r.stdout == plain.stdout and log_of(r) == log_of(plain), r.stderr.decode()[-800:]
    data = open(path, "rb").read()
    assert gzip.decompress(data) == want[cmd]
    assert sum(_bgzf_blocks(data)) == len(want[cmd])


@pytest.mark.parametrize("route", ["text_chain", "regroup", "host_ingest", "device_fasta", "debug", "out_wrap"])
def test_every_input_route(ds, want, tmp_path, route):
    path = str(tmp_path / "edits.vcf")
    flags, env, kind = {"text_chain": (["--text_chain"], None, "sam"), "regroup": (["--regroup"], None, "bam"),
                        "host_ingest": ([], dict(PP_DEVICE_INGEST="0"), "sam"), "device_fasta": ([], dict(PP_DEVICE_FASTA="1"), "sam"),
                        "debug": (["--debug", str(tmp_path / "d.tsv")], None, "sam"),
                        "out_wrap": (["--out", str(tmp_path / "o.fa"), "--wrap", "60", "--index"], None, "bam")}[route]
    for cmd in ("polish", "filter-polish"):
        plain = run(*_command(ds, cmd, kind, *flags), env=env)
        kept = [open(f, "rb").read() for f in (str(tmp_path / "d.tsv"), str(tmp_path / "o.fa"), str(tmp_path / "o.fa.fai")) if os.path.exists(f)]
        r = run(*_command(ds, cmd, kind, *flags, "--vcf", path), env=env)
        assert plain.returncode == 0 and r.returncode == 0, (cmd, r.stderr.decode()[-800:])
        assert r.stdout == plain.stdout and log_of(r) == log_of(plain), cmd
        assert kept == [open(f, "rb").read() for f in (str(tmp_path / "d.tsv"), str(tmp_path / "o.fa"), str(tmp_path / "o.fa.fai")) if os.path.exists(f)]
        assert open(path, "rb").read() == want[cmd], cmd
        os.remove(path)


@pytest.mark.parametrize("env", [dict(PP_SHARE_GPU="2"), dict(PP_GPUS="2")], ids=["share_gpu", "gpus"])
def test_several_contexts_are_refused_and_leave_no_file(ds, tmp_path, env):
    path = str(tmp_path / "edits.vcf")
    r = run(*_command(ds, "polish", "sam", "--vcf", path), env=env)
    assert r.returncode == 1 and r.stdout == b"" and b"--vcf runs on one GPU" in r.stderr and not os.path.exists(path)
    assert b"Loading" not in r.stderr, "refused before any file is opened"


def test_usage_errors_failed_runs_and_unwritable_paths(ds, tmp_path):
    path = str(tmp_path / "edits.vcf")
    for cmd in ("polish", "filter-polish"):
        r = run(*_command(ds, cmd, "sam", "--vcf_bgzf"))
        assert r.returncode == 2 and r.stdout == b"" and b"--vcf_bgzf needs --vcf" in r.stderr
        nowhere = str(tmp_path / "no" / "such" / "dir" / "edits.vcf")
        r = run(*_command(ds, cmd, "sam", "--vcf", nowhere))
        assert r.returncode == 1 and r.stdout == b"" and b"unable to write the VCF to" in r.stderr and nowhere.encode() in r.stderr
    # a run that fails leaves no file behind
    r = run("polish", "--vcf", path, ds["forms"]["lf60"], str(tmp_path / "missing.sam"))
    assert r.returncode == 1 and not os.path.exists(path)
    r = run("polish", "--vcf", path, "--fraction_valid", "2", ds["forms"]["lf60"], *ds["sams"])
    assert r.returncode == 1 and not os.path.exists(path)


def test_the_same_bytes_through_the_python_wrapper(ds, want, pp, tmp_path):
    path, fa = str(tmp_path / "py.vcf"), ds["forms"]["lf60"]
    c = pp.Context(0)
    try:
        with pytest.raises(pp.PolypolishError) as e:
            c.vcf()
        assert e.value.code == pp.ERR_ARG and "pp_ctx_set_vcf" in e.value.msg
        fasta = c.polish_files(fa, ds["sams"], max_errors=MAX_ERRORS, vcf=path)
        assert fasta == ds["polish"]["fasta"] and open(path, "rb").read() == want["polish"] and c.vcf() == want["polish"]
        fasta, _ = c.filter_polish_files(fa, ds["bams"][0], ds["bams"][1], max_errors=MAX_ERRORS, vcf=path, vcf_bgzf=True)
        assert fasta == ds["polish_filtered"] and gzip.decompress(open(path, "rb").read()) == want["filter-polish"]
        os.remove(path)
        assert c.polish_files(fa, ds["sams"], max_errors=MAX_ERRORS) == ds["polish"]["fasta"]  # off again behind the call ...
        with pytest.raises(pp.PolypolishError):
            c.vcf()  # ... and a run that begins drops the file of the run before
        with pytest.raises(pp.PolypolishError) as e:
            c.polish_files(fa, ds["sams"], vcf_bgzf=True)
        assert "vcf_bgzf=True needs vcf=" in e.value.msg
        with pytest.raises(pp.PolypolishError) as e:
            c.polish_files(fa, ds["sams"], vcf=str(tmp_path / "no" / "dir" / "x.vcf"))
        assert e.value.code == pp.ERR_QUIT and "unable to write the VCF" in e.value.msg
        # pp_polish_files_multi: one context makes the file, two are refused by name before any input is looked at
        L = pp.lib()
        opt = pp.PolishOptions(0.2, 0.5, MAX_ERRORS, 5, 0, None, 1)
        sams = (C.c_char_p * 2)(*[s.encode() for s in ds["sams"]])
        c.set_vcf(True)
        one = (C.c_void_p * 1)(c._h)
        res = pp.Bytes()
        assert L.pp_polish_files_multi(one, 1, fa.encode(), sams, 2, C.byref(opt), C.byref(res)) == 0
        L.pp_bytes_free(C.byref(res))
        assert c.vcf() == want["polish"]
        c2 = pp.Context(0)
        try:
            two = (C.c_void_p * 2)(c._h, c2._h)
            rc = L.pp_polish_files_multi(two, 2, b"/no/such/assembly.fasta", sams, 2, C.byref(opt), C.byref(res))
            assert rc == pp.ERR_QUIT and b"--vcf runs on one GPU" in L.pp_last_error(c._h)
            with pytest.raises(pp.PolypolishError):
                c.vcf()
        finally:
            c2.close()
        c.set_vcf(False)
    finally:
        c.close()
