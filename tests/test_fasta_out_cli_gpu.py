"""`polypolish polish` and `filter-polish` with --out, --wrap, --out_bgzf and --index (pp_ctx_set_fasta_form: the FASTA made by
pp_fasta_text and pp_bgzf_deflate on the device) against the same commands without them: the bytes against
tests/fasta_text_model.py's wrap of the plain run's stdout, the indexes against the model's, the log line by line.  On the derived
golden case and on a generated job of three contigs, from SAM text and from BAM, and with two contexts on one GPU (PP_SHARE_GPU=2: the
host-memory form).  Every command runs bin/polypolish as a child process.  Needs an MI355X: `-m gpu`."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import bam_model as bm
import bgzf_deflate_model as dm
import fasta_model as fm
import fasta_text_model as tm
from test_bgzf_chain_gpu import bgzf_file, cut_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "polypolish")
GOLDEN = os.path.join(ROOT, "tests", "golden", "derived_e2e")
pytestmark = pytest.mark.gpu
DROP = ("PP_SHARE_GPU", "PP_GPUS", "PP_DEVICE")


def run(*argv, env=None):
    base = {k: v for k, v in os.environ.items() if k not in DROP}
    r = subprocess.run([EXE, *map(str, argv)], capture_output=True, env=dict(base, **(env or {})), timeout=300)
    if r.returncode < 0 or r.returncode in (134, 139) or b"illegal memory access" in r.stderr:  # a crash is a finding: nothing more is started on the device
        pytest.exit(f"polypolish {' '.join(map(str, argv))} ended with {r.returncode}: {r.stderr.decode()[-600:]}", returncode=3)
    return r


def log_of(r, path=None):
    """stderr without what differs from run to run: the durations -- and with the one line that names --out put back"""
    log = re.sub(rb"(Time to run: )[^\n]*", rb"\1-", r.stderr)
    if path is not None:
        named = b"Polished sequence (to %s):" % str(path).encode()
        assert log.count(named) == 1, log[-600:]
        log = log.replace(named, b"Polished sequence (to stdout):")
    return log


def bam_of(sam_path, fasta_path, out_path):
    names, _, off, _ = fm.parse(open(fasta_path, "rb").read())
    enc = bm.encode(open(sam_path, "rb").read(), [n.decode() for n in names], [off[i + 1] - off[i] for i in range(len(names))])
    data = enc["header"] + enc["records"]
    starts = set((enc["rec_off"] + np.uint64(len(enc["header"]))).tolist())
    with open(out_path, "wb") as f:
        f.write(bgzf_file(data, cut_points(len(data), starts)))
    return str(out_path)


@pytest.fixture(scope="module")
def jobs(tmp_path_factory):
    """name -> (assembly, [sam1, sam2], [bam1, bam2])"""
    import synth
    d = str(tmp_path_factory.mktemp("fasta_out_cli"))
    s = synth.rich_dataset(d, seed=29, contig_lens=(3000, 2000, 1500), coverage=30, repeat_len=300, repeat_copies=2, zp_frac=0.02)
    sets = {"golden": (os.path.join(GOLDEN, "case.fasta"), [os.path.join(GOLDEN, "case_1.sam"), os.path.join(GOLDEN, "case_2.sam")]),
            "gen3": (s["fasta"], [s["sam1"], s["sam2"]])}
    out = {}
    for name, (fa, sams) in sets.items():
        bams = [bam_of(p, fa, os.path.join(d, f"{name}_{i + 1}.bam")) for i, p in enumerate(sams)]
        out[name] = (fa, sams, bams)
    return out


def command(jobs, job, cmd, kind):
    fa, sams, bams = jobs[job]
    files = sams if kind == "sam" else bams
    return ["polish", fa, *files] if cmd == "polish" else ["filter-polish", "--in1", files[0], "--in2", files[1], fa]


_plain = {}


def plain(jobs, job, cmd, kind):
    """the run without any of the flags: (stdout, log), once per command"""
    key = (job, cmd, kind)
    if key not in _plain:
        r = run(*command(jobs, job, cmd, kind))
        assert r.returncode == 0 and r.stdout.startswith(b">"), r.stderr.decode()[-800:]
        _plain[key] = (r.stdout, log_of(r))
    return _plain[key]


CASES = [(j, c, k) for j in ("golden", "gen3") for c in ("polish", "filter-polish") for k in ("sam", "bam")]


@pytest.mark.parametrize("job,cmd,kind", CASES)
def test_wrap_0_and_out_give_the_plain_bytes(jobs, tmp_path, job, cmd, kind):
    want, log = plain(jobs, job, cmd, kind)
    r = run(*command(jobs, job, cmd, kind), "--wrap", 0)
    assert r.returncode == 0 and r.stdout == want and log_of(r) == log, r.stderr.decode()[-800:]
    path = tmp_path / "polished.fasta"
    r = run(*command(jobs, job, cmd, kind), "--out", path)
    assert r.returncode == 0 and r.stdout == b"" and open(path, "rb").read() == want, r.stderr.decode()[-800:]
    assert log_of(r, path) == log
    assert os.listdir(tmp_path) == ["polished.fasta"]


@pytest.mark.parametrize("job,cmd,kind", CASES)
def test_wrap_60_bgzf_and_index(jobs, tmp_path, job, cmd, kind):
    want, log = plain(jobs, job, cmd, kind)
    headers, seqs = tm.parse_headers(want)
    wrapped = tm.text(headers, seqs, 60)
    assert tm.text(headers, seqs, 0) == want and wrapped != want
    r = run(*command(jobs, job, cmd, kind), "--wrap", 60)
    assert r.returncode == 0 and r.stdout == wrapped and log_of(r) == log, r.stderr.decode()[-800:]
    path = tmp_path / "polished.fa.gz"
    r = run(*command(jobs, job, cmd, kind), "--out", path, "--out_bgzf", "--index", "--wrap", 60)
    assert r.returncode == 0 and r.stdout == b"", r.stderr.decode()[-800:]
    file = open(path, "rb").read()
    assert gzip.decompress(file) == wrapped
    model_file, model_off, _ = dm.deflate_file(wrapped)
    assert file == model_file
    assert open(str(path) + ".fai", "rb").read() == tm.fai(headers, seqs, 60)
    assert open(str(path) + ".gzi", "rb").read() == tm.gzi(model_off)
    assert log_of(r, path) == log
    assert sorted(os.listdir(tmp_path)) == ["polished.fa.gz", "polished.fa.gz.fai", "polished.fa.gz.gzi"]


@pytest.mark.parametrize("job", ["golden", "gen3"])
def test_two_contexts_take_the_host_memory_form(jobs, tmp_path, job):
    """PP_SHARE_GPU=2: the ranks' results are assembled in host memory, pp_fasta_text reads them there"""
    want, _ = plain(jobs, job, "polish", "sam")
    headers, seqs = tm.parse_headers(want)
    wrapped = tm.text(headers, seqs, 60)
    env = dict(PP_SHARE_GPU="2")
    base = run(*command(jobs, job, "polish", "sam"), env=env)
    assert base.returncode == 0 and base.stdout == want, base.stderr.decode()[-800:]
    r = run(*command(jobs, job, "polish", "sam"), "--wrap", 0, env=env)
    assert r.returncode == 0 and r.stdout == want and log_of(r) == log_of(base), r.stderr.decode()[-800:]
    path = tmp_path / "two.fa.gz"
    r = run(*command(jobs, job, "polish", "sam"), "--out", path, "--out_bgzf", "--index", "--wrap", 60, env=env)
    assert r.returncode == 0 and r.stdout == b"", r.stderr.decode()[-800:]
    assert gzip.decompress(open(path, "rb").read()) == wrapped
    assert open(str(path) + ".fai", "rb").read() == tm.fai(headers, seqs, 60)
    assert open(str(path) + ".gzi", "rb").read() == tm.gzi(dm.deflate_file(wrapped)[1])
    assert log_of(r, path) == log_of(base)


@pytest.mark.parametrize("cmd", ["polish", "filter-polish"])
def test_refusals(jobs, tmp_path, cmd):
    # --index without --out: refused by name before any input is read (the inputs do not exist)
    missing = {"x": (str(tmp_path / "no.fasta"), [str(tmp_path / "no_1.sam"), str(tmp_path / "no_2.sam")], [])}
    r = run(*command(missing, "x", cmd, "sam"), "--index")
    assert r.returncode == 1 and r.stdout == b"" and b"--index" in r.stderr and b"--out" in r.stderr and b"does not exist" not in r.stderr
    # a --wrap that is no number, or above 2^31 - 1: the usage error --min_depth gives
    for bad in ("sixty", "2147483648", "-1", ""):
        r = run(*command(missing, "x", cmd, "sam"), "--wrap=" + bad)
        d = run(*command(missing, "x", cmd, "sam"), "--min_depth=sixty")
        assert r.returncode == d.returncode == 2 and r.stdout == b""
        assert r.stderr.startswith(b"error: invalid value '" + bad.encode() + b"' for '--wrap <N>': ")
        assert r.stderr.endswith(d.stderr[d.stderr.index(b"\n\nFor more information"):])
    r = run(*command(missing, "x", cmd, "sam"), "--wrap", 2147483647, "--index", "--out", tmp_path / "never.fa")
    # (the largest width is taken; the run then ends at its inputs, in the command's own words)
    assert r.returncode == 1 and b"invalid value" not in r.stderr and str(tmp_path / "no").encode() in r.stderr.split(b"\nError: ")[-1]
    # an --out that cannot be written: its words, exit 1, nothing created
    path = tmp_path / "no_such_directory" / "polished.fa"
    r = run(*command(jobs, "golden", cmd, "sam"), "--out", path, "--index", "--wrap", 60)
    assert r.returncode == 1 and r.stdout == b""
    assert r.stderr.endswith(b'\nError: unable to write the polished sequence to "%s"\n' % str(path).encode())
    # a failed polish leaves nothing behind
    r = run(*command(jobs, "golden", cmd, "sam"), "--out", tmp_path / "failed.fa", "--index", "--fraction_valid", "0.1")
    assert r.returncode == 1
    assert os.listdir(tmp_path) == []


def test_the_python_face(jobs, tmp_path):
    import polypolish_amd as pp
    fa, sams, _ = jobs["gen3"]
    ctx = pp.Context(0)
    want = ctx.polish_files(fa, sams)
    assert want == plain(jobs, "gen3", "polish", "sam")[0]
    headers, seqs = tm.parse_headers(want)
    assert ctx.polish_files(fa, sams, wrap=0) == want
    assert ctx.polish_files(fa, sams, wrap=80) == tm.text(headers, seqs, 80)
    out = tmp_path / "py.fa.gz"
    got = ctx.polish_files(fa, sams, wrap=60, bgzf=True, out=out, index=True)
    assert open(out, "rb").read() == got and gzip.decompress(got) == tm.text(headers, seqs, 60)
    assert open(str(out) + ".fai", "rb").read() == tm.fai(headers, seqs, 60) == ctx.fasta_index()[0]
    assert open(str(out) + ".gzi", "rb").read() == ctx.fasta_index()[1]
    fused, _ = ctx.filter_polish_files(fa, sams[0], sams[1], wrap=60)
    plain_fused, _ = ctx.filter_polish_files(fa, sams[0], sams[1])
    assert fused == tm.text(*tm.parse_headers(plain_fused), 60)
    with pytest.raises(pp.PolypolishError):
        ctx.polish_files(fa, sams, index=True)
    assert ctx.polish_files(fa, sams) == want  # the form is off again
    ctx.close()


def test_the_distributed_module_refuses_the_flags_by_name(jobs):
    from polypolish_amd import distributed
    fa, sams, _ = jobs["golden"]
    for flag in (["--wrap", "60"], ["--out", "x.fa"], ["--out_bgzf"], ["--index"]):
        with pytest.raises(SystemExit) as e:  # (a message as the exit's code: the interpreter prints it and exits 1)
            distributed.main(["polish", *flag, fa, *sams])
        assert isinstance(e.value.code, str) and e.value.code.startswith("Error: " + flag[0] + " "), e.value.code
