"""`polypolish polish` and `filter-polish` with --depth, --depth_bin and --depth_bgzf (pp_ctx_set_depth: pp_polish_depth behind the
drivers' polish) on the golden pair (tests/golden/derived_e2e), from SAM text and from BAM, with --regroup, --text_chain and the host
ingest: the file is the model's text (tests/depth_model.py) of the ORACLE's per-position depths -- whose tenths are column 4 of the
oracle's --debug TSV --, plain and bgzipped; stdout and the log are the plain run's; a --vcf and a --bed alongside are their own runs'
files; the log's "depth of zero" counts are the track's zero positions; the usage errors, the refusal of several contexts and an
unwritable path leave nothing behind; the same through Python.  Every command test runs bin/polypolish as a child process.  Needs an
MI355X: `-m gpu`."""
import gzip
import os
import re
import zlib

import pytest

import bam_model
import bed_jobs as bj
import depth_model as dm
import fasta_model as fm
import sam_bam_model as sb
from test_bam_cli_gpu import put, run
from test_bgzf_chain_gpu import bgzf_file, cut_points

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "derived_e2e")
W = 250  # the bin of the binned runs


def log_of(r):
    """stderr without what differs from run to run: the durations"""
    return re.sub(rb"(Time to run: )[^\n]*", rb"\1-", r.stderr)


@pytest.fixture(scope="module")
def pp():
    import polypolish_amd
    return polypolish_amd


@pytest.fixture(scope="module")
def ds(tmp_path_factory, orc):
    d = str(tmp_path_factory.mktemp("depth_cli"))
    fa = os.path.join(GOLDEN, "case.fasta")
    names, _, off, bases = fm.parse(open(fa, "rb").read())
    off = [int(x) for x in off]
    lens = {n.decode(): off[i + 1] - off[i] for i, n in enumerate(names)}
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
        res = orc.polish_files(fa, files, debug=True, positions=True)
        depth = res["positions"]["depth"]
        w = {"fasta": res["fasta"], "runs": dm.bedgraph(depth, off, names), "bins": dm.bedgraph(depth, off, names, W),
             "zeros": [dm.summary(depth[off[c]:off[c + 1]])["zero_positions"] for c in range(len(names))]}
        assert dm.expand(w["runs"], off, names) == dm.depth_column_of_debug_tsv(res["debug"]), "the model is fed what the oracle's TSV prints"
        assert len(dm.parse(w["runs"])) > 10 and len(dm.parse(w["bins"])) == sum(-(-n // W) for n in lens.values())
        want[cmd] = w
    return {"dir": d, "fasta": fa, "sams": sams, "bams": bams, "want": want}


def _command(ds, cmd, kind, *flags):
    files = ds["sams"] if kind == "sam" else ds["bams"]
    return ("polish", *flags, ds["fasta"], *files) if cmd == "polish" else ("filter-polish", *flags, "--in1", files[0], "--in2", files[1], ds["fasta"])


def _through_zlib(data):
    assert data[:4] == b"\x1f\x8b\x08\x04" and data[12:16] == b"BC\x02\x00", "BGZF blocks"
    text, at = b"", data
    while at:  # member by member
        z = zlib.decompressobj(31)
        text += z.decompress(at)
        at = z.unused_data
    assert text == gzip.decompress(data)
    return text


@pytest.mark.parametrize("kind", ["sam", "bam"])
@pytest.mark.parametrize("cmd", ["polish", "filter-polish"])
def test_the_track_is_the_models_and_the_run_is_the_plain_one(ds, tmp_path, cmd, kind):
    w = ds["want"][cmd]
    path, gz, vcf, vcf0, bed, bed0 = (str(tmp_path / n) for n in ("d.bedgraph", "d.bedgraph.gz", "with.vcf", "plain.vcf", "with.bed", "plain.bed"))
    plain = run(*_command(ds, cmd, kind, "--vcf", vcf0, "--bed", bed0))
    assert plain.returncode == 0 and plain.stdout == w["fasta"], plain.stderr.decode()[-800:]
    r = run(*_command(ds, cmd, kind, "--depth", path, "--vcf", vcf, "--bed", bed))
    assert r.returncode == 0 and r.stdout == plain.stdout and log_of(r) == log_of(plain), r.stderr.decode()[-800:]
    assert open(path, "rb").read() == w["runs"]
    assert open(vcf, "rb").read() == open(vcf0, "rb").read() and open(bed, "rb").read() == open(bed0, "rb").read(), "--vcf and --bed alongside give their own runs' files"
    assert len(os.listdir(str(tmp_path))) == 5, "with --depth alone no TSV is written"
    # the log's "depth of zero" counts, contig by contig, are the track's zero positions
    zeros = [int(m.replace(b",", b"")) for m in re.findall(rb"\n  ([0-9,]+) bp ha(?:s|ve) a depth of zero", r.stderr)]
    assert zeros == w["zeros"]
    r = run(*_command(ds, cmd, kind, "--depth", gz, "--depth_bgzf"))
    assert r.returncode == 0 and r.stdout == plain.stdout and log_of(r) == log_of(plain), r.stderr.decode()[-800:]
    assert _through_zlib(open(gz, "rb").read()) == w["runs"], "the bgzipped file is the plain one"
    r = run(*_command(ds, cmd, kind, "--depth", gz, "--depth_bgzf", "--depth_bin", W))
    assert r.returncode == 0 and r.stdout == plain.stdout and log_of(r) == log_of(plain), r.stderr.decode()[-800:]
    assert _through_zlib(open(gz, "rb").read()) == w["bins"]
    r = run(*_command(ds, cmd, kind, "--depth_bin=1", "--depth", path))
    assert r.returncode == 0 and r.stdout == plain.stdout
    assert [ln.rsplit(b"\t", 1)[1] for ln in open(path, "rb").read().split(b"\n")[:-1]] == [v + b"0" for v in dm.expand(w["runs"], *_table(ds))]


def _table(ds):
    names, _, off, _ = fm.parse(open(ds["fasta"], "rb").read())
    return [int(x) for x in off], names


@pytest.mark.parametrize("route", ["text_chain", "regroup", "host_ingest", "debug"])
def test_every_input_route(ds, tmp_path, route):
    path = str(tmp_path / "d.bedgraph")
    flags, env, kind = {"text_chain": (["--text_chain"], None, "sam"), "regroup": (["--regroup"], None, "bam"),
                        "host_ingest": ([], dict(PP_DEVICE_INGEST="0"), "sam"), "debug": (["--debug", str(tmp_path / "d.tsv")], None, "sam")}[route]
    for cmd in ("polish", "filter-polish"):
        plain = run(*_command(ds, cmd, kind, *flags), env=env)
        kept = open(str(tmp_path / "d.tsv"), "rb").read() if route == "debug" else None
        r = run(*_command(ds, cmd, kind, *flags, "--depth", path, "--depth_bin", W), env=env)
        assert plain.returncode == 0 and r.returncode == 0, (cmd, r.stderr.decode()[-800:])
        assert r.stdout == plain.stdout == ds["want"][cmd]["fasta"] and log_of(r) == log_of(plain), cmd
        assert open(path, "rb").read() == ds["want"][cmd]["bins"], cmd
        if route == "debug":  # the TSV is the plain run's, and its column 4 is the runs form expanded
            tsv = open(str(tmp_path / "d.tsv"), "rb").read()
            assert tsv == kept and dm.depth_column_of_debug_tsv(tsv) == dm.expand(ds["want"][cmd]["runs"], *_table(ds))
        os.remove(path)


def test_usage_errors_leave_nothing_behind(ds, tmp_path):
    path = str(tmp_path / "d.bedgraph")
    for cmd in ("polish", "filter-polish"):
        for flags, words in ((["--depth_bin", "100"], b"--depth_bin needs --depth"), (["--depth_bgzf"], b"--depth_bgzf needs --depth"),
                             (["--depth", path, "--depth_bin", "ten"], b"invalid value 'ten' for '--depth_bin <N>'"),
                             (["--depth", path, "--depth_bin", "-1"], b"--depth_bin <N>"),
                             (["--depth", path, "--depth_bin", "1.5"], b"invalid value '1.5' for '--depth_bin <N>'"),
                             (["--depth", path, "--depth_bin", "16777217"], b"invalid value '16777217' for '--depth_bin <N>': 16777217 is not in 0..=16777216"),
                             (["--depth", path, "--depth_bin", "99999999999"], b"invalid value '99999999999' for '--depth_bin <N>'"),
                             (["--depth", "--careful"], b"a value is required for '--depth <PATH>'"), (["--depth", path, "--depth", path], b"multiple times")):
            r = run(*_command(ds, cmd, "sam", *flags))
            assert r.returncode == 2 and r.stdout == b"" and words in r.stderr and b"For more information, try '--help'." in r.stderr, (cmd, flags, r.stderr[-300:])
            assert os.listdir(str(tmp_path)) == []
        assert b"--depth <PATH>" in run(cmd, "--help").stdout and b"--depth_bin" in run(cmd, "--help").stdout
    # a run that fails leaves no file behind
    r = run("polish", "--depth", path, ds["fasta"], str(tmp_path / "missing.sam"))
    assert r.returncode == 1 and os.listdir(str(tmp_path)) == []
    r = run("polish", "--depth", path, "--fraction_valid", "2", ds["fasta"], *ds["sams"])
    assert r.returncode == 1 and r.stdout == b"" and os.listdir(str(tmp_path)) == []


@pytest.mark.parametrize("env", [dict(PP_SHARE_GPU="2"), dict(PP_GPUS="2")], ids=["share_gpu", "gpus"])
def test_several_contexts_are_refused_and_leave_no_file(ds, tmp_path, env):
    path = str(tmp_path / "d.bedgraph")
    r = run(*_command(ds, "polish", "sam", "--depth", path), env=env)
    assert r.returncode == 1 and r.stdout == b"" and b"--depth runs on one GPU" in r.stderr and os.listdir(str(tmp_path)) == []
    assert b"Loading" not in r.stderr, "refused before any file is opened"


def test_an_unwritable_path_leaves_no_fasta_half_written(ds, tmp_path):
    nowhere = str(tmp_path / "no" / "such" / "dir" / "d.bedgraph")
    out = str(tmp_path / "o.fa")
    for cmd in ("polish", "filter-polish"):
        r = run(*_command(ds, cmd, "sam", "--depth", nowhere, "--out", out))
        assert r.returncode == 1 and r.stdout == b"" and b'Error: unable to write the depth track to "' + nowhere.encode() + b'"' in r.stderr
        assert os.listdir(str(tmp_path)) == [], "the depth track is written before the FASTA: no FASTA is left"


def test_the_distributed_launcher_refuses_by_name():
    from polypolish_amd import distributed
    for argv in (["polish", "--depth", "x.bedgraph", "a.fasta"], ["polish", "--depth_bin", "5", "a.fasta"], ["polish", "--depth_bgzf", "a.fasta"]):
        with pytest.raises(SystemExit) as e:
            distributed.main(argv)
        assert "--depth runs on one GPU" in str(e.value)


def test_the_same_through_python(ds, pp, orc, tmp_path):
    import ctypes as C
    w, wf = ds["want"]["polish"], ds["want"]["filter-polish"]
    path, fa = str(tmp_path / "py.bedgraph"), ds["fasta"]
    off, names = _table(ds)
    c = pp.Context(0)
    try:
        with pytest.raises(pp.PolypolishError) as e:
            c.depth()
        assert e.value.code == pp.ERR_ARG and "pp_ctx_set_depth" in e.value.msg
        fasta = c.polish_files(fa, ds["sams"], depth=path)
        assert fasta == w["fasta"] and open(path, "rb").read() == w["runs"] == c.depth()
        fasta = c.polish_files(fa, ds["bams"], depth=path, depth_bin=W)
        assert fasta == w["fasta"] and open(path, "rb").read() == w["bins"]
        fasta, _ = c.filter_polish_files(fa, ds["bams"][0], ds["bams"][1], depth=path, depth_bin=W, depth_bgzf=True)
        assert fasta == wf["fasta"] and gzip.decompress(open(path, "rb").read()) == wf["bins"]
        os.remove(path)
        assert c.polish_files(fa, ds["sams"]) == w["fasta"]  # off again behind the call ...
        with pytest.raises(pp.PolypolishError):
            c.depth()  # ... and a run that begins drops the file of the run before
        for kw, words in ((dict(depth_bgzf=True), "depth_bgzf=True needs depth="), (dict(depth_bin=5), "depth_bin= needs depth="),
                          (dict(depth=path, depth_bin=(1 << 24) + 1), "is not an integer in 0..16777216"), (dict(depth=path, depth_bin=-1), "is not an integer in"),
                          (dict(depth=path, depth_bin="ten"), "is not an integer in")):
            with pytest.raises(pp.PolypolishError) as e:
                c.polish_files(fa, ds["sams"], **kw)
            assert words in e.value.msg and not os.path.exists(path), kw
        with pytest.raises(pp.PolypolishError) as e:
            c.polish_files(fa, ds["sams"], depth=str(tmp_path / "no" / "dir" / "x.bedgraph"))
        assert e.value.code == pp.ERR_QUIT and "unable to write the depth track" in e.value.msg
        with pytest.raises(pp.PolypolishError) as e:
            c.set_depth(True, (1 << 24) + 1)
        assert e.value.code == pp.ERR_ARG and "2^24" in e.value.msg
        assert pp.polish(fa, ds["sams"], depth=path, depth_bin=W) == w["fasta"] and open(path, "rb").read() == w["bins"]  # the module's own route
        # Context.polish_depth and Context.depth_bedgraph: a job of records on the same context, against the model on the oracle's depths
        job = bj.job(pp.depth_geometry()[1], 0)
        res = orc.polish_records(job["off"], job["bases"], job["recs"], min_depth=1, positions=True)
        assert c.polish_records(job["off"], job["bases"], job["recs"], min_depth=1, debug=True)["polished"] == res["polished"]
        for track in (c.polish_depth(job["names"], W), c.depth_bedgraph(res["positions"]["depth"], job["off"], job["names"], W)):
            assert track.bytes() == dm.bedgraph(res["positions"]["depth"], job["off"], job["names"], W)
            assert track.summary() == dm.summary(res["positions"]["depth"])
            track.close()
        # pp_polish_files_multi: one context makes the file, two are refused by name before any input is looked at
        L = pp.lib()
        opt = pp.PolishOptions(0.2, 0.5, 10, 5, 0, None, 1)
        sams = (C.c_char_p * 2)(*[s.encode() for s in ds["sams"]])
        c.set_depth(True, W)
        one = (C.c_void_p * 1)(c._h)
        res = pp.Bytes()
        assert L.pp_polish_files_multi(one, 1, fa.encode(), sams, 2, C.byref(opt), C.byref(res)) == 0
        assert C.string_at(res.data, res.len) == w["fasta"]
        L.pp_bytes_free(C.byref(res))
        assert c.depth() == w["bins"]
        c2 = pp.Context(0)
        try:
            two = (C.c_void_p * 2)(c._h, c2._h)
            rc = L.pp_polish_files_multi(two, 2, b"/no/such/assembly.fasta", sams, 2, C.byref(opt), C.byref(res))
            assert rc == pp.ERR_QUIT and b"--depth runs on one GPU" in L.pp_last_error(c._h)
            with pytest.raises(pp.PolypolishError):
                c.depth()
        finally:
            c2.close()
        c.set_depth(False)
    finally:
        c.close()
