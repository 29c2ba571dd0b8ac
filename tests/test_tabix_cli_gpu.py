"""--vcf_tbi, --bed_tbi and --depth_tbi of `polish` and `filter-polish` (pp_ctx_set_tbi: pp_tabix_index behind pp_bgzf_deflate in the
drivers' make_vcf, make_bed and make_depth) on the golden pair (tests/golden/derived_e2e), from SAM text and from BAM.  Every .tbi is
the model's index (tests/tabix_model.py) of the track that was written, read back block by block; the model's reader finds every
contig's lines through it; the tracks, stdout and the log are the run's without the flags.  Then the usage errors, several contexts,
an index path that cannot be written (no track and no index are left behind), the distributed launcher, and the same through Python.
Needs an MI355X: `-m gpu`."""
import gzip
import os
import shutil

import pytest

import bgzf_model as zm
import tabix_model as tx
from test_bam_cli_gpu import run
from test_depth_cli_gpu import _command, _through_zlib, ds, log_of  # noqa: F401 (ds: the fixture)

pytestmark = pytest.mark.gpu
TRACKS = (("vcf", "--vcf", tx.VCF), ("bed", "--bed", tx.BED), ("depth", "--depth", tx.BED))


@pytest.fixture(scope="module")
def pp():
    import polypolish_amd
    return polypolish_amd


def _is_the_models_index(track_path, preset):
    """<track_path>.tbi against the model's index of the written file; -> the data lines it indexes"""
    f = open(track_path, "rb").read()
    text = _through_zlib(f)
    blocks, _, end, ok = zm.walk(f)
    assert ok and end == len(f)
    blk = list(blocks)                                         # (the EOF block's offset is the last: walk lists it as a block)
    assert len(blk) == (len(text) + tx.PAYLOAD - 1) // tx.PAYLOAD + 1
    tbi = open(track_path + ".tbi", "rb").read()
    raw = gzip.decompress(tbi)
    assert tbi[:4] == b"\x1f\x8b\x08\x04" and raw == tx.tbi_raw(text, preset, blk)
    rs = tx.rows(text, preset)
    for name in tx.parse_tbi(raw)["names"] + [b"absent"]:
        assert tx.fetch(f, raw, preset, name, 0, tx.MAX_END) == tx.scan(text, preset, name, 0, tx.MAX_END, rs)
    return len(rs)


@pytest.mark.parametrize("kind", ["sam", "bam"])
@pytest.mark.parametrize("cmd", ["polish", "filter-polish"])
def test_the_indexes_are_the_models_and_the_run_is_the_plain_one(ds, tmp_path, cmd, kind):
    a, b = tmp_path / "with", tmp_path / "without"
    a.mkdir()
    b.mkdir()
    flags = lambda d, tbi: [x for what, flag, _ in TRACKS for x in (flag, str(d / (what + ".gz")), flag + "_bgzf", *([flag + "_tbi"] if tbi else []))]
    plain = run(*_command(ds, cmd, kind, *flags(b, False)))
    r = run(*_command(ds, cmd, kind, *flags(a, True)))
    assert plain.returncode == 0 and r.returncode == 0, r.stderr.decode()[-800:]
    assert r.stdout == plain.stdout == ds["want"][cmd]["fasta"] and log_of(r) == log_of(plain)
    assert sorted(os.listdir(str(a))) == sorted([w + ".gz" for w, _, _ in TRACKS] + [w + ".gz.tbi" for w, _, _ in TRACKS]) and len(os.listdir(str(b))) == 3
    lines = {}
    for what, _, preset in TRACKS:
        assert open(str(a / (what + ".gz")), "rb").read() == open(str(b / (what + ".gz")), "rb").read(), "the track is the run's without the flag"
        lines[what] = _is_the_models_index(str(a / (what + ".gz")), preset)
    assert lines["depth"] > 10, lines
    # one flag alone, and the binned depth track
    one = tmp_path / "one"
    one.mkdir()
    r = run(*_command(ds, cmd, kind, "--depth", str(one / "d.gz"), "--depth_bgzf", "--depth_bin", "250", "--depth_tbi", "--vcf", str(one / "v.vcf")))
    assert r.returncode == 0 and r.stdout == plain.stdout and sorted(os.listdir(str(one))) == ["d.gz", "d.gz.tbi", "v.vcf"]
    assert _through_zlib(open(str(one / "d.gz"), "rb").read()) == ds["want"][cmd]["bins"] and _is_the_models_index(str(one / "d.gz"), tx.BED) > 4


def test_usage_errors_leave_nothing_behind(ds, tmp_path):
    p = str(tmp_path / "t.gz")
    for cmd in ("polish", "filter-polish"):
        for flags, words in ((["--vcf_tbi"], b"--vcf_tbi needs --vcf_bgzf"), (["--vcf", p, "--vcf_tbi"], b"--vcf_tbi needs --vcf_bgzf"),
                             (["--bed_tbi"], b"--bed_tbi needs --bed_bgzf"), (["--bed", p, "--bed_tbi"], b"--bed_tbi needs --bed_bgzf"),
                             (["--depth_tbi"], b"--depth_tbi needs --depth_bgzf"), (["--depth", p, "--depth_bin", "5", "--depth_tbi"], b"--depth_tbi needs --depth_bgzf"),
                             (["--vcf", p, "--vcf_bgzf", "--vcf_tbi", "--bed_tbi"], b"--bed_tbi needs --bed_bgzf"),
                             (["--vcf", p, "--vcf_bgzf", "--vcf_tbi", "--vcf_tbi"], b"multiple times"), (["--vcf_tbi=1"], b"--vcf_tbi")):
            r = run(*_command(ds, cmd, "sam", *flags))
            assert r.returncode == 2 and r.stdout == b"" and words in r.stderr and b"For more information, try '--help'." in r.stderr, (cmd, flags, r.stderr[-300:])
            assert os.listdir(str(tmp_path)) == []
        for flag in (b"--vcf_tbi", b"--bed_tbi", b"--depth_tbi"):
            assert flag in run(cmd, "--help").stdout
    # a run that fails leaves neither file behind
    r = run("polish", "--depth", p, "--depth_bgzf", "--depth_tbi", ds["fasta"], str(tmp_path / "missing.sam"))
    assert r.returncode == 1 and os.listdir(str(tmp_path)) == []


@pytest.mark.parametrize("env", [dict(PP_SHARE_GPU="2"), dict(PP_GPUS="2")], ids=["share_gpu", "gpus"])
def test_several_contexts_are_refused_by_the_tracks_name(ds, tmp_path, env):
    for flag in ("--vcf", "--bed", "--depth"):
        r = run(*_command(ds, "polish", "sam", flag, str(tmp_path / "t.gz"), flag + "_bgzf", flag + "_tbi"), env=env)
        assert r.returncode == 1 and r.stdout == b"" and flag.encode() + b" runs on one GPU" in r.stderr and os.listdir(str(tmp_path)) == []
        assert b"Loading" not in r.stderr, "refused before any file is opened"


def test_an_index_that_cannot_be_written_leaves_no_track_and_no_index(ds, tmp_path):
    out = str(tmp_path / "o.fa")
    for cmd in ("polish", "filter-polish"):
        for what, flag, _ in TRACKS:
            track = str(tmp_path / (what + ".gz"))
            os.makedirs(track + ".tbi/full")                    # (a directory that is not empty stands where the index would go)
            r = run(*_command(ds, cmd, "sam", flag, track, flag + "_bgzf", flag + "_tbi", "--out", out))
            assert r.returncode == 1 and r.stdout == b"" and b"Error: unable to write the index of the " in r.stderr and (track + ".tbi").encode() in r.stderr, r.stderr[-400:]
            shutil.rmtree(track + ".tbi")
            assert os.listdir(str(tmp_path)) == [], "the index is written before the FASTA, and the track is taken back"


def test_the_distributed_launcher_refuses_by_name():
    from polypolish_amd import distributed
    for flag in ("--vcf_tbi", "--bed_tbi", "--depth_tbi"):
        with pytest.raises(SystemExit) as e:
            distributed.main(["polish", flag, "a.fasta"])
        assert flag + " runs on one GPU" in str(e.value)


def test_the_same_through_python(ds, pp, tmp_path):
    import ctypes as C
    fa, w = ds["fasta"], ds["want"]["polish"]
    v, b, d = (str(tmp_path / n) for n in ("py.vcf.gz", "py.bed.gz", "py.bedgraph.gz"))
    c = pp.Context(0)
    try:
        with pytest.raises(pp.PolypolishError) as e:
            c.tbi("depth")
        assert e.value.code == pp.ERR_ARG and "pp_ctx_set_tbi" in e.value.msg
        fasta = c.polish_files(fa, ds["sams"], vcf=v, vcf_bgzf=True, bed=b, bed_bgzf=True, depth=d, depth_bgzf=True, tbi=True)
        assert fasta == w["fasta"] and sorted(os.listdir(str(tmp_path))) == sorted(os.path.basename(p) + s for p in (v, b, d) for s in ("", ".tbi"))
        for path, preset, which in ((v, tx.VCF, "vcf"), (b, tx.BED, "bed"), (d, tx.BED, "depth")):
            _is_the_models_index(path, preset)
            assert c.tbi(which) == open(path + ".tbi", "rb").read() == c.tbi(pp.TBI_TRACKS.index(which))
        assert _through_zlib(open(d, "rb").read()) == w["runs"]
        for p in os.listdir(str(tmp_path)):
            os.remove(str(tmp_path / p))
        fasta, _ = c.filter_polish_files(fa, ds["bams"][0], ds["bams"][1], depth=d, depth_bgzf=True, depth_bin=250, bed=b, tbi=["depth"])
        assert fasta == ds["want"]["filter-polish"]["fasta"] and sorted(os.listdir(str(tmp_path))) == sorted(os.path.basename(p) for p in (b, d, d + ".tbi"))
        assert _is_the_models_index(d, tx.BED) > 4
        assert c.polish_files(fa, ds["sams"]) == w["fasta"]      # off again behind the call ...
        with pytest.raises(pp.PolypolishError):
            c.tbi("depth")                                      # ... and a run that begins drops the index of the run before
        for p in os.listdir(str(tmp_path)):
            os.remove(str(tmp_path / p))
        for kw, words in ((dict(tbi=True), "tbi=True needs a bgzipped track"), (dict(depth=d, tbi="depth"), "tbi='depth' needs depth_bgzf=True"),
                          (dict(vcf=v, vcf_bgzf=True, tbi=["vcf", "bed"]), "tbi='bed' needs bed_bgzf=True"), (dict(vcf=v, vcf_bgzf=True, tbi="gff"), "is not one of vcf, bed, depth")):
            with pytest.raises(pp.PolypolishError) as e:
                c.polish_files(fa, ds["sams"], **kw)
            assert words in e.value.msg and os.listdir(str(tmp_path)) == [], kw
        os.makedirs(d + ".tbi/full")
        with pytest.raises(pp.PolypolishError) as e:
            c.polish_files(fa, ds["sams"], depth=d, depth_bgzf=True, tbi=True)
        shutil.rmtree(d + ".tbi")
        assert e.value.code == pp.ERR_QUIT and "unable to write the index of the depth track" in e.value.msg and os.listdir(str(tmp_path)) == []
        # the C side: an index without its bgzipped track is refused before any input is looked at; an unknown track
        c.set_tbi(depth=True)
        with pytest.raises(pp.PolypolishError) as e:
            c.polish_files(fa, ds["sams"])
        assert e.value.code == pp.ERR_ARG and "a .tbi indexes a bgzipped track" in e.value.msg
        c.set_depth(True, 0, False)
        with pytest.raises(pp.PolypolishError) as e:
            c.polish_files(fa, ds["sams"])
        assert e.value.code == pp.ERR_ARG
        c.set_depth(True, 0, True)
        assert c.polish_files(fa, ds["sams"]) == w["fasta"] and gzip.decompress(c.tbi("depth"))[:4] == b"TBI\1"
        c.set_tbi()
        c.set_depth(False)
        out = pp.Bytes()
        assert pp.lib().pp_ctx_tbi(c._h, 3, C.byref(out)) == pp.ERR_ARG and pp.lib().pp_ctx_tbi(c._h, -1, C.byref(out)) == pp.ERR_ARG
        assert pp.lib().pp_ctx_tbi(c._h, 0, None) == pp.ERR_ARG and pp.lib().pp_ctx_set_tbi(None, 1, 1, 1) == pp.ERR_ARG
        # pp_polish_files_multi: two contexts are refused by the track's name before any input is looked at
        c2 = pp.Context(0)
        try:
            c.set_depth(True, 0, True)
            c.set_tbi(depth=True)
            L = pp.lib()
            opt = pp.PolishOptions(0.2, 0.5, 10, 5, 0, None, 1)
            sams = (C.c_char_p * 2)(*[s.encode() for s in ds["sams"]])
            cs = (C.c_void_p * 2)(c._h, c2._h)
            res = pp.Bytes()
            assert L.pp_polish_files_multi(cs, 2, fa.encode(), sams, 2, C.byref(opt), C.byref(res)) == pp.ERR_QUIT
            assert b"--depth runs on one GPU" in L.pp_last_error(c._h)
        finally:
            c.set_tbi()
            c.set_depth(False)
            c2.close()
    finally:
        c.close()
