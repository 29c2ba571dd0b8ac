"""The device tokenizer (pp_dev_ingest_*: pp_tokenize.hip on pp_devtext.h) against the plain model of tests/ingest_model.py,
which tests/test_ingest_model_cpu.py pins to the host ingest and the oracle on the same named cases: texts built to the byte
around the tokenizer's seams -- the three instances of the line staging with lines on either side of the staged / unstaged
boundary at every offset of the wave's start, files whose average line length picks the wrong instance, file sizes and
newlines on the edges of the newline kernels' threads and workgroups, QNAMEs around the eight-byte compare, SEQ lengths around
the 16-byte chunks and the 128-byte trips of the copy with lower case and its neighbours in every byte lane, "*" records filled
from any line of their group, assemblies around the LDS limit of the window split, the split over one, two, seven and more than
64 workgroups, batches over several files with and without pp_dev_ingest_expect, the filtered entry point, and every error the
model knows.  The same texts go through the filter's device loader, which stages its lines the same way.  Needs an MI355X."""
import os
import subprocess

import numpy as np
import pytest

import filter_model as fm
import ingest_model as im
from layout_check import check_seq4_mirror, check_seq_layout, check_window_order_mirror, same_ingest, same_records

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pp():
    import polypolish_amd
    return polypolish_amd


@pytest.fixture(scope="module")
def ctx(pp):
    c = pp.Context(0)
    yield c
    c.close()


def _expected(pp, c, fa, sams):
    """the model's records, or the host ingest's error where the model says there is one (same code; the CPU pin has tied the two
    messages together)"""
    try:
        return c.model(sams), None
    except im.ModelError as e:
        with pytest.raises(pp.PolypolishError) as he:
            pp.ingest(fa, sams, max_errors=c.max_errors, careful=c.careful, verdicts=c.verdicts)
        assert he.value.code == e.code
        return None, (he.value.code, he.value.msg)


def _check(pp, ctx, c, fa, sams, m, err, what, seq_layout=None, expect=None):
    """one batch of the device tokenizer against the model: the records, the layout of the seq array, both mirrors, the counts"""
    try:
        got, gerr = pp.ingest_device(ctx, fa, sams, max_errors=c.max_errors, careful=c.careful, seq_layout=seq_layout, expect=expect,
                                     verdicts=c.verdicts), None
    except pp.PolypolishError as e:
        got, gerr = None, (e.code, e.msg)
    assert gerr == err, (what, gerr, err)
    if err is not None:
        return None
    _, _, off, _, recs, counts = got
    assert counts == m["counts"], (what, counts, m["counts"])
    used = [cnt[1] for cnt in counts]
    if seq_layout == 0:
        for k, want in m["recs"].items():
            assert np.array_equal(recs[k], want), (what, k, np.flatnonzero(recs[k] != want)[:5] if len(recs[k]) == len(want)
                                                   else (len(recs[k]), len(want)))
    else:
        try:
            same_records(m["recs"], recs)
        except AssertionError as e:
            raise AssertionError((what, str(e)))
    check_seq_layout(recs, off, used, grouped=seq_layout != 0)
    check_seq4_mirror(pp, recs, expect=os.environ.get("PP_SEQ4") != "0")
    if os.environ.get("PP_WO") == "0":
        assert "wo" not in recs, what
    elif len(recs["contig"]):
        check_window_order_mirror(recs, off, used)
    return got


@pytest.mark.parametrize("name", list(im.CASES))
def test_tokenizer_equals_the_model(pp, ctx, tmp_path, monkeypatch, name):
    """every named case (its seed and knobs are in ingest_model.CASES under this name) in the window-grouped layout and in file
    order; the cases about the mirrors also without each of them; the batches over several files also with
    pp_dev_ingest_expect announcing the truth, half of it and ten times as much"""
    c = im.case(name)
    fa, sams = im.write_case(c, tmp_path)
    m, err = _expected(pp, c, fa, sams)
    for layout in (None, 0):
        _check(pp, ctx, c, fa, sams, m, err, (name, "seq_layout", layout), seq_layout=layout)
    if c.family == "several_files":
        total = sum(len(t) for t in c.texts)
        for expect in (total, total // 2, 10 * total):
            for layout in (None, 0):
                _check(pp, ctx, c, fa, sams, m, err, (name, "seq_layout", layout, "expect", expect), seq_layout=layout, expect=expect)
    if c.about_mirrors:
        for var in ("PP_SEQ4", "PP_WO"):
            monkeypatch.setenv(var, "0")
            for layout in (None, 0):
                _check(pp, ctx, c, fa, sams, m, err, (name, "seq_layout", layout, var + "=0"), seq_layout=layout)
            monkeypatch.delenv(var)


def test_window_split_over_more_than_64_workgroups(pp, ctx, tmp_path):
    """more than 64 x 16,384 aligned records: the column scan of the window split carries from one step to the next.  Against the
    host ingest (the CPU pin holds the same generator at a tenth of the size against the model)."""
    c = im.many_blocks(im.MANY_BLOCKS_N)
    fa, sams = im.write_case(c, tmp_path)
    for layout in (None, 0):
        want, err = same_ingest(pp, ctx, fa, sams, seq_layout=layout)
        assert err is None
        assert im.split_blocks(want[5][0][0]) == c.shape["nb"][0] >= 65 and want[5][0][1] > 900_000


@pytest.mark.parametrize("name", im.END_TO_END)
def test_cases_end_to_end(pp, ctx, orc, tmp_path, name):
    """one case per family through the command with either ingest, against the oracle's bytes, and the device tokenizer's batch
    through the polish against the oracle polishing the model's records"""
    c = im.case(name)
    assert not c.careful and c.max_errors == 10     # (the command's defaults)
    fa, sams = im.write_case(c, tmp_path)
    want = orc.polish_files(fa, sams, max_errors=c.max_errors, careful=c.careful)
    for mode in ("1", "0"):
        r = subprocess.run([os.path.join(ROOT, "bin", "polypolish"), "polish", fa, *sams], capture_output=True,
                           env=dict(os.environ, PP_DEVICE_INGEST=mode))
        assert r.returncode == 0 and r.stdout == want["fasta"], (name, "PP_DEVICE_INGEST=" + mode, r.stderr.decode()[-800:])
    m = c.model(sams)
    for layout in (None, 0):
        _, _, off, bases, recs, _ = pp.ingest_device(ctx, fa, sams, max_errors=c.max_errors, careful=c.careful, seq_layout=layout)
        got = ctx.polish_records(off, bases, recs)
        assert got["polished"] == orc.polish_records(off, bases, m["recs"])["polished"] == im.seqs(want["fasta"]), (name, layout)


# ---- the filter's front end on the same texts -------------------------------------------------------------------------------

PAIRS = [(n, i) for n in im.CASES if im.case(n).filter_pair for i in range(len(im.case(n).texts))]
PAIR_IDS = [n if len(im.case(n).texts) == 1 else f"{n}-file{i}" for n, i in PAIRS]


def _pair(name, i, d):
    """text i of the case and its mate (the same lines on the other strand) as the two files of a pair"""
    paths = []
    for f, mate in enumerate((False, True)):
        p = d / f"in{f + 1}.sam"
        p.write_bytes(im.case(name, mate=mate).texts[i])
        paths.append(str(p))
    return paths


@pytest.mark.parametrize("name,i", PAIRS, ids=PAIR_IDS)
def test_filter_device_loader_equals_the_host_loader(pp, ctx, tmp_path, name, i):
    """pp_filter_load_device (its lines staged by the same stage_wave_lines) against pp_filter_load on a text and its mate, array
    by array: RNAME ids up to renaming, the device loader's ends against the ends of the host loader's runs"""
    paths = _pair(name, i, tmp_path)
    try:
        host = pp.FilterLoaded(paths[0], paths[1])
    except pp.PolypolishError as e:     # (the filter takes no empty lines: the case with runs of them ends in the same error)
        assert name == "block_edge_newlines" and "too few columns" in e.msg
        with pytest.raises(pp.PolypolishError) as de:
            pp.FilterLoadedDevice(ctx, paths[0], paths[1])
        assert (de.value.code, de.value.msg) == (e.code, e.msg)
        return
    dev = pp.FilterLoadedDevice(ctx, paths[0], paths[1])
    try:
        n_aligned = [im.model(c.contigs, [c.texts[i]])["counts"][0][0] for c in (im.case(name), im.case(name, mate=True))]
        assert dev.n_reads == host.n_reads and dev.counts == host.counts
        pairs = set()
        for f in range(2):
            d, h = dev.files[f], host.files[f]
            assert len(h["flags"]) == n_aligned[f]
            for k in ("read", "grp_off", "grp_idx", "flags", "ref_start"):
                assert np.array_equal(d[k], h[k]), (name, f, k, np.flatnonzero(d[k] != h[k])[:5] if len(d[k]) == len(h[k]) else (len(d[k]), len(h[k])))
            he = fm.ends_array(h)
            assert np.array_equal(d["ref_end"], he), (name, f, "ref_end", np.flatnonzero(d["ref_end"] != he)[:5])
            pairs |= set(zip(d["ref_id"].tolist(), h["ref_id"].tolist()))
        assert len({a for a, _ in pairs}) == len(pairs) == len({b for _, b in pairs}), (name, "ref_id is not a renaming")
    finally:
        dev.close()
        host.close()


@pytest.mark.parametrize("name,i", PAIRS, ids=PAIR_IDS)
def test_filter_command_on_the_same_texts(pp, ctx, orc, tmp_path, monkeypatch, name, i):
    """pp_filter_files with either loader against the oracle's `filter`: the report and both output files byte for byte"""
    paths = _pair(name, i, tmp_path)
    o1, o2, g1, g2 = (str(tmp_path / n) for n in ("o1.sam", "o2.sam", "g1.sam", "g2.sam"))
    for orientation, low_p, high_p in (("auto", 0.1, 99.9), ("fr", 10.0, 90.0)):
        try:
            want, err = orc.filter_files(paths[0], paths[1], o1, o2, orientation, low_p, high_p), None
        except orc.OrcError as e:
            assert name == "block_edge_newlines" and "too few columns" in e.msg
            want, err = None, e
        for mode in ("1", "0"):
            monkeypatch.setenv("PP_DEVICE_FILTER", mode)
            what = (name, orientation, low_p, high_p, "PP_DEVICE_FILTER=" + mode)
            if err is not None:
                with pytest.raises(pp.PolypolishError) as ge:
                    ctx.filter_files(paths[0], paths[1], g1, g2, orientation, low_p, high_p)
                assert (ge.value.code, ge.value.msg) == (err.code, err.msg), what
                continue
            got = ctx.filter_files(paths[0], paths[1], g1, g2, orientation, low_p, high_p)
            assert got == want, what
            for g, o in ((g1, o1), (g2, o2)):
                with open(g, "rb") as a, open(o, "rb") as b:
                    assert a.read() == b.read(), (what, os.path.basename(g))
            os.remove(g1)
            os.remove(g2)
