"""The plain model of the filter (tests/filter_model.py) pinned to the oracle, on the CPU: every generator configuration that
the GPU tests of the seam use (the same table, the same seeds and knobs) is written as two SAM texts and goes through the
oracle's `filter`; the model's orientation counts, chosen orientation, thresholds, before/after counts and the verdict of every
line must be the oracle's, and where the reference would end with an error, the model must end with the same one.  This is
the check that the reference side of tests/test_filter_seam_gpu.py is right.  Also here: the host loader (pp_filter_load
needs no GPU) gives back the generator's arrays from those texts."""
import numpy as np
import pytest

import filter_model as fm

# the orientation and percentiles every seam configuration is run with (the seam tests themselves hand thresholds over)
SEAM_RUNS = (("auto", 0.1, 99.9), ("fr", 10.0, 90.0), ("rf", 49.9, 50.1), ("ff", 25.0, 75.0), ("rr", 30.0, 60.0))


def _oracle_vs_model(orc, inp, paths, tmp_path, runs):
    o1, o2 = str(tmp_path / "o1.sam"), str(tmp_path / "o2.sam")
    for orientation, low_p, high_p in runs:
        what = (orientation, low_p, high_p)
        try:
            want, err = orc.filter_files(paths[0], paths[1], o1, o2, orientation, low_p, high_p), None
        except orc.OrcError as e:
            want, err = None, e
        try:
            got, gerr = fm.command(inp, orientation, low_p, high_p), None
        except (fm.Quit, fm.Panic) as e:
            got, gerr = None, e
        if err is not None:
            assert gerr is not None, (what, "the oracle ends with", err.code, err.msg, "the model does not")
            if err.code == orc.PANIC:
                assert isinstance(gerr, fm.Panic), (what, err.msg, gerr)
            else:
                assert err.code == orc.QUIT and isinstance(gerr, fm.Quit), (what, err.msg, gerr)
                if gerr.msg.startswith("no alignments found in"):   # (the reference names the file)
                    assert err.msg == f'no alignments found in "{paths[0]}"', (what, err.msg)
                else:
                    assert gerr.msg == err.msg, what
            continue
        assert gerr is None, (what, "the model ends with", gerr, "the oracle does not")
        for k in ("counts", "orientation", "low", "high", "before", "after"):
            assert got[k] == want[k], (what, k, got[k], want[k])
        for f, path in enumerate((o1, o2)):
            with open(path, "rb") as fh:
                tags = fm.failed_lines(fh.read())
            assert len(tags) == len(got["pass"][f]), (what, f)
            bad = np.flatnonzero(tags != got["pass"][f])
            assert not len(bad), (what, f"file {f + 1}: the verdicts of alignments {bad[:8].tolist()} differ",
                                  "reads", inp["files"][f]["read"][bad[:8]].tolist())


def _check_loader(inp, paths):
    """pp.FilterLoaded on the texts gives back the generator's arrays (the reads numbered by first appearance, ends from the
    runs, ref_id up to renaming)."""
    import polypolish_amd as pp
    want = fm.canonical(inp)
    try:
        got = pp.FilterLoaded(paths[0], paths[1])
    except pp.PolypolishError as e:
        assert len(inp["files"][0]["ref_id"]) + len(inp["files"][1]["ref_id"]) == 0 or len(inp["files"][0]["ref_id"]) == 0, e
        assert e.code == 1 and "no alignments found" in e.msg, e
        return
    try:
        assert got.n_reads == want["n_reads"]
        pairs = set()
        for f in range(2):
            g, w = got.files[f], want["files"][f]
            for k in ("read", "grp_off", "grp_idx", "flags", "ref_start"):
                assert np.array_equal(g[k], w[k]), (f, k)
            assert np.array_equal(fm.ends_array(g), fm.ends_array(w)), (f, "ends")
            pairs |= set(zip(g["ref_id"].tolist(), w["ref_id"].tolist()))
        # one renaming for both files: equal names <=> equal ids
        assert len({a for a, _ in pairs}) == len(pairs) == len({b for _, b in pairs})
    finally:
        got.close()


@pytest.mark.parametrize("name", list(fm.SEAM_CASES))
def test_model_is_the_oracle_on_every_seam_configuration(orc, tmp_path, name):
    build, _ = fm.SEAM_CASES[name]
    inp = build()
    paths = fm.write_sams(inp, tmp_path)
    runs = SEAM_RUNS[:2] if inp["n_reads"] > 100_000 else SEAM_RUNS
    _oracle_vs_model(orc, inp, paths, tmp_path, runs)
    _check_loader(inp, paths)


@pytest.mark.parametrize("name", list(fm.TEXT_CASES))
def test_model_is_the_oracle_on_every_text_configuration(orc, tmp_path, name):
    build, read_name, ref_name, runs = fm.TEXT_CASES[name]
    inp = build()
    paths = fm.write_sams(inp, tmp_path, read_name=read_name, ref_name=ref_name)
    _oracle_vs_model(orc, inp, paths, tmp_path, runs)
    _check_loader(inp, paths)


def test_thresholds_of_the_seam_cases_are_explicit_or_derived_by_the_model():
    """every configuration names its thresholds; the derived ones (an insert size that occurs) do occur"""
    for name, (build, thr) in fm.SEAM_CASES.items():
        if callable(thr):
            inp = build()
            orient, insert, _ = fm.samples(inp)
            for low, high, correct in thr(inp):
                assert low == high and low in insert[orient != fm.NOT_SAMPLED].tolist(), name
        else:
            assert thr and all(len(t) == 3 and 0 <= t[2] <= 3 for t in thr), name


def test_the_model_against_the_reference_s_own_vectors(orc):
    """get_orientation / get_insert_size on the reference's unit-test inputs (src/filter.rs tests: 150M reads at 100000 /
    200000 on either strand), through the oracle's single-function entry points."""
    for p1 in (100000, 200000, 150000):
        for p2 in (100000, 200000, 150000):
            for fl1 in (0, 16):
                for fl2 in (0, 16):
                    for c1, r1 in (("150M", [(150 << 4)]), ("10S100M5D40M", [(10 << 4) | 4, (100 << 4), (5 << 4) | 2, (40 << 4)])):
                        e1, e2 = fm.ref_end_of(p1, r1), fm.ref_end_of(p2, [(150 << 4)])
                        assert e1 == orc.get_ref_end(p1, c1)
                        assert fm.orientation_of(fl1, p1, e1, fl2, p2, e2) == \
                            fm.ORIENTATIONS.index(orc.get_orientation(fl1, p1, c1, fl2, p2, "150M"))
                        assert fm.insert_of(p1, e1, p2, e2) == orc.get_insert_size(p1, c1, p2, "150M")
    for n in (1, 2, 3, 10, 999, 1000, 1001):
        s = list(range(5, 5 + n))
        for p in (0.0001, 0.1, 1.0, 33.3, 49.9, 50.1, 99.0, 99.9, 99.9999):
            assert fm.percentile(s, p) == orc.get_percentile(s, p), (n, p)
