"""The plain model of pp_filter_records (tests/filter_records_model.py) pinned to the oracle, on the CPU: the raw batches of every
case of its table are written as the equivalent SAM texts (the QNAME derived from the id, unaligned records as lines with
FLAG & 4) and go through the oracle's `filter`; the verdict of every aligned line, the report and the way the command ends must
be the model's.  This is the check that the reference side of tests/test_filter_records_gpu.py is right.  Also here: the shape
of the generated cases (what their names promise)."""
import numpy as np
import pytest

import filter_model as fm
import filter_records_model as frm


@pytest.mark.parametrize("name", list(frm.CASES))
def test_model_is_the_oracle_on_every_case(orc, tmp_path, name):
    build, runs = frm.CASES[name]
    raws = build()
    paths = frm.write_sams(raws, tmp_path)
    o1, o2 = str(tmp_path / "o1.sam"), str(tmp_path / "o2.sam")
    for orientation, low_p, high_p in runs:
        what = (name, orientation, low_p, high_p)
        try:
            want, err = orc.filter_files(paths[0], paths[1], o1, o2, orientation, low_p, high_p), None
        except orc.OrcError as e:
            want, err = None, e
        try:
            got, gerr = frm.command(raws, orientation, low_p, high_p), None
        except (fm.Quit, fm.Panic) as e:
            got, gerr = None, e
        if err is not None:
            assert gerr is not None, (what, "the oracle ends with", err.code, err.msg, "the model does not")
            if err.code == orc.PANIC:
                assert isinstance(gerr, fm.Panic), (what, err.msg, gerr)
            else:
                assert err.code == orc.QUIT and isinstance(gerr, fm.Quit), (what, err.msg, gerr)
                if gerr.msg == frm.MSG_FILE1:   # (the reference names the file)
                    assert err.msg == f'no alignments found in "{paths[0]}"', (what, err.msg)
                else:
                    assert gerr.msg == err.msg, what
            continue
        assert gerr is None, (what, "the model ends with", gerr, "the oracle does not")
        for k in ("counts", "orientation", "low", "high", "before", "after"):
            assert got["report"][k] == want[k], (what, k, got["report"][k], want[k])
        for f, path in enumerate((o1, o2)):
            with open(path, "rb") as fh:
                tags = fm.failed_lines(fh.read())
            assert len(tags) == len(got["pass"][f]) == got["counts"][f][0], (what, f)
            bad = np.flatnonzero(tags != got["pass"][f])
            assert not len(bad), (what, f"file {f + 1}: the verdicts of aligned records {bad[:8].tolist()} differ")


def test_cases_have_the_shape_their_names_promise():
    def ids(raw):
        return raw["read_id"][frm.aligned(raw)].tolist()
    r = frm.CASES["ids_0_and_2_64_minus_1"][0]()
    assert {0, frm.U64_MAX} <= set(ids(r[0])) and {0, frm.U64_MAX} <= set(ids(r[1]))
    r = frm.CASES["ids_equal_in_the_low_32_bits"][0]()
    assert len({i & 0xFFFFFFFF for i in ids(r[0]) + ids(r[1])}) == 1 and len(set(ids(r[0]))) > 100
    r = frm.CASES["ids_multiples_of_the_table_capacity"][0]()
    cap = frm.table_capacity(len(ids(r[0])) + len(ids(r[1])))
    assert all(i % cap == 0 for i in ids(r[0]) + ids(r[1])) and len(set(ids(r[0]))) > 100
    r = frm.CASES["a_read_far_apart_in_its_file"][0]()
    at = np.flatnonzero(r[0]["read_id"] == 0)
    n = len(r[0]["flag"])
    assert len(at) == 3 and at[0] == 0 and 1000 <= at[1] < n - 1000 and at[2] == n - 1 and int(r[1]["read_id"][-1]) == 0
    r = frm.CASES["unaligned_records_interleaved"][0]()
    a = frm.aligned(r[0])
    assert (r[0]["flag"] & 4).any() and (a != np.arange(len(a))).any()
    r = frm.CASES["reads_only_in_file_2"][0]()
    assert set(ids(r[1])) - set(ids(r[0]))
    assert len(frm.aligned(frm.CASES["file_2_empty"][0]()[1])) == 0 and len(frm.aligned(frm.CASES["file_1_empty"][0]()[0])) == 0
    r = frm.CASES["one_read_300_here_2_there"][0]()
    big = [i for i in set(ids(r[0])) if ids(r[0]).count(i) == 300]
    assert len(big) == 1 and ids(r[1]).count(big[0]) == 2
    r = frm.CASES["no_runs_at_all"][0]()
    assert not r[0]["n_cig"].any() and not r[1]["n_cig"].any()
    r = frm.CASES["two_unknown_references"][0]()
    assert {1000, 1001} <= set(r[0]["contig"].tolist())
    for n in (255, 256, 257):
        r = frm.CASES[f"aligned_{n}"][0]()
        assert len(frm.aligned(r[0])) == n == len(frm.aligned(r[1])) and len(r[0]["flag"]) > n
    sizes = [len(frm.aligned(frm.CASES[k][0]()[0])) for k in ("large_a", "tiny", "large_b")]
    assert sizes[0] > 1000 * sizes[1] and sizes[2] > 1000 * sizes[1]


def test_a_cigar_range_outside_the_array_is_an_argument_error_of_the_model():
    raws = frm.CASES["aligned_255"][0]()
    r = int(frm.aligned(raws[1])[7])
    raws[1]["cig_off"][r] = len(raws[1]["cigar"])
    with pytest.raises(frm.ArgError) as e:
        frm.command(raws)
    assert (e.value.file, e.value.record) == (1, r)
