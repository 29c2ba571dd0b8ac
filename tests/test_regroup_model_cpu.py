"""tests/regroup_model.py -- the plain model of pp_batch_regroup -- pinned to the models of its neighbours and to the oracle (no GPU):
the gate model on the regrouped raw records of a file is the ingest model on regroup_text of that file; a name-grouped text regroups
to itself and regrouping is idempotent; and on the coordinate-sorted dataset of the chain tests the oracle refuses the sorted text,
accepts the regrouped one with the counts of the name-grouped original -- while enough records move, "*" records among them, for
the GPU tests on that dataset to mean something."""
import numpy as np
import pytest

import gate_model as gm
import ingest_model as im
import regroup_model as rm

MAX_ERRORS = 10


@pytest.fixture(scope="module")
def ds(tmp_path_factory):
    return rm.sorted_dataset(str(tmp_path_factory.mktemp("regroup_model")))


def test_perm_groups_in_the_order_of_first_records_and_keeps_file_order_inside():
    ids = np.array([7, 3, 7, 9, 3, 7, 1], np.uint64)
    assert rm.perm(ids).tolist() == [0, 2, 5, 1, 4, 3, 6]
    got = rm.regroup({**{k: np.arange(7).astype(np.uint32) for k in rm.PER_RECORD}, "read_id": ids, "seq": None, "cigar": None})
    assert got["counts"] == (4, 4) and got["raw"]["read_id"].tolist() == [7, 7, 7, 3, 3, 9, 1]
    assert rm.perm(np.zeros(0, np.uint64)).tolist() == [] and rm.perm(np.array([5], np.uint64)).tolist() == [0]
    # ids that differ only above bit 32, id 0 and id 2^64-1 are ids like any other
    ids = np.array([1 << 40, 0, 0xFFFFFFFFFFFFFFFF, (1 << 40) + (1 << 33), 1 << 40, 0xFFFFFFFFFFFFFFFF, 0], np.uint64)
    assert rm.perm(ids).tolist() == [0, 4, 1, 6, 2, 5, 3]


def test_carry_pass_follows_the_aligned_records():
    flag = np.array([0, 4, 0, 0, 4, 0], np.uint16)
    ids = np.array([1, 9, 2, 1, 2, 2], np.uint64)
    p = rm.perm(ids)
    assert p.tolist() == [0, 3, 1, 2, 4, 5]
    assert rm.carry_pass(flag, p, [10, 20, 30, 40]).tolist() == [10, 30, 20, 40]
    assert rm.carry_pass(flag, np.arange(6, dtype=np.uint32), [1, 0, 1, 0]).tolist() == [1, 0, 1, 0]


def test_a_name_grouped_text_regroups_to_itself_and_regrouping_is_idempotent(ds):
    for f in range(2):
        grouped = open(ds["sams"][f], "rb").read()
        again, p = rm.regroup_text(grouped)
        assert again == grouped and p.tolist() == list(range(len(p)))
        twice, p2 = rm.regroup_text(ds["regrouped"][f])
        assert twice == ds["regrouped"][f] and p2.tolist() == list(range(len(p2)))
        raw, _ = gm.raw_from_text(ds["contigs"], ds["sorted"][f])
        once = rm.regroup(raw)
        assert np.array_equal(once["perm"], ds["moved"][f]), "the records' perm is the lines' perm"
        back = rm.regroup(once["raw"])
        assert back["counts"][1] == 0 and back["counts"][0] == once["counts"][0]
        rm.same_raw(back["raw"], once["raw"])


@pytest.mark.parametrize("careful, max_errors", [(False, MAX_ERRORS), (True, MAX_ERRORS), (False, 2)])
def test_gate_of_the_regrouped_records_is_the_ingest_model_of_the_regrouped_text(ds, careful, max_errors):
    for f in range(2):
        raw, zp = gm.raw_from_text(ds["contigs"], ds["sorted"][f])
        g = rm.regroup(raw)
        got = gm.gate(g["raw"], max_errors, careful, rm.carry_pass(raw["flag"], g["perm"], zp))
        want = im.model(ds["contigs"], [ds["regrouped"][f]], None, max_errors, careful)
        gm.same(got["recs"], want["recs"])
        assert [got["counts"]] == [tuple(c) for c in want["counts"]]
        with pytest.raises(gm.GateError) as e:      # ... while the sorted records as they lie are refused
            gm.gate(raw, max_errors, False, zp)
        assert e.value.kind == "no_sequence"


def test_the_oracle_refuses_the_sorted_text_and_takes_the_regrouped_one(ds, orc):
    with pytest.raises(orc.OrcError) as e:
        orc.polish_files(ds["fasta"], ds["sorted_paths"], max_errors=MAX_ERRORS)
    assert e.value.args and "no alignments for read r114 contain sequence" in str(e.value)
    want = orc.polish_files(ds["fasta"], ds["sams"], max_errors=MAX_ERRORS)
    got = orc.polish_files(ds["fasta"], ds["regrouped_paths"], max_errors=MAX_ERRORS)
    assert tuple(got["counts"]) == tuple(want["counts"]) == (2466, 2382, 1924)
    assert got["fasta"] == want["fasta"]


def test_enough_records_move_and_enough_of_them_carry_no_sequence(ds):
    """a condition on the input: what the GPU tests on this dataset rely on"""
    for f in range(2):
        p = ds["moved"][f]
        moved = np.flatnonzero(p != np.arange(len(p), dtype=np.uint32))
        assert 3 * len(moved) > len(p), (f, len(moved), len(p))
        lines = [ln for ln in ds["regrouped"][f].split(b"\n") if ln and ln[:1] != b"@"]
        stars = sum(1 for j in moved.tolist() if lines[j].split(b"\t")[9] == b"*")
        assert stars > 200, (f, stars)
