"""The plain model of pp_shard_split / pp_shard_count (tests/shard_model.py) pinned on the CPU: to a handful of answers worked
out by hand, so that it cannot drift together with the code, and pp.shard_split_host / the host pp.shard_count to it -- every
array of every rank's part of every case, with exact equality.  tests/test_shard_split_gpu.py holds the kernels to the same
model on the same cases.  No GPU needed."""
import numpy as np
import pytest

import polypolish_amd as pp
import shard_model as sm



@pytest.fixture(scope="module")
def plan():
    return sm.seam_plan(pp)


def host_agrees(plan, recs, what, wo_idx_base=0, world=sm.WORLD):
    sizes = []
    for r in range(world):
        got, got_orig = pp.shard_split_host(plan, r, recs, wo_idx_base)
        want, want_orig = sm.split(plan, r, recs, wo_idx_base)
        sm.assert_part(got, got_orig, want, want_orig, (what, "rank", r))
        sizes.append(len(want_orig))
    return sizes


# ---- the model against answers worked out by hand ------------------------------------------------------------------------------

HAND_PLAN = sm.PlanModel(4, [(0, 0, 2048, 0), (0, 2048, 4096, 1), (0, 4096, 6144, 2), (1, 0, 300, 1), (2, 0, 2048, 2), (3, 0, 5000, 0)])


def test_the_model_gives_the_part_worked_out_by_hand():
    rows = [(0, 2046, 1, b"ACGT", [sm.op(4, sm.M)]),                                   # windows 0 and 1
            (1, 0, 2, b"N-", [sm.op(2, sm.M)]),                                        # contig 1: rank 1
            (0, 5000, 3, b"a*T", [sm.op(1, sm.M), sm.op(1, sm.I), sm.op(1, sm.M)]),    # window 2
            (0, 2050, 1, b"G" * 33, [sm.op(33, sm.M)])]                                # window 1
    recs = sm.batch(rows)
    assert recs["seq_off"].tolist() == [0, 32, 64, 96] and len(recs["seq"]) == 160
    assert [sm.span(recs, i) for i in range(4)] == [4, 2, 2, 33]
    assert [sm.selected(HAND_PLAN, r, recs) for r in range(3)] == [[0], [0, 1, 3], [2]]
    recs["wo"] = sm.mirror(recs, order=[3, 1, 0, 2])
    recs["wo_runs"] = np.array([1, 4], dtype=np.uint64)
    part, orig = sm.split(HAND_PLAN, 1, recs)
    assert orig.tolist() == [0, 1, 3]
    assert part["contig"].tolist() == [0, 1, 0] and part["ref_start"].tolist() == [2046, 0, 2050] and part["k"].tolist() == [1, 2, 1]
    assert part["seq_len"].tolist() == [4, 2, 33] and part["seq_off"].tolist() == [0, 32, 64]
    assert part["n_cig"].tolist() == [1, 1, 1] and part["cig_off"].tolist() == [0, 1, 2] and part["cigar"].tolist() == [64, 32, 528]
    assert bytes(part["seq"]) == b"ACGT" + bytes(28) + b"N-" + bytes(30) + b"G" * 33 + bytes(31)
    assert bytes(part["seq4"]) == bytes([0x10, 0x23]) + b"\xff" * 14 + bytes([0x54]) + b"\xff" * 15 + b"\x33" * 16 + b"\xf3" + b"\xff" * 15
    wo = part["wo"]
    assert wo["file_idx"].tolist() == [2, 1, 0] and wo["seq_off"].tolist() == [64, 32, 0] and wo["op0"].tolist() == [528, 32, 64]
    assert wo["contig"].tolist() == [0, 1, 0] and wo["ref_start"].tolist() == [2050, 0, 2046] and wo["k"].tolist() == [1, 2, 1]
    assert wo["seq_len"].tolist() == [33, 2, 4] and part["wo_runs"].tolist() == [1, 3]
    # rank 2: the three-run record, its entry the last of the mirror
    part, orig = sm.split(HAND_PLAN, 2, recs)
    assert orig.tolist() == [2] and part["cigar"].tolist() == [16, 17, 16] and part["wo"]["op0"].tolist() == [sm.WO_MULTI_RUN]
    assert bytes(part["seq4"]) == bytes([0xFF, 0xF2]) + b"\xff" * 14 and part["wo_runs"].tolist() == [0, 1]
    # the rooms follow the source's seq array when the records start on slots of their own, the records otherwise
    recs = sm.batch(rows, order=[3, 0, 1, 2])
    assert recs["seq_off"].tolist() == [64, 96, 128, 0]
    assert sm.split(HAND_PLAN, 1, recs)[0]["seq_off"].tolist() == [64, 96, 0]
    recs = sm.batch(rows, "tight", order=[3, 0, 1, 2])
    assert recs["seq_off"].tolist() == [33, 37, 39, 0]
    assert sm.split(HAND_PLAN, 1, recs)[0]["seq_off"].tolist() == [0, 32, 64]
    # a record without SEQ bytes takes no room: it sits in front of the room of the record that starts in its slot
    rows[1] = (1, 0, 2, b"", [sm.op(2, sm.I)])
    recs = sm.batch(rows, order=[3, 1, 0, 2])
    assert recs["seq_off"].tolist() == [64, 64, 96, 0]
    part = sm.split(HAND_PLAN, 1, recs)[0]
    assert part["seq_off"].tolist() == [64, 64, 0] and len(part["seq"]) == 96
    recs["seq_off"][1] = 17                                                            # ... wherever in the slot it says it is
    assert sm.split(HAND_PLAN, 1, recs)[0]["seq_off"].tolist() == [64, 0, 0]
    # counting adds
    assert sm.count(np.array([0, 3, 4, 3, 0xFFFFFFFF], np.uint32), 4, [5, 0, 0, 1]) == [6, 0, 0, 3]


def test_the_seam_batch_goes_where_the_hand_says(plan):
    """every record of the seam batch against the units it must reach, worked out by hand next to the record: the model and
    the host loop"""
    recs, where = sm.seam_batch()
    first = {c: plan.unit_contig.tolist().index(c) for c in range(4)}
    last = {c: len(plan.unit_contig) - 1 - plan.unit_contig.tolist()[::-1].index(c) for c in range(4)}

    def ranks(units):
        us = [len(plan.unit_contig) - 1 if u == "fallback" else last[u[1]] if u[0] == "last" else first[u[0]] + u[1] for u in units]
        return {int(plan.unit_rank[u]) for u in us}
    spans = [sm.span(recs, i) for i in range(len(where))]
    assert spans[:16] == [1, 2, 1, 8, 3020, 3020, 3020, 3020, 1, 1, 1, 8, 32 * sm.BIG, 32 * sm.BIG, 1 << 32, 4]
    assert sorted(int(x) for x in recs["seq_len"][-len(sm.SEAM_SEQ_LENS):]) == list(sm.SEAM_SEQ_LENS)
    assert set(np.unique(recs["seq"]).tolist()) == set(sm.ALPHABET.tolist())
    for r in range(sm.WORLD):
        by_hand = [i for i, units in enumerate(where) if r in ranks(units)]
        assert sm.selected(plan, r, recs) == by_hand, r
        assert pp.shard_split_host(plan, r, recs)[1].tolist() == by_hand, r


# ---- the host loop against the model --------------------------------------------------------------------------------------------

def test_case_a_the_seam_batch(plan):
    recs, _ = sm.seam_batch()
    host_agrees(plan, recs, "seam")
    with_mirror = dict(recs, wo=sm.mirror(recs), wo_runs=np.array([len(recs["contig"])], dtype=np.uint64))
    host_agrees(plan, with_mirror, "seam with a mirror")


@pytest.mark.parametrize("n", sm.SIZES)
def test_case_b_sizes(plan, n):
    recs = sm.size_batch(n)
    sizes = host_agrees(plan, recs, n)
    assert sum(sizes) >= n
    if n:
        host_agrees(plan, dict(recs, wo=sm.mirror(recs), wo_runs=np.array([n], dtype=np.uint64)), (n, "with a mirror"))


def test_case_b_one_rank_takes_everything_and_a_rank_may_take_nothing(plan):
    recs = sm.size_batch(257)
    n = len(recs["contig"])
    one = pp.Plan(sm.CONTIG_OFF, [200, 20, 20, 17], 1, sm.MIN_WINDOW)
    for src in (recs, dict(recs, wo=sm.mirror(recs), wo_runs=np.array([n], dtype=np.uint64))):
        assert host_agrees(one, src, "world 1", world=1) == [n]
    rows = [r for r in sm.random_rows(400, 11) if r[0] == 0 and r[1] + 120 < 2048]   # window 0 of contig 0 only
    assert len(rows) > 20
    recs = sm.batch(rows)
    for src in (recs, dict(recs, wo=sm.mirror(recs), wo_runs=np.array([len(rows)], dtype=np.uint64))):
        sizes = host_agrees(plan, src, "a rank without records")
        assert sorted(sizes) == [0, 0, len(rows)]


@pytest.mark.parametrize("case", range(9))
def test_case_c_seq_layouts(plan, case):
    name, recs = sm.layout_cases()[case]
    host_agrees(plan, recs, name)
    host_agrees(plan, dict(recs, wo=sm.mirror(recs), wo_runs=np.array([len(recs["contig"])], dtype=np.uint64)), (name, "with a mirror"))


def test_case_c_covers_both_orders(plan):
    """the layout cases do reach both rules: parts whose rooms follow the source's seq array and not the records, and parts in
    record order from a source that is not"""
    follows = {}
    for name, recs in sm.layout_cases():
        part, orig = sm.split(plan, 1, recs)
        has = part["seq_len"] > 0
        src = recs["seq_off"][orig][has].astype(np.int64)
        got = part["seq_off"][has].astype(np.int64)
        follows[name] = (bool((np.diff(got[np.argsort(src, kind="stable")]) > 0).all()), bool((np.diff(got) > 0).all()), bool((np.diff(src) > 0).all()))
    assert follows["rooms shuffled"] == (True, False, False)
    assert follows["tight out of record order"] == (False, True, False)
    assert follows["two records sharing one room"][:2] == (False, True)
    for name in ("zero-length records at the offset of a record elsewhere in the file", "a zero-length record at seq_bytes",
                 "zero-length records at unaligned offsets"):
        assert follows[name] == (True, False, False), name


@pytest.mark.parametrize("case", range(9))
def test_case_d_mirrors(plan, case):
    name, recs, base = sm.mirror_cases()[case]
    host_agrees(plan, recs, name, wo_idx_base=base)
    want = sm.split(plan, 0, recs, base)[0]
    assert ("wo" in want) == ("outside" not in name), name
    assert ("wo_runs" in want) == (name in ("empty runs", "sixteen runs") or name.endswith("as a view")), name


@pytest.mark.parametrize("n_contigs", sm.COUNT_CONTIGS)
@pytest.mark.parametrize("n", sm.COUNT_SIZES)
def test_case_e_count(n, n_contigs):
    contig, before = sm.count_case(n, n_contigs)
    want = sm.count(contig.tolist(), n_contigs, [int(x) for x in before])
    got = pp.shard_count(None, n, contig.ctypes.data, pp.MEM_HOST, n_contigs, into=before.copy())
    assert [int(x) for x in got] == want
    assert sum(want) - int(before.sum()) == int((contig < n_contigs).sum())
    assert n < 100 or int((contig >= n_contigs).sum()) > 0
