"""pp_bam_tagged_head plus pp_bam_index (pp_bam_out.hip) against tests/bam_sort_model.py's bai(), BYTE FOR BYTE: over the level-0
file's block table and over the compressed file's (host and device offsets), with the bytes in host and in device memory.  The records
start and end at and across every bin boundary, end at 2^29 and one base behind it, span three windows with one N run and leave
windows empty, leave a reference between two others empty, are unplaced or unmapped but placed, and end exactly where a block ends --
with and without the eight appended bytes of failing records in front.  Every refusal is checked with its record, the first offender
of a file out of order among them.  The model's plain reader then runs on the device's index over the device's file: every record is
found through the chunks of its own interval.  Every case is a few hundred records at most.  Needs an MI355X: `-m gpu`."""
import ctypes as C

import numpy as np
import pytest

import bam_model as bm
import bam_sort_model as sm
import bam_tag_model as tm

pytestmark = pytest.mark.gpu
P = tm.PAYLOAD


@pytest.fixture(scope="module")
def pp():
    import polypolish_amd
    return polypolish_amd


@pytest.fixture(scope="module")
def ctx(pp):
    c = pp.Context(0)
    yield c
    c.close()


def on_device(b, off):
    import torch
    dev = torch.device("cuda:0")
    tb = torch.from_numpy(np.frombuffer(bytes(b), np.uint8).copy()).to(dev) if len(b) else torch.zeros(1, dtype=torch.uint8, device=dev)
    to = torch.from_numpy(np.ascontiguousarray(off, np.uint64).view(np.int64).copy()).to(dev) if len(off) else torch.zeros(1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    return (tb.data_ptr(), len(b)), (to.data_ptr(), len(off)), (tb, to)


def in_order(recs, header=sm.HEADER, seed=0, fail=0.3):
    """(b, records_at, rec_off in coordinate order, the carried verdicts, the sorted header, n_ref) of records in any order"""
    b, at, off = sm.stream(recs, header)
    s = sm.sort(b, at, off)
    n_al = int(((s["flag"] & 4) == 0).sum())
    passed = (np.random.default_rng(seed).random(n_al) >= fail).astype(np.uint8)
    return b, at, s["rec_off"], sm.carry_pass(s["flag"], s["perm"], passed), s["head"], len(bm.header(header)["names"])


def check(pp, ctx, b, at, off, passed, head, n_ref, read=True):
    """the file and its index in every form against the model; -> the level-0 index"""
    u = sm.tagged_head(b, at, off, passed, head)
    first = None
    for mem in (pp.MEM_HOST, pp.MEM_DEVICE):
        data, rec_off, keep = (b, off, None) if mem == pp.MEM_HOST else on_device(b, off)
        t = pp.BamTagged(ctx, data, at, rec_off, passed, mem, head=head)
        z = t.deflate()
        try:
            assert t.host().tobytes() == tm.frame(u)
            flat = sm.level0_blk_off(len(u))
            want = sm.bai(b, len(head), off, passed, n_ref, flat)
            got = pp.BamIndex(ctx, data, len(head), rec_off, passed, n_ref, flat, mem).bytes
            assert got == want, (mem, "the level-0 block table")
            first = got
            blk = z.blk_off()
            want = sm.bai(b, len(head), off, passed, n_ref, blk)
            for table in (blk, (z.blk_off_ptr, z.n_blocks)):
                got = pp.BamIndex(ctx, data, len(head), rec_off, passed, n_ref, table, mem).bytes
                assert got == want, (mem, "the compressed file's block table", type(table))
            if read and mem == pp.MEM_DEVICE:          # the model's reader on the device's bytes over the device's file
                f = z.host().tobytes()
                starts = bm.walk(u, len(head))[0]
                for o in starts:
                    pos, end, _, ref_id = sm.ref_end(u, o)
                    if ref_id >= 0:
                        assert o in sm.read_chunks(f, sm.query(got, ref_id, pos, end)), (ref_id, pos, end)
                assert sm.parse_bai(got)[1] == sum(1 for o in starts if sm.fields(u, o)[0] < 0)
        finally:
            z.close()
            t.close()
            del keep
    return first


def cig(ref_id, pos, runs, flag=0, qname=b"c"):
    """a record with the CIGAR runs [(length, op)]"""
    return bm.record(qname, flag, ref_id, pos, [(n << 4) | "MIDNSHP=X".index(op) for n, op in runs], "ACGT", bm.aux("NM", "C", 0))


def test_records_at_and_across_every_bin_boundary(pp, ctx):
    recs = []
    for shift in (14, 17, 20, 23, 26):
        edge = 1 << shift
        for k, pos in enumerate((edge - 5, edge - 4, edge - 3, edge - 1, edge, edge + 1)):      # ends at edge - 1, at edge, across; starts at edge - 1, edge, edge + 1
            recs.append(sm.rec(2, pos, (k & 1) << 4, b"e%d_%d" % (shift, k), n=4))
    args = in_order(recs[::-1], seed=1)
    refs, _ = sm.parse_bai(check(pp, ctx, *args))
    assert {585, 73, 9, 1, 0} < set(refs[2]["bins"]) and not refs[0]["bins"] and not refs[1]["bins"]
    assert refs[2]["bins"][0] and len(refs[2]["linear"]) == ((1 << 26) + 4) // 16384 + 1


def test_a_record_ending_at_two_to_the_29_and_one_behind_it(pp, ctx):
    ok = [sm.rec(2, 5), sm.rec(2, (1 << 29) - 4, n=4)]
    refs, _ = sm.parse_bai(check(pp, ctx, *in_order(ok)))
    assert 37448 in refs[2]["bins"] and len(refs[2]["linear"]) == 32768
    b, at, off, v, head, n_ref = in_order(ok + [sm.rec(2, (1 << 29) - 3, n=4)])
    refused(pp, ctx, b, len(head), off, v, n_ref, [0, 70000], pp.ERR_LIMIT, 2, sm.END)


def test_a_long_skip_over_three_windows_and_empty_windows(pp, ctx):
    recs = [sm.rec(1, 100), cig(1, 16000, [(2, "M"), (40000, "N"), (2, "M")]), cig(1, 16100, [(4, "S"), (3, "="), (2, "I"), (5, "D"), (1, "X")]),
            sm.rec(1, 16384 * 5 + 7), sm.rec(1, 16384 * 9)]
    refs, _ = sm.parse_bai(check(pp, ctx, *in_order(recs, fail=0.0)))
    lin = refs[1]["linear"]
    assert len(lin) == 10 and lin[0] < lin[1] == lin[2] == lin[3] and lin[4] == lin[5] > lin[3] and lin[6] == lin[7] == lin[8] == lin[9]
    check(pp, ctx, *in_order(recs, seed=3, fail=0.5))


def test_an_empty_reference_unplaced_and_unmapped_records(pp, ctx):
    recs = ([sm.rec(0, 10 * i, 0, b"a%d" % i) for i in range(40)] + [sm.rec(0, 77, 4, b"um"), sm.rec(0, 0, 4 | 16, b"um0")] + [sm.rec(2, 16384 * i, 16, b"c%d" % i) for i in range(30)]
            + [sm.rec(-1, -1, 4, b"u%d" % i) for i in range(9)] + [sm.rec(-1, 500, 4, b"up")])
    got = check(pp, ctx, *in_order(recs, seed=4))
    refs, n_no_coor = sm.parse_bai(got)
    assert n_no_coor == 10 and refs[1] == {"bins": {}, "linear": []}
    assert refs[0]["bins"][sm.PSEUDO_BIN][1] == (40, 2) and refs[2]["bins"][sm.PSEUDO_BIN][1] == (30, 0)
    only_unplaced = [sm.rec(-1, -1, 4, b"u%d" % i) for i in range(5)]
    assert sm.parse_bai(check(pp, ctx, *in_order(only_unplaced)))[1] == 5
    none = in_order([])
    assert check(pp, ctx, *none) == b"BAI\1" + (3).to_bytes(4, "little") + bytes(24) + bytes(8)


@pytest.mark.parametrize("blocks", (1, 2))
@pytest.mark.parametrize("verdicts", ("pass", "fail_first", "fail_last", "fail_two"))
def test_records_that_end_where_a_block_ends(pp, ctx, blocks, verdicts):
    head = sm.head_sorted(tm.HEADER)
    n_fail = {"pass": 0, "fail_first": 1, "fail_last": 1, "fail_two": 2}[verdicts]
    left = blocks * P - len(head) - 8 * n_fail           # the records in front of the cut, their appended bytes counted
    recs = []
    while left >= 3000 + 64:
        recs.append(tm.rec(3000, qname=b"q%d" % len(recs)))
        left -= 3000
    recs.append(tm.rec(left, qname=b"last"))
    v = np.ones(len(recs) + 3, np.uint8)
    v[{"pass": [], "fail_first": [0], "fail_last": [len(recs) - 1], "fail_two": [0, 1]}[verdicts]] = 0
    behind = [tm.rec(100, qname=b"n0"), tm.rec(64, qname=b"n1"), tm.rec(4000, qname=b"n2")]
    b, at, off, _ = tm.stream(recs + behind, [1] * (len(recs) + 3))
    u = sm.tagged_head(b, at, off, v, head)
    starts = bm.walk(u, len(head))[0]
    assert starts[len(recs)] == blocks * P, "a record ends exactly at the cut and the next one starts there"
    got = check(pp, ctx, b, at, off, v, head, 2)
    for moved in (0, 1):                                  # the same records with one more / one fewer failing: a neighbour crosses the cut
        w = v.copy()
        w[2] ^= 1
        w[3] ^= moved
        check(pp, ctx, b, at, off, w, head, 2, read=False)
    span = sm.parse_bai(got)[0][0]["bins"][sm.PSEUDO_BIN][0]
    assert span[0] == len(head) and span[1] >> 16 == (len(u) // P) * tm.BLOCK


def refused(pp, ctx, b, n_head, off, passed, n_ref, blk_off, code, bad, kind=None):
    try:
        sm.bai(b, n_head, off, passed, n_ref, blk_off)
    except sm.SortError as m:
        assert (m.code, m.bad_record) == (code, bad) and (kind is None or m.kind == kind), ("the model refuses the same record", m)
    else:
        raise AssertionError("the model takes these records")
    for mem in (pp.MEM_HOST, pp.MEM_DEVICE):
        data, rec_off, keep = (b, off, None) if mem == pp.MEM_HOST else on_device(b, off)
        with pytest.raises(pp.PolypolishError) as e:
            pp.BamIndex(ctx, data, n_head, rec_off, passed, n_ref, blk_off, mem)
        assert (e.value.code, e.value.bad_record) == (code, bad), (mem, e.value)


def test_a_file_out_of_order_is_refused_with_its_first_offender(pp, ctx):
    good = [sm.rec(0, 5 * i, 0, b"g%d" % i) for i in range(300)] + [sm.rec(1, 3, 0, b"h")] + [sm.rec(-1, 9 - i, 4, b"u%d" % i) for i in range(4)]
    b, at, off = sm.stream(good)
    v = np.ones(301, np.uint8)
    blk = [0, 1 << 20]
    sm.bai(b, at, off, v, 3, blk)
    for swap, bad in (((100, 200), 101), ((0, 299), 1), ((300, 301), 301), ((299, 300), 300), ((150, 151), 151)):
        o = off.copy()
        o[[swap[0], swap[1]]] = o[[swap[1], swap[0]]]
        refused(pp, ctx, b, at, o, v, 3, blk, pp.ERR_ARG, bad, sm.ORDER)
    twice = np.concatenate([off[:50], off[40:60]])        # a stretch again: its first record stands in front of its predecessor
    refused(pp, ctx, b, at, twice, np.ones(70, np.uint8), 3, blk, pp.ERR_ARG, 50, sm.ORDER)
    same = np.concatenate([off[:50], off[49:50], off[50:60]])
    sm.bai(b, at, same, np.ones(61, np.uint8), 3, blk)    # (a record twice in a row is in order)


def test_every_other_refusal(pp, ctx):
    recs = [sm.rec(0, 5 * i, 0, b"g%d" % i) for i in range(40)]
    b, at, off = sm.stream(recs)
    v, blk, last = np.ones(40, np.uint8), [0, 70000], int(sm.stream(recs)[2][-1])
    for kind, data, o in ((tm.CUT, b, len(b) + 1), (tm.CUT, b, len(b) - 3), (tm.PAST, b[:-1], last), (tm.SMALL, b[:last] + (31).to_bytes(4, "little") + b[last + 4:], last)):
        planted = np.concatenate([off[:2], [o], off[2:4], [o]]).astype(np.uint64)
        refused(pp, ctx, data, at, planted, np.ones(4, np.uint8), 3, blk, pp.ERR_ARG, 2, kind)
    for kind, code, bad in ((sm.REF, pp.ERR_ARG, sm.rec(3, 500)), (sm.REF, pp.ERR_ARG, sm.rec(-2, 500)), (sm.PLACED, pp.ERR_ARG, sm.rec(0, -1)), (sm.PLACED, pp.ERR_ARG, sm.rec(1, -5)),
                            ("cigar", pp.ERR_ARG, bm.record(b"x", 0, 0, 500, [], "", n_cigar_op=9)), ("cigar", pp.ERR_ARG, bm.record(b"x", 0, 0, 500, [], "", l_read_name=200))):
        b2, at2, off2 = sm.stream(recs[:5] + [bad] + recs[5:] + [sm.rec(0, 0, 0, b"late")])
        refused(pp, ctx, b2, at2, off2, np.ones(42, np.uint8), 3, blk, code, 5, kind)
    refused(pp, ctx, b, at, off, v[:-1], 3, blk, pp.ERR_ARG, None, "n_pass")
    refused(pp, ctx, b, at, off, None, 3, blk, pp.ERR_ARG, None, "n_pass")
    refused(pp, ctx, b, at, off, v, 3, [0, 1 << 48], pp.ERR_LIMIT, None, "blk_off")
    refused(pp, ctx, b, at, off, v, 3, [1 << 50, 5], pp.ERR_LIMIT, None, "blk_off")
    for wrong in ([0], [0, 70000, 140000]):               # the stream has one block: two offsets
        with pytest.raises(pp.PolypolishError) as e:
            pp.BamIndex(ctx, b, at, off, v, 3, wrong)
        assert e.value.code == pp.ERR_ARG and "block" in str(e.value)
    with pytest.raises(pp.PolypolishError) as e:
        pp.BamIndex(ctx, (0, 0), 0, (0, 0), None, 3, blk, pp.MEM_PEER)
    assert e.value.code == pp.ERR_ARG
    L = pp.lib()
    arr, offs, kb = np.frombuffer(b, np.uint8), np.ascontiguousarray(off, np.uint64), np.array(blk, np.uint64)
    out, bad = pp.Bytes(), C.c_uint64(0)
    call = lambda bp, n_bytes, op, n_rec, n_ref=3, kp=kb.ctypes.data, outp=C.byref(out): L.pp_bam_index(      # noqa: E731
        ctx._h, bp, n_bytes, at, op, n_rec, pp.MEM_HOST, v.ctypes.data, len(v), n_ref, kp, 1, pp.MEM_HOST, outp, C.byref(bad))
    assert call(arr.ctypes.data, 1 << 40, offs.ctypes.data, len(offs)) == pp.ERR_LIMIT and not out.data
    assert call(arr.ctypes.data, len(arr), offs.ctypes.data, 0xFFFFFFFF) == pp.ERR_LIMIT
    assert call(arr.ctypes.data, len(arr), offs.ctypes.data, len(offs), n_ref=(1 << 24) + 1) == pp.ERR_LIMIT
    assert call(None, len(arr), offs.ctypes.data, len(offs)) == pp.ERR_ARG
    assert call(arr.ctypes.data, len(arr), None, len(offs)) == pp.ERR_ARG
    assert call(arr.ctypes.data, len(arr), offs.ctypes.data, len(offs), kp=None) == pp.ERR_ARG
    assert call(arr.ctypes.data, len(arr), offs.ctypes.data, len(offs), outp=None) == pp.ERR_ARG
    assert call(arr.ctypes.data, len(arr), offs.ctypes.data, len(offs)) == pp.OK and out.len > 8
    L.pp_bytes_free(C.byref(out))


def test_a_few_hundred_mixed_records_through_sort_and_index(pp, ctx):
    recs = sm.random_records(800, seed=77, max_pos=60000, unplaced=0.1)
    got = check(pp, ctx, *in_order(recs, seed=5))
    refs, n_no_coor = sm.parse_bai(got)
    assert n_no_coor > 30 and all(len(R["bins"]) > 3 for R in refs)


def test_stage_times_need_profiling(pp, ctx):
    b, at, off, v, head, n_ref = in_order(sm.random_records(3000, seed=9, max_pos=60000))
    blk = sm.level0_blk_off(len(sm.tagged_head(b, at, off, v, head)))
    x = pp.BamIndex(ctx, b, len(head), off, v, n_ref, blk)
    with pytest.raises(pp.PolypolishError) as e:
        x.stage_ms()
    assert e.value.code == pp.ERR_ARG
    ctx.set_profiling(True)
    try:
        y = pp.BamIndex(ctx, b, len(head), off, v, n_ref, blk)
        ms = y.stage_ms()
        assert set(ms) == {"scans", "records", "chunks", "linear"} and all(t > 0 for t in ms.values()) and y.bytes == x.bytes
    finally:
        ctx.set_profiling(False)
    pp.BamIndex(ctx, b, len(head), off, v, n_ref, blk)
    with pytest.raises(pp.PolypolishError):
        x.stage_ms()                                      # the last call had none
