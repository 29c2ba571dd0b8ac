"""pp_bam_sort (pp_bam_sort.hip) against its plain model (tests/bam_sort_model.py): perm, the offsets in its order and the rewritten
header BYTE FOR BYTE, the counts and the carried verdicts, with the bytes in host memory and in device memory.  The counts stand around
a wave and the sort's tile (regroup_geometry: the sort is pp_rg_sort.h's); the keys are made so that each of the key's eight bytes
decides the order alone -- bytes 0..6 exactly (byte 6 needs 2^16 and more references: a header of 1.7 MB whose names are empty), byte
7 through unplaced records, since a ref_id of 2^24 and more needs a header of 150 MB --, then ties, sorted and reversed input, the
strand bit, pos == -1 and unplaced records.  Offsets are odd, unordered and duplicated, and device bytes start at every alignment and
end where their tensor ends.  Every refusal is checked with its record: nothing here depends on a fault.  Needs an MI355X: `-m gpu`."""
import ctypes as C
import struct

import numpy as np
import pytest

import bam_model as bm
import bam_sort_model as sm
import bam_tag_model as tm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pp():
    import polypolish_amd
    return polypolish_amd


@pytest.fixture(scope="module")
def ctx(pp):
    c = pp.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tile(pp):
    t = pp.regroup_geometry()
    assert t >= 256 and t % 64 == 0
    return t


def on_device(b, off, shift=0):
    """(data, rec_off, keep) for mem = MEM_DEVICE: the bytes `shift` bytes into a tensor that ends with them"""
    import torch
    dev = torch.device("cuda:0")
    host = np.zeros(shift + max(len(b), 1), np.uint8)
    host[shift:shift + len(b)] = np.frombuffer(bytes(b), np.uint8)
    tb = torch.from_numpy(host).to(dev)
    to = torch.from_numpy(np.ascontiguousarray(off, np.uint64).view(np.int64).copy()).to(dev) if len(off) else torch.zeros(1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    return (tb.data_ptr() + shift, len(b)), (to.data_ptr(), len(off)), (tb, to)


def sorted_on(pp, ctx, b, at, off, mem, shift=0):
    if mem == pp.MEM_HOST:
        return pp.BamSorted(ctx, b, at, off, mem), None
    data, rec_off, keep = on_device(b, off, shift)
    return pp.BamSorted(ctx, data, at, rec_off, mem), keep


def check(pp, ctx, b, at, off, mems=None, shift=0, passed=None):
    """the link on (b, at, off) is the model on it, in both memory forms; -> the model's answer"""
    want = sm.sort(b, at, off)
    n_al = int(((want["flag"] & 4) == 0).sum())
    v = np.asarray(passed, np.uint8) if passed is not None else (np.arange(n_al) * 7 % 251).astype(np.uint8)
    for mem in mems or (pp.MEM_HOST, pp.MEM_DEVICE):
        s, keep = sorted_on(pp, ctx, b, at, off, mem, shift)
        try:
            perm = s.perm()
            assert s.n_rec == len(off) and perm.dtype == np.uint32
            assert np.array_equal(perm, want["perm"]), (mem, perm[:16], want["perm"][:16])
            assert np.array_equal(s.rec_off(), want["rec_off"]), mem
            assert s.head == want["head"], mem
            assert s.counts() == want["counts"], (mem, s.counts(), want["counts"])
            assert np.array_equal(s.carry_pass(v), sm.carry_pass(want["flag"], want["perm"], v)), mem
        finally:
            s.close()
            del keep
    return want


def sizes(tile):
    return [0, 1, 63, 64, 65, tile - 1, tile, tile + 1, 2 * tile + 1]


def test_counts_around_a_wave_and_the_tile(pp, ctx, tile):
    for n in sizes(tile):
        want = check(pp, ctx, *sm.stream(sm.random_records(n, seed=n)))
        assert n < 3 or want["counts"][0] > 0, n


def many_refs(n_ref):
    """a header of n_ref references whose names are empty (l_name 1: the NUL alone), 9 bytes each"""
    one = np.frombuffer(struct.pack("<i", 1) + b"\0" + struct.pack("<i", 1000), np.uint8)
    text = b"@HD\tVN:1.6\n"
    return b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", n_ref) + np.tile(one, n_ref).tobytes()


@pytest.fixture(scope="module")
def wide_header():
    return many_refs((3 << 16) + 1)


@pytest.mark.parametrize("byte", range(8))
def test_keys_that_differ_in_one_byte_of_the_eight(pp, ctx, wide_header, byte):
    rng = np.random.default_rng(byte)
    n = 700
    if byte < 4:                     # the low word: (pos + 1) << 1 | strand
        low = rng.integers(0, 256, n).astype(np.uint64) << np.uint64(8 * byte)
        recs = [sm.rec(2, (int(w) >> 1) - 1, (int(w) & 1) << 4, b"q%d" % i) for i, w in enumerate(low)]
        header = sm.HEADER
    elif byte < 7:                   # ref_id's bits 0..7, 8..15, 16..23
        top = 256 if byte < 6 else 4
        recs = [sm.rec(int(k) << (8 * (byte - 4)), 77, 16, b"q%d" % i) for i, k in enumerate(rng.integers(0, top, n))]
        header = wide_header
    else:                            # placed on reference 0 or unplaced: the high word is 0 or 0xFFFFFFFF
        recs = [sm.rec(-int(k), -1, 4, b"q%d" % i) for i, k in enumerate(rng.integers(0, 2, n))]
        header = sm.HEADER
    b, at, off = sm.stream(recs, header)
    k, _ = sm.keys(b, at, off)
    differ = np.bitwise_or.reduce(k ^ k[0])
    assert differ and all((int(differ) >> (8 * j)) & 0xFF == 0 for j in range(8) if j != byte and not (byte == 7 and j >= 4))
    want = check(pp, ctx, b, at, off)
    assert want["counts"][0] > n // 2


def test_ties_sorted_reversed_strand_and_unplaced(pp, ctx):
    n = 5000
    same = [sm.rec(1, 500, 0, b"q%d" % i) for i in range(n)]
    want = check(pp, ctx, *sm.stream(same))
    assert want["counts"] == (0, 0) and np.array_equal(want["perm"], np.arange(n, dtype=np.uint32)), "all keys equal: the input's order"
    ordered = [sm.rec(i // 2000, 3 * (i % 2000), 0, b"q%d" % i) for i in range(n)] + [sm.rec(-1, -1, 4, b"u")] * 3
    want = check(pp, ctx, *sm.stream(ordered))
    assert want["counts"] == (0, 3), "already sorted"
    want = check(pp, ctx, *sm.stream(ordered[::-1]))
    assert want["counts"][0] >= n and want["perm"][0] == len(ordered) - 1, "reversed: the unplaced records are the first of the input and the last of the output"
    assert want["perm"][-3:].tolist() == [0, 1, 2], "... in the input's order"
    strand = [sm.rec(0, 100, (i & 1) << 4, b"q%d" % i) for i in range(n)]
    want = check(pp, ctx, *sm.stream(strand))
    assert want["perm"][:3].tolist() == [0, 2, 4] and want["perm"][-1] == n - 1, "the strand bit alone: forward first"
    minus_one = [sm.rec(1, -1 + (i % 3), 0, b"q%d" % i) for i in range(n)] + [sm.rec(0, -1, 16, b"z"), sm.rec(-1, 5, 4, b"w"), sm.rec(0, -1, 0, b"y")]
    want = check(pp, ctx, *sm.stream(minus_one))
    assert want["perm"][:2].tolist() == [n + 2, n] and want["perm"][-1] == n + 1, "pos == -1 is the first of its reference; ref_id == -1 the last whatever its pos"
    mixed = sm.random_records(n, seed=5, unplaced=0.4)
    want = check(pp, ctx, *sm.stream(mixed))
    assert 0 < want["counts"][1] < n


def test_unaligned_unordered_and_duplicate_offsets(pp, ctx):
    recs = sm.random_records(600, seed=8)
    pad = lambda i: (i % 7) if i + 1 < len(recs) else 0      # noqa: E731 (nothing behind the last record: it ends the bytes)
    b, at, off = sm.stream(recs, lead=3, pad=pad)
    assert set((off % 16).tolist()) == set(range(16)) and int(off[-1]) + len(recs[-1]) == len(b)
    check(pp, ctx, b, at, off)
    rng = np.random.default_rng(9)
    shuffled = rng.permutation(off)
    check(pp, ctx, b, at, shuffled)
    twice = np.concatenate([shuffled[:200], shuffled[:200], off[-1:], off[-1:]])
    want = check(pp, ctx, b, at, twice)
    assert len(np.unique(want["rec_off"])) < len(twice)
    check(pp, ctx, b, at, off[::3])


@pytest.mark.parametrize("shift", range(16))
def test_device_bytes_at_every_alignment_that_end_with_their_tensor(pp, ctx, shift):
    recs = sm.random_records(130, seed=20 + shift)
    b, at, off = sm.stream(recs)
    assert int(off[-1]) + len(recs[-1]) == len(b)
    check(pp, ctx, b, at, np.concatenate([off[-1:], off]), mems=(pp.MEM_DEVICE,), shift=shift)


def test_sorting_is_idempotent_and_two_calls_give_identical_bytes(pp, ctx):
    b, at, off = sm.stream(sm.random_records(9000, seed=30))
    first, second = pp.BamSorted(ctx, b, at, off), pp.BamSorted(ctx, b, at, off)
    try:
        assert np.array_equal(first.perm(), second.perm()) and np.array_equal(first.rec_off(), second.rec_off())
        assert first.head == second.head and first.counts() == second.counts() and first.counts()[0] > 0
        again = check(pp, ctx, first.head + b[at:], len(first.head), first.rec_off() + np.uint64(len(first.head) - at))
        assert again["counts"][0] == 0 and again["head"] == first.head, "what is sorted stays, and its header too"
    finally:
        first.close()
        second.close()


def test_a_large_job_and_then_a_small_one_on_one_context(pp, ctx):
    big = sm.random_records(4000, seed=40)
    b, at, off = sm.stream(big)
    rng = np.random.default_rng(41)
    check(pp, ctx, b, at, rng.choice(off, 150_000), mems=(pp.MEM_DEVICE,))
    check(pp, ctx, *sm.stream(sm.random_records(100, seed=42)))
    check(pp, ctx, b, at, off[:70], mems=(pp.MEM_HOST,))


def test_carried_verdicts_with_unaligned_records_between(pp, ctx):
    recs = sm.random_records(3000, seed=50, unplaced=0.3)
    b, at, off = sm.stream(recs)
    n_al = sum(1 for r in recs if not r[18] & 4)
    passed = (np.random.default_rng(51).random(n_al) < 0.6).astype(np.uint8)
    check(pp, ctx, b, at, off, passed=passed)
    s = pp.BamSorted(ctx, b, at, off)
    try:
        for wrong in (n_al - 1, n_al + 1, 0):
            with pytest.raises(pp.PolypolishError) as e:
                s.carry_pass(np.ones(wrong, np.uint8))
            assert e.value.code == pp.ERR_ARG and f"{n_al} aligned" in str(e.value)
    finally:
        s.close()
    none = [sm.rec(0, 9 - i, 4, b"u%d" % i) for i in range(10)]
    check(pp, ctx, *sm.stream(none), passed=np.zeros(0, np.uint8))


HEADERS = {"so_replaced": "@HD\tVN:1.6\tSO:unsorted\tGO:query\n@SQ\tSN:a\tLN:9\n", "so_appended": "@HD\tVN:1.5\n@CO\tx\n", "other_first": "@SQ\tSN:a\tLN:9\n@HD\tVN:1.0\n",
           "no_text": "", "hd_alone_no_newline": "@HD", "hdx": "@HDX\tSO:queryname\n", "crlf": "@HD\tVN:1.6\r\n@CO\tSO:x\r\n", "padded": "@HD\tVN:1.6\tSO:queryname\n\0\0\0"}


@pytest.mark.parametrize("name", sorted(HEADERS))
def test_the_header_of_every_form(pp, ctx, name):
    header = bm.header_bytes([("a", 9), ("bb", 10)], HEADERS[name])
    want = check(pp, ctx, *sm.stream(sm.random_records(20, seed=1, n_ref=2), header))
    assert b"SO:coordinate" in want["head"] and want["head"].count(b"SO:coordinate") == 1
    assert bm.header(want["head"])["names"] == [b"a", b"bb"] and bm.header(want["head"])["records_at"] == len(want["head"])


def refused(pp, ctx, b, at, off, code, bad, kind=None):
    try:
        sm.sort(b, at, off)
    except sm.SortError as m:
        assert (m.code, m.bad_record) == (code, bad) and (kind is None or m.kind == kind), ("the model refuses the same record", m)
    else:
        raise AssertionError("the model takes these records")
    for mem in (pp.MEM_HOST, pp.MEM_DEVICE):
        with pytest.raises(pp.PolypolishError) as e:      # (an exception: no object)
            sorted_on(pp, ctx, b, at, off, mem)
        assert (e.value.code, e.value.bad_record) == (code, bad), (mem, e.value)


def test_defective_records(pp, ctx):
    recs = sm.random_records(40, seed=6)
    b, at, off = sm.stream(recs)
    last = int(off[-1])
    for kind, data, o in ((tm.CUT, b, len(b) + 1), (tm.CUT, b, 2 ** 63), (tm.CUT, b, len(b)), (tm.CUT, b, len(b) - 3), (tm.PAST, b[:-1], last),
                          (tm.SMALL, b[:last] + (31).to_bytes(4, "little") + b[last + 4:], last)):
        planted = np.concatenate([off[:2], [o], off[2:4], [o]]).astype(np.uint64)      # the defect twice: the first one is named
        refused(pp, ctx, data, at, planted, pp.ERR_ARG, 2, kind)
    for kind, bad in ((sm.POS, sm.rec(0, -2)), (sm.POS, sm.rec(-1, -(2 ** 31))), (sm.REF, sm.rec(-2, 5)), (sm.REF, sm.rec(3, 5)), (sm.REF, sm.rec(2 ** 31 - 1, 5)),
                      (sm.REF, sm.rec(-(2 ** 31), 5))):
        planted = recs[:5] + [bad] + recs[5:9] + [sm.rec(0, -7), sm.rec(9, 0)]
        refused(pp, ctx, *sm.stream(planted), pp.ERR_ARG, 5, kind)
    check(pp, ctx, *sm.stream(recs[:5] + [sm.rec(2, 2 ** 31 - 1)]))                    # the last reference, the largest position
    refused(pp, ctx, *sm.stream([sm.rec(0, 5)], bm.header_bytes([], "@HD\tVN:1.6\n")), pp.ERR_ARG, 0, sm.REF)      # no references: none to stand on
    check(pp, ctx, *sm.stream([sm.rec(-1, 5, 4)], bm.header_bytes([], "")))


def test_headers_that_are_refused_and_other_arguments(pp, ctx):
    b, at, off = sm.stream(sm.random_records(40, seed=6))
    refused(pp, ctx, b"SAM\1" + b[4:], at, off, pp.ERR_ARG, None, "header")
    refused(pp, ctx, b, at - 1, off, pp.ERR_ARG, None, "header")                       # the table runs past records_at
    refused(pp, ctx, b, at + 1, off, pp.ERR_ARG, None, "header")                       # the header ends in front of records_at
    refused(pp, ctx, b, 0, off, pp.ERR_ARG, None, "header")
    refused(pp, ctx, b, len(b) + 1, off, pp.ERR_ARG, None, "records_at")
    refused(pp, ctx, b[:4] + b"\xff\xff\xff\x7f" + b[8:], at, off[:0], pp.ERR_ARG, None, "header")
    with pytest.raises(pp.PolypolishError) as e:
        pp.BamSorted(ctx, (0, 0), 0, (0, 0), pp.MEM_PEER)
    assert e.value.code == pp.ERR_ARG
    # the limits and the null arguments are looked at before anything is read
    L = pp.lib()
    arr = np.frombuffer(b, np.uint8)
    offs = np.ascontiguousarray(off, np.uint64)
    out, bad = C.c_void_p(), C.c_uint64(0)
    call = lambda bp, n_bytes, op, n_rec, outp=C.byref(out): L.pp_bam_sort(ctx._h, bp, n_bytes, at, op, n_rec, pp.MEM_HOST, outp, C.byref(bad))      # noqa: E731
    assert call(arr.ctypes.data, 1 << 40, offs.ctypes.data, len(offs)) == pp.ERR_LIMIT and not out.value
    assert call(arr.ctypes.data, len(arr), offs.ctypes.data, 0xFFFFFFFF) == pp.ERR_LIMIT and not out.value
    assert call(None, len(arr), offs.ctypes.data, len(offs)) == pp.ERR_ARG and not out.value
    assert call(arr.ctypes.data, len(arr), None, len(offs)) == pp.ERR_ARG and not out.value
    assert call(arr.ctypes.data, len(arr), offs.ctypes.data, len(offs), None) == pp.ERR_ARG
    assert L.pp_bam_sort(None, arr.ctypes.data, len(arr), at, offs.ctypes.data, len(offs), pp.MEM_HOST, C.byref(out), C.byref(bad)) == pp.ERR_ARG
    check(pp, ctx, b, at, off)                                                         # the context is fine afterwards


def test_stage_times_need_profiling(pp, ctx):
    b, at, off = sm.stream(sm.random_records(5000, seed=60))
    s = pp.BamSorted(ctx, b, at, off)
    with pytest.raises(pp.PolypolishError) as e:
        s.kernel_ms()
    assert e.value.code == pp.ERR_ARG
    s.close()
    ctx.set_profiling(True)
    try:
        s = pp.BamSorted(ctx, b, at, off)
        ms = s.stage_ms()
        assert set(ms) == {"keys", "sort", "gather"} and all(v > 0 for v in ms.values())
        assert abs(s.kernel_ms() - sum(ms.values())) < 1e-3
        s.close()
    finally:
        ctx.set_profiling(False)
