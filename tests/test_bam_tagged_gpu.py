"""pp_bam_tagged (pp_bam_out.hip) against tests/bam_tag_model.py's frame(tagged(...)) BYTE FOR BYTE -- so every header, every patched
block_size word, every appended tag and every CRC32 is checked -- with the bytes in host memory and in device memory; there the
allocation is exactly n_bytes long.  The shapes are the smallest at which each part of the framing kernel can go wrong: lengths of the
uncompressed stream around one and two payloads, a record's word / end / appended bytes against the cut, a record longer than a block,
every source alignment against a destination that shifts by 8, the record kinds, the empty inputs, and every defect of the contract
(refused from the range checks: nothing here depends on a fault).  The model is pinned on the CPU (tests/test_bam_tag_model_cpu.py).
A block_size above 0xFFFFFFF7 needs 4 GiB of input and is not run.  Needs an MI355X: `-m gpu`."""
import ctypes as C

import numpy as np
import pytest

import bam_model as bm
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
    """(data, rec_off, keep) for mem = MEM_DEVICE: the bytes in an allocation of exactly their length"""
    import torch
    dev = torch.device("cuda:0")
    tb = torch.from_numpy(np.frombuffer(bytes(b), np.uint8).copy()).to(dev) if len(b) else torch.zeros(1, dtype=torch.uint8, device=dev)
    to = torch.from_numpy(np.ascontiguousarray(off, np.uint64).view(np.int64).copy()).to(dev) if len(off) else torch.zeros(1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    return (tb.data_ptr(), len(b)), (to.data_ptr(), len(off)), (tb, to)


def tagged_on(pp, ctx, b, at, off, passed, mem):
    if mem == pp.MEM_HOST:
        return pp.BamTagged(ctx, b, at, off, passed, mem), None
    data, rec_off, keep = on_device(b, off)
    return pp.BamTagged(ctx, data, at, rec_off, passed, mem), keep


def check(pp, ctx, b, at, off, passed):
    """both memory forms against the model; -> U'"""
    u = tm.tagged(b, at, off, passed)
    want = tm.frame(u)
    n_fail = 0 if passed is None else int((np.asarray(passed) == 0).sum())
    n_al = 0 if passed is None else len(passed)
    for mem in (pp.MEM_HOST, pp.MEM_DEVICE):
        t, keep = tagged_on(pp, ctx, b, at, off, passed, mem)
        try:
            got = t.host().tobytes()
            assert t.n_bytes == len(want), mem
            if got != want:
                first = next(i for i, (x, y) in enumerate(zip(got, want)) if x != y)
                raise AssertionError(f"mem {mem}: byte {first} (block {first // tm.BLOCK}, byte {first % tm.BLOCK} of it) is {got[first]:#x}, not {want[first]:#x}")
            assert t.counts == (n_al - n_fail, n_fail, (len(u) + P - 1) // P), mem
        finally:
            t.close()
    return u


@pytest.mark.parametrize("u_len", (0, 1, P - 1, P, P + 1, 2 * P - 1, 2 * P, 2 * P + 1))
def test_lengths_of_the_stream_around_the_payload(pp, ctx, u_len):
    assert len(check(pp, ctx, *tm.stream_of(u_len))) == u_len
    if u_len > 1:
        assert len(check(pp, ctx, *tm.stream_of(u_len, fail_last=True))) == u_len


def behind(u_len, fail_last, more, verdicts):
    """records that bring U' to u_len, then `more` with their verdicts"""
    recs, v = tm.records_to(u_len, fail_last)
    return tm.stream(recs + more, v + verdicts)


@pytest.mark.parametrize("split", (1, 2, 3))
def test_block_size_word_split_by_the_cut(pp, ctx, split):
    two = [tm.rec(200, qname=b"x"), tm.rec(90, qname=b"y")]
    for v in ([0, 1], [1, 0]):
        u = check(pp, ctx, *behind(P - split, False, two, v))
        assert tm._le32(u, P - split) == 196 + 8 * (1 - v[0]), "the word that is cut is the first record's"


def test_record_and_tag_end_on_the_cut(pp, ctx):
    two = [tm.rec(64, qname=b"x"), tm.rec(3000, flag=4, qname=b"u")]
    for fail_last in (False, True):
        u = check(pp, ctx, *behind(P, fail_last, two, [0]))
        assert (u[P - 8:P] == tm.TAG) == fail_last


@pytest.mark.parametrize("in_front", (1, 2, 3, 4, 5, 6, 7, 0))
def test_appended_bytes_split_by_the_cut(pp, ctx, in_front):
    """in_front bytes of the tag are a block's last, the others the next one's first; 0: the eight are a block's first"""
    u = check(pp, ctx, *behind(P + 8 - in_front, True, [tm.rec(100, qname=b"x")], [0]))
    assert u[P - in_front:P + 8 - in_front] == tm.TAG


@pytest.mark.parametrize("verdict", (0, 1))
def test_one_record_over_three_blocks(pp, ctx, verdict):
    u = check(pp, ctx, *behind(P - 100, False, [tm.rec(70000, qname=b"long"), tm.rec(80, qname=b"z")], [verdict, 0]))
    assert (P - 100) // P == 0 and (P - 100 + 70000) // P == 2


@pytest.mark.parametrize("lead", (0, 5))
def test_every_source_alignment_against_a_shifting_destination(pp, ctx, lead):
    recs = [tm.rec(100 + (7 * i) % 13, qname=b"a%d" % i) for i in range(96)]
    pad = lambda i: (i % 5) if i + 1 < len(recs) else 0      # noqa: E731 (nothing behind the last record: it ends the allocation)
    b, at, off, passed = tm.stream(recs, [i & 1 for i in range(len(recs))], lead, pad)
    assert set((off % 16).tolist()) == set(range(16)) and int(off[-1]) + len(recs[-1]) == len(b)
    check(pp, ctx, b, at, off, passed)


def test_record_kinds(pp, ctx):
    kinds = [tm.rec(120, qname=b"a"), tm.rec(77, flag=4, qname=b"u1"), tm.rec(130, qname=b"b", tags=bm.aux("ZP", "Z", "fail")), tm.rec(64, flag=4 | 16, qname=b"u2"),
             tm.rec(300, flag=16, qname=b"c"), tm.rec(99, flag=4, qname=b"u3")]
    b, at, off, _ = tm.stream(kinds, [1, 1, 1])
    for v in ([1, 1, 1], [0, 0, 0], [1, 0, 1]):
        u = check(pp, ctx, b, at, off, np.array(v, np.uint8))
        got_off, _, ok = bm.walk(u, at)
        assert ok and bm.decode(u, got_off)["zp"].tolist() == [v[0], 0, v[2]], "the record that came with the tag keeps it"
    u = check(pp, ctx, b, at, off, np.array([1, 0, 1], np.uint8))
    assert u.count(tm.TAG) == 2, "a failing record that carries the tag gets a second one"
    back = off[::-1].copy()
    back[1] = back[2]                                   # reverse order, one record twice
    n_al = sum(1 for o in back if not b[int(o) + 18] & 4)
    check(pp, ctx, b, at, back, np.arange(n_al, dtype=np.uint8) & 1)
    check(pp, ctx, b, at, off[1::2], None)              # a subset: the unaligned records alone take no verdict
    check(pp, ctx, b, at, off[0::2], np.array([0, 1, 0], np.uint8))


def test_no_records(pp, ctx):
    assert check(pp, ctx, tm.HEADER, len(tm.HEADER), np.zeros(0, np.uint64), None) == tm.HEADER
    assert check(pp, ctx, b"", 0, np.zeros(0, np.uint64), np.zeros(0, np.uint8)) == b""
    b, at, off, _ = tm.stream([tm.rec(100)], [1])
    assert check(pp, ctx, b, 0, off[:0], None) == b"", "records_at 0 and no records: the EOF block alone"


def mixed(n, seed, times=1):
    recs = bm.mixed_records(n, seed)
    body, off = bm.lay_out(recs)
    body, off = body * times, np.concatenate([off + np.uint64(k * len(body)) for k in range(times)])
    n_al = times * sum(1 for r in recs if not r[18] & 4)
    passed = (np.random.default_rng(seed).random(n_al) < 0.7).astype(np.uint8)
    return tm.HEADER + body, len(tm.HEADER), off + np.uint64(len(tm.HEADER)), passed


def test_mixed_records_with_random_verdicts(pp, ctx):
    b, at, off, passed = mixed(5000, 11)
    assert len(off) == 5000 and 0 < (passed == 0).sum() < len(passed) < 5000
    check(pp, ctx, b, at, off, passed)


def test_twenty_megabytes(pp, ctx):
    b, at, off, passed = mixed(5000, 12, times=22)
    u = check(pp, ctx, b, at, off, passed)
    assert len(u) > 19_000_000 and len(u) // P > 290


def test_write_and_kernel_ms(pp, ctx, tmp_path):
    b, at, off, passed = mixed(400, 3)
    ctx.set_profiling(True)
    try:
        t = pp.BamTagged(ctx, b, at, off, passed)
    finally:
        ctx.set_profiling(False)
    try:
        path = tmp_path / "tagged.bam"
        t.write(path)
        assert path.read_bytes() == t.host().tobytes() == tm.frame(tm.tagged(b, at, off, passed))
        assert t.host(5, 40).tobytes() == path.read_bytes()[5:40]
        ms = t.stage_ms()
        assert t.kernel_ms() == pytest.approx(sum(ms.values())) and ms["pass_b"] > 0
        with pytest.raises(pp.PolypolishError) as e:
            t.write(tmp_path / "no_such_directory" / "tagged.bam")
        assert e.value.code == pp.ERR_QUIT and "unable to write alignments to" in e.value.msg
    finally:
        t.close()
    u = pp.BamTagged(ctx, b, at, off, passed)
    try:
        with pytest.raises(pp.PolypolishError) as e:
            u.kernel_ms()
        assert e.value.code == pp.ERR_ARG
    finally:
        u.close()


def refused(pp, ctx, b, at, off, passed, code, bad, kind=None):
    try:
        tm.tagged(b, at, off, passed)
    except tm.TagError as m:
        assert (m.code, m.bad_record) == (code, bad) and (kind is None or m.kind == kind), "the model refuses the same record"
    else:
        raise AssertionError("the model takes these records")
    for mem in (pp.MEM_HOST, pp.MEM_DEVICE):
        with pytest.raises(pp.PolypolishError) as e:      # (an exception: no object)
            tagged_on(pp, ctx, b, at, off, passed, mem)
        assert (e.value.code, e.value.bad_record) == (code, bad), (mem, e.value)


def test_defective_records(pp, ctx):
    b, at, off, passed = mixed(40, 6)
    last = int(off[-1])
    for kind, data, o in ((tm.CUT, b, len(b) + 1), (tm.CUT, b, 2 ** 63), (tm.CUT, b, len(b)), (tm.CUT, b, len(b) - 3), (tm.PAST, b[:-1], last),
                          (tm.SMALL, b[:last] + (31).to_bytes(4, "little") + b[last + 4:], last)):
        planted = np.concatenate([off[:2], [o], off[2:4], [o]]).astype(np.uint64)      # the defect twice: the first one is named
        n_al = sum(1 for x in planted if int(x) < last and not b[int(x) + 18] & 4)
        for n_pass in (n_al, n_al + 1):                                                 # ... and it is named before a wrong n_pass is
            refused(pp, ctx, data, at, planted, np.ones(n_pass, np.uint8), pp.ERR_ARG, 2, kind)


def test_other_arguments(pp, ctx):
    b, at, off, passed = mixed(40, 6)
    refused(pp, ctx, b, at, off, passed[:-1], pp.ERR_ARG, None, "n_pass")
    refused(pp, ctx, b, at, off, np.concatenate([passed, [1]]).astype(np.uint8), pp.ERR_ARG, None, "n_pass")
    refused(pp, ctx, b, at, off, None, pp.ERR_ARG, None, "n_pass")                      # pass == NULL with aligned records
    refused(pp, ctx, b, len(b) + 1, off, passed, pp.ERR_ARG, None, "records_at")
    with pytest.raises(pp.PolypolishError) as e:
        pp.BamTagged(ctx, (0, 0), 0, (0, 0), None, pp.MEM_PEER)
    assert e.value.code == pp.ERR_ARG
    # the limits and the null arguments are looked at before anything is read
    L = pp.lib()
    arr = np.frombuffer(b, np.uint8)
    offs = np.ascontiguousarray(off, np.uint64)
    out, bad = C.c_void_p(), C.c_uint64(0)
    call = lambda bp, n_bytes, op, n_rec, outp=C.byref(out): L.pp_bam_tagged(ctx._h, bp, n_bytes, at, op, n_rec, pp.MEM_HOST, passed.ctypes.data,      # noqa: E731
                                                                              len(passed), outp, C.byref(bad))
    assert call(arr.ctypes.data, 1 << 40, offs.ctypes.data, len(offs)) == pp.ERR_LIMIT and not out.value
    assert call(arr.ctypes.data, len(arr), offs.ctypes.data, 0xFFFFFFFF) == pp.ERR_LIMIT and not out.value
    assert call(None, len(arr), offs.ctypes.data, len(offs)) == pp.ERR_ARG and not out.value
    assert call(arr.ctypes.data, len(arr), None, len(offs)) == pp.ERR_ARG and not out.value
    assert call(arr.ctypes.data, len(arr), offs.ctypes.data, len(offs), None) == pp.ERR_ARG
