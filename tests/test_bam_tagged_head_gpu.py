"""pp_bam_tagged_head (pp_bam_out.hip) against tests/bam_sort_model.py's tagged_head framed by tests/bam_tag_model.py, BYTE FOR BYTE,
with the bytes in host memory and in device memory: headers of 0, 1, 15, 16, 17 bytes and of more than one block (the header is a
source of the framing kernel like a record: its last piece, its seam with the first record and its pieces in a second block are
what can go wrong), shorter and longer than the bytes' own; then the whole sorted file -- pp_bam_sort's offsets, header and carried
verdicts -- against the model's, and compressed.  pp_bam_tagged's own bytes are held by tests/test_bam_tagged_gpu.py.  Needs an
MI355X: `-m gpu`."""
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


def check(pp, ctx, b, at, off, passed, head):
    u = sm.tagged_head(b, at, off, passed, head)
    want = tm.frame(u)
    for mem in (pp.MEM_HOST, pp.MEM_DEVICE):
        if mem == pp.MEM_HOST:
            t, keep = pp.BamTagged(ctx, b, at, off, passed, mem, head=head), None
        else:
            data, rec_off, keep = on_device(b, off)
            t = pp.BamTagged(ctx, data, at, rec_off, passed, mem, head=head)
        try:
            got = t.host().tobytes()
            assert t.n_bytes == len(want), mem
            if got != want:
                first = next(i for i, (x, y) in enumerate(zip(got, want)) if x != y)
                raise AssertionError(f"mem {mem}: byte {first} (block {first // tm.BLOCK}, byte {first % tm.BLOCK} of it) is {got[first]:#x}, not {want[first]:#x}")
            n_fail = 0 if passed is None else int((np.asarray(passed) == 0).sum())
            assert t.counts == ((0 if passed is None else len(passed)) - n_fail, n_fail, (len(u) + P - 1) // P), mem
        finally:
            t.close()
            del keep
    return u


def noise(n, seed=1):
    return np.random.default_rng(seed).integers(1, 256, n, dtype=np.uint8).tobytes()


@pytest.mark.parametrize("n_head", (0, 1, 15, 16, 17, 31, 32, 33, len(tm.HEADER) - 1, len(tm.HEADER) + 1, P - 1, P, P + 1, 2 * P + 5))
def test_headers_of_every_length_in_front_of_records(pp, ctx, n_head):
    recs = [tm.rec(100 + (7 * i) % 13, qname=b"a%d" % i) for i in range(40)] + [tm.rec(70000, qname=b"long")]
    b, at, off, passed = tm.stream(recs, [i & 1 for i in range(len(recs))])
    head = noise(n_head, n_head)
    u = check(pp, ctx, b, at, off, passed, head)
    assert u[:n_head] == head and len(u) == n_head + len(tm.tagged(b, at, off, passed)) - at
    check(pp, ctx, b, at, off[:0], None, head)                   # the header alone; no bytes: the EOF block alone


def test_a_header_of_its_own_and_records_at_of_no_meaning(pp, ctx):
    recs = [tm.rec(64 + i, qname=b"b%d" % i) for i in range(30)]
    b, at, off, passed = tm.stream(recs, [1] * 30)
    u = check(pp, ctx, b, at, off, passed, b[:at])
    assert u == tm.tagged(b, at, off, passed), "the bytes' own header: pp_bam_tagged's stream"
    for records_at in (0, 5, len(b)):
        assert check(pp, ctx, b, records_at, off, passed, b[:at]) == u


def test_refusals_are_pp_bam_tagged_s(pp, ctx):
    recs = [tm.rec(64 + i, qname=b"b%d" % i) for i in range(30)]
    b, at, off, passed = tm.stream(recs, [1] * 30)
    for args, code, bad in (((b, at, np.concatenate([off[:3], [len(b) - 3]]).astype(np.uint64), passed), pp.ERR_ARG, 3), ((b, at, off, passed[:-1]), pp.ERR_ARG, None),
                            ((b, len(b) + 1, off, passed), pp.ERR_ARG, None)):
        for mem in (pp.MEM_HOST, pp.MEM_DEVICE):
            with pytest.raises(pp.PolypolishError) as e:
                if mem == pp.MEM_HOST:
                    pp.BamTagged(ctx, *args, mem, head=b"x" * 40)
                else:
                    data, rec_off, keep = on_device(args[0], args[2])
                    pp.BamTagged(ctx, data, args[1], rec_off, args[3], mem, head=b"x" * 40)
            assert (e.value.code, e.value.bad_record) == (code, bad) and "pp_bam_tagged_head" in str(e.value), (mem, e.value)
    L = pp.lib()
    arr, offs = np.frombuffer(b, np.uint8), np.ascontiguousarray(off, np.uint64)
    out, bad = C.c_void_p(), C.c_uint64(0)
    assert L.pp_bam_tagged_head(ctx._h, arr.ctypes.data, len(arr), at, offs.ctypes.data, len(offs), pp.MEM_HOST, passed.ctypes.data, len(passed), None, 5,
                                C.byref(out), C.byref(bad)) == pp.ERR_ARG and not out.value
    assert L.pp_bam_tagged_head(ctx._h, arr.ctypes.data, len(arr), at, offs.ctypes.data, len(offs), pp.MEM_HOST, passed.ctypes.data, len(passed), arr.ctypes.data,
                                1 << 40, C.byref(out), C.byref(bad)) == pp.ERR_LIMIT and not out.value


@pytest.mark.parametrize("n", (0, 1, 700, 9000))
def test_the_sorted_file_through_sort_pass_and_head(pp, ctx, n):
    recs = sm.random_records(n, seed=n, unplaced=0.2)
    b, at, off = sm.stream(recs)
    n_al = sum(1 for r in recs if not r[18] & 4)
    passed = (np.random.default_rng(n).random(n_al) < 0.7).astype(np.uint8)
    want = sm.sorted_stream(b, at, off, passed)
    data, rec_off, keep = on_device(b, off)
    s = pp.BamSorted(ctx, data, at, rec_off, pp.MEM_DEVICE)
    t = pp.BamTagged(ctx, data, at, (s.rec_off_ptr, s.n_rec), s.carry_pass(passed), pp.MEM_DEVICE, head=s.head)
    z = t.deflate()
    try:
        assert t.host().tobytes() == tm.frame(want)
        assert tm.unframe(z.host().tobytes()) == want, "compressed: the same stream"
        got_off, end, ok = bm.walk(want, len(s.head))
        assert ok and len(got_off) == n
        k = [sm.key_of(*sm.fields(want, o)) for o in got_off]
        assert k == sorted(k), "the file's records stand in key order"
        if n:
            plain = tm.tagged(b, at, off, passed)
            cut = lambda u, a: sorted(u[o:o + 4 + bm._le32(u, o)] for o in bm.walk(u, a)[0])      # noqa: E731
            assert cut(want, len(s.head)) == cut(plain, at), "the same records, tags included, as the file in input order"
    finally:
        z.close()
        t.close()
        s.close()
        del keep
