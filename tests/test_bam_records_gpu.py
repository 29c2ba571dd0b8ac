"""pp_bam_records (pp_bam.hip) against tests/bam_model.py's decode, byte for byte -- the rooms and their zeros, the name ranges and the
pass bytes included -- with the bytes in host memory and in device memory; there the allocation is exactly n_bytes long and the last
record ends at its last byte.  The shape of the generated inputs is pinned on the CPU (tests/test_bam_model_cpu.py).  The malformed
records are refused from the decode's range checks: nothing here depends on a fault.  Needs an MI355X: `-m gpu`."""
import ctypes as C

import numpy as np
import pytest

import bam_model as bm

pytestmark = pytest.mark.gpu
REF_MAP = [0, 1, 2, 9]      # three references and the "*"


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


def decoded(pp, ctx, b, off, ref_map, mem):
    if mem == pp.MEM_HOST:
        return pp.BamRecords(ctx, b, off, ref_map, mem), None
    data, rec_off, keep = on_device(b, off)
    return pp.BamRecords(ctx, data, rec_off, ref_map, mem), keep


def check(pp, ctx, b, off, ref_map=None):
    want = bm.decode(b, off, ref_map)
    for mem in (pp.MEM_HOST, pp.MEM_DEVICE):
        rec, keep = decoded(pp, ctx, b, off, ref_map, mem)
        try:
            got = rec.host()
            bm.same(got, want)
            assert rec.zp.dtype == np.uint8 and np.array_equal(rec.zp, want["zp"]), mem
            assert (rec.n_rec, rec.seq_bytes, rec.n_cig_total) == (len(off), len(want["seq"]), len(want["cigar"]))
            raw = rec.raw()
            assert raw["read_id"] == rec.read_id_ptr and (raw["n_rec"], raw["seq_bytes"]) == (len(off), len(want["seq"]))
        finally:
            rec.close()
    return want


def refused(pp, ctx, b, off, code, bad, ref_map=None, text=None):
    try:
        bm.decode(b, off, ref_map)
    except bm.BamError as m:
        assert (m.code, m.bad_record) == (code, bad), "the model refuses the same record"
    else:
        raise AssertionError("the model takes these records")
    for mem in (pp.MEM_HOST, pp.MEM_DEVICE):
        with pytest.raises(pp.PolypolishError) as e:
            decoded(pp, ctx, b, off, ref_map, mem)
        assert (e.value.code, e.value.bad_record) == (code, bad), (mem, e.value)
        if text:
            assert text in e.value.msg


def closing_pad(n, f):
    return lambda i: f(i) if i + 1 < n else 0      # nothing behind the last record: it ends at the array's last byte


@pytest.mark.parametrize("lead", (0, 1))
def test_seams_of_the_expansion(pp, ctx, lead):
    recs = bm.seam_records()
    b, off = bm.lay_out(recs, lead, closing_pad(len(recs), lambda i: (3 * i) % 7))
    check(pp, ctx, b, off)
    back = off[::-1].copy()
    back[5] = back[6]                               # reverse order, one record twice
    want = check(pp, ctx, b, back)
    assert want["name_off"][5] == want["name_off"][6]


def test_aux_walk(pp, ctx):
    cases = bm.aux_records()
    b, off = bm.lay_out([r for _, r, _, _ in cases], 0, closing_pad(len(cases), lambda i: i % 3))
    want = check(pp, ctx, b, off)
    assert want["nm"].tolist() == [nm for _, _, nm, _ in cases]
    assert want["zp"].tolist() == [ok for _, _, _, ok in cases if ok is not None]
    assert [w for w, _, _, ok in cases if ok == 0] == ["ZP:Z:fail", "zp:Z:FAIL", "ZP:Z:fail in front of NM"]


def test_values_and_ref_maps(pp, ctx):
    recs = bm.mixed_records(300, seed=4)
    b, off = bm.lay_out(recs, 3)
    ident = check(pp, ctx, b, off)
    assert (ident["contig"] == bm.NO_CONTIG).any() and set(ident["contig"].tolist()) >= {0, 1, 2}
    perm = check(pp, ctx, b, off, ref_map=[2, 0, 1, 77])
    assert set(perm["contig"].tolist()) == {0, 1, 2, 77} and not np.array_equal(perm["contig"], ident["contig"])
    assert (ident["ref_start"] == 0).sum() > 20, "pos -1 is ref_start 0"


def test_quit_and_panic(pp, ctx):
    good = bm.record(b"g", 0, 0, 0, [(4 << 4)], "ACGT", bm.aux("NM", "C", 0))
    no_nm = bm.record(b"n", 16, 0, 0, [(4 << 4)], "ACGT", bm.aux("AS", "C", 3))
    umax = bm.record(b"u", 0, 0, 0, [(4 << 4)], "ACGT", bm.aux("NM", "I", 0xFFFFFFFF))
    for ty, v in (("c", -1), ("s", -300), ("i", -70000)):
        neg = bm.record(b"m", 4, -1, -1, [], "", bm.aux("NM", ty, v) + bm.aux("NM", "C", 3))
        b, off = bm.lay_out([good, good, neg, no_nm], 1)
        refused(pp, ctx, b, off, pp.ERR_PANIC, 2)
    b, off = bm.lay_out([good, no_nm, good, neg])
    refused(pp, ctx, b, off, pp.ERR_QUIT, 1, text="missing NM tag")
    b, off = bm.lay_out([good] * 5 + [umax])
    refused(pp, ctx, b, off, pp.ERR_QUIT, 5, text="missing NM tag")
    refused(pp, ctx, b, off[::-1].copy(), pp.ERR_QUIT, 0)


def test_every_defect_is_refused_from_the_range_checks(pp, ctx):
    good = [r for _, r, _, _ in bm.aux_records()[:6]]
    no_nm = bm.record(b"n", 0, 0, 0, [(4 << 4)], "ACGT", b"")
    for kind, rec in bm.defect_records():
        b, off = bm.lay_out(good[:3] + [rec] + good[3:], 1, lambda i: i % 4)            # mid-array
        refused(pp, ctx, b, off, pp.ERR_ARG, 3, ref_map=REF_MAP)
        b, off = bm.lay_out(good + [rec], 0, closing_pad(7, lambda i: 1))             # the last record, the array ends with it
        assert int(off[-1]) + len(rec) == len(b)
        refused(pp, ctx, b, off, pp.ERR_ARG, 6, ref_map=REF_MAP)
    # ... with an earlier record that Alignment::new refuses: the defect is reported
    b, off = bm.lay_out([good[0], no_nm, good[1], bm.defect_records()[3][1], good[2]])
    refused(pp, ctx, b, off, pp.ERR_ARG, 3, ref_map=REF_MAP)
    # offsets and records outside the array
    b, off = bm.lay_out(good)
    for o in (len(b) + 1, len(b) - 3, 1 << 63, (1 << 64) - 2):
        bad = off.copy()
        bad[4] = o
        refused(pp, ctx, b, bad, pp.ERR_ARG, 4)
    refused(pp, ctx, b[:-1], off, pp.ERR_ARG, 5)                                      # the last record one byte short
    # a refID behind the references needs a map to be one
    b, off = bm.lay_out(good + [bm.defect_records()[7][1]])
    assert check(pp, ctx, b, off)["contig"][-1] == 3


def test_a_refused_call_returns_no_object(pp, ctx):
    b, off = bm.lay_out([bm.defect_records()[0][1]])
    data = np.frombuffer(b, np.uint8)
    out, bad = C.c_void_p(12345), C.c_uint64(0)
    rc = pp.lib().pp_bam_records(ctx._h, data.ctypes.data, len(data), off.ctypes.data, 1, pp.MEM_HOST, None, 0, C.byref(out), C.byref(bad))
    assert rc == pp.ERR_ARG and out.value is None and bad.value == 0


def test_5000_mixed_records(pp, ctx):
    recs = bm.mixed_records()
    b, off = bm.lay_out(recs, 0, closing_pad(len(recs), lambda i: i % 2))
    want = check(pp, ctx, b, off, ref_map=[1, 2, 0, 50])
    assert len(off) > 4 * bm.BAM_BLOCK and len(want["seq"]) > (1 << 19)


def test_edge_contracts(pp, ctx):
    recs = bm.seam_records()[40:60]
    b, off = bm.lay_out(recs)
    empty = check(pp, ctx, b, off[:0])
    assert len(empty["flag"]) == 0 and len(empty["seq"]) == 0
    check(pp, ctx, b"", off[:0])
    walked = pp.BamRecords(ctx, b)                        # rec_off = None on the host: the library walks the chain
    try:
        bm.same(walked.host(), bm.decode(b, off))
    finally:
        walked.close()
    with pytest.raises(pp.PolypolishError) as e:          # a chain that breaks: the records in front of the break
        pp.BamRecords(ctx, b[:-1])
    assert (e.value.code, e.value.bad_record) == (pp.ERR_ARG, len(off) - 1)
    data, _, keep = on_device(b, off)
    with pytest.raises(pp.PolypolishError) as e:
        pp.BamRecords(ctx, data, None, None, pp.MEM_DEVICE)
    assert e.value.code == pp.ERR_ARG and "rec_off" in e.value.msg
    with pytest.raises(pp.PolypolishError) as e:
        pp.BamRecords(ctx, b, off, None, pp.MEM_PEER)
    assert e.value.code == pp.ERR_ARG


def test_kernel_ms_needs_profiling(pp):
    c = pp.Context(0)
    try:
        b, off = bm.lay_out(bm.seam_records())
        rec = pp.BamRecords(c, b, off)
        with pytest.raises(pp.PolypolishError) as e:
            rec.kernel_ms()
        assert e.value.code == pp.ERR_ARG
        rec.close()
        c.set_profiling(True)
        rec = pp.BamRecords(c, b, off)
        assert rec.kernel_ms() > 0
        rec.close()
    finally:
        c.close()


def test_a_second_decode_on_the_context_keeps_nothing(pp, ctx):
    small, large = bm.seam_records()[:30], bm.mixed_records(2500, seed=8)
    bs, os_ = bm.lay_out(small, 1)
    want = check(pp, ctx, bs, os_)
    bad, ob = bm.lay_out(small[:10] + [bm.defect_records()[8][1]] + small[10:])
    refused(pp, ctx, bad, ob, pp.ERR_ARG, 10)
    assert np.array_equal(check(pp, ctx, bs, os_)["seq"], want["seq"])
    bl, ol = bm.lay_out(large)
    check(pp, ctx, bl, ol)
    assert np.array_equal(check(pp, ctx, bs, os_)["seq"], want["seq"])
