"""pp_bam_walk_device (pp_bam_walk.hip) against pp_bam_walk on the same bytes: the number of records, the end and every offset, with
the bytes in host memory and in device memory; there the allocation is exactly n_bytes long.  The inputs are the hand-built ones of
tests/bam_walk_model.py, laid on the seams of the library's own geometry (pp_bam_walk_geometry_): chunk, band, zone and group seams,
long records, hostile filler, every kind of break in every place.  The path counts the library reports (pp_bam_offs_stats_) are held
against the model's, so a case proves which path it ran; tests/test_bam_walk_model_cpu.py pins the model and the paths on the CPU.
Every hostile input is one the contract answers with a return code: nothing here depends on a fault.  Needs an MI355X: `-m gpu`."""
import ctypes as C

import numpy as np
import pytest

import bam_model as bm
import bam_walk_model as wm

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
def geo(pp):
    return pp.bam_walk_geometry()


@pytest.fixture(scope="module")
def hand_built(geo):
    return wm.cases(*geo)


@pytest.fixture(scope="module")
def planted(geo):
    return wm.breaks(*geo)


def on_device(b):
    """(data, keep) for mem = MEM_DEVICE: the bytes in an allocation of exactly their length"""
    import torch
    dev = torch.device("cuda:0")
    tb = torch.from_numpy(np.frombuffer(bytes(b), np.uint8).copy()).to(dev) if len(b) else torch.zeros(1, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    return (tb.data_ptr(), len(b)), tb


def device_walk(pp, ctx, b, start, mem):
    if mem == pp.MEM_HOST:
        return pp.bam_walk_device(ctx, b, start, mem)
    data, keep = on_device(b)
    try:
        return pp.bam_walk_device(ctx, data, start, mem)      # (the bytes are borrowed for the call only)
    finally:
        del keep


def check(pp, ctx, geo, b, start=0, path=None):
    """the device walk over b from start, in both memory forms, against the host walk: -> the stats of a chain that holds"""
    L = pp.lib()
    try:
        want_off, want_end = pp.bam_walk(b, start)
        want_err = None
    except pp.PolypolishError as e:
        want_err = (e.code, e.n_rec, e.end, e.msg)
    model = wm.walk(b, start, *geo)
    stats = None
    for mem in (pp.MEM_HOST, pp.MEM_DEVICE):
        if want_err is None:
            o = device_walk(pp, ctx, b, start, mem)
            try:
                got = o.host()
                assert (o.n_rec, o.end) == (len(want_off), want_end), (mem, o.n_rec, o.end, len(want_off), want_end)
                assert got.dtype == np.uint64 and np.array_equal(got, want_off), mem
                stats = o.stats()
                assert [stats[k] for k in ("chain", "zone", "slow", "pass")] == model[4], (mem, stats, model[4])
                assert o.ptr
            finally:
                o.close()
        else:
            with pytest.raises(pp.PolypolishError) as e:
                device_walk(pp, ctx, b, start, mem)
            assert (e.value.code, e.value.n_rec, e.value.end) == (pp.ERR_ARG,) + want_err[1:3], (mem, e.value, want_err)
            assert L.pp_bam_last_error().decode() == want_err[3] and want_err[3].startswith("pp_bam_walk: ")
            assert e.value.msg == "pp_bam_walk_device: " + want_err[3]
    if path is not None:
        assert path(model[4]), model[4]
    return stats


def test_hand_built_seams(pp, ctx, geo, hand_built):
    assert len(hand_built) >= 30
    for name, b, start, path in hand_built:
        try:
            assert check(pp, ctx, geo, b, start, path) is not None
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}") from e


def test_breaks(pp, ctx, geo, planted):
    assert len(planted) == 18
    for name, b, start, kind, path, at in planted:
        try:
            assert check(pp, ctx, geo, b, start, path) is None
            n_rec, end, got_kind = wm.walk(b, start, *geo)[:3]
            assert (got_kind, end) == (kind, at)
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}") from e
    one = wm.rec(36)
    for n in (1, 3, 4, 35):                                     # the bytes end inside the first record
        assert check(pp, ctx, geo, one[:n]) is None
    for b, start in ((b"", 1), (one, 37), (one + one, 2 ** 40)):   # the start lies behind the bytes
        assert check(pp, ctx, geo, b, start) is None


def test_ordinary_records_stay_on_the_fast_path(pp, ctx, geo):
    C_, Z, G = geo
    body = bm.lay_out(bm.mixed_records(n=3000))[0]
    b = body * (2 * G * C_ // len(body) + 1)
    assert len(b) < 4 * G * C_
    st = check(pp, ctx, geo, b)
    assert st["chain"] > 2 * G and st["slow"] == 0 and st["zone"] == st["chain"] - 1 - st["pass"], st
    hdr = bm.header_bytes([("chr1", 1000), ("chr2", 5000)], "@HD\tVN:1.6\n")     # ... behind a BAM header
    st = check(pp, ctx, geo, hdr + body, len(hdr))
    assert st["slow"] == 0


def test_contract(pp, ctx, geo):
    L = pp.lib()
    b = np.frombuffer(bm.lay_out(bm.mixed_records(n=300))[0], np.uint8)
    p, n, end = C.c_void_p(), C.c_uint64(7), C.c_uint64(7)
    args = (b.ctypes.data, len(b), 0, pp.MEM_HOST)
    assert L.pp_bam_walk_device(None, *args, C.byref(p), C.byref(n), C.byref(end)) == pp.ERR_ARG
    assert L.pp_bam_walk_device(ctx._h, *args, None, C.byref(n), C.byref(end)) == pp.ERR_ARG
    assert L.pp_bam_walk_device(ctx._h, *args, C.byref(p), None, C.byref(end)) == pp.ERR_ARG and not p.value
    assert L.pp_bam_walk_device(ctx._h, *args, C.byref(p), C.byref(n), None) == pp.ERR_ARG and not p.value
    assert L.pp_bam_walk_device(ctx._h, None, len(b), 0, pp.MEM_HOST, C.byref(p), C.byref(n), C.byref(end)) == pp.ERR_ARG and not p.value
    assert L.pp_bam_walk_device(ctx._h, b.ctypes.data, len(b), 0, pp.MEM_PEER, C.byref(p), C.byref(n), C.byref(end)) == pp.ERR_ARG and not p.value
    assert L.pp_bam_walk_device(ctx._h, None, 1 << 40, 0, pp.MEM_DEVICE, C.byref(p), C.byref(n), C.byref(end)) == pp.ERR_ARG and not p.value
    assert L.pp_bam_walk_device(ctx._h, b.ctypes.data, 1 << 40, 1 << 40, pp.MEM_PEER, C.byref(p), C.byref(n), C.byref(end)) == pp.ERR_ARG
    assert L.pp_bam_walk_device(ctx._h, None, 0, 0, pp.MEM_HOST, C.byref(p), C.byref(n), C.byref(end)) == pp.OK and p.value     # no bytes: no records
    assert (n.value, end.value, L.pp_bam_offs_count(p)) == (0, 0, 0) and L.pp_bam_offs_dev(p)
    L.pp_bam_offs_free(p)
    L.pp_bam_offs_free(None)
    ms = C.c_float()
    assert L.pp_bam_offs_kernel_ms(None, C.byref(ms)) == pp.ERR_ARG and L.pp_bam_offs_count(None) == 0 and not L.pp_bam_offs_dev(None)
    # walk after walk on one context, freed in any order; without profiling no time, with it one above zero
    want, want_end = pp.bam_walk(b)
    other = wm.cases(*geo)[0][1]
    a = pp.bam_walk_device(ctx, b)
    c = pp.bam_walk_device(ctx, other)
    d = pp.bam_walk_device(ctx, b, int(want[5]))
    assert np.array_equal(a.host(), want) and np.array_equal(c.host(), pp.bam_walk(other)[0]) and np.array_equal(d.host(), want[5:])
    with pytest.raises(pp.PolypolishError) as e:
        a.kernel_ms()
    assert e.value.code == pp.ERR_ARG and "profiling" in e.value.msg
    c.close()
    assert np.array_equal(a.host(), want) and (a.end, d.end) == (want_end, want_end)
    a.close()
    d.close()
    ctx.set_profiling(1)
    try:
        t = pp.bam_walk_device(ctx, other)
        stages = t.stage_ms()
        assert t.kernel_ms() > 0 and t.kernel_ms() == pytest.approx(sum(stages.values())) and stages["tables"] > 0
        t.close()
    finally:
        ctx.set_profiling(0)


def test_the_next_link_and_bgzf(pp, ctx, geo):
    """BamRecords from device bytes and the device walk's offsets == the decode from the host walk's offsets; Bgzf.bam_walk == the
    device walk over the inflated bytes"""
    import zlib
    import bgzf_model as zm
    recs = bm.mixed_records(n=400)
    hdr = bm.header_bytes([("a", 200000), ("b", 200000), ("c", 200000)])
    whole = hdr + bm.lay_out(recs)[0]
    ref_map = [0, 1, 2, 9]
    host_off, _ = pp.bam_walk(whole, len(hdr))
    want = pp.BamRecords(ctx, whole, host_off, ref_map)
    data, keep = on_device(whole)
    offs = pp.bam_walk_device(ctx, data, len(hdr), pp.MEM_DEVICE)
    got = pp.BamRecords(ctx, data, (offs.ptr, offs.n_rec), ref_map, mem=pp.MEM_DEVICE)
    try:
        assert offs.n_rec == len(host_off) == len(recs)
        bm.same(got.host(), want.host())
        assert np.array_equal(got.zp, want.zp)
    finally:
        got.close()
        want.close()
    blocks = b"".join(zm.block(whole[i:i + 30000]) for i in range(0, len(whole), 30000)) + zm.EOF_BLOCK
    z = pp.Bgzf(ctx, blocks)
    try:
        assert z.n_bytes == len(whole) and zlib.crc32(z.host().tobytes()) == zlib.crc32(whole)
        ptr, n_rec, end = z.bam_walk(len(hdr))
        mine = pp.bam_walk_device(ctx, (z.bytes_ptr, z.n_bytes), len(hdr), pp.MEM_DEVICE)
        down = np.zeros(n_rec, np.uint64)
        ctx._chk(pp.lib().pp_ctx_download(ctx._h, down.ctypes.data, ptr, down.nbytes))
        assert (n_rec, end) == (mine.n_rec, mine.end) == (offs.n_rec, len(whole))
        assert np.array_equal(down, mine.host()) and np.array_equal(down, host_off)
        mine.close()
        with pytest.raises(pp.PolypolishError) as e:        # a chain that breaks: pp_bam_walk's words behind the call's name
            z.bam_walk(len(hdr) + 1)
        with pytest.raises(pp.PolypolishError) as h:
            pp.bam_walk(whole, len(hdr) + 1)
        assert (e.value.code, e.value.n_rec, e.value.end) == (pp.ERR_ARG, h.value.n_rec, h.value.end)
        assert e.value.msg == "pp_bgzf_bam_walk: " + h.value.msg
    finally:
        z.close()
        offs.close()
        del keep
