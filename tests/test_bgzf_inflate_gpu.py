"""pp_bgzf_inflate (pp_bgzf.hip) against tests/bgzf_model.py and zlib, byte for byte, with the compressed bytes in host memory and in
device memory; there the allocation is exactly n_bytes long.  What the inputs exercise is pinned on the CPU
(tests/test_bgzf_model_cpu.py).  Every defect stream is built from valid ones by the model's writer and is refused by the kernel's
own checks: nothing here depends on a fault.  Needs an MI355X: `-m gpu`."""
import numpy as np
import pytest

import bgzf_model as zm


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
def table():
    return zm.table_inputs()


@pytest.fixture(scope="module")
def seams():
    return zm.seam_streams()


def on_device(b, off):
    """(data, blk_off, keep) for mem = MEM_DEVICE: the bytes in an allocation of exactly their length"""
    import torch
    dev = torch.device("cuda:0")
    tb = torch.from_numpy(np.frombuffer(bytes(b), np.uint8).copy()).to(dev) if len(b) else torch.zeros(1, dtype=torch.uint8, device=dev)
    to = torch.from_numpy(np.ascontiguousarray(off, np.uint64).view(np.int64).copy()).to(dev) if len(off) else torch.zeros(1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    return (tb.data_ptr(), len(b)), (to.data_ptr(), len(off)), (tb, to)


def inflate_both(pp, ctx, blob, off):
    """the blocks at `off` of `blob` through both forms of `mem` -> the inflated bytes (the two agree)"""
    z = pp.Bgzf(ctx, blob, off)
    host = z.host().tobytes()
    assert len(host) == z.n_bytes
    z.close()
    data, blk, keep = on_device(blob, off)
    z = pp.Bgzf(ctx, data, blk, mem=pp.MEM_DEVICE)
    dev = z.host().tobytes()
    z.close()
    del keep
    assert dev == host
    return host


def lay(blocks):
    off = np.cumsum([0] + [len(b) for b in blocks])[:-1].astype(np.uint64)
    return b"".join(blocks), off


@pytest.mark.gpu
def test_every_input_of_the_table_alone_and_together(pp, ctx, table):
    blocks, datas = [], []
    for name, (data, raw) in table.items():
        blk = zm.wrap(raw, data)
        assert inflate_both(pp, ctx, blk, [0]) == data, name
        blocks.append(blk)
        datas.append(data)
    blocks.insert(3, zm.EOF_BLOCK)
    datas.insert(3, b"")
    blob, off = lay(blocks + [zm.EOF_BLOCK])
    assert inflate_both(pp, ctx, blob, off) == b"".join(datas)
    z = pp.Bgzf(ctx, blob)                         # blk_off == NULL with host bytes: the library walks
    assert z.host().tobytes() == b"".join(datas) and z.host(5, 70000).tobytes() == b"".join(datas)[5:70000]
    z.close()


@pytest.mark.gpu
def test_hand_built_seams(pp, ctx, seams):
    blocks, datas = [], []
    for name, (data, raw) in seams.items():
        blk = zm.wrap(raw, data, extra_front=b"XY\x03\x00abc" if name == "five_blocks_mixed" else b"")      # (BC behind another subfield)
        assert inflate_both(pp, ctx, blk, [0]) == data, name      # (alone: in the device form the block's footer ends the allocation)
        blocks.append(blk)
        datas.append(data)
    # all together, the block whose last code ends on the payload's last bit as the last bytes of the allocation
    last = list(seams).index("last_code_ends_on_the_last_bit")
    order = [i for i in range(len(blocks)) if i != last] + [last]
    blob, off = lay([blocks[i] for i in order])
    assert inflate_both(pp, ctx, blob, off) == b"".join(datas[i] for i in order)
    assert len(datas[list(seams).index("isize_65536")]) == 65536


@pytest.mark.gpu
def test_subset_order_and_repeats(pp, ctx, table):
    names = ["dynamic_bam", "one_byte", "fixed", "zeros", "two_stored"]
    blob, off = lay([zm.wrap(table[n][1], table[n][0]) for n in names] + [zm.EOF_BLOCK])
    pick = [4, 5, 1, 1, 0, 3, 1, 2, 0]
    want = b"".join(table[names[i]][0] if i < 5 else b"" for i in pick)
    assert inflate_both(pp, ctx, blob, off[pick]) == want
    assert inflate_both(pp, ctx, blob, off[::-1]) == b"".join(table[n][0] for n in names[::-1])


@pytest.mark.gpu
def test_two_thousand_blocks_against_zlib(pp, ctx):
    blob, datas = zm.many_blocks(2000)
    off, out, end = pp.bgzf_walk(blob)
    assert len(off) == 2000 and end == len(blob)
    got = inflate_both(pp, ctx, blob, off)
    assert len(got) == int(out[-1])
    for b in range(2000):
        assert got[int(out[b]):int(out[b + 1])] == datas[b], b


@pytest.mark.gpu
def test_defects_are_refused_with_the_first_bad_block(pp, ctx, table):
    good_data, good_raw = table["dynamic_bam"]
    good = zm.wrap(good_raw, good_data)
    defects = zm.defect_blocks()
    second = defects["distance_beyond_the_output"][0]
    for name, (bad, kind, _) in defects.items():
        for tail in (good, second):
            blob, off = lay([good, bad, tail])
            for device in (False, True):
                data, blk, keep = on_device(blob, off) if device else (blob, off, None)
                with pytest.raises(pp.PolypolishError) as e:
                    pp.Bgzf(ctx, data, blk, mem=pp.MEM_DEVICE if device else pp.MEM_HOST)
                assert (e.value.code, e.value.bad_block) == (pp.ERR_ARG, 1), (name, kind, e.value.msg)
            assert inflate_both(pp, ctx, good, [0]) == good_data, "a valid call on the same context after the refusal"
    # a stream defect in block 1 in front of a header defect in block 2, and the other way round
    for blocks, want in (([good, second, defects["bad_magic"][0]], 1), ([good, defects["bad_magic"][0], second], 1)):
        blob, off = lay(blocks)
        with pytest.raises(pp.PolypolishError) as e:
            pp.Bgzf(ctx, blob, off)
        assert (e.value.code, e.value.bad_block) == (pp.ERR_ARG, want)
    # a blk_off outside the array, and one whose header runs past its end
    blob, off = lay([good, good, good])
    for bad_off in (len(blob), len(blob) + 1, 1 << 63, len(blob) - 11, int(off[2]) + 1):
        o = off.copy()
        o[1] = bad_off
        for device in (False, True):
            data, blk, keep = on_device(blob, o) if device else (blob, o, None)
            with pytest.raises(pp.PolypolishError) as e:
                pp.Bgzf(ctx, data, blk, mem=pp.MEM_DEVICE if device else pp.MEM_HOST)
            assert (e.value.code, e.value.bad_block) == (pp.ERR_ARG, 1), bad_off
    # blk_off == NULL: the library's own walk refuses the chain
    with pytest.raises(pp.PolypolishError) as e:
        pp.Bgzf(ctx, good + defects["bsize_past_the_end"][0])
    assert (e.value.code, e.value.bad_block) == (pp.ERR_ARG, 1)
    assert inflate_both(pp, ctx, good, [0]) == good_data


@pytest.mark.gpu
def test_an_incomplete_code_that_zlib_takes_is_taken(pp, ctx):
    import zlib
    w = zm.Writer()
    cl = w.dynamic_header(257, 1, {0: 2, 1: 2, 18: 1})
    w.code(cl[18]).bits(127, 7).code(cl[18]).bits(118 - 11, 7).code(cl[1]).code(cl[1])
    raw = w.bits(0, 1).bytes()
    assert zlib.decompress(raw, -15) == b""
    assert inflate_both(pp, ctx, zm.wrap(raw, b""), [0]) == b""


@pytest.mark.gpu
def test_edge_contracts(pp, ctx, table):
    import ctypes as C
    L = pp.lib()
    z = pp.Bgzf(ctx, b"", [])                                      # n_blk == 0
    assert z.n_bytes == 0 and z.host().size == 0 and z.bam_walk(0)[1:] == (0, 0)
    z.close()
    z = pp.Bgzf(ctx, zm.EOF_BLOCK)                                 # only the EOF block
    assert z.n_bytes == 0 and z.host().size == 0
    with pytest.raises(pp.PolypolishError) as e:
        z.kernel_ms()
    assert e.value.code == pp.ERR_ARG and "profiling" in e.value.msg
    z.close()
    b = np.frombuffer(zm.EOF_BLOCK, np.uint8)
    off = np.zeros(1, np.uint64)
    p, bad = C.c_void_p(), C.c_uint64(0)
    assert L.pp_bgzf_inflate(None, b.ctypes.data, len(b), off.ctypes.data, 1, pp.MEM_HOST, C.byref(p), C.byref(bad)) == pp.ERR_ARG
    assert L.pp_bgzf_inflate(ctx._h, b.ctypes.data, len(b), off.ctypes.data, 1, pp.MEM_HOST, None, C.byref(bad)) == pp.ERR_ARG
    assert L.pp_bgzf_inflate(ctx._h, None, len(b), off.ctypes.data, 1, pp.MEM_HOST, C.byref(p), C.byref(bad)) == pp.ERR_ARG and not p.value
    assert L.pp_bgzf_inflate(ctx._h, b.ctypes.data, len(b), off.ctypes.data, 1, pp.MEM_PEER, C.byref(p), C.byref(bad)) == pp.ERR_ARG and not p.value
    assert L.pp_bgzf_inflate(ctx._h, b.ctypes.data, len(b), None, 0, pp.MEM_DEVICE, C.byref(p), C.byref(bad)) == pp.ERR_ARG and not p.value
    assert L.pp_bgzf_inflate(ctx._h, b.ctypes.data, len(b), off.ctypes.data, 0xFFFFFFFF, pp.MEM_HOST, C.byref(p), C.byref(bad)) == pp.ERR_LIMIT
    assert L.pp_bgzf_inflate(ctx._h, b.ctypes.data, len(b), off.ctypes.data, 1, pp.MEM_HOST, C.byref(p), None) == pp.OK and p.value
    L.pp_bgzf_free(p)
    L.pp_bgzf_free(None)
    # a second inflate on the same context keeps nothing of the first; with profiling the stages are timed
    ctx.set_profiling(1)
    try:
        whole = zm.bam_like(20000, 31, whole=True)
        a = pp.Bgzf(ctx, zm.block(whole))
        c = pp.Bgzf(ctx, zm.wrap(table["one_byte"][1], table["one_byte"][0]))
        assert c.n_bytes == 1 and c.host().tobytes() == b"x" and a.host().tobytes() == whole
        stages = a.stage_ms()
        assert stages["inflate"] > 0 and stages["crc"] > 0 and stages["staging"] == 0 and a.kernel_ms() == pytest.approx(sum(stages.values()))
        with pytest.raises(pp.PolypolishError) as e:        # the chain from offset 1 breaks
            a.bam_walk(1)
        assert e.value.code == pp.ERR_ARG
        ptr, n_rec, end = a.bam_walk(0)
        assert ptr and n_rec > 50 and end == len(whole) and a.stage_ms()["staging"] > 0
        a.close()
        c.close()
    finally:
        ctx.set_profiling(0)
