"""pp_bgzf_deflate / pp_bam_out_deflate (pp_bgzf_deflate.hip) against tests/bgzf_deflate_model.py BYTE FOR BYTE -- so every token, every
code length, every header bit, the choice of the form, every CRC32 and every offset is checked -- with the bytes in host memory and in
device memory; there the allocation is exactly n_bytes long.  The shapes are the smallest at which each part of the kernel can go wrong:
the lengths around the 4-byte group, the strip and the piece; the seams of the strip rule; the contents that reach each form, each header
and the repair; many pieces in one call.  The model is pinned on the CPU (tests/test_bgzf_deflate_model_cpu.py).  Needs an MI355X: `-m gpu`."""
import ctypes as C
import gzip
import random

import numpy as np
import pytest

import bam_tag_model as tm
import bgzf_deflate_model as D
import bgzf_model as M

pytestmark = pytest.mark.gpu
S, P = D.S, D.PIECE


def _filler(n, seed):
    """32 letters in which (checked by the tests that use it) no 4-byte group occurs twice: the dynamic form wins, so the tokens show"""
    r = random.Random(seed)
    return bytes(r.randrange(64, 96) for _ in range(n))


def _same_hash_pair():
    seen = {}
    for w in range(0x41414141, 0x41414141 + 100000):
        h = ((w * 2654435761) & 0xFFFFFFFF) >> (32 - D.HB)
        if h in seen:
            return seen[h].to_bytes(4, "little"), w.to_bytes(4, "little")
        seen[h] = w
    raise AssertionError("no pair")


def _with(base, *puts):
    d = bytearray(base)
    for at, b in puts:
        d[at:at + len(b)] = b
    return bytes(d)


X = b"\xf1\xf2\xf3\xf4\xf5\xf6\xf7\xf8"
G1, G2 = _same_hash_pair()
SIZES = (0, 1, 3, 4, 5, S - 1, S, S + 1, 2 * S + 3, P - 1, P, P + 1)
SEAMS = {
    "source_in_the_same_strip": _with(_filler(S, 1), (10, X), (100, X)),
    "source_in_the_strip_in_front": _with(_filler(2 * S, 4), (10, X), (300, X)),
    "match_ends_at_n": _with(_filler(2 * S, 4), (10, X), (2 * S - 8, X)),
    "run_of_259_groups": _with(_filler(3 * S, 4), (S - 4, b"z" * 266)),
    "one_hash_two_groups": _with(_filler(2 * S, 5), (10, G1), (300, G2)),
}
CONTENT = {
    "zeros": bytes(P), "one_value": b"\xa7" * 5000, "all_values": D.all_values_equally(), "noise": M.noise(60000), "text_40": D.TEXT_40,
    "acgt": M.acgt(), "bam_like": M.bam_like(), "fibonacci": D.fibonacci_counts(), "cl_repair": M.bam_like(), "skewed": D.skewed(),
    "zeros_514": bytes(514), "far_32768": D.far_repeat(32768), "far_32769": D.far_repeat(32769),
}


def _many():
    """40 pieces of mixed content"""
    r = random.Random(40)
    parts = [M.bam_like(P, 31), M.acgt(P, 32), bytes(P), M.noise(P, 33)]
    out = bytearray()
    for k in range(39):
        src = parts[k % 4] if k % 5 else bytes(r.choice(b"ACGT\x00\x11\x22") for _ in range(P))
        out += src[:P]
    out += D.TEXT_40
    for at in (P - 2, 7 * P - 1, 20 * P):      # groups across the cut between two pieces: nothing survives it
        out[at:at + 8] = X
    return bytes(out)


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
def want():
    """the model's files, computed once: name -> (data, (file, blk_off, counts))"""
    inputs = {f"size_{n}": M.bam_like(n, 2) for n in SIZES}
    inputs.update(SEAMS)
    inputs.update(CONTENT)
    inputs["twice"] = M.bam_like(5000, 9) * 2 + bytes(P - 10000) + M.bam_like(5000, 9) * 2 + bytes(P - 10000)
    inputs["many"] = _many()
    return {k: (d, D.deflate_file(d)) for k, d in inputs.items()}


def on_device(b):
    import torch
    t = torch.from_numpy(np.frombuffer(bytes(b), np.uint8).copy()).to("cuda:0") if len(b) else torch.zeros(1, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    return (t.data_ptr(), len(b)), t


def check(pp, ctx, data, model):
    """both memory forms against the model's file, offsets and counts"""
    file, off, counts = model
    for mem in (pp.MEM_HOST, pp.MEM_DEVICE):
        arg, keep = (data, None) if mem == pp.MEM_HOST else on_device(data)
        z = pp.BgzfDeflated(ctx, arg, mem)
        try:
            got = z.host().tobytes()
            if got != file:
                first = next((i for i, (x, y) in enumerate(zip(got, file)) if x != y), min(len(got), len(file)))
                raise AssertionError(f"mem {mem}: {len(got)} bytes for {len(file)}; byte {first} is {got[first:first + 1].hex()}, not {file[first:first + 1].hex()} "
                                     f"(counts {z.counts}, the model's {counts})")
            assert z.n_bytes == len(file) and z.n_blocks == len(off) - 1 and z.blk_off().tolist() == off and list(z.counts) == counts, mem
        finally:
            z.close()


@pytest.mark.parametrize("n", SIZES)
def test_sizes_around_the_group_the_strip_and_the_piece(pp, ctx, want, n):
    data, model = want[f"size_{n}"]
    assert len(data) == n and len(model[1]) == (n + P - 1) // P + 1
    check(pp, ctx, data, model)


@pytest.mark.parametrize("name", list(SEAMS))
def test_strip_seams(pp, ctx, want, name):
    data, model = want[name]
    toks = D.tokens(data)
    matches = [t for t in toks if isinstance(t, tuple)]
    if name == "source_in_the_same_strip":
        assert not matches
    elif name == "source_in_the_strip_in_front":
        assert matches == [(8, 290)]
    elif name == "match_ends_at_n":
        assert matches == [(8, 2 * S - 18)] and isinstance(toks[-1], tuple)
    elif name == "run_of_259_groups":
        assert matches == [(258, 1), (4, 3)], "258 bytes, then a new token for the four that are left"
    else:
        assert D._hash(G1, 0) == D._hash(G2, 0) and G1 != G2 and not matches
    assert model[2][D.STORED] == 0, "the tokens are in the stream"
    check(pp, ctx, data, model)


@pytest.mark.parametrize("name", list(CONTENT))
def test_contents(pp, ctx, want, name):
    data, model = want[name]
    form = {"noise": D.STORED, "text_40": D.FIXED, "bam_like": D.DYNAMIC, "fibonacci": D.DYNAMIC, "all_values": D.STORED}.get(name)
    assert form is None or model[2][form] == 1
    check(pp, ctx, data, model)


def test_two_identical_pieces_give_identical_streams(pp, ctx, want):
    data, model = want["twice"]
    file, off, counts = model
    assert len(off) == 3 and data[:P] == data[P:] and file[off[0]:off[1]] == file[off[1]:off[2]], "nothing survives in the table"
    check(pp, ctx, data, model)


def test_forty_pieces_in_one_call(pp, ctx, want):
    data, model = want["many"]
    file, off, counts = model
    assert len(off) == 41 and all(counts) and off == [sum(off[b + 1] - off[b] for b in range(k)) for k in range(41)]
    assert gzip.decompress(file) == data
    check(pp, ctx, data, model)
    arg, keep = on_device(data)
    z = pp.BgzfDeflated(ctx, arg, pp.MEM_DEVICE)
    z2 = pp.BgzfDeflated(ctx, arg, pp.MEM_DEVICE)
    try:
        assert z.host().tobytes() == z2.host().tobytes() == file, "a second call gives identical bytes"
        back = pp.Bgzf(ctx, (z.bytes_ptr, z.n_bytes), (z.blk_off_ptr, z.n_blocks), mem=pp.MEM_DEVICE)      # blk_off is what the reader takes
        try:
            assert back.n_bytes == len(data) and back.host().tobytes() == data
        finally:
            back.close()
    finally:
        z.close()
        z2.close()


def test_a_tagged_file_compressed_equals_its_stream_compressed(pp, ctx, tmp_path):
    b, at, off, passed = tm.stream_of(3 * P + 4321, fail_last=True)
    u = tm.tagged(b, at, off, passed)
    assert len(u) > 3 * P
    file, blk, counts = D.deflate_file(u)
    t = pp.BamTagged(ctx, b, at, off, passed)
    z = t.deflate()
    d = pp.BgzfDeflated(ctx, u)
    try:
        assert t.counts[2] == 4 and z.n_blocks == 4
        assert z.host().tobytes() == d.host().tobytes() == file and list(z.counts) == counts and z.blk_off().tolist() == blk
        assert t.host().tobytes() == tm.frame(u), "the level-0 file is what it was"
        assert z.n_bytes <= t.n_bytes
        path = tmp_path / "tagged.bam"
        z.write(path)
        assert path.read_bytes() == file and gzip.decompress(path.read_bytes()) == u
        with pytest.raises(pp.PolypolishError) as e:
            z.write(tmp_path / "no_such_directory" / "tagged.bam")
        assert e.value.code == pp.ERR_QUIT and "unable to write alignments to" in e.value.msg
    finally:
        for o in (d, z, t):
            o.close()


def test_stage_times(pp, want):
    c = pp.Context(0)
    try:
        z = pp.BgzfDeflated(c, want["bam_like"][0])
        with pytest.raises(pp.PolypolishError):
            z.kernel_ms()
        z.close()
        c.set_profiling(True)
        z = pp.BgzfDeflated(c, want["bam_like"][0])
        ms = z.stage_ms()
        assert set(ms) == {"pieces", "scan", "place"} and ms["pieces"] > 0 and z.kernel_ms() == pytest.approx(sum(ms.values()))
        z.close()
    finally:
        c.close()


def test_what_is_refused(pp, ctx):
    L = pp.lib()
    arr = np.frombuffer(b"some bytes", np.uint8)
    out = C.c_void_p()
    assert L.pp_bgzf_deflate(ctx._h, None, 5, pp.MEM_HOST, C.byref(out)) == pp.ERR_ARG and not out.value
    assert L.pp_bgzf_deflate(ctx._h, arr.ctypes.data, len(arr), pp.MEM_HOST, None) == pp.ERR_ARG
    assert L.pp_bgzf_deflate(ctx._h, arr.ctypes.data, len(arr), pp.MEM_PEER, C.byref(out)) == pp.ERR_ARG and not out.value
    assert L.pp_bgzf_deflate(ctx._h, arr.ctypes.data, 1 << 40, pp.MEM_HOST, C.byref(out)) == pp.ERR_LIMIT and not out.value
    assert L.pp_bgzf_deflate(None, arr.ctypes.data, len(arr), pp.MEM_HOST, C.byref(out)) == pp.ERR_ARG
    assert L.pp_bam_out_deflate(ctx._h, None, C.byref(out)) == pp.ERR_ARG and not out.value
    assert L.pp_bgzf_out_write(None, b"x") == pp.ERR_ARG and L.pp_bgzf_out_kernel_ms(None, None) == pp.ERR_ARG
    with pytest.raises(pp.PolypolishError) as e:
        pp.BgzfDeflated(ctx, (0, 0), pp.MEM_PEER)
    assert e.value.code == pp.ERR_ARG
    z = pp.BgzfDeflated(ctx, b"")
    try:
        assert z.host().tobytes() == M.EOF_BLOCK and z.n_blocks == 0 and z.blk_off().tolist() == [0] and z.counts == (0, 0, 0)
        assert L.pp_bgzf_out_write(z._p, None) == pp.ERR_ARG
    finally:
        z.close()
