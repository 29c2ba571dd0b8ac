"""tests/bgzf_model.py -- the plain model of the BGZF front end -- pinned from both sides, without a GPU:
  * its inflate equals zlib.decompress(raw, -15) on every stream tests/test_bgzf_inflate_gpu.py uses, and refuses every defect
    stream that zlib refuses (zlib decides which malformed code sets are refused);
  * the feature reports of the chosen inputs show what the GPU tests rely on: all three block types, distances beyond 16384, codes
    longer than the kernel's first-level tables (10 bits literal/length, 8 bits distance), the three repeat symbols, overlapping
    matches, a stream without a distance code, the short fixed streams, the eight bit phases in front of a stored block;
  * the library's host walk, pp_bgzf_walk, is the model's walk() on a three-block file and on every truncation of it."""
import ctypes as C
import zlib

import numpy as np
import pytest

import bgzf_model as zm


@pytest.fixture(scope="module")
def table():
    return zm.table_inputs()


@pytest.fixture(scope="module")
def seams():
    return zm.seam_streams()


def test_model_equals_zlib_on_every_stream(table, seams):
    for name, (data, raw) in {**table, **seams}.items():
        got, rep = zm.inflate(raw)
        assert got == data == zlib.decompress(raw, -15), name
        assert rep["end_bit"] <= 8 * len(raw) and (rep["end_bit"] + 7) // 8 == len(raw), name
        assert zm.inflate_block(zm.wrap(raw, data)) == data, name
    blob, datas = zm.many_blocks(60)
    off, out, end, ok = zm.walk(blob)
    assert ok and end == len(blob) and len(off) == 60 and out[-1] == sum(map(len, datas))
    for at, data in zip(off, datas):
        assert zm.inflate_block(blob, at) == data


def test_feature_reports_show_what_the_gpu_tests_rely_on(table, seams):
    rep = {k: zm.inflate(raw)[1] for k, (_, raw) in {**table, **seams}.items()}
    assert set(rep["stored"]["types"]) == {0} and rep["stored"]["blocks"] >= 1
    assert set(rep["fixed"]["types"]) == {1} and rep["fixed"]["max_dist"] > 16384 and rep["fixed"]["max_dist_code"] == 5
    bam = rep["dynamic_bam"]
    assert set(bam["types"]) == {2} and bam["max_lit_code"] > 10 and bam["max_dist_code"] > 8 and 16 in bam["repeats"], bam
    assert bam["max_dist"] > 16384 and bam["max_len"] > 64 and bam["overlaps"] > 0
    assert rep["dynamic_acgt"]["repeats"] == {16, 17, 18}
    zeros = rep["zeros"]
    assert zeros["max_len"] == 258 and zeros["max_dist"] == 1 and zeros["overlaps"] >= 250
    assert rep["huffman_only"]["max_dist_code"] == 0 and rep["huffman_only"]["max_len"] == 0 and set(rep["huffman_only"]["types"]) == {2}
    assert rep["two_stored"]["types"] == [0, 0] and sum(rep["two_stored"]["stored"]) == 60000
    assert rep["empty"]["types"] == [1] and len(table["empty"][1]) == 2 and len(table["one_byte"][1]) == 3
    # the seams
    first = rep["match_258_at_32768_first_in_a_fixed_block"]
    assert first["types"] == [0, 1] and first["max_dist"] == 32768 and first["stored"] == [32768]
    small = rep["matches_3_and_258_at_small_distances"]
    assert small["overlaps"] == 9 and small["max_len"] == 258      # length 3 at distance 1 and 2, length 258 at all seven
    assert rep["stored_len_0_and_1"]["stored"] == [0, 1, 0]
    assert len(zm.wrap(*seams["stored_largest"][::-1])) == 65536 and rep["stored_largest"]["stored"] == [65505]
    assert len([k for k in seams if k.startswith("stored_after_huffman_phase_")]) == 8
    assert rep["five_blocks_mixed"]["types"] == [0, 1, 0, 1, 0]
    assert rep["last_code_ends_on_the_last_bit"]["end_bit"] == 8 * len(seams["last_code_ends_on_the_last_bit"][1]) == 64
    assert len(seams["isize_65536"][0]) == 65536


def test_every_defect_is_refused_by_the_model_and_by_zlib():
    for name, (blk, kind, how) in zm.defect_blocks().items():
        with pytest.raises(zm.Defect) as e:
            zm.inflate_block(blk)
        assert e.value.kind == kind, name
        if how == "raw":
            _, pay, n, _, _ = zm.unwrap(blk)
            with pytest.raises(zlib.error):
                zlib.decompress(blk[pay:pay + n], -15)
        elif how == "gzip":
            with pytest.raises(zlib.error):
                zlib.decompress(blk, 31)
    # where zlib accepts an incomplete code, so does the model: a distance code of a single 1-bit length
    w = zm.Writer()
    cl = w.dynamic_header(257, 1, {0: 2, 1: 2, 18: 1})
    w.code(cl[18]).bits(127, 7).code(cl[18]).bits(118 - 11, 7).code(cl[1]).code(cl[1])      # 256 zeros, end-of-block: 1 bit, distance 0: 1 bit
    raw = w.bits(0, 1).bytes()                                                                  # the end-of-block code
    assert zm.inflate(raw)[0] == zlib.decompress(raw, -15) == b""


# ---- the library's host walk (no device) -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pp():
    import polypolish_amd
    polypolish_amd.lib()
    return polypolish_amd


def three_blocks():
    a, b = zm.bam_like(700, 4), zm.acgt(300, 5)
    return zm.block(a) + zm.wrap(zm.deflate(b, 0), b, extra_front=b"XY\x03\x00abc") + zm.EOF_BLOCK, [a, b, b""]


def test_walk_equals_the_model(pp):
    data, parts = three_blocks()
    off, out, end = pp.bgzf_walk(data)
    w_off, w_out, w_end, ok = zm.walk(data)
    assert ok and off.tolist() == w_off and out.tolist() == w_out == [0, 700, 1000, 1000] and end == w_end == len(data)
    assert data[w_off[2]:] == zm.EOF_BLOCK and len(zm.EOF_BLOCK) == 28, "the EOF block is an ordinary block"
    off2, out2, end2 = pp.bgzf_walk(data, w_off[1])
    assert off2.tolist() == w_off[1:] and out2.tolist() == [0, 300, 300] and end2 == len(data)
    assert pp.bgzf_walk(b"")[0].size == 0 and pp.bgzf_walk(data, len(data))[2] == len(data)
    with pytest.raises(pp.PolypolishError) as e:
        pp.bgzf_walk(data, len(data) + 1)
    assert e.value.code == pp.ERR_ARG and "behind" in e.value.msg
    # filling by pieces of two blocks: every call goes on where the one before stopped
    L, b = pp.lib(), np.frombuffer(data, np.uint8)
    piece, sums, n, e2 = np.zeros(2, np.uint64), np.zeros(3, np.uint64), C.c_uint64(0), C.c_uint64(0)
    assert L.pp_bgzf_walk(b.ctypes.data, len(b), 0, piece.ctypes.data, sums.ctypes.data, 2, C.byref(n), C.byref(e2)) == pp.OK
    assert (n.value, e2.value, piece.tolist(), sums.tolist()) == (2, w_off[2], w_off[:2], [0, 700, 1000])
    assert L.pp_bgzf_walk(b.ctypes.data, len(b), e2.value, piece.ctypes.data, None, 2, C.byref(n), C.byref(e2)) == pp.OK
    assert (n.value, e2.value, int(piece[0])) == (1, len(data), w_off[2])


def test_every_truncation_is_refused_or_stops_at_the_cut(pp):
    data, _ = three_blocks()
    ends = set(zm.walk(data)[0]) | {len(data)}
    for cut in range(len(data) + 1):
        piece = data[:cut]
        w_off, w_out, w_end, w_ok = zm.walk(piece)
        try:
            off, out, end = pp.bgzf_walk(piece)
        except pp.PolypolishError as e:
            assert e.code == pp.ERR_ARG and e.msg and not w_ok and (e.n_blk, e.end) == (len(w_off), w_end) and cut not in ends, cut
            continue
        assert w_ok and cut in ends and end == cut and off.tolist() == w_off and out.tolist() == w_out, cut


def test_header_defects_of_the_walk(pp):
    good, _ = three_blocks()
    first = zm.walk(good)[0][1]

    def refused(b, n_blk, end, word):
        with pytest.raises(pp.PolypolishError) as e:
            pp.bgzf_walk(bytes(b))
        assert (e.value.code, e.value.n_blk, e.value.end) == (pp.ERR_ARG, n_blk, end) and word in e.value.msg, e.value.msg
        assert zm.walk(bytes(b))[2:] == (end, False)

    for at, value, word in ((0, 0x1e, "1f 8b"), (2, 9, "1f 8b"), (3, 0, "FEXTRA")):
        b = bytearray(good)
        b[first + at] = value
        refused(b, 1, first, word)
    b = bytearray(good)
    b[first + 10:first + 12] = (0xFFFF).to_bytes(2, "little")           # XLEN past the bytes
    refused(b, 1, first, "XLEN")
    b = bytearray(good)
    b[first + 14:first + 16] = (60000).to_bytes(2, "little")            # the first subfield's SLEN past XLEN
    refused(b, 1, first, "XLEN")
    b = bytearray(good)
    b[first + 19] = ord("D")                                            # XY abc | BD: no BC
    refused(b, 1, first, "BC")
    b = bytearray(good)
    b[first + 23:first + 25] = (20).to_bytes(2, "little")               # BSIZE + 1 below header + footer
    refused(b, 1, first, "BSIZE")
    b = bytearray(good)
    b[16:18] = (0xFFFF).to_bytes(2, "little")                           # block 0 past the end
    refused(b, 0, 0, "past")
    big = zm.wrap(zm.deflate(b"x"), b"x", isize=65537)
    refused(good[:first] + big, 1, first, "ISIZE")
    assert pp.bgzf_walk(good[:first] + zm.wrap(zm.deflate(b"x"), b"x", isize=65536))[1].tolist() == [0, 700, 700 + 65536]
