"""pp_bam_sam / pp_bam_sam_encoded (pp_bam_sam.hip) against the plain model (tests/bam_sam_model.py, pinned by
tests/test_bam_sam_model_cpu.py), byte for byte, with the bytes and the offsets in host and in device memory -- the device array some
bytes into its allocation and ending where the test's bytes end, hostile bytes in the header text, the one place in front of records_at
where the contract allows any: record counts around pass A's workgroup, every part of a line across a tile boundary of pass B at every
offset, l_seq around the lane's bytes and the lane group's stride, a record longer than a tile, 65,535 CIGAR ops, a B:f array of the
exponent / mantissa floats, unordered offsets, the verdicts, every refusal with its code and record, determinism and the stage times.
None of these inputs is out of bounds: every offset a kernel follows lies inside the test's own allocation or is refused before it
is followed.  Needs an MI355X: `-m gpu`."""
import struct

import numpy as np
import pytest

import bam_model as bm
import bam_sam_model as bs
from test_bam_sam_model_cpu import REFS3, SQ3, arg_records, good, limit_records

pytestmark = pytest.mark.gpu

REFS = (("c1", 1000000), ("chromosome_two", 500))
TEXT = "@HD\tVN:1.6\n@CO\thostile \xff\x80\x01 bytes\r\n@PG\tID:x"      # (no @SQ line: two are synthesised; no final newline: one is added)


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
    recs, tile, store, lane, group = pp.bam_sam_geometry()
    assert tile % store == 0 and tile >= 1024 and lane == store == 16 and group >= 1
    return {"recs": recs, "tile": tile, "store": store, "lane": lane, "stride": lane * group}


def on_device(data, lead=0):
    import torch
    t = torch.from_numpy(np.frombuffer(b"\xa5" * lead + bytes(data), np.uint8).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return t, t.data_ptr() + lead


def device_text(pp, ctx, b, at, off, passed, mem, lead=0):
    """-> (the text, counts) of the device decode; MEM_DEVICE: the bytes `lead` bytes into their allocation, nothing of the test's behind"""
    off = np.ascontiguousarray(off, dtype=np.uint64)
    if mem == pp.MEM_HOST:
        o = pp.SamOut.from_bam(ctx, b, at, off, passed)
    else:
        keep, p = on_device(b, lead)
        keep_off, po = on_device(off.tobytes() if len(off) else bytes(8))
        o = pp.SamOut.from_bam(ctx, (p, len(b)), at, (po if len(off) else 0, len(off)), passed, mem=pp.MEM_DEVICE)
        del keep, keep_off
    try:
        assert o.dev() == (o.bytes_ptr, o.n_bytes) and o.bytes_ptr % 16 == 0
        return o.bytes(), o.counts()
    finally:
        o.close()


def first_difference(a, b):
    n = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    return len(a), len(b), n, a[max(0, n - 32):n + 32], b[max(0, n - 32):n + 32]


def check(pp, ctx, recs, passed=None, lead=3, mems=None, refs=REFS, text=TEXT, off=None, twice=False):
    b, at, own = bs.bam_of(recs, refs, text)
    off = own if off is None else off
    want = bs.decode(b, at, off, passed)
    for mem in mems or (pp.MEM_HOST, pp.MEM_DEVICE):
        got, counts = device_text(pp, ctx, b, at, off, passed, mem, lead)
        assert got == want, (mem, first_difference(got, want))
        n_fail = 0 if passed is None else int((np.asarray(passed) == 0).sum())
        n_al = sum(1 for o in off if not struct.unpack_from("<H", b, int(o) + 18)[0] & 4)
        assert counts == (n_al - n_fail, n_fail, want.count(b"\n")), mem
        if twice:
            assert device_text(pp, ctx, b, at, off, passed, mem, lead + 1)[0] == got, "two calls give identical bytes"
    return want


def mixed_record(i):
    """a record that changes with i: names, l_seq, QUAL or 0xFF, CIGARs, aux fields of every type, unaligned ones"""
    n = (i * 7) % 45
    seq = "".join(bm.NIBBLE[(i + 3 * k) % 16] for k in range(n))
    qual = None if i % 3 == 0 else bytes((i + k) % 94 for k in range(n))
    aux = [bm.aux("NM", "C", i % 200), bm.aux("AS", "i", -i * 37 - 70000), bm.aux("MD", "Z", "5A" * (i % 9)), bm.aux("XA", "A", chr(33 + i % 94)),
           bm.aux("XH", "H", "0aF" * 2 * (i % 4)), bm.aux("XB", "B", ("cCsSiI"[i % 6], [1, 2, 3][: i % 4])), bm.aux("Xf", "f", i / 8.0)][: i % 8]
    if i % 11 == 5:
        return bm.record(b"u%d" % i, 4 | 64, -1, -1, [], seq, b"".join(aux), qual=qual, mapq=0)
    runs = [] if n == 0 else ([(n << 4) | 0] if i % 2 else [(1 << 4) | 4, (max(n - 2, 1) << 4) | 7, (2 << 4) | 2, (1 << 4) | 1])
    return bm.record(b"read%d" % i * (1 + i % 3), 16 * (i % 2), i % 2, i * 3, runs, seq, b"".join(aux), qual=qual, mapq=i % 256,
                     next_ref=(i % 2, -1, 1)[i % 3], next_pos=i, tlen=-i if i % 2 else i * 1000)


def verdicts_of(recs, rule):
    al = [r for r in recs if not struct.unpack_from("<H", r, 18)[0] & 4]
    return np.array([rule(k) for k in range(len(al))], np.uint8)


def test_record_counts_around_pass_a_s_workgroup(pp, ctx, geo):
    w = geo["recs"]
    for n in (0, 1, w - 1, w, w + 1, 2 * w + 1):
        recs = [mixed_record(i) for i in range(n)]
        check(pp, ctx, recs, lead=n % 16)
        check(pp, ctx, recs, verdicts_of(recs, lambda k: (k * 7) % 5 != 0), lead=1 + n % 15, mems=(pp.MEM_DEVICE,))


def test_no_records_with_and_without_a_header(pp, ctx):
    assert check(pp, ctx, [], refs=(), text="") == b""
    assert check(pp, ctx, [], refs=(), text="@HD\tVN:1.6") == b"@HD\tVN:1.6\n"
    assert check(pp, ctx, [], passed=np.zeros(0, np.uint8)).endswith(b"@SQ\tSN:chromosome_two\tLN:500\n")
    long_text = "@CO\t" + "x" * 40000 + "\n"                    # a header longer than two tiles, then records
    check(pp, ctx, [mixed_record(i) for i in range(40)], text=long_text + "@SQ\tSN:c1\tLN:1000000\n")
    check(pp, ctx, [], text=long_text)


def probe():
    """a record with every part of a line: QNAME, each number column, both names, CIGAR, SEQ, QUAL, each of the eleven aux types
    (A c C s S i I Z H f B)"""
    aux = (bm.aux("XA", "A", "Q") + bm.aux("Xc", "c", -128) + bm.aux("XC", "C", 255) + bm.aux("Xs", "s", -32768) + bm.aux("XS", "S", 65535) +
           bm.aux("Xi", "i", -2**31) + bm.aux("XI", "I", 4294967295) + bm.aux("XZ", "Z", "some text") + bm.aux("XH", "H", "1aF0") + bm.aux("Xf", "f", 1.234565e-05) + bm.aux("XB", "B", ("s", [-3, 3])) + bm.aux("Xg", "B", ("f", [0.1, 3.4028235e38])) +
           bm.aux("ZP", "Z", "fail"))
    return bm.record(b"a_query_name/1", 147, 0, 123456, [(5 << 4) | 4, (30 << 4) | 0, (2 << 4) | 1], "ACGTNMRSVWYHKDB=ACGTNMRSVWYHKDB=ACGTN", aux, qual=bytes(range(37)),
                     mapq=29, next_ref=1, next_pos=300, tlen=-2**31)


def test_every_part_across_a_tile_boundary_at_every_offset(pp, ctx, geo):
    tile = geo["tile"]
    P = probe()
    names = [n.encode() for n, _ in REFS]
    head = len(bs.header_text(*bs.bam_of([], REFS, TEXT)[:2])[0])
    plen = len(bs.line(bs._fields(P, 0), names, True))
    pad = lambda z: bm.record(b"pad", 4, -1, -1, [], "", bm.aux("XP", "Z", "p" * z))      # noqa: E731
    base = len(bs.line(bs._fields(pad(0), 0), names))
    recs, pos = [], head
    for k in range(plen + 1):                       # the probe's line begins k bytes in front of a tile boundary: k = 0 .. its length
        boundary = (pos + base + plen + tile - 1) // tile * tile
        z = boundary - k - pos - base
        recs += [pad(z), P]
        pos += base + z + plen
        assert (pos - plen + k) % tile == 0
    passed = np.zeros(len(recs) // 2, np.uint8)     # (the pads are unaligned: one verdict per probe, all failing)
    want = check(pp, ctx, recs, passed, lead=7)
    assert want.count(b"ZP:Z:fail\tZP:Z:fail\n") == plen + 1 and len(want) > plen * tile


def test_l_seq_around_the_lane_s_bytes_and_the_group_s_stride(pp, ctx, geo):
    lane, stride = geo["lane"], geo["stride"]
    lens = sorted({0, 1, 2, lane - 1, lane, lane + 1, 2 * lane - 1, 2 * lane, 2 * lane + 1, stride - 1, stride, stride + 1, 2 * stride - 1, 2 * stride, 2 * stride + 1})
    recs = []
    for n in lens:
        seq = "".join(bm.NIBBLE[(5 * k + n) % 16] for k in range(n))
        for qual in ((None,) if n == 0 else (None, bytes((k * 7 + n) % 94 for k in range(n)))):
            recs.append(bm.record(b"s%d" % n, 0, 0, 1, [(max(n, 1) << 4) | 0], seq, bm.aux("NM", "C", 1), qual=qual, seq_pad_nibble=0xF))
    for n in (1, 2, lane - 1, lane, lane + 1, 254):   # QNAME lengths
        recs.append(bm.record(bytes(33 + (k * 5 + n) % 90 for k in range(n)).replace(b"@", b"a"), 0, 0, 1, [(3 << 4)], "ACG", b"", qual=bytes([0, 40, 93])))
    check(pp, ctx, recs, lead=5)
    check(pp, ctx, recs[::-1], verdicts_of(recs, lambda k: k % 2), lead=11)


def test_a_record_longer_than_a_tile_and_65535_cigar_ops(pp, ctx, geo):
    n = 40000
    assert n > 2 * geo["tile"]
    seq = "".join(bm.NIBBLE[(k * 11 + k // 97) % 16] for k in range(n))
    long_rec = bm.record(b"long", 0, 0, 7, [(n << 4) | 0], seq, bm.aux("NM", "C", 3) + bm.aux("XZ", "Z", "behind the bases"), qual=bytes((k * 13) % 94 for k in range(n)))
    many = bm.record(b"many", 16, 1, 0, [((1 + k % 300) << 4) | (k % 9) for k in range(65535)], "ACGT", bm.aux("XZ", "Z", "behind the words"), qual=bytes(4))
    recs = [good(0), long_rec, good(1), many, good(2)]
    want = check(pp, ctx, recs, lead=9)
    assert max(len(ln) for ln in want.split(b"\n")) > 3 * 65535 > geo["tile"]
    check(pp, ctx, recs, np.zeros(5, np.uint8), lead=2, mems=(pp.MEM_DEVICE,))


def test_b_f_array_of_the_exponent_and_mantissa_floats(pp, ctx):
    bits = bs.exponent_floats()                      # (exponent 255 is inf / nan: refused, see the refusals)
    assert len(bits) == 1020
    r = bytearray(bm.record(b"q", 4, -1, -1, [], "", bm.aux("XB", "B", ("f", []))))
    r[-4:] = struct.pack("<I", 2 * len(bits))
    r += np.array(bits + [b | 0x80000000 for b in bits], "<u4").tobytes()
    r[0:4] = struct.pack("<I", len(r) - 4)
    singles = [bm.record(b"f%d" % i, 0, 0, 1, [(1 << 4)], "A", b"XFf" + struct.pack("<I", b)) for i, b in enumerate(bits[::37] + [0x3DCCCCCD, 0x49742450, 0x4974240F, 0x7F7FFFFF, 1])]
    want = check(pp, ctx, [bytes(r)] + singles, lead=13)
    assert want.count(b"XF:f:1e+06\n") == 2 and b",1.4013e-45," in want and b",-3.40282e+38" in want and b"XF:f:0.1\n" in want


def test_rec_off_unordered_with_gaps_and_a_repeated_record(pp, ctx):
    recs = [mixed_record(i) for i in range(60)]
    b, at, off = bs.bam_of(recs)
    order = np.array([off[k] for k in (59, 0, 30, 30, 7, 58, 1, 30)], np.uint64)
    want = check(pp, ctx, recs, off=order, refs=(("c1", 1000), ("c2", 2000)), text="@HD\tVN:1.6\n")
    assert want.count(b"\n") == 1 + 2 + 8


def test_verdicts_all_0_all_1_mixed_and_a_tag_behind_a_tag(pp, ctx):
    recs = [mixed_record(i) for i in range(300)]
    recs[10] = bm.record(b"tagged", 0, 0, 1, [(1 << 4)], "A", bm.aux("NM", "C", 0) + bm.aux("ZP", "Z", "fail"))
    plain = check(pp, ctx, recs, None, twice=True)
    assert check(pp, ctx, recs, verdicts_of(recs, lambda k: 1)) == plain
    zeros = check(pp, ctx, recs, verdicts_of(recs, lambda k: 0), twice=True)
    assert b"\tZP:Z:fail\tZP:Z:fail\n" in zeros and zeros.count(b"ZP:Z:fail\n") == len(verdicts_of(recs, lambda k: 0))
    check(pp, ctx, recs, verdicts_of(recs, lambda k: k % 3 != 1), lead=15)


def refused(pp, ctx, b, at, off, passed=None, mem=None, lead=3):
    """(code, bad record) of a refused call, checked to leave no object and the context serving a good one"""
    with pytest.raises(pp.PolypolishError) as err:
        device_text(pp, ctx, b, at, off, passed, pp.MEM_HOST if mem is None else mem, lead)
    gb, gat, goff = bs.bam_of([good(0), good(1)])
    assert device_text(pp, ctx, gb, gat, goff, None, pp.MEM_HOST)[0] == bs.decode(gb, gat, goff), "the context serves a good call after a refusal"
    return err.value.code, err.value.bad_record


def test_every_refusal_with_its_bad_record(pp, ctx, geo):
    w = geo["recs"]
    for cases in (arg_records(), limit_records()):
        for i, (what, r) in enumerate(cases):
            k = (0, 2, w + 1)[i % 3]
            recs = [good(j) for j in range(k)] + [r, good(9)]
            b, at, off = bs.bam_of(recs, REFS3, SQ3)
            want = bs.refusal(b, at, off)
            assert want is not None and want[1] == k
            assert refused(pp, ctx, b, at, off, mem=(pp.MEM_HOST, pp.MEM_DEVICE)[i % 2]) == want, what
            assert refused(pp, ctx, b, at, off, passed=[1]) == want, "in front of the verdicts' number"
    # the first refused record in index order wins, whatever its kind; inside one record ARG goes in front of LIMIT
    lim, arg = limit_records()[0][1], arg_records()[0][1]
    both = bm.record(b"a\tb", 0, 0, -2, [], "", b"")
    for recs, want in (([good(), lim, arg], (bs.LIMIT, 1)), ([good(), arg, lim], (bs.ARG, 1)), ([both], (bs.ARG, 0))):
        b, at, off = bs.bam_of(recs, REFS3, SQ3)
        assert bs.refusal(b, at, off) == want and refused(pp, ctx, b, at, off, mem=pp.MEM_DEVICE) == want
    # the three of the walk
    b, at, off = bs.bam_of([good(0), good(1)], REFS3, SQ3)
    n = len(b)
    for o, nb in ((n + 1, n), (n, n), (n - 3, n), (int(off[1]), n - 1)):
        for mem in (pp.MEM_HOST, pp.MEM_DEVICE):
            assert refused(pp, ctx, b[:nb], at, np.array([off[0], o], np.uint64), mem=mem) == (bs.ARG, 1), (o, nb)
    small = bytearray(b)
    small[int(off[0]):int(off[0]) + 4] = struct.pack("<I", 31)
    assert refused(pp, ctx, bytes(small), at, off) == (bs.ARG, 0)
    # the verdicts' number, once the records are free of defects; the header
    for passed in ([], [1], [1, 1, 1]):
        assert refused(pp, ctx, b, at, off, passed=np.array(passed, np.uint8)) == (bs.ARG, None)
    assert refused(pp, ctx, b, at - 1, off) == (bs.ARG, None) and refused(pp, ctx, b, at + 1, off, mem=pp.MEM_DEVICE) == (bs.ARG, None)
    assert refused(pp, ctx, b, len(b) + 1, off) == (bs.ARG, None)
    for refs in ((("a b", 5),), (("ok", 0),), (("*", 5),)):
        hb, hat, hoff = bs.bam_of([], refs, "@HD\n")
        assert bs.refusal(hb, hat, hoff) == (bs.LIMIT, None) and refused(pp, ctx, hb, hat, hoff) == (bs.LIMIT, None)


def test_the_twin_call_and_the_stage_times(pp, ctx):
    import sam_bam_model as sb
    text = b"@SQ\tSN:c\tLN:100\nr1\t0\tc\t5\t60\t4M\t=\t9\t12\tACGT\tIIII\tNM:i:0\tXf:f:0.5\n" + b"r2\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*\n"
    assert bs.canonical(text) == text
    ctx.set_profiling(True)
    enc = o = None
    try:
        enc = pp.BamEncoded(ctx, text)
        o = enc.sam()
        assert o.bytes() == text and o.counts() == (1, 0, 3)
        ms = o.stage_ms()
        assert set(ms) == {"newline_index", "pass_a", "scans", "pass_b"} and ms["newline_index"] == 0 and ms["pass_b"] > 0 and abs(o.kernel_ms() - sum(ms.values())) < 1e-3
        o.close()
        o = enc.sam([0])
        assert o.bytes() == text.replace(b"\tXf:f:0.5\n", b"\tXf:f:0.5\tZP:Z:fail\n") and o.counts() == (0, 1, 3)
        z = o.deflate()
        try:
            assert z.n_bytes > 28
        finally:
            z.close()
        assert sb.encode(o.bytes())["bytes"][:4] == b"BAM\1"
    finally:
        ctx.set_profiling(False)
        for x in (o, enc):
            if x is not None:
                x.close()
