"""pp_tabix_index (pp_tabix.hip) against tests/tabix_model.py's tbi_raw(), BYTE FOR BYTE, with gzip.decompress(tbi) == raw: both
presets, the text in host and in device memory, the block table of the level-0 file (b * 65,311) and pp_bgzf_deflate's own from host
and from device memory.  The texts aim at the seams of the code: line counts around the wave, the workgroup and the scan's tile;
texts of only meta lines, meta lines between data lines, a last line without a newline; a line that starts and ends at and around the
65,280-byte block seam; columns closed just inside and just outside the PP_TBX_LANE_BYTES a lane looks at, and a REF as long as a
block (the workgroup pass); positions at the window and bin boundaries and at 2^29; many names and one long name run; a device text at
every alignment that ends where its allocation ends; every refusal with its line; call after call on one context.  Every case is a
few thousand lines at most.  Needs an MI355X: `-m gpu`."""
import gzip

import numpy as np
import pytest

import tabix_model as tx

pytestmark = pytest.mark.gpu
P = tx.PAYLOAD
VCF, BED = tx.VCF, tx.BED


@pytest.fixture(scope="module")
def pp():
    import polypolish_amd
    return polypolish_amd


@pytest.fixture(scope="module")
def ctx(pp):
    c = pp.Context(0)
    yield c
    c.close()


def on_device(b, skip=0, behind=b""):
    """(device address, n_bytes) of the bytes, `skip` hostile bytes in front and `behind` behind them; without `behind` the allocation
    ends where they end"""
    import torch
    whole = np.concatenate([np.full(skip, 0x09, np.uint8), np.frombuffer(bytes(b), np.uint8), np.frombuffer(bytes(behind), np.uint8)])
    t = torch.from_numpy(whole.copy()).to("cuda:0") if len(whole) else torch.zeros(1, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert t.data_ptr() % 16 == 0
    return (t.data_ptr() + skip, len(b)), t


def table_on_device(blk):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(blk, np.uint64).view(np.int64).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return (t.data_ptr(), len(blk) - 1), t


def check(pp, ctx, text, preset, full=False):
    """the index in every form against the model; -> the index over pp_bgzf_deflate's own block table"""
    text = bytes(text)
    flat = tx.level0_blk_off(len(text))
    want_flat = tx.tbi_raw(text, preset, flat)
    dev, keep = on_device(text)
    z = pp.BgzfDeflated(ctx, dev, pp.MEM_DEVICE)
    try:
        blk = z.blk_off()
        assert len(blk) == len(flat)
        want_own = tx.tbi_raw(text, preset, blk)
        flat_dev, keep2 = table_on_device(flat)
        forms = [(text, pp.MEM_HOST, flat, want_flat), (dev, pp.MEM_DEVICE, (z.blk_off_ptr, z.n_blocks), want_own)]
        if full:
            forms += [(text, pp.MEM_HOST, blk, want_own), (text, pp.MEM_HOST, (z.blk_off_ptr, z.n_blocks), want_own), (dev, pp.MEM_DEVICE, blk, want_own),
                      (dev, pp.MEM_DEVICE, flat, want_flat), (dev, pp.MEM_DEVICE, flat_dev, want_flat), (text, pp.MEM_HOST, flat_dev, want_flat)]
        for data, mem, table, want in forms:
            tbi, raw = pp.tabix_index(ctx, data, preset, table, mem)
            assert raw == want, (mem, type(table), len(raw), len(want))
            assert gzip.decompress(tbi) == raw and tbi[-28:] == bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
        only_tbi, none = pp.tabix_index(ctx, dev, preset, (z.blk_off_ptr, z.n_blocks), pp.MEM_DEVICE, raw=False)
        assert none is None and gzip.decompress(only_tbi) == want_own
        assert z.host().tobytes()[:4] == b"\x1f\x8b\x08\x04"
    finally:
        z.close()
        del keep
    return want_own


def refused(pp, ctx, text, preset, code, line, blk=None, mems=None):
    with pytest.raises(tx.TabixError) as m:
        tx.tbi_raw(text, preset, tx.level0_blk_off(len(text)) if blk is None else blk)
    assert (m.value.code, m.value.bad_line) == (code, line), ("the model", m.value)
    for mem in mems or (pp.MEM_HOST, pp.MEM_DEVICE):
        data, keep = (text, None) if mem == pp.MEM_HOST else on_device(text)
        with pytest.raises(pp.PolypolishError) as e:
            pp.tabix_index(ctx, data, preset, tx.level0_blk_off(len(text)) if blk is None else blk, mem)
        assert (e.value.code, e.value.bad_line) == (code, line), (mem, e.value)
        del keep


def sorted_lines(preset, n, name=b"ctg", step=3, span=2):
    return [tx.vcf_line(name, 1 + step * i, b"A" * span) if preset == VCF else tx.bed_line(name, step * i, step * i + span) for i in range(n)]


@pytest.mark.parametrize("preset", [VCF, BED])
def test_line_counts_around_the_wave_the_workgroup_and_the_scans_tile(pp, ctx, preset):
    for n in (0, 1, 63, 64, 65, 255, 256, 257, 1025):
        raw = check(pp, ctx, tx.join(sorted_lines(preset, n)), preset, full=n in (0, 1, 257))
        t = tx.parse_tbi(raw)
        assert len(t["names"]) == (1 if n else 0) and (not n or t["refs"][0]["bins"][tx.PSEUDO_BIN][1] == (n, 0))


@pytest.mark.parametrize("preset", [VCF, BED])
def test_meta_lines_and_a_last_line_without_a_newline(pp, ctx, preset):
    data = sorted_lines(preset, 200)
    check(pp, ctx, b"##only\n#meta\tlines\n", preset, full=True)
    check(pp, ctx, b"#", preset)
    check(pp, ctx, b"#x\n#", preset)
    check(pp, ctx, tx.join([b"##head", b"#CHROM\tPOS"] + data), preset)
    mixed = []
    for i, ln in enumerate(data):
        mixed.append(ln)
        if i % 7 == 3 or i in (62, 63, 64, 199):
            mixed.append(b"#between %d" % i)
    got = tx.parse_tbi(check(pp, ctx, tx.join(mixed), preset))
    assert len(got["refs"][0]["bins"][4681]) > 20, "a meta line ends a chunk"
    check(pp, ctx, tx.join(data, last_newline=False), preset, full=True)
    check(pp, ctx, tx.join(data[:1], last_newline=False), preset)
    check(pp, ctx, tx.join(data + [b"#tail"], last_newline=False), preset)


def _line_at(start, length, preset=BED):
    """a text whose line `at` starts at stream offset `start` and is `length` bytes long with its newline; lines in front and behind"""
    lines, size, i = [], 0, 0
    while size + 40 < start:
        ln = tx.bed_line(b"ctg", i, i + 1)
        lines.append(ln)
        size += len(ln) + 1
        i += 1
    base = tx.bed_line(b"ctg", i, i + 1, b"")                          # name, beg, end and a tab: the filler grows its fourth column
    lines.append(base + b"x" * (start - size - len(base) - 1))
    i += 1
    base = tx.bed_line(b"ctg", i, i + 5, b"")
    assert length > len(base)
    lines.append(base + b"y" * (length - len(base) - 1))
    at = len(lines) - 1
    lines += [tx.bed_line(b"ctg", i + 1 + k, i + 2 + k) for k in range(5)]
    text = tx.join(lines)
    cuts = tx.cut(text)
    assert cuts[at][0] == start and cuts[at][1] == start + length
    return text


def test_a_line_that_starts_and_ends_at_and_around_the_block_seam(pp, ctx):
    for start in (P - 1, P, P + 1):
        check(pp, ctx, _line_at(start, 30), BED, full=start == P)
    for end in (P, 2 * P):
        text = _line_at(end - 30, 30)
        check(pp, ctx, text, BED, full=True)
        cutoff = text[:end]                                             # ... and as the text's last line: its end is the EOF block's offset 0
        assert len(cutoff) == end and cutoff.endswith(b"\n")
        raw = check(pp, ctx, cutoff, BED, full=True)
        span = tx.parse_tbi(raw)["refs"][0]["bins"][tx.PSEUDO_BIN][0]
        assert span[1] & 0xFFFF == 0 and span[1] >> 16 > 0


def test_a_ref_as_long_as_a_block_and_columns_around_the_lanes_bound(pp, ctx):
    B = pp.TBX_LANE_BYTES
    assert B == tx.LANE_BYTES
    long_ref = [tx.vcf_line(b"ctg", 5), tx.vcf_line(b"ctg", 9, b"ACGT" * 17_500, b"<DEL>"), tx.vcf_line(b"ctg", 12), tx.vcf_line(b"ctg", 70_100, b"G" * 4_097),
                tx.vcf_line(b"ctg", 70_200, b"G" * 4_096, id_=b"i" * 4_090), tx.vcf_line(b"c2", 1, b"T" * 8_193)]
    raw = check(pp, ctx, tx.join(long_ref), VCF, full=True)
    assert 585 in tx.parse_tbi(raw)["refs"][0]["bins"] or 73 in tx.parse_tbi(raw)["refs"][0]["bins"]
    # column 4's closing tab at every place around the bound: "c\t1000\t.\t" is 9 bytes, so REF lengths B - 12 .. B + 3; and REF lengths
    # B - 1, B, B + 1 themselves
    lens = sorted(set(range(B - 12, B + 4)) | {B - 1, B, B + 1, 2 * B, 15, 16, 17, 31, 32, 33})
    lines = [tx.vcf_line(b"c", 1000 + 10 * k, b"A" * n) for k, n in enumerate(lens)]
    assert {len(ln.split(b"\t")[0]) + 1 + 4 + 1 + 1 + 1 + n for ln, n in zip(lines, lens)} >= {B - 2, B - 1, B, B + 1}
    check(pp, ctx, tx.join(lines), VCF, full=True)
    check(pp, ctx, tx.join(lines, last_newline=False), VCF)
    # ... and the same tab under 16 name lengths: the line's start, and with it every load, moves through its sixteen bytes
    lines = [tx.vcf_line(b"n" * k, 7, b"C" * 300, id_=b"rs%d" % k) for k in range(1, 17)]
    check(pp, ctx, tx.join(lines), VCF)
    # BED: a name, a begin and an end that reach over the bound; a column 3 that ends at the line's end behind it
    lines = [tx.bed_line(b"N" * n, 10 ** 9 // 4 - 1, 10 ** 9 // 4, rest) for n in range(B - 22, B - 16) for rest in (None, b"x" * 70)]
    lines += [tx.bed_line(b"M" * n, 5, 6) for n in (B - 1, B, B + 1, 4_095, 4_096, 4_097, 70_000)]
    check(pp, ctx, tx.join(lines), BED, full=True)
    check(pp, ctx, tx.join(lines, last_newline=False), BED)


@pytest.mark.parametrize("preset", [VCF, BED])
def test_positions_at_the_window_and_bin_boundaries(pp, ctx, preset):
    def line(beg, end):
        return tx.vcf_line(b"ctg", beg + 1, b"A" * (end - beg)) if preset == VCF else tx.bed_line(b"ctg", beg, end)
    spans = []
    for k in (1, 2, 5):
        e = k << 14
        spans += [(e - 2, e - 1), (e - 2, e), (e - 1, e), (e - 1, e + 1), (e, e + 1), (e + 1, e + 2)]
    for shift in (17, 20, 23, 26):
        e = 1 << shift
        spans += [(e - 3, e - 1), (e - 3, e), (e - 3, e + 1), (e - 1, e + 1), (e, e + 2), (e + 1, e + 3)]
    spans = sorted(spans)
    if preset == BED:                                                   # (a VCF REF of 2^26 bytes is no test case)
        spans += [((1 << 26) + 5, (1 << 27) + 5), ((1 << 27) + 5, (1 << 27) + 5), ((1 << 29) - 1, 1 << 29)]
    else:
        spans += [((1 << 29) - 2, 1 << 29), ((1 << 29) - 1, 1 << 29)]
    raw = check(pp, ctx, tx.join([line(b, e) for b, e in spans]), preset, full=True)
    R = tx.parse_tbi(raw)["refs"][0]
    assert {585, 73, 9, 1, 0} <= set(R["bins"]) and 37448 in R["bins"] and len(R["linear"]) == 32768
    if preset == BED:
        refused(pp, ctx, tx.join([line(5, 6), tx.bed_line(b"ctg", 7, (1 << 29) + 1), line(9, 10)]), BED, tx.LIMIT, 1)
        refused(pp, ctx, tx.join([tx.bed_line(b"ctg", (1 << 29) + 1, (1 << 29) + 1)]), BED, tx.LIMIT, 0)
        refused(pp, ctx, tx.join([tx.bed_line(b"ctg", 1, 9_999_999_999)]), BED, tx.LIMIT, 0)
    else:
        refused(pp, ctx, tx.join([line(5, 6), tx.vcf_line(b"ctg", 1 << 29, b"AC"), line(9, 10)]), VCF, tx.LIMIT, 1)
        refused(pp, ctx, tx.join([tx.vcf_line(b"ctg", 9_999_999_999)]), VCF, tx.LIMIT, 0)


def test_end_equal_to_begin_and_equal_begins(pp, ctx):
    lines = [tx.bed_line(b"c", 4, 4), tx.bed_line(b"c", 4, 4, b"again"), tx.bed_line(b"c", 4, 9), tx.bed_line(b"c", 16384, 16384), tx.bed_line(b"c", 16384, 16385)]
    R = tx.parse_tbi(check(pp, ctx, tx.join(lines), BED))["refs"][0]
    assert sorted(R["bins"]) == [4681, 4682, tx.PSEUDO_BIN] and len(R["linear"]) == 2
    check(pp, ctx, tx.join([tx.vcf_line(b"c", 5)] * 70), VCF)


def test_names_of_every_length_many_names_and_one_long_run(pp, ctx):
    names = [bytes([65 + k % 26]) * k for k in range(1, 41)]
    for preset in (VCF, BED):
        t = tx.parse_tbi(check(pp, ctx, tx.join([ln for nm in names for ln in sorted_lines(preset, 3, nm)]), preset))
        assert t["names"] == names
        many = [b"s%03d" % k for k in range(300)]                      # one line each: the name runs cross the wave and the workgroup
        t = tx.parse_tbi(check(pp, ctx, tx.join([ln for nm in many for ln in sorted_lines(preset, 1, nm)]), preset, full=True))
        assert t["names"] == many
        t = tx.parse_tbi(check(pp, ctx, tx.join(sorted_lines(preset, 5000, b"one", step=40, span=50) + sorted_lines(preset, 2, b"two")), preset))
        assert t["names"] == [b"one", b"two"] and t["refs"][0]["bins"][tx.PSEUDO_BIN][1] == (5000, 0) and len(t["refs"][0]["linear"]) == 13
    # names that differ in their last byte only, beyond eight bytes, and a name that is the front of the next
    near = [b"contig_0001", b"contig_0002", b"contig_000", b"contig_00021", b"c", b"cc", b"contig_0001x"]
    assert tx.parse_tbi(check(pp, ctx, tx.join([tx.bed_line(nm, 1, 2) for nm in near]), BED))["names"] == near


def test_a_long_line_over_later_starts_where_the_linear_minimum_matters(pp, ctx):
    lines = [tx.bed_line(b"c", 100, 101), tx.bed_line(b"c", 200, 5 * 16384 + 7, b"long"), tx.bed_line(b"c", 16384 + 5, 16384 + 9), tx.bed_line(b"c", 3 * 16384, 3 * 16384 + 1),
             tx.bed_line(b"c", 7 * 16384, 7 * 16384 + 1), tx.bed_line(b"c", 7 * 16384, 9 * 16384)]
    raw = check(pp, ctx, tx.join(lines), BED, full=True)
    lin = tx.parse_tbi(raw)["refs"][0]["linear"]
    second = tx.voffset(len(lines[0]) + 1, tx.level0_blk_off(100))
    assert len(lin) == 9 and lin[1:6] == [lin[1]] * 5 and lin[1] & 0xFFFF == second & 0xFFFF and lin[6] == lin[7], "window 6 is untouched: it takes window 7's"
    vcf = [tx.vcf_line(b"c", 101), tx.vcf_line(b"c", 201, b"A" * 40_000, b"<DEL>"), tx.vcf_line(b"c", 16390), tx.vcf_line(b"c", 60_000)]
    check(pp, ctx, tx.join(vcf), VCF)


@pytest.mark.parametrize("preset", [VCF, BED])
def test_random_texts(pp, ctx, preset):
    for seed in range(20):
        check(pp, ctx, tx.random_text(preset, seed, n_lines=400 + 37 * seed, n_names=1 + seed % 5), preset, full=seed < 2)


@pytest.mark.parametrize("preset", [VCF, BED])
def test_a_device_text_at_every_alignment_that_ends_where_its_allocation_ends(pp, ctx, preset):
    lines = sorted_lines(preset, 150) + ([tx.vcf_line(b"ctg", 5000, b"A" * 100), tx.vcf_line(b"ctg", 5001, b"C" * 61)] if preset == VCF else
                                         [tx.bed_line(b"ctg", 5000, 5001, b"z" * 100), tx.bed_line(b"ctg", 5001, 5002)])
    junk = b"\t12\t34\n56\t\t78\nctg\t1\t2\t\n" * 8
    for last_newline in (True, False):
        text = tx.join(lines, last_newline)
        flat = tx.level0_blk_off(len(text))
        want = tx.tbi_raw(text, preset, flat)
        for skip in range(16):
            dev, keep = on_device(text, skip)
            assert pp.tabix_index(ctx, dev, preset, flat, pp.MEM_DEVICE)[1] == want, (skip, "the allocation ends with the text")
            dev, keep2 = on_device(text, skip, junk)
            assert pp.tabix_index(ctx, dev, preset, flat, pp.MEM_DEVICE)[1] == want, (skip, "tabs, digits and newlines behind the text")
            del keep, keep2
    short = b"c\t1\t2" if preset == BED else b"c\t1\t.\tA\t"             # a text shorter than any wide load
    for skip in range(16):
        dev, keep = on_device(short, skip)
        assert pp.tabix_index(ctx, dev, preset, [0, 30], pp.MEM_DEVICE)[1] == tx.tbi_raw(short, preset, [0, 30])
        del keep


def test_every_refusal_with_its_line(pp, ctx):
    ok_b, ok_v = b"c\t1\t2\n", tx.vcf_line(b"c", 7) + b"\n"
    for bad in (b"\n", b"\t1\t2\n", b"c\t1\n", b"c\n", b"c\t1x\t2\n", b"c\t\t2\n", b"c\t1\t\n", b"c\t1\t-2\n", b"c\t12345678901\t12345678902\n", b"c\t5\t4\n",
                b"c\t0\t3\n", b"c\t1\t2 \n", b"c" * 100 + b"\n", b"c\t1\t" + b"7" * 80 + b"\n", b"c" * 70 + b"\t1\n"):
        refused(pp, ctx, b"#m\n" + ok_b + bad + ok_b, BED, tx.ARG, 2)
    for bad in (b"\n", b"\t1\t.\tA\tC\n", b"c\t9\t.\tA\n", b"c\t9\n", b"c\t0\t.\tA\tC\n", b"c\t9\t.\t\tC\n", b"c\t+9\t.\tA\tC\n", b"c\t6\t.\tA\tC\n",
                b"c\t9\t.\t" + b"A" * 5000 + b"\n", b"c\t9\t" + b"i" * 5000 + b"\t\tC\n", b"c\t9x\t.\t" + b"A" * 5000 + b"\tC\n"):
        refused(pp, ctx, b"##m\n#n\n" + ok_v + bad + ok_v, VCF, tx.ARG, 3)
    refused(pp, ctx, ok_b + b"c\t1", BED, tx.ARG, 1)                   # the last line, without its newline
    refused(pp, ctx, b"a\t1\t2\nb\t1\t2\n#x\na\t5\t6\n", BED, tx.ARG, 3)  # a name that comes back
    refused(pp, ctx, b"a\t1\t2\nb\t1\t2\na\t5\t6\nb\t0\tx\n", BED, tx.ARG, 2)  # the first of two offenders, the host's in front of the device's
    refused(pp, ctx, b"a\t1\t2\nb\t1\tx\na\t5\t6\n", BED, tx.ARG, 1)   # ... and the device's in front of the host's
    refused(pp, ctx, b"a\t1\t2\na\t1\tx\na\t0\t6\n\n", BED, tx.ARG, 1)
    many = [b"c\t%d\t%d" % (i, i + 1) for i in range(3000)]
    many[2900], many[1500], many[1501] = b"c\t5\t6", b"c\tx\t6", b""
    refused(pp, ctx, tx.join(many), BED, tx.ARG, 1500)
    text = ok_b * 3
    flat = tx.level0_blk_off(len(text))
    refused(pp, ctx, text, 2, tx.ARG, None)
    refused(pp, ctx, text, -1, tx.ARG, None)
    refused(pp, ctx, text, BED, tx.ARG, None, flat + [200_000])
    refused(pp, ctx, text, BED, tx.ARG, None, flat[:1])
    refused(pp, ctx, text, BED, tx.LIMIT, None, [0, 1 << 48])
    refused(pp, ctx, text, BED, tx.LIMIT, None, [1 << 48, 5])
    for args in ((None, 5, 0, BED, flat, 1, 0), (text, len(text), 2, BED, flat, 1, 0), (text, len(text), 0, BED, None, 1, 0), (text, len(text), 0, BED, flat, 1, 2)):
        import ctypes as C
        t, n, mem, preset, table, n_blk, blk_mem = args
        out, bad = pp.Bytes(), C.c_uint64(0)
        arr = None if table is None else np.ascontiguousarray(table, np.uint64)
        rc = pp.lib().pp_tabix_index(ctx._h, t, n, mem, preset, None if arr is None else arr.ctypes.data, n_blk, blk_mem, C.byref(out), None, C.byref(bad))
        assert rc == pp.ERR_ARG and not out.data, args
    assert pp.lib().pp_tabix_index(ctx._h, text, len(text), 0, BED, np.ascontiguousarray(flat, np.uint64).ctypes.data, 1, 0, None, None, None) == pp.ERR_ARG


def test_call_after_call_on_one_context(pp, ctx):
    a, b = tx.random_text(VCF, 3), tx.random_text(BED, 4, n_lines=900)
    first = [check(pp, ctx, a, VCF), check(pp, ctx, b, BED)]
    refused(pp, ctx, b"c\t5\t4\n", BED, tx.ARG, 0)
    check(pp, ctx, b"", BED)
    refused(pp, ctx, b"a\t1\t2\nb\t1\t2\na\t5\t6\n", BED, tx.ARG, 2)
    assert [check(pp, ctx, a, VCF), check(pp, ctx, b, BED)] == first
