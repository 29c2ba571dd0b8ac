"""pp_sam_tagged / pp_sam_tagged_records (pp_sam_out.hip) against the plain model (tests/sam_tag_model.py, pinned to pp_filter_write_text
and to the oracle by tests/test_sam_tag_model_cpu.py), byte for byte, with the text in host and in device memory: every line length
around the store width, a failing line's end at every residue of the store width in source and destination, the output tile's seams
(a tile boundary at each byte of the tag and the newline, between the source's "\\r" and "\\n", inside a FLAG column), lines longer than
tiles, the seams of pass A's workgroups, a mixed text, hostile bytes behind a device text, the twin call, determinism, the contract's
errors and pp_sam_out_write.  None of these inputs is out of bounds: the hostile bytes lie inside the test's own allocation.
Needs an MI355X: `-m gpu`."""
import ctypes as C
import os

import numpy as np
import pytest

import sam_tag_model as sm

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
def geometry(pp):
    lines, tile, store = pp.sam_out_geometry()
    assert (lines, tile, store) == (1024, 16384, 16), "the header's geometry"
    return lines, tile, store


def on_device(data, lead=0):
    """`data` in device memory behind `lead` other bytes -> (the tensor to keep, the device address of data[0])"""
    import torch
    t = torch.from_numpy(np.frombuffer(b"\xa5" * lead + bytes(data) + b"\x00", np.uint8).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return t, t.data_ptr() + lead


def device_tagged(pp, ctx, text, v, mem, lead=0, behind=b""):
    """-> (bytes, counts) of SamOut.tagged; MEM_DEVICE: the text at `lead` bytes into its allocation, `behind` following it"""
    if mem == pp.MEM_HOST:
        o = pp.SamOut.tagged(ctx, text, v)
    else:
        keep, at = on_device(bytes(text) + behind, lead)
        o = pp.SamOut.tagged(ctx, (at, len(text)), v, mem=pp.MEM_DEVICE)
        del keep
    try:
        assert o.dev()[1] == o.n_bytes and (o.n_bytes == 0 or o.bytes_ptr % 16 == 0)
        return o.bytes(), o.counts()
    finally:
        o.close()


def check(pp, ctx, text, v, lead=1, mems=None):
    want = sm.tagged(text, v)
    for mem in mems or (pp.MEM_HOST, pp.MEM_DEVICE):
        got, counts = device_tagged(pp, ctx, text, v, mem, lead)
        assert got == want[0], (mem, len(text), first_difference(got, want[0]))
        assert counts == want[1:], mem
    return want[0]


def first_difference(a, b):
    n = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    return len(a), len(b), n, a[max(0, n - 20):n + 20], b[max(0, n - 20):n + 20]


def verdict_sets(n):
    return [np.ones(n, np.uint8), np.zeros(n, np.uint8), (np.arange(n) % 2).astype(np.uint8)]


def line_of(length, i=0):
    """an aligned record whose content has exactly `length` bytes (>= 3: "q\\t0"), else a line that is none"""
    if length < 3:
        return b"@" * length
    name = (b"r%d" % i)[:length - 2]
    return name + b"\t0" + (b"\t" + b"ACGT" * length)[:length - len(name) - 2]


def fill(total, seed=0):
    """(text, verdicts) whose output -- every record passing -- has exactly `total` bytes: header lines, empty lines and aligned records"""
    rng = np.random.default_rng(seed + total)
    out, v = [], []
    while total:
        m = int(min(total, rng.integers(1, 240)))
        line = line_of(m - 1, len(out)) if rng.integers(0, 3) else (b"@CO\t" + b"c" * m)[:m - 1]
        v += [1] * sm.aligned(line)
        out.append(line + b"\n")
        total -= m
    return b"".join(out), v


LENGTHS = list(range(0, 81)) + [250, 251, 255, 256, 257, 258, 266, 267, 268]      # ... around 16, 64 and 256 bytes, with and without the tag


@pytest.mark.parametrize("verdicts", ["pass", "fail", "alternate"])
def test_texts_of_one_line_length(pp, ctx, verdicts):
    for length in LENGTHS:
        n_lines = 37 if length <= 80 else 9
        text = b"".join(line_of(length, i) + b"\n" for i in range(n_lines))
        n = sm.n_aligned(text)
        assert n == (n_lines if length >= 3 else 0)
        v = verdict_sets(n)[("pass", "fail", "alternate").index(verdicts)]
        check(pp, ctx, text, v, lead=length % 16)
        check(pp, ctx, text[:-1], v, lead=(length + 5) % 16, mems=(pp.MEM_DEVICE,))       # ... and the last line without its newline


def test_a_failing_line_s_end_at_every_residue_of_the_store_width(pp, ctx, geometry):
    store = geometry[2]
    seen = set()
    for h in range(store):              # a header line in front: moves source and destination together ...
        for k in range(store):          # ... as does the line itself
            lead = h                    # the text's place in its allocation: moves the source alone
            text = b"@" + b"h" * h + b"\n" + line_of(40 + k, 1) + b"\n" + line_of(33, 2) + b"\r\n" + line_of(50, 3) + b"\n" + line_of(21 + k, 4)
            out = check(pp, ctx, text, [0, 1, 0, 0], lead=lead, mems=(pp.MEM_DEVICE,))
            end_src, end_dst = h + 2 + 40 + k, out.index(sm.TAG)
            seen.add(((lead + end_src) % store, end_dst % store))
            if k == h:
                check(pp, ctx, text, [0, 1, 0, 0], mems=(pp.MEM_HOST,))
    assert len(seen) == store * store, "every residue of the source against every residue of the destination"


def test_total_output_around_the_tile(pp, ctx, geometry):
    tile = geometry[1]
    for total in (tile - 1, tile, tile + 1, 3 * tile - 1, 3 * tile + 1):
        text, v = fill(total)
        assert len(check(pp, ctx, text, v)) == total
        text, v = fill(total - 41, seed=1)      # ... with the last record failing: its tag and newline are the output's last bytes
        assert len(check(pp, ctx, text + line_of(30) + b"\n", v + [0])) == total
        assert len(check(pp, ctx, text + line_of(30) + b"\r", v + [0])) == total


def test_a_tile_boundary_at_every_byte_of_the_tag_and_the_newline(pp, ctx, geometry):
    tile = geometry[1]
    after = line_of(70, 8) + b"\n" + line_of(25, 9) + b"\n"
    for cut in range(12):               # `cut` bytes of "\tZP:Z:fail\n" lie in front of the boundary
        head, v = fill(2 * tile - cut - 45, seed=cut)
        text = head + line_of(45, 7) + b"\n" + after
        out = check(pp, ctx, text, v + [0, 1, 0], lead=cut)
        assert out.index(sm.TAG + b"\n", 2 * tile - 60) == 2 * tile - cut
        check(pp, ctx, text, v + [1, 0, 1], lead=cut, mems=(pp.MEM_DEVICE,))


def test_a_tile_boundary_between_cr_and_lf_and_inside_a_flag_column(pp, ctx, geometry):
    tile = geometry[1]
    for at in (-1, 0, 1):               # the output's "\n" of a "\r\n" line at tile - 1, tile, tile + 1
        head, v = fill(tile + at - 45)
        text = head + line_of(45, 7) + b"\r\n" + line_of(30, 8) + b"\r\n"
        for tail in ([1, 1], [1, 0], [0, 1]):
            out = check(pp, ctx, text, v + tail)
            if tail[0]:
                assert out[tile + at] == 10 and text[tile + at:tile + at + 2] == b"\r\n"
    for inside in range(1, 12):         # the boundary `inside` bytes into a line "read_name\t+16\t..."
        head, v = fill(tile - inside)
        line = b"read_name\t+16\tctg\t1\t60\t4M\t*\t0\t0\tACGT\tIIII\tNM:i:0"
        text = head + line + b"\n" + line.replace(b"+16", b"+4") + b"\n"
        for verdict in (0, 1):
            check(pp, ctx, text, v + [verdict])


def test_lines_longer_than_tiles(pp, ctx, geometry):
    tile = geometry[1]
    long_line = line_of(3 * tile + 77)
    short = [line_of(20, 1), b"@CO\tx", line_of(33, 2), b""]
    for text in (long_line, long_line + b"\n", long_line + b"\r\n", b"\n".join(short + [long_line] + short) + b"\n",
                 b"\n".join([long_line, long_line + b"\r", short[0]])):
        n = sm.n_aligned(text)
        for v in verdict_sets(n):
            check(pp, ctx, text, v, lead=3)
    check(pp, ctx, b"@" + long_line + b"\n" + b"no tab " * tile, None)


def test_newlines_only_and_header_lines_only(pp, ctx):
    assert check(pp, ctx, b"\n" * 3000, None) == b"\n" * 3000
    assert check(pp, ctx, b"\r\n" * 3000, None) == b"\n" * 3000
    for n in (2047, 2048, 2049, 2050, 20000):       # around the 2,048 line starts of a tile that pass B keeps at hand, and far beyond
        assert check(pp, ctx, b"\n" * n, None) == b"\n" * n
    tiny = b"".join((b"q\t0\n", b"\r\n", b"@\n", b"q\t+16")[i % 4] + (b"\n" if i % 4 == 3 else b"") for i in range(12000))
    for v in verdict_sets(6000):                    # ... and such tiles with records in them, tagged and not
        check(pp, ctx, tiny, v)
    assert check(pp, ctx, b"\n", None) == b"\n" and check(pp, ctx, b"x", None) == b"x\n"
    assert check(pp, ctx, b"", None) == b""
    header = b"".join(b"@SQ\tSN:contig_%d\tLN:%d\n" % (i, 1000 + i) for i in range(700))
    assert check(pp, ctx, header, None) == header
    assert check(pp, ctx, header[:-1], np.zeros(0, np.uint8)) == header


def test_line_counts_around_pass_a_s_workgroups(pp, ctx, geometry):
    per = geometry[0]
    for n_lines in (per - 1, per, per + 1, 2 * per - 1, 2 * per, 2 * per + 1):
        lines = [line_of(12 + i % 7, i) if i % 11 != 5 else (b"@CO\t%d" % i if i % 2 else b"u\t4\t*") for i in range(n_lines)]
        text = b"\n".join(lines) + b"\n"
        rank = np.cumsum([sm.aligned(ln) for ln in lines]) - 1      # the rank of line i, where it is aligned
        n = int(rank[-1]) + 1
        edge = [i for i in sorted({0, per - 2, per - 1, per, per + 1, 2 * per - 1, 2 * per, n_lines - 1}) if i < n_lines and sm.aligned(lines[i])]
        assert {0, n_lines - 1, min(per, n_lines) - 1} <= set(edge)
        only_edges, but_edges = np.ones(n, np.uint8), np.zeros(n, np.uint8)
        only_edges[rank[edge]] = 0      # a failing record first and last in a workgroup, every other record passing: the rank is carried over
        but_edges[rank[edge]] = 1
        for v in (only_edges, but_edges, (np.arange(n) % 3 == 0).astype(np.uint8)):
            check(pp, ctx, text, v)


@pytest.mark.parametrize("fraction", [0.02, 0.5])
def test_a_mixed_text(pp, ctx, fraction):
    text, n = sm.mixed_text(5000, 77)
    assert n == sm.n_aligned(text) and len(text) > 150_000
    v = (np.random.default_rng(5).random(n) >= fraction).astype(np.uint8)
    out = check(pp, ctx, text, v, lead=9)
    assert out.count(b"\n") == 5000 and 0 < int((v == 0).sum()) < n


def test_bytes_behind_a_device_text_change_nothing(pp, ctx):
    r = sm.record()
    hostile = [b"\n" + r + b"\n", b"\t0\t\n", b"4\tx\n", b"6789\n\xff\xff\n\n", b"\xff" * 40, b"\r\n\r\n", b"\t" * 40, b"0" * 40]
    texts = [r, r + b"\r", r + b"\n", r + b"\n" + b"q\t0", r + b"\n" + b"q\t", r + b"\n" + b"q", r + b"\n@", r + b"\n" + b"q\t1", b"q\t+", b"\r",
             r + b"\n" + r[:20], sm.mixed_text(300, 4)[0]]
    for i, text in enumerate(texts):
        n = sm.n_aligned(text)
        for v in verdict_sets(n)[:2]:
            want = sm.tagged(text, v)
            for lead in (0, 1 + i % 15):
                for behind in [b"\x00" * 64] + hostile:
                    got, counts = device_tagged(pp, ctx, text, v, pp.MEM_DEVICE, lead, behind)
                    assert got == want[0] and counts == want[1:], (text[-20:], behind)


def test_the_twin_call_on_a_decoded_text(pp, ctx):
    import sam_records_model as srm
    text = srm.count_text(2500)
    assert all(b < 0x80 for b in text)
    rec = pp.SamRecords(ctx, text)
    try:
        n = len(rec.zp)
        assert n == sm.n_aligned(text) and 1000 < n < rec.n_rec, "the decode and the copy number the aligned records alike"
        for v in verdict_sets(n) + [rec.zp]:
            twin = rec.tagged(v)
            try:
                assert twin.bytes() == check(pp, ctx, text, v, mems=(pp.MEM_HOST,)) and twin.counts() == sm.tagged(text, v)[1:]
            finally:
                twin.close()
        with pytest.raises(pp.PolypolishError) as e:
            rec.tagged(np.ones(n + 1, np.uint8))
        assert e.value.code == pp.ERR_ARG and f"{n + 1} verdicts for {n} aligned records" in str(e.value)
    finally:
        rec.close()
    empty = pp.SamRecords(ctx, b"")
    try:
        twin = empty.tagged(None)
        assert twin.bytes() == b"" and twin.counts() == (0, 0, 0)
        twin.close()
    finally:
        empty.close()


def test_two_calls_give_the_same_bytes(pp, ctx):
    text, n = sm.mixed_text(3000, 12)
    v = (np.arange(n) % 7 != 0).astype(np.uint8)
    first = device_tagged(pp, ctx, text, v, pp.MEM_DEVICE, 5)
    assert first == device_tagged(pp, ctx, text, v, pp.MEM_DEVICE, 5) == device_tagged(pp, ctx, text, v, pp.MEM_HOST)


def test_the_contract_s_errors_and_a_good_call_behind_each(pp, ctx):
    L = pp.lib()
    text, n = sm.mixed_text(200, 3)
    buf = np.frombuffer(text, np.uint8).copy()
    v = np.ones(n + 1, np.uint8)
    out = C.c_void_p()

    def refused(code, words, *args):
        out.value = 0xDEAD
        assert L.pp_sam_tagged(ctx._h, *args, C.byref(out)) == code
        assert not out.value, "no object"
        msg = L.pp_last_error(ctx._h).decode()
        for w in words:
            assert w in msg, (w, msg)
        check(pp, ctx, text, v[:n], mems=(pp.MEM_HOST,))       # the context serves the next call

    refused(pp.ERR_ARG, ["pp_sam_tagged", "host memory or memory of the context's device"], buf.ctypes.data, len(buf), pp.MEM_PEER, v.ctypes.data, n)
    refused(pp.ERR_ARG, ["null text"], None, len(buf), pp.MEM_HOST, v.ctypes.data, n)
    refused(pp.ERR_ARG, ["null pass", f"{n} aligned records"], buf.ctypes.data, len(buf), pp.MEM_HOST, None, n)
    for k in (n - 1, n + 1, 0):
        refused(pp.ERR_ARG, [f"{k} verdicts for {n} aligned records"], buf.ctypes.data, len(buf), pp.MEM_HOST, v.ctypes.data, k)
    refused(pp.ERR_ARG, ["1 verdicts for 0 aligned records"], None, 0, pp.MEM_HOST, v.ctypes.data, 1)
    refused(pp.ERR_ARG, ["3 verdicts for 0 aligned records"], buf.ctypes.data, 0, pp.MEM_HOST, v.ctypes.data, 3)
    refused(pp.ERR_LIMIT, ["2^40"], buf.ctypes.data, 1 << 40, pp.MEM_HOST, v.ctypes.data, n)     # (refused before a byte is read)
    assert L.pp_sam_tagged(ctx._h, buf.ctypes.data, len(buf), pp.MEM_HOST, v.ctypes.data, n, None) == pp.ERR_ARG
    assert "null argument" in L.pp_last_error(ctx._h).decode()
    assert L.pp_sam_tagged(None, buf.ctypes.data, len(buf), pp.MEM_HOST, v.ctypes.data, n, C.byref(out)) == pp.ERR_ARG
    out.value = 0xDEAD
    assert L.pp_sam_tagged_records(ctx._h, None, v.ctypes.data, n, C.byref(out)) == pp.ERR_ARG and not out.value
    assert L.pp_sam_tagged_records(ctx._h, None, v.ctypes.data, n, None) == pp.ERR_ARG
    # the accessors of no object
    dev, nb, a, b, c, ms = C.c_void_p(1), C.c_uint64(1), C.c_uint64(1), C.c_uint64(1), C.c_uint64(1), C.c_float()
    L.pp_sam_out_bytes(None, C.byref(dev), C.byref(nb))
    L.pp_sam_out_counts(None, C.byref(a), C.byref(b), C.byref(c))
    assert not dev.value and (nb.value, a.value, b.value, c.value) == (0, 0, 0, 0)
    assert L.pp_sam_out_write(None, b"/tmp/x") == pp.ERR_ARG and L.pp_sam_out_kernel_ms(None, C.byref(ms)) == pp.ERR_ARG
    L.pp_sam_out_free(None)
    check(pp, ctx, text, v[:n])


def test_write_and_the_times(pp, tmp_path):
    ctx = pp.Context(0)
    text, n = sm.mixed_text(2000, 21)
    v = (np.arange(n) % 4 != 1).astype(np.uint8)
    plain = pp.SamOut.tagged(ctx, text, v)
    try:
        with pytest.raises(pp.PolypolishError) as e:
            plain.kernel_ms()
        assert e.value.code == pp.ERR_ARG and "profiling" in str(e.value)
    finally:
        plain.close()
    ctx.set_profiling(True)
    o = pp.SamOut.tagged(ctx, text, v)
    try:
        path = os.path.join(str(tmp_path), "tagged.sam")
        o.write(path)
        assert open(path, "rb").read() == o.bytes() == sm.tagged(text, v)[0]
        with pytest.raises(pp.PolypolishError) as e:
            o.write(os.path.join(str(tmp_path), "no_such_directory", "tagged.sam"))
        assert e.value.code == pp.ERR_QUIT and "unable to write alignments to" in str(e.value) and "no_such_directory" in str(e.value)
        with pytest.raises(pp.PolypolishError) as e:
            o.write(str(tmp_path))      # a directory
        assert e.value.code == pp.ERR_QUIT and "unable to write alignments to" in str(e.value)
        stages = o.stage_ms()
        assert list(stages) == ["newline_index", "pass_a", "scans", "pass_b"] and all(t > 0 for t in stages.values())
        assert abs(o.kernel_ms() - sum(stages.values())) < 1e-3
        z = o.deflate()
        try:
            assert z.n_blocks == (o.n_bytes + 65279) // 65280
        finally:
            z.close()
    finally:
        o.close()
        ctx.close()
