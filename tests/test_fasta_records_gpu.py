"""pp_fasta_records (pp_fasta.hip) against tests/fasta_model.py's parse, byte for byte -- names, descriptions, offsets, bases -- with the
text in host memory and in device memory; a text the model refuses is refused with the model's code, line and words.  The model is pinned
on the CPU (tests/test_fasta_model_cpu.py).  The shapes are built to the byte around the kernels' seams, from fasta_geometry(): L bytes per
lane, T per tile, W per workgroup; a few multiples of W at the most.  Nothing here depends on a fault.  Needs an MI355X: `-m gpu`."""
import numpy as np
import pytest

import fasta_model as fm

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
    lane, tile, group = pp.fasta_geometry()
    assert lane == 16 and tile % lane == 0 and group % tile == 0 and group >= 2 * tile
    return tile, group


# ---- texts ----------------------------------------------------------------------------------------------------------------------
def bases(n, seed):
    return np.random.RandomState(seed).choice(np.frombuffer(b"ACGTacgtNnRy", np.uint8), n).tobytes()


def body(p, tag=b"c"):
    """a valid FASTA text of exactly p bytes: one header, lines of 60 columns, a final newline"""
    head = b">" + tag + b" the filler\n"
    r = p - len(head)
    assert r >= 2, p
    out, seed = [head], len(tag) * 7919 + p
    while r > 64:
        out.append(bases(60, seed + r) + b"\n")
        r -= 61
    out.append(bases(r - 1, seed) + b"\n")
    t = b"".join(out)
    assert len(t) == p
    return t


def mixed(n_lines, seed):
    """a valid text of many line forms: LF and CRLF ends, empty lines, a lone CR inside a line, headers with and without descriptions,
    unnamed headers in front of a header, lower case, blanks"""
    r = np.random.RandomState(seed)
    out, k, open_ = [], 0, False
    for _ in range(n_lines):
        end = b"\r\n" if r.rand() < 0.4 else b"\n"
        x = r.rand()
        if not open_ or x < 0.08:
            if open_ and x < 0.03:
                out.append(b">" + [b"", b" d", b"\xe2\x80\x83d", b"\xc2\xa0"][r.randint(4)] + end)
                out.append(b"\n" * r.randint(3))
            out.append(b">m%d" % k + [b"", b" desc", b"\xe3\x80\x80wide", b"\tx y"][r.randint(4)] + end)
            out.append(bases(1 + r.randint(90), seed + k) + end)
            k, open_ = k + 1, True
        elif x < 0.2:
            out.append(end)
        elif x < 0.25:
            out.append(b"AC\rG T" + end)
        else:
            out.append(bases(1 + r.randint(120), seed * 31 + len(out)) + end)
    return b"".join(out)


# ---- the device against the model ---------------------------------------------------------------------------------------------------
def on_device(whole, skip=0):
    """a device copy of `whole` in an allocation of its length; the text begins `skip` bytes into it"""
    import torch
    dev = torch.device("cuda:0")
    t = torch.from_numpy(np.frombuffer(bytes(whole), np.uint8).copy()).to(dev) if len(whole) else torch.zeros(1, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    assert t.data_ptr() % 16 == 0
    return t.data_ptr() + skip, t


def parsed(pp, ctx, whole, lo, n, mem):
    """FastaRecords on whole[lo : lo + n], which lies in memory as it is: what surrounds the text surrounds it there, too"""
    if mem == pp.MEM_HOST:
        return pp.FastaRecords(ctx, np.frombuffer(bytes(whole), np.uint8)[lo:lo + n], mem)
    ptr, keep = on_device(whole, lo)
    rec = pp.FastaRecords(ctx, (ptr, n), mem)
    del keep  # (the caller's text may go when the call has returned)
    return rec


def modelled(text):
    try:
        return fm.parse(text)
    except fm.FastaError as e:
        return e


def check(pp, ctx, text, whole=None, lo=0, mems=None, want=None):
    whole = text if whole is None else whole
    assert bytes(whole[lo:lo + len(text)]) == bytes(text)
    want = modelled(text) if want is None else want
    for mem in mems or (pp.MEM_HOST, pp.MEM_DEVICE):
        if isinstance(want, fm.FastaError):
            with pytest.raises(pp.PolypolishError) as e:
                parsed(pp, ctx, whole, lo, len(text), mem)
            assert (e.value.code, e.value.bad_record, fm.words_of(e.value.msg, "text")) == (want.code, want.bad_line, want.words), (mem, e.value)
            continue
        rec = parsed(pp, ctx, whole, lo, len(text), mem)
        try:
            names, descs, off, b = want
            assert (rec.names, rec.descriptions, rec.offsets.tolist(), rec.n_contigs, rec.n_bases) == (names, descs, off, len(names), len(b)), mem
            got = rec.host()["bases"]
            assert got == b, (mem, "first difference at", next((i for i in range(min(len(got), len(b))) if got[i] != b[i]), None))
        finally:
            rec.close()
    return want


@pytest.mark.parametrize("name", sorted(fm.CASES))
def test_the_models_cases(pp, ctx, name):
    """every line form and every refusal the CPU test pins, among them a text of headers only, the empty text and one of newlines only"""
    check(pp, ctx, fm.CASES[name])


def seams(geo):
    T, W = geo
    return {"tile": T, "group": W, "second_group": 2 * W, "tile_in_group": W + 3 * T}


@pytest.mark.parametrize("where", ["tile", "group", "second_group", "tile_in_group"])
def test_line_ends_and_headers_at_the_seams(pp, ctx, geo, where):
    S = seams(geo)[where]
    tail = body(300, b"tail")
    for text in (body(S) + b"ACGT\n" + tail,                                  # "\n" the last byte in front of the seam
                 body(S - 4) + b"ACGT\nTT\n" + tail,                          # "\n" the first byte behind it
                 body(S - 5) + b"ACGT\r\nTT\r\n" + tail,                      # "\r" | "\n"
                 body(S - 5) + b"ACGT\r\r\nTT\n" + tail,                      # "\r" | "\r\n": the first one is a base
                 body(S - 4) + b"ACG\rTT\n" + tail,                           # a lone "\r" the last byte in front of the seam: a base
                 body(S) + b">x d\nAC\n" + tail,                              # ">" the first byte behind the seam
                 body(S - 1) + b">x d\nAC\n" + tail,                          # ">" the last byte in front of it
                 body(S - 1) + b">\n>y\nAC\n" + tail,                         # ... of an unnamed header, its "\n" behind the seam
                 body(S - 2) + b">\xe2\x80\x83d\n>y\nAC\n" + tail,            # ... unnamed by a three-byte blank cut by the seam
                 body(S - 3) + b">\xe2\x80\x83d\n>y\nAC\n" + tail,
                 body(S - 2) + b">\xc2\xa0d\n>y\nAC\n" + tail,                # ... by a two-byte blank cut by the seam
                 body(S - 2) + b">\xe2\x80\x8bd\nAC\n" + tail,                # U+200B is no blank: a name
                 body(S - 1) + b">\r\nAC\n" + tail,                           # unnamed, then bases: refused
                 body(S - 10) + b">name " + b"d" * 30 + b"\nAC\n" + tail,     # a header line across the seam
                 body(S - 3) + b">name\tdescr\r\nAC\n" + tail,                # ... its name across it
                 body(S - 1) + b"A>\n" + tail,                                # ">" behind the seam inside a sequence line
                 body(S - 2) + b"\n\n\n\nAC\n" + tail):                       # empty lines around the seam
        check(pp, ctx, text)


def test_lines_longer_than_a_tile(pp, ctx, geo):
    T, W = geo
    long = bases(3 * W + 1, 5)
    check(pp, ctx, b">a\n" + long + b"\n>b\nAC\n")                                      # tiles and a whole workgroup with no newline
    check(pp, ctx, b">" + b"h" * (T - 3) + b"\n" + long + b"\r\n>b\nAC\n")              # ... behind a header that ends one byte before a seam
    check(pp, ctx, b">" + b"h" * (W - 3) + b"\n" + long)                                # ... before a workgroup's, no final newline
    check(pp, ctx, b">n " + b"d" * (T + 100) + b"\nACGT\n")                             # a header line longer than a tile
    check(pp, ctx, b">" + b"n" * (T + 5) + b"\nACGT\n>" + b"m" * (W + T) + b" d\nAC\n")  # ... than a workgroup, all of it the name
    check(pp, ctx, b">a\nAC\n> " + b"d" * (W + T + 7) + b"\n>b\nGT\n")                  # ... unnamed: dropped


def test_text_lengths(pp, ctx, geo):
    T, W = geo
    check(pp, ctx, b"")
    for one in (b"A", b">", b"\n", b"\r", b"\xff"):
        check(pp, ctx, one)
    for n in (T - 1, T, T + 1, W - 1, W, W + 1, 2 * W - 1, 2 * W, 2 * W + 1):
        check(pp, ctx, body(n))                  # a final newline the text's last byte
        check(pp, ctx, body(n - 1) + b"a")       # none
        check(pp, ctx, body(n - 1) + b"\r")      # a "\r" the text's last byte: dropped
    check(pp, ctx, b">a\n>b x\n>c\n" * 2000)     # headers only, across tiles: refused behind the walk
    check(pp, ctx, b">\n> x\n" * 3000)


@pytest.mark.parametrize("part", range(4))
def test_no_final_newline_at_every_offset_of_the_last_tile(pp, ctx, geo, part):
    """one text in memory, cut at every offset of its second tile: what lies behind the cut is the rest of the text"""
    T, _ = geo
    whole = body(T - 7, b"first") + mixed(260, 11)
    assert len(whole) >= 2 * T
    ptr, keep = on_device(whole)
    host = np.frombuffer(whole, np.uint8)
    for n in range(T + part * (T // 4), T + (part + 1) * (T // 4)):
        want = modelled(whole[:n])
        for mem, data in ((pp.MEM_HOST, host[:n]), (pp.MEM_DEVICE, (ptr, n))):
            if isinstance(want, fm.FastaError):
                with pytest.raises(pp.PolypolishError) as e:
                    pp.FastaRecords(ctx, data, mem)
                assert (e.value.code, e.value.bad_record, fm.words_of(e.value.msg, "text")) == (want.code, want.bad_line, want.words), (n, mem)
                continue
            rec = pp.FastaRecords(ctx, data, mem)
            try:
                assert (rec.names, rec.descriptions, rec.offsets.tolist()) == want[:3], (n, mem)
                assert rec.host()["bases"] == want[3], (n, mem)
            finally:
                rec.close()
    del keep


def test_line_count_extremes(pp, ctx):
    check(pp, ctx, b">a\n" + b"A\n" * 10000)
    check(pp, ctx, b">a\n" + b"".join(bytes([c]) + b"\n" for c in bases(10000, 3)))
    check(pp, ctx, b">a\nACGT\n" + b"\n" * 5000 + b"TTGA\n")
    check(pp, ctx, b">a\nACGT\r\n" + b"\r\n" * 5000 + b"TTGA\r\n")


def test_device_text_at_every_alignment(pp, ctx, geo):
    """the first byte of a device text 0 to 15 bytes behind a multiple of 16: the seams move with it, the bytes in front of the text and
    behind it are hostile, and the allocation ends where the text ends"""
    T, W = geo
    text = body(T - 3, b"head") + mixed(1500, 23)
    assert len(text) > W + T
    want = modelled(text)
    assert not isinstance(want, fm.FastaError)
    for a in range(16):
        check(pp, ctx, text, whole=b">\n\xff>x\nAC\n\xffAC\n>\xff\n"[:a] + text, lo=a, mems=(pp.MEM_DEVICE,), want=want)
        short = text[:W + 5 - a]  # ... and the text's last byte at every place in its 16
        check(pp, ctx, short, whole=b"\n" * a + short, lo=a, mems=(pp.MEM_DEVICE,))


def test_hostile_bytes_behind_the_text(pp, ctx, geo):
    T, W = geo
    for n in (T - 20, T, W - 1, W + T + 9):
        text = body(n)
        for behind in (b">", b"\n", b"\xff", b">x\n\xff\n>" * 40, b"\nAC\n", b"\xc3\xa9\n"):
            check(pp, ctx, text, whole=text + behind)
            check(pp, ctx, text[:-1], whole=text[:-1] + behind)  # no final newline: the bytes behind would continue the line
            check(pp, ctx, text[:-1] + b"\r", whole=text[:-1] + b"\r" + behind)


REFUSED = {  # a line that is refused on its own -> (code, words); each begins a line and ends one
    "headless": (b">\nAC\n", 1, fm.QUIT, fm.NOT_FORMATTED),
    "header_not_utf8": (b">h\xff\nAC\n", 0, fm.QUIT, fm.UNABLE),
    "sequence_not_utf8": (b"AC\xffGT\n", 0, fm.QUIT, fm.UNABLE),
    "non_ascii": (b"AC\xc3\xa9GT\n", 0, fm.LIMIT, fm.NOT_ASCII),
}


def placed(geo):
    T, W = geo
    return {"first": 61, "middle": W + T + 17, "last": 2 * W + 5 * T - 40}


@pytest.mark.parametrize("kind", sorted(REFUSED))
def test_every_refusal_in_the_first_a_middle_and_the_last_tile(pp, ctx, geo, kind):
    T, W = geo
    total = 2 * W + 5 * T
    bad, line_in, code, words = REFUSED[kind]
    for where, p in placed(geo).items():
        text = body(p, b"front") + bad
        text += body(total - len(text), b"back") if total - len(text) > 40 else b""
        want = check(pp, ctx, text)
        assert isinstance(want, fm.FastaError) and (want.code, want.words) == (code, words), where
        assert want.bad_line == text[:p].count(b"\n") + line_in
    if kind == "headless":  # ... and with no header at all in front
        check(pp, ctx, b"ACGT\n" + body(total, b"back"))
        check(pp, ctx, b"\n\n\r\nACGT\n" + body(total, b"back"))


def test_refusals_behind_the_walk(pp, ctx, geo):
    """the empty contig and the second of a name in the first, a middle and the last tile"""
    T, W = geo
    total = 2 * W + 5 * T
    for where, p in placed(geo).items():
        for extra, w in ((b">e\n", fm.EMPTY_SEQUENCE), (b">front again\nAC\n", fm.DUPLICATED)):
            text = body(p, b"front") + extra + body(total - p, b"back")
            want = check(pp, ctx, text)
            assert isinstance(want, fm.FastaError) and want.words == w and want.bad_line is None


@pytest.mark.parametrize("first", sorted(REFUSED))
@pytest.mark.parametrize("second", sorted(REFUSED))
def test_the_earlier_of_two_refusals_wins(pp, ctx, geo, first, second):
    if first == second:
        return
    T, W = geo
    a, b = REFUSED[first], REFUSED[second]
    for gap in (30, T + 3, W + 77):  # in one tile, in two tiles, in two workgroups
        text = body(W - 200, b"front") + a[0] + body(gap, b"mid") + b[0] + body(100, b"back")
        want = check(pp, ctx, text)
        assert isinstance(want, fm.FastaError) and (want.code, want.words) == (a[2], a[3])


def test_non_ascii_bytes_at_a_seam(pp, ctx, geo):
    T, W = geo
    for S in (T, W):
        for text in (body(S - 3) + b"AC\xc3\xa9\nAC\n",       # the byte the last one in front of the seam, its second behind it
                     body(S - 2) + b"AC\xc3\xa9\nAC\n",       # the first byte behind the seam
                     body(S - 4) + b"AC\xc3\xa9\nAC\n",       # the last byte in front of it
                     body(S - 1) + b"\xff\n",                 # not UTF-8, the last byte of a tile
                     body(S) + b"\xff\n",                     # ... the first
                     body(S - 2) + b">h\xc3\xa9 d\nAC\n"):    # in a header: taken
            check(pp, ctx, text)


def test_the_same_call_twice_gives_the_same_bytes(pp, ctx, geo):
    T, W = geo
    text = mixed(4000, 7)
    assert len(text) > 2 * W
    ptr, keep = on_device(text)
    got = []
    for _ in range(2):
        rec = pp.FastaRecords(ctx, (ptr, len(text)), pp.MEM_DEVICE)
        got.append((rec.host()["bases"], rec.names, rec.descriptions, rec.offsets.tolist()))
        rec.close()
    assert got[0] == got[1] and got[0][0] == fm.parse(text)[3]
    del keep


def test_arguments(pp, ctx):
    import ctypes as C
    L = pp.lib()
    out, bad = C.c_void_p(), C.c_uint64(0)
    buf = np.frombuffer(b">a\nAC\n", np.uint8)
    assert L.pp_fasta_records(ctx._h, buf.ctypes.data, 6, pp.MEM_HOST, None, C.byref(bad)) == pp.ERR_ARG
    assert L.pp_fasta_records(ctx._h, buf.ctypes.data, 6, 2, C.byref(out), C.byref(bad)) == pp.ERR_ARG and not out.value  # PP_MEM_PEER
    assert L.pp_fasta_records(ctx._h, None, 6, pp.MEM_HOST, C.byref(out), C.byref(bad)) == pp.ERR_ARG and not out.value
    assert L.pp_fasta_records(ctx._h, buf.ctypes.data, 1 << 40, pp.MEM_HOST, C.byref(out), C.byref(bad)) == pp.ERR_LIMIT and not out.value
    assert L.pp_fasta_records(ctx._h, buf.ctypes.data, 6, pp.MEM_HOST, C.byref(out), None) == 0 and out.value  # bad_line may be NULL
    L.pp_fasta_free(out)
    rec = pp.FastaRecords(ctx, b">a\nAC\n")
    with pytest.raises(pp.PolypolishError):
        rec.kernel_ms()  # the context had no profiling on
    rec.close()
    ctx.set_profiling(True)
    try:
        rec = pp.FastaRecords(ctx, b">a\nAC\n")
        assert rec.kernel_ms() >= 0 and set(rec.stage_ms()) == {"copy", "sums", "place", "headers"}
        rec.close()
    finally:
        ctx.set_profiling(False)
