"""pp_sam_bam / pp_sam_bam_records (pp_sam_bam.hip) against the plain model (tests/sam_bam_model.py, pinned by
tests/test_sam_bam_model_cpu.py), byte for byte, with the text in host and in device memory -- the device text at every offset 0 .. 15
of its allocation with hostile bytes behind it: line counts around the wave and the workgroup, SEQ and QNAME lengths around the
16-byte loads, CIGARs of no, one and 65,535 runs (a record longer than a tile, a line longer than the stage), aux integers at the
type limits, float forms, B arrays, line ends, every part of a record across a tile boundary of pass B, every refusal of the header's
table with its code and line, the first-in-file-order rule, the twin call, determinism and the stage times.  None of these inputs is
out of bounds: the hostile bytes lie inside the test's own allocation.  Needs an MI355X: `-m gpu`."""
import numpy as np
import pytest

import sam_bam_model as sb

pytestmark = pytest.mark.gpu

HEADER = b"@HD\tVN:1.6\r\n@SQ\tSN:c1\tLN:1000000\n@SQ\tSN:c2\tLN:500\n@PG\tID:x\n"
HOSTILE = b"\xff\t@\n\x80=\r\n" * 4


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
def tile(pp):
    lines, tile, store = pp.sam_bam_geometry()
    assert tile % store == 0 and tile >= 1024
    return tile


def line(qname=b"q", flag=0, rname=b"c1", pos=1, mapq=60, cigar=b"*", rnext=b"*", pnext=0, tlen=0, seq=b"*", qual=b"*", aux=()):
    cols = [qname, b"%d" % flag, rname, b"%d" % pos, b"%d" % mapq, cigar, rnext, b"%d" % pnext, b"%d" % tlen, seq, qual]
    return b"\t".join(cols + list(aux))


def mixed_line(i):
    """a record that changes with i: SEQ / QNAME lengths, QUAL or "*", CIGARs, aux fields, unmapped ones"""
    n = (i * 7) % 40
    seq = bytes(b"ACGTNacgtn=MRSVWYHKDB"[(i + k) % 21] for k in range(n)) or b"*"
    qual = b"*" if seq == b"*" or i % 3 == 0 else bytes(33 + (i + k) % 60 for k in range(n))
    aux = [b"NM:i:%d" % (i % 300), b"AS:i:-%d" % (i * 37), b"XS:f:%d.%d" % (i, i % 10), b"MD:Z:" + b"5A" * (i % 9)][: i % 5]
    if i % 11 == 5:
        return line(b"u%d" % i, 4, b"*", 0, 0, b"*", b"*", 0, 0, seq, qual, aux)
    cigar = b"*" if seq == b"*" else (b"%dM" % n if i % 2 else b"1S%dM2D1I" % max(n - 2, 1))
    return line(b"read%d" % i * (1 + i % 3), 16 * (i % 2), (b"c1", b"c2")[i % 2], 1 + i * 3, i % 256, cigar, (b"=", b"*", b"c2")[i % 3], i, -i, seq, qual, aux)


def on_device(data, lead=0):
    import torch
    t = torch.from_numpy(np.frombuffer(b"\xa5" * lead + bytes(data), np.uint8).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return t, t.data_ptr() + lead


def encoded(pp, ctx, text, mem, lead=0):
    """-> {"bytes", "records_at", "rec_off"} of the device encode; MEM_DEVICE: the text `lead` bytes into its allocation, HOSTILE behind"""
    if mem == pp.MEM_HOST:
        e = pp.BamEncoded(ctx, text)
    else:
        keep, at = on_device(bytes(text) + HOSTILE, lead)
        e = pp.BamEncoded(ctx, (at, len(text)), mem=pp.MEM_DEVICE)
        del keep
    try:
        assert e.dev() == (e.bytes_ptr, e.n_bytes) and e.bytes_ptr % 16 == 0
        return {"bytes": e.bytes(), "records_at": e.records_at, "rec_off": e.rec_off()}
    finally:
        e.close()


def first_difference(a, b):
    n = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    return len(a), len(b), n, a[max(0, n - 24):n + 24].hex(), b[max(0, n - 24):n + 24].hex()


def check(pp, ctx, text, lead=1, mems=None):
    want = sb.encode(text)
    for mem in mems or (pp.MEM_HOST, pp.MEM_DEVICE):
        got = encoded(pp, ctx, text, mem, lead)
        assert got["records_at"] == want["records_at"], mem
        assert got["bytes"] == want["bytes"], (mem, first_difference(got["bytes"], want["bytes"]))
        assert got["rec_off"].dtype == np.uint64 and np.array_equal(got["rec_off"], want["rec_off"]), mem
    return want


def refused(pp, ctx, text, mem=None, lead=3):
    """(code, bad line) of a refused call, checked to leave the context serving a good one"""
    with pytest.raises(pp.PolypolishError) as err:
        encoded(pp, ctx, text, pp.MEM_HOST if mem is None else mem, lead)
    good = HEADER + mixed_line(1) + b"\n"
    assert encoded(pp, ctx, good, pp.MEM_HOST)["bytes"] == sb.encode(good)["bytes"], "the context serves a good call after a refusal"
    return err.value.code, err.value.bad_record, str(err.value)


@pytest.mark.parametrize("n_lines", [0, 1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_line_counts(pp, ctx, n_lines):
    text = HEADER + b"".join(mixed_line(i) + b"\n" for i in range(n_lines))
    want = check(pp, ctx, text, lead=n_lines % 16)
    assert len(want["rec_off"]) == n_lines
    if n_lines == 0:
        assert check(pp, ctx, b"")["bytes"] == b"BAM\1" + bytes(8)
        check(pp, ctx, b"\n\n")
        check(pp, ctx, b"@CO\tno references")


def test_device_text_at_every_offset_of_its_allocation(pp, ctx):
    text = HEADER + b"".join(mixed_line(i) + b"\n" for i in range(70))
    for lead in range(16):
        check(pp, ctx, text[:-1] if lead & 1 else text, lead=lead, mems=(pp.MEM_DEVICE,))


def test_seq_and_qname_lengths(pp, ctx):
    lines = []
    for n in (0, 1, 2, 15, 16, 17, 31, 32, 33, 255):
        seq = bytes(b"=ACMGRSVTWYHKDBNacmgrsvtwyhkdbn"[k % 31] for k in range(n)) or b"*"
        for qual in ((b"*",) if n == 0 else (b"*", bytes(33 + k % 94 for k in range(n)))):
            lines.append(line(b"s%d" % n, seq=seq, qual=qual, cigar=b"*" if n == 0 else b"%dM" % n))
    for n in (1, 7, 8, 9, 254):
        lines.append(line(bytes(33 + (k * 5 + n) % 90 for k in range(n)).replace(b"@", b"a"), seq=b"ACG", qual=b"II!"))
    text = HEADER + b"\n".join(lines) + b"\n"
    check(pp, ctx, text, lead=5)
    check(pp, ctx, text.replace(b"\n", b"\r\n"), lead=6)             # "\r\n" line ends
    check(pp, ctx, text[:-1], lead=7)                                # no final newline
    check(pp, ctx, HEADER + b"\n".join(lines[::-1]) + b"\r", lead=8, mems=(pp.MEM_DEVICE,))   # the text ends in a bare "\r"


def test_cigars(pp, ctx, tile):
    many = b"1M" * 65535
    text = HEADER + line(b"none", cigar=b"*", seq=b"ACGT", qual=b"IIII") + b"\n" + line(b"one", cigar=b"268435455M", flag=4) + b"\n" + \
        line(b"ops", cigar=b"1M2I3D4N5S6H7P8=9X", aux=[b"NM:i:1"]) + b"\n" + line(b"many", pos=7, cigar=many, aux=[b"XZ:Z:behind the words"]) + b"\n" + \
        line(b"after", cigar=b"3M", seq=b"acg") + b"\n"
    want = check(pp, ctx, text, lead=9)
    assert int(want["rec_off"][4] - want["rec_off"][3]) > 4 * 65535 > tile, "a record longer than a tile, its line longer than the stage"


def test_aux_values(pp, ctx):
    ints = [0, 255, 256, -1, -128, -129, 65535, 65536, -32768, -32769, 2**32 - 1, -2**31, 2**31 - 1, 2**31]
    floats = [b"1", b"-1", b"+2.5", b"0", b"-0", b"0.000", b"-0e5", b"1e10", b"1E-10", b"3.14159e+2", b"123456789012345", b"0.00000000000001",
              b"12345.6789012345e-10", b"1e22", b"1e-22", b"000001.5"]
    lines = [line(b"i", aux=[b"X%c:i:%d" % (65 + k, v) for k, v in enumerate(ints)] + [b"XP:i:+7"]),
             line(b"f", aux=[b"F%c:f:%s" % (65 + k, v) for k, v in enumerate(floats)]),
             line(b"zh", aux=[b"XZ:Z:", b"YZ:Z:some text: with colons", b"XH:H:", b"YH:H:00ffAb", b"XA:A::", b"YA:A:!"])]
    for sub, vals in (("c", (-128, 127)), ("C", (0, 255)), ("s", (-32768, 32767)), ("S", (0, 65535)), ("i", (-2**31, 2**31 - 1)), ("I", (0, 2**32 - 1)),
                      ("f", (1.5, -2.25))):
        for count in (0, 1, 17):
            v = [vals[k % 2] for k in range(count)]
            lines.append(line(b"B%s%d" % (sub.encode(), count), aux=[b"XB:B:" + ",".join([sub] + [str(x) for x in v]).encode(), b"NM:i:%d" % count]))
    check(pp, ctx, HEADER + b"\n".join(lines) + b"\n", lead=11)


def filler_to(target, at):
    """record lines whose records fill [at, target) exactly (each 42 + m bytes: name "f", a Z field of m bytes)"""
    out = []
    while target - at > 700:
        out.append(line(b"f", aux=[b"XZ:Z:" + b"z" * 200]))
        at += 242
    assert target - at >= 42
    out.append(line(b"f", aux=[b"XZ:Z:" + b"z" * (target - at - 42)]))
    return out


@pytest.mark.parametrize("part", ["block_size", "name", "cigar", "nibbles", "qual", "aux"])
def test_every_part_of_a_record_across_a_tile_boundary(pp, ctx, tile, part):
    name, cigar, seq = b"straddler_name", b"10M5I10M5D14M", b"ACGTNacgtn" * 3 + b"ACGTACGTA"
    qual, aux = bytes(40 + k for k in range(39)), [b"NM:i:70000", b"MD:Z:10A10^ACGTA14", b"XB:B:S,1,2,3,4,5"]
    starts = {"block_size": 0, "name": 36, "cigar": 36 + 15, "nibbles": 36 + 15 + 20, "qual": 36 + 15 + 20 + 20, "aux": 36 + 15 + 20 + 20 + 39}
    lens = {"block_size": 4, "name": 15, "cigar": 20, "nibbles": 20, "qual": 39, "aux": 7 + 17 + 18}
    records_at = sb.encode(HEADER)["records_at"]
    for boundary in (tile, 2 * tile):
        for inside in (1, lens[part] // 2, lens[part] - 1):                 # bytes of the part in front of the boundary
            rec_at = boundary - starts[part] - inside
            lines = filler_to(rec_at, records_at) + [line(name, 16, b"c2", 100, 7, cigar, b"=", 90, -40, seq, qual, aux), mixed_line(3)]
            text = HEADER + b"\n".join(lines) + b"\n"
            want = check(pp, ctx, text, lead=inside % 16)
            r = len(lines) - 2
            assert int(want["rec_off"][r]) == rec_at and int(want["rec_off"][r + 1]) - rec_at == starts["aux"] + lens["aux"]
            assert rec_at + starts[part] < boundary < rec_at + starts[part] + lens[part]


REFUSALS = [  # (what, the line, code)
    ("ten columns", b"q\t0\tc1\t1\t60\t*\t*\t0\t0\t*", sb.QUIT),
    ("FLAG", line(b"q").replace(b"\t0\t", b"\tx\t", 1), sb.QUIT),
    ("POS", line(b"q", rname=b"c1").replace(b"c1\t1", b"c1\t1x"), sb.QUIT),
    ("MAPQ", line(b"q").replace(b"\t60\t", b"\t\t"), sb.QUIT),
    ("PNEXT", line(b"q").replace(b"*\t*\t0\t0", b"*\t*\t-1\t0"), sb.QUIT),
    ("TLEN", line(b"q").replace(b"*\t*\t0\t0", b"*\t*\t0\t1.5"), sb.QUIT),
    ("CIGAR op", line(b"q", cigar=b"5Q"), sb.QUIT),
    ("CIGAR digits", line(b"q", cigar=b"M5"), sb.QUIT),
    ("CIGAR tail", line(b"q", cigar=b"5M3"), sb.QUIT),
    ("QUAL with SEQ *", line(b"q", seq=b"*", qual=b"II"), sb.QUIT),
    ("QUAL length", line(b"q", seq=b"ACG", qual=b"II"), sb.QUIT),
    ("QUAL byte", line(b"q", seq=b"ACG", qual=b"I I"), sb.QUIT),
    ("aux shape", line(b"q", aux=[b"NM:i"]), sb.QUIT),
    ("aux tag", line(b"q", aux=[b"NMX:i:5"]), sb.QUIT),
    ("aux type", line(b"q", aux=[b"NM:q:5"]), sb.QUIT),
    ("aux A", line(b"q", aux=[b"XA:A:ab"]), sb.QUIT),
    ("aux i", line(b"q", aux=[b"NM:i:5x"]), sb.QUIT),
    ("aux i signs", line(b"q", aux=[b"NM:i:+-5"]), sb.QUIT),
    ("aux H odd", line(b"q", aux=[b"XH:H:abc"]), sb.QUIT),
    ("aux H byte", line(b"q", aux=[b"XH:H:ag"]), sb.QUIT),
    ("aux B sub-type", line(b"q", aux=[b"XB:B:q,1"]), sb.QUIT),
    ("aux B empty element", line(b"q", aux=[b"XB:B:c,1,,2"]), sb.QUIT),
    ("aux B nothing behind the comma", line(b"q", aux=[b"XB:B:c,"]), sb.QUIT),
    ("aux B value", line(b"q", aux=[b"XB:B:c,128"]), sb.QUIT),
    ("aux B unsigned", line(b"q", aux=[b"XB:B:S,-1"]), sb.QUIT),
    ("a trailing tab", line(b"q", aux=[b"NM:i:1"]) + b"\t", sb.QUIT),
    ("RNAME", line(b"q", rname=b"c3"), sb.QUIT),
    ("RNAME =", line(b"q", rname=b"="), sb.QUIT),
    ("RNEXT", line(b"q", rnext=b"c"), sb.QUIT),
    ("FLAG above", line(b"q", flag=65536), sb.LIMIT),
    ("POS above", line(b"q", pos=2**31 + 1), sb.LIMIT),
    ("MAPQ above", line(b"q", mapq=256), sb.LIMIT),
    ("PNEXT above", line(b"q", pnext=2**31 + 1), sb.LIMIT),
    ("TLEN above", line(b"q", tlen=2**31), sb.LIMIT),
    ("TLEN below", line(b"q", tlen=-2**31 - 1), sb.LIMIT),
    ("aux i above", line(b"q", aux=[b"XI:i:4294967296"]), sb.LIMIT),
    ("aux i below", line(b"q", aux=[b"XI:i:-2147483649"]), sb.LIMIT),
    ("QNAME long", line(b"n" * 255), sb.LIMIT),
    ("QNAME empty", line(b""), sb.LIMIT),
    ("CIGAR runs", line(b"q", cigar=b"1M" * 65536), sb.LIMIT),
    ("CIGAR run long", line(b"q", cigar=b"268435456M"), sb.LIMIT),
    ("CIGAR run 0", line(b"q", cigar=b"5M0I5M"), sb.LIMIT),
    ("SEQ byte", line(b"q", seq=b"ACGU"), sb.LIMIT),
    ("SEQ dot", line(b"q", seq=b"AC.T"), sb.LIMIT),
    ("bin", line(b"q", pos=2**29 - 3, cigar=b"5M"), sb.LIMIT),
    ("bin without a CIGAR", line(b"q", pos=2**29 + 1), sb.LIMIT),
    ("bin of an unmapped line", line(b"q", flag=4, pos=2**29 + 1, cigar=b"5M"), sb.LIMIT),
    ("float nan", line(b"q", aux=[b"de:f:nan"]), sb.LIMIT),
    ("float inf", line(b"q", aux=[b"de:f:-inf"]), sb.LIMIT),
    ("float digits", line(b"q", aux=[b"de:f:1234567890123456"]), sb.LIMIT),
    ("float exponent", line(b"q", aux=[b"de:f:1e23"]), sb.LIMIT),
    ("float in B", line(b"q", aux=[b"XB:B:f,1,1e-30"]), sb.LIMIT),
]


@pytest.mark.parametrize("what,bad,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(pp, ctx, what, bad, code):
    good = [mixed_line(i) for i in range(1, 70)]
    text = HEADER + b"\n".join(good[:66] + [bad] + good[66:]) + b"\n"
    assert sb.refusal(text) == (code, 4 + 66), "the model"
    got = refused(pp, ctx, text, pp.MEM_DEVICE if len(what) & 1 else pp.MEM_HOST)
    assert got[:2] == (code, 4 + 66), got
    assert '"text"' in got[2] and "line 71" in got[2], got[2]


def test_a_good_bin_at_the_limit_and_the_accepted_neighbours(pp, ctx):
    check(pp, ctx, HEADER + line(b"q", pos=2**29 - 4, cigar=b"5M") + b"\n" + line(b"u", flag=4, pos=2**29, pnext=2**31, cigar=b"5M") + b"\n" +
          line(b"t", tlen=-2**31, mapq=255, flag=65535, aux=[b"XI:i:4294967295", b"XJ:i:-2147483648", b"de:f:123456789012345e-22"]) + b"\n")


def test_the_first_refused_line_in_file_order_wins(pp, ctx):
    good = [mixed_line(i) for i in range(1, 200)]
    late_kind, early_kind = line(b"q", rname=b"nope"), line(b"q", flag=70000)      # found by the name lookup / by pass A
    for first, second, code in ((late_kind, early_kind, sb.QUIT), (early_kind, late_kind, sb.LIMIT)):
        text = HEADER + b"\n".join(good[:70] + [first] + good[70:130] + [second] + good[130:]) + b"\n"
        assert sb.refusal(text) == (code, 74)
        assert refused(pp, ctx, text)[:2] == (code, 74)
    # a line that begins with '@' behind the first record, against a later and an earlier defect
    text = HEADER + b"\n@CO\tstill in front\n" + good[0] + b"\n@CO\tlate\n" + early_kind + b"\n"
    assert sb.refusal(text) == (sb.QUIT, 7) and refused(pp, ctx, text)[:2] == (sb.QUIT, 7)
    text = HEADER + early_kind + b"\n@CO\tlate\n"
    assert sb.refusal(text) == (sb.LIMIT, 4) and refused(pp, ctx, text)[:2] == (sb.LIMIT, 4)
    check(pp, ctx, HEADER + b"\n@CO\tskipped: no record in front of it\n" + good[0] + b"\n")


def test_refusals_of_the_call(pp, ctx):
    text = HEADER + mixed_line(2) + b"\n"
    code, bad, msg = refused(pp, ctx, text.replace(b"read2", b"re\xc3\xa4d"))
    assert (code, bad) == (sb.NOT_ASCII, None)
    code, bad, msg = refused(pp, ctx, b"@HD\tVN:1\n@SQ\tSN:a\tLN:5\n@SQ\tSN:a\tLN:5\n" + mixed_line(2) + b"\n", pp.MEM_DEVICE)
    assert (code, bad) == (sb.QUIT, 2) and "line 3" in msg and "pp_sam_header" in msg
    assert sb.refusal(b"@HD\tVN:1\n@SQ\tSN:a\tLN:5\n@SQ\tSN:a\tLN:5\n") == (sb.QUIT, 2)
    with pytest.raises(pp.PolypolishError) as err:
        pp.BamEncoded(ctx, (0, 5), mem=pp.MEM_DEVICE)
    assert err.value.code == sb.ARG
    with pytest.raises(pp.PolypolishError) as err:
        pp.BamEncoded(ctx, text, mem=2)
    assert err.value.code == sb.ARG
    keep, at = on_device(text)
    with pytest.raises(pp.PolypolishError) as err:
        pp.BamEncoded(ctx, (at, 1 << 40), mem=pp.MEM_DEVICE)         # refused before a byte is read
    assert err.value.code == sb.LIMIT
    check(pp, ctx, text)


def test_twin_call_determinism_and_stage_times(pp, ctx):
    # every aligned line carries NM: pp_sam_records takes the text, too
    text = HEADER + b"".join(line(b"r%d" % i, 16 * (i & 1), b"c1", 5 + i, 30, b"20M", b"=", 9, 3, b"ACGTA" * 4, b"I" * 20, [b"NM:i:%d" % (i % 4), b"AS:i:20"]) + b"\n"
                             for i in range(3000))
    want = sb.encode(text)
    ctx.set_profiling(True)
    try:
        a, b = pp.BamEncoded(ctx, text), pp.BamEncoded(ctx, text)
        rec = pp.SamRecords(ctx, text)
        c = rec.bam()
        try:
            assert a.bytes() == b.bytes() == c.bytes() == want["bytes"]
            assert np.array_equal(c.rec_off(), want["rec_off"]) and c.records_at == want["records_at"] and c.n_rec == rec.n_rec == 3000
            stages = a.stage_ms()
            assert list(stages) == ["newline_index", "pass_a", "names", "scans", "pass_b"] and all(v > 0 for v in stages.values())
            assert abs(a.kernel_ms() - sum(stages.values())) <= 1e-4 * sum(stages.values())
        finally:
            for o in (a, b, c, rec):
                o.close()
    finally:
        ctx.set_profiling(False)
    with pytest.raises(pp.PolypolishError):
        e = pp.BamEncoded(ctx, text)
        try:
            e.kernel_ms()
        finally:
            e.close()
