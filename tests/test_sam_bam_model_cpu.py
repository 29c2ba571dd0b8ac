"""tests/sam_bam_model.py -- the plain model of pp_sam_header and pp_sam_bam -- pinned from several sides, without a GPU:
  * hand-written bytes for a header and three records, and the four hand values of reg2bin;
  * on synth.rich_dataset and on the synth.mutate_sam mutants that both models accept, its records are bam_model.encode's apart from
    the two bin bytes (bam_model writes 4680 everywhere), and bam_model.decode of its bytes is gate_model.raw_from_text of the text;
  * its float rule is struct.pack('<f', float(s)) on generated strings inside the rule's range;
  * the library's host helper pp_sam_header is the model's header(): arrays, refusals with their line, every truncation of a small
    header, the cap convention."""
import ctypes as C
import re
import struct

import numpy as np
import pytest

import bam_model as bm
import gate_model as gm
import sam_bam_model as sb
import synth

HDR = b"@SQ\tSN:c\tLN:100\n"
HDR_HEX = "42414d01" "10000000" + HDR.hex() + "01000000" "02000000" "6300" "64000000"
HAND = [
    # unmapped: refID -1, pos -1, bin 4680
    (b"r1\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\t!!!!",
     "29000000" "ffffffff" "ffffffff" "03" "00" "4812" "0000" "0400" "04000000" "ffffffff" "ffffffff" "00000000" "723100" "1248" "00000000"),
    # an odd-length lower-case SEQ with QUAL "*", RNEXT "=", a negative TLEN
    (b"q\t16\tc\t11\t30\t3M\t=\t21\t-5\tacg\t*",
     "2b000000" "00000000" "0a000000" "02" "1e" "4912" "0100" "1000" "03000000" "00000000" "14000000" "fbffffff" "7100" "30000000" "1240" "ffffff"),
    # every aux type
    (b"a\t0\tc\t1\t0\t*\t*\t0\t0\t*\t*\tXA:A:Q\tXi:i:-129\tXZ:Z:hi\tXH:H:1aF0\tXf:f:1.5\tXB:B:s,1,-2",
     "4c000000" "00000000" "00000000" "02" "00" "4912" "0000" "0000" "00000000" "ffffffff" "ffffffff" "00000000" "6100"
     "58414151" "5869737fff" "585a5a686900" "5848483161463000" "5866660000c03f" "58424273" "02000000" "0100" "feff"),
]


def test_hand_written_bytes():
    text = HDR + b"".join(line + b"\n" for line, _ in HAND)
    got = sb.encode(text)
    want = bytes.fromhex(HDR_HEX) + b"".join(bytes.fromhex(h) for _, h in HAND)
    assert got["records_at"] == len(bytes.fromhex(HDR_HEX)) == 38
    assert got["bytes"].hex() == want.hex()
    offs, at = [], 38
    for _, h in HAND:
        offs.append(at)
        at += len(h) // 2
    assert got["rec_off"].tolist() == offs and got["lines"].tolist() == [1, 2, 3]
    assert sb.encode(b"")["bytes"] == b"BAM\1" + bytes(8)
    only = sb.encode(HDR.replace(b"\n", b"\r\n"))
    assert only["bytes"].hex() == HDR_HEX and len(only["rec_off"]) == 0, "the CR in front of a header line's end is dropped"


def test_reg2bin_hand_values():
    assert sb.reg2bin(-1, 0) == 4680
    assert sb.reg2bin(0, 1) == 4681
    assert sb.reg2bin(16383, 16385) == 585
    assert sb.reg2bin(2**29 - 1, 2**29) == 37448


def records_of(enc):
    b, off = enc["bytes"], enc["rec_off"].tolist() + [len(enc["bytes"])]
    return [b[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def without_bin(rec):
    return rec[:14] + rec[16:]


def against_bam_model(text, names, lens):
    """-> the records compared, 0 where one of the two models refuses the text"""
    try:
        mine = sb.encode(text)
    except sb.Refused:
        return 0
    try:
        theirs = bm.encode(text, names, lens)
    except (bm.NotBam, UnicodeDecodeError):
        return 0
    a, b = records_of(mine), records_of({"bytes": theirs["records"], "rec_off": theirs["rec_off"]})
    assert len(a) == len(b)
    for r, (x, y) in enumerate(zip(a, b)):
        assert without_bin(x) == without_bin(y), r
    return len(a)


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    ds = synth.rich_dataset(str(tmp_path_factory.mktemp("sam_bam")), seed=23, contig_lens=(4000, 2500), coverage=30, repeat_len=400,
                            repeat_copies=3, zp_frac=0.02)
    contigs = [(c.name, c.assembly) for c in ds["contigs"]]
    texts = [open(p, "rb").read() for p in (ds["sam1"], ds["sam2"])]
    # (the dataset's QUAL has the nominal read length on every line; a read with an indel is refused as it stands)
    assert all(sb.refusal(t) is not None and sb.refusal(t)[0] == sb.QUIT for t in texts)
    return {"contigs": contigs, "texts": [sb.with_fitting_qual(t) for t in texts]}


def test_records_are_bam_model_s_apart_from_the_bin(dataset):
    names, lens = [n for n, _ in dataset["contigs"]], [len(s) for _, s in dataset["contigs"]]
    for text in dataset["texts"]:
        assert against_bam_model(text, names, lens) > 500
    rng = np.random.default_rng(7)
    head = dataset["texts"][0].decode().split("\n")
    small = "\n".join(head[:60]) + "\n"
    compared = accepted = 0
    for _ in range(300):
        n = against_bam_model(synth.mutate_sam(small, rng, n_mut=2).encode("latin-1"), names, lens)
        compared += n
        accepted += n > 0
    assert accepted > 20 and compared > 1000, (accepted, compared)


def test_decode_of_the_model_is_the_text(dataset):
    contigs = dataset["contigs"]
    for text in dataset["texts"]:
        enc = sb.encode(text)
        got = bm.decode(enc["bytes"], enc["rec_off"])
        raw, zp = gm.raw_from_text(contigs, text)
        for k in ("flag", "contig", "ref_start", "nm", "seq_len", "n_cig", "cigar"):
            assert got[k].dtype == raw[k].dtype and np.array_equal(got[k], raw[k]), k
        assert np.array_equal(got["zp"], zp)
        lines = [ln.split(b"\t") for ln in text.split(b"\n") if ln and ln[:1] != b"@"]
        assert len(lines) == len(got["flag"])
        for r, cols in enumerate(lines):
            so, sl = int(got["seq_off"][r]), int(got["seq_len"][r])
            assert got["seq"][so:so + sl].tobytes() == (b"" if cols[9] == b"*" else cols[9].upper()), r
            no, nl = int(got["name_off"][r]), int(got["name_len"][r])
            assert enc["bytes"][no:no + nl] == cols[0], r
        # the walk of the bytes from records_at is rec_off
        off, end, ok = bm.walk(enc["bytes"], enc["records_at"])
        assert ok and end == len(enc["bytes"]) and off == enc["rec_off"].tolist()
        assert bm.header(enc["bytes"])["records_at"] == enc["records_at"]


def test_float_rule_is_python_s_float():
    rng = np.random.default_rng(11)
    n = 0
    for _ in range(20000):
        nd = int(rng.integers(1, 16))
        digits = "".join(str(int(d)) for d in rng.integers(0, 10, nd))
        cut = int(rng.integers(0, nd + 1))
        s = str(rng.choice(["", "+", "-"])) + (digits[:cut] or "0")
        frac = digits[cut:]
        if frac:
            s += "." + frac
        e = None
        if rng.random() < 0.6:
            e = int(rng.integers(-22 + len(frac), 23)) if len(frac) <= 22 else 0
            s += str(rng.choice(["e", "E"])) + str(rng.choice(["", "+"]) if e >= 0 else "") + str(e)
        got = sb.float_bits(s.encode())
        e10 = (e or 0) - len(frac)
        if abs(e10) > 22:
            assert got is None or int(digits) == 0, s
            continue
        assert got == struct.pack("<f", float(s)), s
        n += 1
    assert n > 15000
    for s, want in (("0", 0.0), ("-0.000", -0.0), ("0e99", 0.0), ("1e22", 1e22), ("123456789012345", 123456789012345.0), ("1.5E-3", 1.5e-3)):
        assert sb.float_bits(s.encode()) == struct.pack("<f", want), s
    for s in ("", "+", ".5", "1.", "1e", "1e+", "nan", "inf", "-inf", "1234567890123456", "1e23", "1e-23", "0x10", "1 "):
        assert sb.float_bits(s.encode()) is None, s


# ---- pp_sam_header --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pp():
    import polypolish_amd
    return polypolish_amd


def lib_header(pp, text):
    """-> the model's dict, or ("refused", code, 0-based line)"""
    try:
        h = pp.sam_header(text)
    except pp.PolypolishError as e:
        m = re.search(r"line (\d+)", str(e))
        return ("refused", e.code, int(m.group(1)) - 1 if m else None)
    return h


def same_as_model(pp, text):
    got = lib_header(pp, text)
    try:
        want = sb.header(text)
    except sb.Refused as r:
        assert got == ("refused", r.code, r.line), (text, got)
        return False
    assert not isinstance(got, tuple), (text, got)
    assert got["header_end"] == want["header_end"] and got["names"] == want["names"]
    for k in ("name_off", "name_len", "ref_len"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    return True


def test_pp_sam_header_on_the_datasets(pp, dataset):
    for text in dataset["texts"]:
        assert same_as_model(pp, text)
        assert pp.sam_header(text)["names"] == [n.encode() for n, _ in dataset["contigs"]]


SMALL = b"@HD\tVN:1.6\r\n@SQ\tSN:one\tLN:12\tM5:x\n@CO\tSN:no\n@SQ\tLN:2147483647\tSN:two\r\n@SQX\tSN:three\n@SQ\tSN:3\tLN:7\nr\t4\t*\n@SQ\tSN:late\n"


def test_pp_sam_header_refusals_and_cuts(pp):
    assert same_as_model(pp, SMALL)
    h = pp.sam_header(SMALL)
    assert h["names"] == [b"one", b"two", b"3"] and h["ref_len"].tolist() == [12, 2147483647, 7] and SMALL[h["header_end"]:h["header_end"] + 2] == b"r\t"
    for cut in range(len(SMALL) + 1):
        same_as_model(pp, SMALL[:cut])                           # every truncation: the model's answer, and no fault
    for text, line in ((b"@HD\n@SQ\tLN:5\n", 1), (b"@SQ\tSN:\tLN:5\n", 0), (b"@SQ\tSN:a\n", 0), (b"@SQ\tSN:a\tLN:0\n", 0), (b"@SQ\tSN:a\tLN:2147483648\n", 0),
                       (b"@SQ\tSN:a\tLN:5x\n", 0), (b"@SQ\tSN:a\tLN:\n", 0), (b"@SQ\tSN:a\tLN:5\n@SQ\tSN:b\tLN:5\n@SQ\tSN:a\tLN:6\n", 2), (b"@SQ", 0)):
        assert lib_header(pp, text) == ("refused", sb.QUIT, line), text
        assert not same_as_model(pp, text)
    assert same_as_model(pp, b"") and same_as_model(pp, b"\n@SQ\tSN:a\n") and same_as_model(pp, b"@SQ\tSN:a\tLN:5") and same_as_model(pp, b"@CO\r")


def test_pp_sam_header_cap_convention(pp):
    L = pp.lib()
    b = np.frombuffer(SMALL, np.uint8)
    n_ref, end = C.c_uint32(0), C.c_uint64(0)
    off, ln, rl = np.full(2, 99, np.uint64), np.full(2, 99, np.uint32), np.full(2, 99, np.uint32)
    rc = L.pp_sam_header(b.ctypes.data, len(b), 1, C.byref(n_ref), off.ctypes.data, ln.ctypes.data, rl.ctypes.data, C.byref(end))
    assert rc == sb.ARG and n_ref.value == 3 and b"room for 1" in L.pp_bam_last_error()
    want = sb.header(SMALL)
    assert (off[0], ln[0], rl[0]) == (want["name_off"][0], 3, 12) and (off[1], ln[1], rl[1]) == (99, 99, 99), "only the first cap entries"
    assert end.value == want["header_end"]
    assert L.pp_sam_header(b.ctypes.data, len(b), 0, None, None, None, None, C.byref(end)) == sb.ARG
    assert L.pp_sam_header(None, 5, 0, C.byref(n_ref), None, None, None, C.byref(end)) == sb.ARG
