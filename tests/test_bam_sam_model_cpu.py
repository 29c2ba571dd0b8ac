"""tests/bam_sam_model.py -- the plain model of pp_bam_sam, the definition of its bytes -- pinned from several sides, without a GPU:
  * hand-written records -> hand-written lines: every aux type, every B sub-type, the extremes, odd / even / zero l_seq, QUAL 0xFF, no CIGAR;
  * C's "%g": the table of the issue, 20,000 random float32 bit patterns and every exponent with the mantissas 0, 1, 0x400000, 0x7FFFFF;
  * the fixed point decode(sam_bam_model.encode(T)) == T on sam_bam_model's own test texts made canonical and on the canonical dataset,
    the verdicts against the oracle's filtered files and against sam_tag_model.tagged, and encode(decode(B)) == B;
  * pp_sam_header of a synthesised header gives back the BAM's reference table;
  * every refusal with its code and record, bam_model.defect_records() included."""
import struct

import numpy as np
import pytest

import bam_model as bm
import bam_sam_model as bs
import bam_tag_model as tm
import sam_bam_model as sb
import sam_tag_model as st
import synth
from test_sam_bam_model_cpu import HAND, HDR

REFS = (("c1", 1000), ("c2", 2000))


def one(rec, passed=None, refs=REFS, text="@HD\tVN:1.6\n"):
    """the line(s) of record(s) behind the header's own"""
    recs = rec if isinstance(rec, list) else [rec]
    b, at, off = bs.bam_of(recs, refs, text)
    out = bs.decode(b, at, off, passed)
    head = bs.header_text(b, at)[0]
    assert out.startswith(head)
    return out[len(head):]


def f32(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def test_hand_written_lines():
    aux = (bm.aux("XA", "A", "Q") + bm.aux("Xc", "c", -128) + bm.aux("XC", "C", 255) + bm.aux("Xs", "s", -32768) + bm.aux("XS", "S", 65535) +
           bm.aux("Xi", "i", -2**31) + bm.aux("XI", "I", 4294967295) + bm.aux("XZ", "Z", "a b~") + bm.aux("Xz", "Z", "") + bm.aux("XH", "H", "1aF0") +
           bm.aux("Xh", "H", "") + bm.aux("Xf", "f", 1.5) + bm.aux("Xg", "f", -0.0))
    want_aux = b"XA:A:Q\tXc:i:-128\tXC:i:255\tXs:i:-32768\tXS:i:65535\tXi:i:-2147483648\tXI:i:4294967295\tXZ:Z:a b~\tXz:Z:\tXH:H:1aF0\tXh:H:\tXf:f:1.5\tXg:f:-0"
    r = bm.record(b"read/1", 99, 0, 9, [(3 << 4) | 4, (5 << 4) | 0, (1 << 4) | 8], "ACGTNACGT", aux, qual=bytes(range(9)), mapq=60, next_ref=1, next_pos=99,
                  tlen=-2**31)
    assert one(r) == b"read/1\t99\tc1\t10\t60\t3S5M1X\tc2\t100\t-2147483648\tACGTNACGT\t!\"#$%&'()\t" + want_aux + b"\n"
    # every B sub-type, count 0 and more
    arrays = [("c", [-128, 127]), ("C", [0, 255]), ("s", [-32768, 32767]), ("S", [65535]), ("i", [-2**31, 2**31 - 1]), ("I", [4294967295, 0]), ("f", [0.1, 1e-45, 100000.0])]
    aux = b"".join(bm.aux("B" + sub, "B", (sub, vals)) + bm.aux("b" + sub, "B", (sub, [])) for sub, vals in arrays)
    want = (b"Bc:B:c,-128,127\tbc:B:c\tBC:B:C,0,255\tbC:B:C\tBs:B:s,-32768,32767\tbs:B:s\tBS:B:S,65535\tbS:B:S\tBi:B:i,-2147483648,2147483647\tbi:B:i\t"
            b"BI:B:I,4294967295,0\tbI:B:I\tBf:B:f,0.1,1.4013e-45,100000\tbf:B:f")
    # pos -1 and 2^31-1, RNEXT "=", an even l_seq, QUAL 0xFF, no CIGAR
    r = bm.record(b"q", 0, 1, -1, [], "=ACMGRSVTWYHKDBN", aux, qual=None, mapq=0, next_ref=1, next_pos=2**31 - 1, tlen=2**31 - 1)
    assert one(r) == b"q\t0\tc2\t0\t0\t*\t=\t2147483648\t2147483647\t=ACMGRSVTWYHKDBN\t*\t" + want + b"\n"
    # l_seq 0; an unaligned record; no reference on either side; pos 2^31-1
    r = bm.record(b"u", 4, -1, 2**31 - 1, [], "", b"", mapq=255, next_ref=-1, next_pos=-1, tlen=0)
    assert one(r) == b"u\t4\t*\t2147483648\t255\t*\t*\t0\t0\t*\t*\n"
    # an odd l_seq whose spare nibble is set, QUAL 0xFF in front of other bytes is "*", RNEXT another reference's name, next_refID alone
    r = bytearray(bm.record(b"o", 16, -1, 0, [(1 << 4) | 1, (2 << 4) | 2, (3 << 4) | 3, (4 << 4) | 5, (5 << 4) | 6, (6 << 4) | 7], "ACG", b"", qual=bytes([0xFF, 1, 2]),
                            next_ref=0, next_pos=0, seq_pad_nibble=0xF))
    assert one(bytes(r)) == b"o\t16\t*\t1\t60\t1I2D3N4H5P6=\tc1\t1\t0\tACG\t*\n"
    # a CG:B:I long CIGAR is an aux field like any other; a zero-length run prints as it is
    r = bm.record(b"cg", 0, 0, 0, [(0 << 4) | 0], "A", bm.aux("CG", "B", ("I", [(70000 << 4) | 0])), qual=bytes([93]))
    assert one(r) == b"cg\t0\tc1\t1\t60\t0M\t*\t0\t0\tA\t~\tCG:B:I,1120000\n"


G_TABLE = [(1000005.0, b"1e+06"), (1000015.0, b"1.00002e+06"), (999999.5, b"1e+06"), (1e-45, b"1.4013e-45"), (3.4028235e38, b"3.40282e+38"),
           (100000.0, b"100000"), (1.234565e-05, b"1.23457e-05"), (0.1, b"0.1")]


def test_percent_g_table_and_random_floats():
    for x, want in G_TABLE:
        assert bs.fmt_g(f32(x)) == want, x
        r = bm.record(b"q", 4, -1, -1, [], "", bm.aux("XF", "f", x))
        assert one(r).endswith(b"\tXF:f:" + want + b"\n"), x
    rng = np.random.default_rng(5)
    bits = [int(b) for b in rng.integers(0, 2**32, 20000, dtype=np.uint64) if (int(b) & 0x7F800000) != 0x7F800000] + bs.exponent_floats()
    vals = np.array(bits, np.uint32).view(np.float32)
    r = bm.record(b"q", 4, -1, -1, [], "", bm.aux("XB", "B", ("f", [])))
    r = bytearray(r)
    r[-4:] = struct.pack("<I", len(bits))
    r += np.array(bits, "<u4").tobytes()
    r[0:4] = struct.pack("<I", len(r) - 4)
    got = one(bytes(r)).rstrip(b"\n").split(b"\t")[-1].split(b",")
    assert got[0] == b"XB:B:f" and len(got) == len(bits) + 1
    for g, v, b in zip(got[1:], vals.tolist(), bits):
        assert g == ("%g" % v).encode(), hex(b)


@pytest.fixture(scope="module")
def dataset(tmp_path_factory, orc):
    d = str(tmp_path_factory.mktemp("bam_sam"))
    ds = synth.rich_dataset(d, seed=23, contig_lens=(4000, 2500), coverage=30, repeat_len=400, repeat_copies=3, zp_frac=0.02)
    texts = [sb.with_fitting_qual(open(p, "rb").read()) for p in (ds["sam1"], ds["sam2"])]
    canon, lower = [], []
    for t in texts:
        lines = t.split(b"\n")
        n = 0
        for i, ln in enumerate(lines):
            p = ln.split(b"\t")
            if ln and ln[:1] != b"@" and p[9] != p[9].upper():
                p[9] = p[9].upper()
                lines[i] = b"\t".join(p)
                n += 1
        lower.append(n)
        canon.append(b"\n".join(lines))
    import os
    sams = []
    for f, t in enumerate(canon):
        sams.append(os.path.join(d, f"canon_{f + 1}.sam"))
        with open(sams[-1], "wb") as fh:
            fh.write(t)
    outs = [os.path.join(d, f"filtered_{i}.sam") for i in (1, 2)]
    orc.filter_files(sams[0], sams[1], outs[0], outs[1])
    return {"texts": texts, "canon": canon, "lower": lower, "filtered": [open(p, "rb").read() for p in outs], "names": [c.name.encode() for c in ds["contigs"]]}


def back(text, passed=None):
    enc = sb.encode(text)
    return bs.decode(enc["bytes"], enc["records_at"], enc["rec_off"], passed)


def test_fixed_point_on_the_models_own_texts():
    text = HDR + b"".join(line + b"\n" for line, _ in HAND)
    canon = back(text)
    assert canon != text and back(canon) == canon
    assert canon.split(b"\n")[2] == b"q\t16\tc\t11\t30\t3M\t=\t21\t-5\tACG\t*"
    assert canon.split(b"\n")[3].endswith(b"\tXf:f:1.5\tXB:B:s,1,-2")
    b = sb.encode(canon)
    assert sb.encode(bs.decode(b["bytes"], b["records_at"], b["rec_off"]))["bytes"] == b["bytes"]
    assert back(b"") == b"" and back(HDR) == HDR and back(HDR.replace(b"\n", b"\r\n")) == HDR


def test_fixed_point_and_verdicts_on_the_dataset(dataset):
    assert dataset["lower"] == [45, 48], "the dataset's only non-canonical property: lines with lower-case SEQ bytes"
    for f, (text, canon) in enumerate(zip(dataset["texts"], dataset["canon"])):
        assert canon.endswith(b"\n") and back(canon) == canon and back(text) == canon
        enc = sb.encode(canon)
        again = sb.encode(bs.decode(enc["bytes"], enc["records_at"], enc["rec_off"]))
        assert again["bytes"] == enc["bytes"] and np.array_equal(again["rec_off"], enc["rec_off"])
        verdict = tm.own_verdicts(canon, dataset["filtered"][f])
        assert (verdict == 0).any() and (verdict == 1).any()
        got = bs.decode(enc["bytes"], enc["records_at"], enc["rec_off"], verdict)
        assert got == dataset["filtered"][f], "the oracle's filtered file of the same text"
        assert got == st.tagged(bs.decode(enc["bytes"], enc["records_at"], enc["rec_off"], None), verdict)[0]
        assert got != canon and bs.decode(enc["bytes"], enc["records_at"], enc["rec_off"], np.ones_like(verdict)) == canon


def test_a_tag_goes_behind_a_tag_and_unaligned_records_take_no_verdict():
    recs = [bm.record(b"a", 0, 0, 1, [(1 << 4)], "A", bm.aux("ZP", "Z", "fail")), bm.record(b"u", 4, -1, -1, [], "", b""), bm.record(b"b", 16, 0, 1, [(1 << 4)], "C", b"")]
    plain = one(recs)
    assert plain == b"a\t0\tc1\t2\t60\t1M\t*\t0\t0\tA\t*\tZP:Z:fail\nu\t4\t*\t0\t60\t*\t*\t0\t0\t*\t*\nb\t16\tc1\t2\t60\t1M\t*\t0\t0\tC\t*\n"
    assert one(recs, [0, 1]) == plain.replace(b"ZP:Z:fail\n", b"ZP:Z:fail\tZP:Z:fail\n")
    assert one(recs, [1, 0]) == plain[:-1] + b"\tZP:Z:fail\n"
    assert one(recs, [1, 1]) == plain
    for passed in ([0, 0], [0, 1], [1, 0], [1, 1]):
        assert one(recs, passed) == st.tagged(plain, passed)[0], "the verdicts are sam_tag_model's on the untagged text"
    for passed in ([], [1], [1, 1, 1]):
        b, at, off = bs.bam_of(recs)
        assert bs.refusal(b, at, off, passed) == (bs.ARG, None)


def test_synthesised_header_reads_back_as_the_reference_table():
    import polypolish_amd as pp
    refs = (("chr1", 1), ("a|b", 2**31 - 1), ("x", 77))
    for text, synth_sq in (("", True), ("@HD\tVN:1.6", True), ("@HD\tVN:1.6\n@SQX\tSN:no\tLN:1\n\0\0\0", True), ("@CO\t@SQ\n", True), ("@SQ\tSN:other\tLN:5\n", False)):
        b, at, off = bs.bam_of([], refs, text)
        out = bs.decode(b, at, off)
        body = text.rstrip("\0")
        body += "\n" if body and not body.endswith("\n") else ""
        sq = "".join(f"@SQ\tSN:{n}\tLN:{ln}\n" for n, ln in refs)
        assert out == (body + (sq if synth_sq else "")).encode(), text
        if synth_sq:
            h = pp.sam_header(out)
            assert h["names"] == [n.encode() for n, _ in refs] and h["ref_len"].tolist() == [ln for _, ln in refs]
    assert bs.decode(*bs.bam_of([], (), "")) == b""
    for refs in ((("", 5),), (("*", 5),), (("=", 5),), (("a b", 5),), (("a\tb", 5),), (("ok", 0),), (("ok", -2**31),)):      # (l_ref 2^31 as the bytes hold it)
        assert bs.refusal(*bs.bam_of([], refs, "@HD\n")) == (bs.LIMIT, None), refs
    b, at, off = bs.bam_of([], REFS)
    assert bs.refusal(b, at - 1, off) == (bs.ARG, None) and bs.refusal(b + b"x", at + 1, off) == (bs.ARG, None) and bs.refusal(b"BAM\0" + b[4:], at, off) == (bs.ARG, None)


def test_the_library_has_the_entry_points_and_the_geometry_the_header_states():
    import polypolish_amd as pp
    L = pp.lib()
    assert all(hasattr(L, name) for name in ("pp_bam_sam", "pp_bam_sam_encoded", "pp_ctx_set_out_sam"))
    recs, tile, store, lane, group = pp.bam_sam_geometry()
    assert (recs, tile, store, lane) == (1024, 16384, 16, 16) and group in (16, 32, 64), "include/polypolish_hip.h states the first three"
    assert hasattr(pp.SamOut, "from_bam") and hasattr(pp.BamEncoded, "sam") and hasattr(pp.Context, "set_out_sam")


def good(i=0):
    return bm.record(b"g%d" % i, 0, 0, 5, [(4 << 4)], "ACGT", bm.aux("NM", "C", 0), qual=bytes(4))


def limit_records():
    """[(what, record)]: valid records that have no SAM line"""
    base = dict(flag=0, ref_id=0, pos=5, runs=[(4 << 4)], seq="ACGT")
    rec = lambda aux=b"", qname=b"q", **kw: bm.record(qname, aux_bytes=aux, **{**base, **kw})      # noqa: E731
    out = [("empty QNAME", rec(qname=b"")), ("QNAME with a tab", rec(qname=b"a\tb")), ("QNAME with a space", rec(qname=b"a b")), ("QNAME 0x7F", rec(qname=b"a\x7f")),
           ("QNAME with a NUL inside", rec(qname=b"a\0b")), ("QNAME begins with @", rec(qname=b"@a")), ("A space", rec(bm.aux("XA", "A", " "))),
           ("A 0x7F", rec(bm.aux("XA", "A", "\x7f"))), ("Z tab", rec(bm.aux("XZ", "Z", "a\tb"))), ("Z 0x7F", rec(bm.aux("XZ", "Z", "\x7f"))), ("Z 0x80", rec(bm.aux("XZ", "Z", b"\x80"))),
           ("H odd", rec(bm.aux("XH", "H", "1AF"))), ("H no hex", rec(bm.aux("XH", "H", "1G"))), ("tag digit first", rec(bm.aux("1X", "C", 1))),
           ("tag punctuation", rec(bm.aux("X_", "C", 1))), ("tag space", rec(bm.aux(" X", "Z", "v"))), ("QUAL 94", rec(qual=bytes([0, 94, 0, 0]))),
           ("QUAL 0xFF behind a byte", rec(qual=bytes([1, 0xFF, 0, 0]))), ("f inf", rec(bm.aux("XF", "f", float("inf")))), ("f nan", rec(bm.aux("XF", "f", float("nan")))),
           ("f -inf", rec(bm.aux("XF", "f", float("-inf")))), ("B:f with a nan", rec(bm.aux("XB", "B", ("f", [1.0, float("nan")])))),
           ("reference name", rec(ref_id=2)), ("next reference name", rec(next_ref=2))]
    return out


def arg_records():
    """[(what, record)]: pp_bam_records' defects (bam_model.defect_records) and this link's own"""
    base = dict(qname=b"name", flag=0, ref_id=1, pos=5, runs=[(8 << 4)], seq="ACGTACGT", aux_bytes=bm.aux("NM", "C", 1))
    out = [(kind, r) for kind, r in bm.defect_records()]
    out += [("next_refID -2", bm.record(next_ref=-2, **base)), ("next_refID n_ref", bm.record(next_ref=3, **base)), ("pos -2", bm.record(**dict(base, pos=-2))),
            ("next_pos -2", bm.record(next_pos=-2, **base))]
    return out


REFS3 = (("c1", 1000), ("c2", 2000), ("bad name", 30))
SQ3 = "@SQ\tSN:c1\tLN:1000\n"      # (a header with an @SQ line: none is synthesised, so the third name is met by the records only)


def test_every_refusal_with_its_code_and_record():
    for cases, code in ((arg_records(), bs.ARG), (limit_records(), bs.LIMIT)):
        for what, r in cases:
            for k in (0, 2):
                recs = [good(i) for i in range(k)] + [r, good(9)]
                b, at, off = bs.bam_of(recs, REFS3, SQ3)
                assert bs.refusal(b, at, off) == (code, k), what
                assert bs.refusal(b, at, off, [1]) == (code, k), "in front of the verdicts' number"
    # the first refused record in index order wins, whatever its kind; inside one record ARG goes in front of LIMIT
    lim, arg = limit_records()[0][1], arg_records()[0][1]
    for recs, want in (([good(), lim, arg], (bs.LIMIT, 1)), ([good(), arg, lim], (bs.ARG, 1))):
        b, at, off = bs.bam_of(recs, REFS3, SQ3)
        assert bs.refusal(b, at, off) == want
    both = bm.record(b"a\tb", 0, 0, -2, [], "", b"")
    assert bs.refusal(*bs.bam_of([both], REFS3, SQ3)) == (bs.ARG, 0)
    # the three of the walk: an offset outside the array or ending inside the word, block_size < 32, a record past the bytes
    b, at, off = bs.bam_of([good(0), good(1)], REFS3, SQ3)
    n = len(b)
    for o, nb in ((n + 1, n), (n, n), (n - 3, n), (int(off[1]), n - 1)):
        assert bs.refusal(b[:nb], at, np.array([off[0], o], np.uint64)) == (bs.ARG, 1), (o, nb)
    small = bytearray(b)
    small[int(off[0]):int(off[0]) + 4] = struct.pack("<I", 31)
    assert bs.refusal(bytes(small), at, off) == (bs.ARG, 0)
    # rec_off unordered, with a gap and a repeated record: fine
    lines = one([good(0), good(1)]).split(b"\n")
    assert bs.decode(b + b"junk", at, np.array([off[1], off[0], off[1]], np.uint64)) == bs.header_text(b, at)[0] + b"\n".join([lines[1], lines[0], lines[1]]) + b"\n"
