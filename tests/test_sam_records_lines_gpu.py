"""pp_sam_records_lines (pp_sam.hip) against tests/sam_records_model.py's decode of text_chain_model.prefix(text, n), byte for byte, with
the text in host memory and in device memory (there in an allocation of exactly its length) -- and pp_sam_first_empty_line against
text_chain_model.first_empty_line.  Whatever stands at or behind line n, hostile bytes included, changes nothing.  Nothing here depends
on a fault.  Needs an MI355X: `-m gpu`."""
import os
import re

import numpy as np
import pytest

import ingest_model as im
import sam_records_model as sm
import text_chain_model as tm
from test_sam_records_gpu import on_device

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pp():
    import polypolish_amd
    return polypolish_amd


@pytest.fixture(scope="module")
def ctx(pp):
    c = pp.Context(0)
    yield c
    c.close()


def geometry():
    """(lines per workgroup of the scan, of the placing kernel), read from pp_sam.hip"""
    src = open(os.path.join(ROOT, "polypolish_amd", "csrc", "pp_sam.hip")).read()
    scan = re.search(r"__launch_bounds__\((\d+)\) void k_sam_scan", src)
    place = re.search(r"constexpr u32 SAM_BLOCK = (\d+);", src)
    return int(scan.group(1)), int(place.group(1))


def limited(pp, ctx, text, n, mem):
    if mem == pp.MEM_HOST:
        return pp.SamRecords(ctx, np.frombuffer(bytes(text), np.uint8), mem, n_lines=n)
    data, keep = on_device(text)
    rec = pp.SamRecords(ctx, data, mem, n_lines=n)
    del keep
    return rec


def check(pp, ctx, text, n):
    """the device on (text, n) against the model on prefix(text, n), both mem forms -> the model's result or error"""
    head = tm.prefix(text, n)
    try:
        want = sm.decode(head)
    except sm.SamError as m:
        for mem in (pp.MEM_HOST, pp.MEM_DEVICE):
            with pytest.raises(pp.PolypolishError) as e:
                limited(pp, ctx, text, n, mem)
            assert (e.value.code, e.value.bad_record) == (m.code, m.bad_line), (mem, n, e.value, m)
        return m
    for mem in (pp.MEM_HOST, pp.MEM_DEVICE):
        rec = limited(pp, ctx, text, n, mem)
        try:
            sm.same(rec.host(), want)
            assert np.array_equal(rec.zp, want["zp"]) and np.array_equal(rec.lines(), want["line"]), (mem, n)
            assert (rec.n_rec, rec.seq_bytes, rec.n_bytes, rec.n_cig_total) == (len(want["flag"]), len(head), len(head), len(want["cigar"])), (mem, n)
            assert rec.first_empty_line() == tm.first_empty_line(head), (mem, n)
            if rec.n_rec:       # the object's copy of the text: the prefix, and nothing of what follows it
                got = ctx.download(rec.raw()["seq"], len(head), np.uint8).tobytes()
                assert got == head, (mem, n)
        finally:
            rec.close()
    return want


@pytest.fixture(scope="module")
def mixed():
    """records, header lines and empty lines in turn (sam_records_model.count_text): more lines than two placing workgroups"""
    scan, place = geometry()
    text = sm.count_text(2 * place + 1)
    assert tm.n_lines(text) > 2 * place + 1
    return text


def test_the_geometry_is_the_kernels():
    assert geometry() == (64, sm.SAM_BLOCK)


def test_limits_around_the_ends_and_the_workgroups(pp, ctx, mixed):
    scan, place = geometry()
    total = tm.n_lines(mixed)
    whole = check(pp, ctx, mixed, total)
    for n in (0, 1, total, total + 1, 1 << 40, scan - 1, scan, scan + 1, place - 1, place, place + 1):
        got = check(pp, ctx, mixed, n)
        assert isinstance(got, dict)
        if n >= total:
            assert len(got["flag"]) == len(whole["flag"])
        else:
            assert len(got["flag"]) == int((whole["line"] < n).sum()), n
    assert len(check(pp, ctx, mixed, 0)["flag"]) == 0


def test_a_limit_on_a_header_line_and_on_an_empty_line(pp, ctx, mixed):
    lines = mixed.split(b"\n")
    header = next(i for i, ln in enumerate(lines) if i > 70 and ln[:1] == b"@")
    empty = next(i for i, ln in enumerate(lines) if i > 70 and ln == b"")
    for n in (header, header + 1, empty, empty + 1):
        check(pp, ctx, mixed, n)
    rec = pp.SamRecords(ctx, mixed, n_lines=empty)
    first = tm.first_empty_line(mixed)
    assert first is not None and first < empty and rec.first_empty_line() == first
    rec.close()


def test_the_last_line_without_a_newline_and_crlf(pp, ctx):
    g, T = im.Gen(401), im.Text("\r\n")
    T.add("@HD\tVN:1.6")
    for i in range(9):
        T.add(g.line(nm=i % 3))
    crlf = T.bytes()
    assert crlf.endswith(b"\r\n")
    for text in (crlf, crlf[:-2], crlf[:-1]):           # ... no final newline; ... a last line that ends with its "\r"
        total = tm.n_lines(text)
        assert total == 10
        for n in (1, 2, total - 1, total):
            got = check(pp, ctx, text, n)
            assert len(got["flag"]) == n - 1
        assert tm.prefix(text, 2).endswith(b"\r\n"), "the cut lies behind the line's whole end"


def test_one_line_in_front_of_a_refused_line_gives_an_object_and_one_past_it_the_refusal(pp, ctx):
    for kind, (text, code, line) in sm.error_texts().items():
        got = check(pp, ctx, text, line)
        assert isinstance(got, dict) and len(got["flag"]) == 5, kind
        for n in (line + 1, line + 2):
            got = check(pp, ctx, text, n)
            assert isinstance(got, sm.SamError) and (got.code, got.bad_line) == (code, line), (kind, n)
    for kind, (text, line) in sm.limit_texts().items():
        if line is None:
            continue
        assert isinstance(check(pp, ctx, text, line), dict), kind
        with pytest.raises(pp.PolypolishError) as e:
            pp.SamRecords(ctx, text, n_lines=line + 1)
        assert (e.value.code, e.value.bad_record) == (pp.ERR_LIMIT, line), kind


HOSTILE = (("high_byte_at_the_limit", b"\x80\xff\n"),
           ("high_byte_inside_the_next_line", b"r\t0\tctg0\t1\t60\t4M\t*\t0\t0\tAC\x80T\t*\tNM:i:0\n"),
           ("too_few_columns", b"x\t0\tctg0\t1\n"),
           ("too_few_columns_no_newline", b"x\t0"),
           ("all_of_it", b"x\t0\n\x80\n\n@late\n" + b"\xfe" * 70000))


@pytest.mark.parametrize("case", HOSTILE, ids=lambda c: c[0])
def test_hostile_bytes_at_and_behind_the_limit_change_nothing(pp, ctx, case):
    """... where the text in device memory ends with its allocation (on_device: exactly len(text) bytes)"""
    g, T = im.Gen(402), im.Text()
    for i in range(70):
        T.add(g.line(nm=i % 3))
    good = T.bytes()
    want = sm.decode(good)
    text = good + case[1]
    with pytest.raises(pp.PolypolishError) as e:        # as a whole the text is refused
        pp.SamRecords(ctx, text)
    assert e.value.code in (pp.ERR_NOT_ASCII, pp.ERR_QUIT)
    got = check(pp, ctx, text, 70)
    sm.same(got, want)
    assert tm.prefix(text, 70) == good
    check(pp, ctx, text, 69)
    with pytest.raises(pp.PolypolishError) as e:        # one line more and the hostile line is in: refused as in the whole text
        pp.SamRecords(ctx, text, n_lines=71)
    assert e.value.code in (pp.ERR_NOT_ASCII, pp.ERR_QUIT)


def test_a_high_byte_in_front_of_the_limit_is_still_refused(pp, ctx):
    g, T = im.Gen(403), im.Text()
    for i in range(8):
        T.add(g.line(nm=0))
    text = T.bytes()
    bad = text.replace(b"\n", b"\tXX:Z:\xc3\xa9\n", 1) + b"\x80\n"
    for n in (1, 5, 8):
        with pytest.raises(pp.PolypolishError) as e:
            pp.SamRecords(ctx, bad, n_lines=n)
        assert e.value.code == pp.ERR_NOT_ASCII and e.value.bad_record is None


REC = "r{}\t0\tctg0\t1\t60\t4M\t*\t0\t0\tACGT\t*\tNM:i:0"
EMPTY_CASES = {
    "none": ["@HD\tVN:1.6", REC.format(1), REC.format(2)],
    "first": ["", REC.format(1), REC.format(2)],
    "last": [REC.format(1), REC.format(2), ""],
    "cr_only": [REC.format(1) + "\r", "\r", REC.format(2) + "\r"],
    "two": [REC.format(1), "", REC.format(2), "", REC.format(3)],
    "only_empty_lines": ["", "", ""],
}


@pytest.mark.parametrize("name", sorted(EMPTY_CASES))
def test_first_empty_line(pp, ctx, name):
    text = "".join(ln + "\n" for ln in EMPTY_CASES[name]).encode()
    want = {"none": None, "first": 0, "last": 2, "cr_only": 1, "two": 1, "only_empty_lines": 0}[name]
    assert tm.first_empty_line(text) == want
    for mem in (pp.MEM_HOST, pp.MEM_DEVICE):
        rec = limited(pp, ctx, text, 1 << 40, mem)
        assert rec.first_empty_line() == want, mem
        rec.close()
    rec = pp.SamRecords(ctx, text)          # pp_sam_records answers as well
    assert rec.first_empty_line() == want
    rec.close()
    if want is not None:                    # an empty line behind the limit is not seen; one line more and it is
        rec = pp.SamRecords(ctx, text, n_lines=want)
        assert rec.first_empty_line() is None
        rec.close()
        rec = pp.SamRecords(ctx, text, n_lines=want + 1)
        assert rec.first_empty_line() == want
        rec.close()
