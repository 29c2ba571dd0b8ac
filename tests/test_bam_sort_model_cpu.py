"""tests/bam_sort_model.py pinned (no GPU): the header rewrite against hand-written headers in each of the four @HD cases, with and
without NUL padding; the key and the order against a hand-written file made by bam_model's encoder; reg2bin at every level boundary;
a .bai worked out by hand for three records; and the semantic check of the index -- region queries through the model's plain reader
over the golden pair, sorted and compressed by the models, find what a brute-force scan finds.  The binding's rows for the new symbols
are held here too: they need the built library only."""
import os
import struct

import numpy as np
import pytest

import bam_model as bm
import bam_sort_model as sm
import bam_tag_model as tm
import bgzf_deflate_model as dm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "derived_e2e")
REFS = [("a", 9), ("bb", 10)]
TABLE = struct.pack("<i", 2) + struct.pack("<i", 2) + b"a\0" + struct.pack("<i", 9) + struct.pack("<i", 3) + b"bb\0" + struct.pack("<i", 10)


def head(text):
    return b"BAM\1" + struct.pack("<i", len(text)) + text + TABLE


HD = b"@HD\tVN:1.6\tSO:coordinate\n"
CASES = [   # the text, the text of the sorted file
    (b"@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:a\tLN:9\n", b"@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:a\tLN:9\n"),           # an SO: field: replaced
    (b"@HD\tSO:queryname\tVN:1.0\tGO:query\n", b"@HD\tSO:coordinate\tVN:1.0\tGO:query\n"),                             # ... wherever it stands
    (b"@HD\tVN:1.5\n@CO\tSO:x\n", b"@HD\tVN:1.5\tSO:coordinate\n@CO\tSO:x\n"),                                       # none: appended
    (b"@HD\tVN:1.5\r\n@CO\tx\r\n", b"@HD\tVN:1.5\tSO:coordinate\r\n@CO\tx\r\n"),                                     # ... in front of a CR
    (b"@HD", b"@HD\tSO:coordinate"),                                                                                # ... of a line that does not end
    (b"@SQ\tSN:a\tLN:9\n@HD\tVN:1.0\tSO:unsorted\n", HD + b"@SQ\tSN:a\tLN:9\n@HD\tVN:1.0\tSO:unsorted\n"),         # no @HD line first
    (b"@HDX\tSO:unsorted\n", HD + b"@HDX\tSO:unsorted\n"),                                                           # (@HDX is none)
    (b"", HD),                                                                                                       # no text
]


@pytest.mark.parametrize("pad", (b"", b"\0", b"\0\0\0\0\0"))
@pytest.mark.parametrize("case", range(len(CASES)))
def test_the_header_rewrite_against_hand_written_headers(case, pad):
    text, want = CASES[case]
    got = sm.head_sorted(head(text + pad))
    assert got == head(want + pad), "the NULs behind the text and the reference table are kept byte for byte"
    assert sm.head_sorted(got) == got, "what says SO:coordinate stays as it is"
    assert bm.header(got)["names"] == [b"a", b"bb"]


def test_what_is_no_header_is_refused():
    good = head(CASES[0][0])
    for bad in (good[:-1], good + b"x", b"BAM\2" + good[4:], good[:4] + b"\xff\xff\xff\x7f" + good[8:], b""):
        with pytest.raises(sm.SortError) as e:
            sm.head_sorted(bad)
        assert e.value.code == sm.ARG


SAM = "\n".join(["@HD\tVN:1.6", "@SQ\tSN:a\tLN:900", "@SQ\tSN:bb\tLN:1000",
                 "r0\t0\tbb\t5\t60\t4M\t*\t0\t0\tACGT\t*\tNM:i:0",       # key (1, 4 + 1, +)
                 "r1\t16\ta\t7\t60\t4M\t*\t0\t0\tACGT\t*\tNM:i:0",       # key (0, 6 + 1, -)
                 "r2\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\t*",                  # unplaced: pos -1
                 "r3\t0\ta\t7\t60\t4M\t*\t0\t0\tACGT\t*\tNM:i:1",        # key (0, 6 + 1, +): in front of r1
                 "r4\t16\ta\t7\t60\t2M2S\t*\t0\t0\tACGT\t*\tNM:i:0",     # r1's key: behind it
                 "r5\t4\ta\t1\t0\t*\t*\t0\t0\tACGT\t*",                  # unmapped but placed: stands at its position
                 "r6\t0\tbb\t5\t60\t4M\t*\t0\t0\tACGT\t*\tNM:i:2", ""])  # r0's key: behind it


def encoded():
    enc = bm.encode(SAM, ["a", "bb"], [900, 1000])
    return enc["header"] + enc["records"], len(enc["header"]), enc["rec_off"] + np.uint64(len(enc["header"]))


def test_key_and_order_on_a_hand_written_file():
    b, at, off = encoded()
    k, flag = sm.keys(b, at, off)
    assert [hex(int(x)) for x in k] == ["0x10000000a", "0xf", "0xffffffff00000000", "0xe", "0xf", "0x2", "0x10000000a"]
    assert flag.tolist() == [0, 16, 4, 0, 16, 4, 0]
    s = sm.sort(b, at, off)
    assert s["perm"].tolist() == [5, 3, 1, 4, 0, 6, 2] and s["counts"] == (7, 1)
    assert s["head"] == bm.header_bytes([("a", 900), ("bb", 1000)], "@HD\tVN:1.6\tSO:coordinate\n")
    assert np.array_equal(s["rec_off"], off[s["perm"]])
    passed = np.array([1, 0, 1, 0, 1], np.uint8)                     # r0 r1 r3 r4 r6
    assert sm.carry_pass(flag, s["perm"], passed).tolist() == [1, 0, 0, 1, 1], "r3 r1 r4 r0 r6"
    u = sm.sorted_stream(b, at, off, passed)
    names = [u[o + 36:o + 38] for o in bm.walk(u, len(s["head"]))[0]]
    assert names == [b"r5", b"r3", b"r1", b"r4", b"r0", b"r6", b"r2"]
    assert u.count(tm.TAG) == 2 and sm.sort(u, len(s["head"]), bm.walk(u, len(s["head"]))[0])["counts"][0] == 0


def test_the_key_s_edges():
    assert sm.key_of(0, -1, 0) == 0 and sm.key_of(0, -1, 16) == 1 and sm.key_of(-1, -1, 0) == 0xFFFFFFFF00000000
    assert sm.key_of(5, 2 ** 31 - 2, 16) == (5 << 32) | 0xFFFFFFFF
    assert sm.key_of(5, 2 ** 31 - 1, 0) == 5 << 32, "the low word is 32 bits: pos + 1 == 2^31 leaves it"
    for bad in (sm.rec(0, -2), sm.rec(-2, 0), sm.rec(3, 0)):
        with pytest.raises(sm.SortError) as e:
            sm.sort(*sm.stream([sm.rec(0, 1), bad]))
        assert (e.value.code, e.value.bad_record) == (sm.ARG, 1)


def test_reg2bin_at_every_level_boundary():
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        edge = 1 << shift
        assert sm.reg2bin(edge - 1, edge) == 4681 + ((edge - 1) >> 14) and sm.reg2bin(edge, edge + 1) == 4681 + (edge >> 14), "one base: the lowest level"
        assert sm.reg2bin(edge, 2 * edge) == first + 1, "the level's second bin, whole"
        parent = {14: 585, 17: 73, 20: 9, 23: 1, 26: 0}[shift]
        assert sm.reg2bin(edge - 1, edge + 1) == parent, "across the boundary: the level above (whose first bin holds both sides)"
        assert sm.reg2bin(0, edge) == first and sm.reg2bin(0, edge + 1) == parent
    assert sm.reg2bin(0, 1 << 29) == 0 and sm.reg2bin((1 << 29) - 1, 1 << 29) == 4681 + 32767 == 37448
    assert sm.reg2bin(7 << 14, (7 << 14) + 1) == 4688 and sm.reg2bin((3 << 26) - 1, (3 << 26) + 1) == 0
    for beg, end in ((0, 1), (16383, 16385), (1 << 20, (1 << 20) + 5), (5, 1 << 29)):
        assert sm.reg2bin(beg, end) in sm.reg2bins(beg, end)
    assert sm.reg2bins(0, 1) == [0, 1, 9, 73, 585, 4681] and len(sm.reg2bins(0, 1 << 29)) == 37449


def test_a_bai_worked_out_by_hand_for_three_records():
    A = sm.rec(0, 100, 0, b"A")                          # [100, 104): bin 4681, window 0
    B = sm.rec(0, 16380, 16, b"B", n=10)                 # [16380, 16390): over 2^14 -> bin 585, windows 0 and 1
    U = sm.rec(-1, -1, 4, b"U")
    header = bm.header_bytes([("a", 20000), ("none", 5)], "@HD\tVN:1.6\tSO:coordinate\n")
    b, at, off = sm.stream([A, B, U], header)
    a0 = at
    a1 = a0 + len(A) + 8                                 # A fails: eight bytes behind it
    b1 = a1 + len(B)
    want = (b"BAI\1" + struct.pack("<i", 2)
            + struct.pack("<i", 3)
            + struct.pack("<IiQQ", 585, 1, a1, b1)
            + struct.pack("<IiQQ", 4681, 1, a0, a1)
            + struct.pack("<IiQQQQ", 37450, 2, a0, b1, 2, 0)
            + struct.pack("<iQQ", 2, a0, a1)
            + struct.pack("<ii", 0, 0)
            + struct.pack("<Q", 1))
    u_len = len(sm.tagged_head(b, at, off, [0, 1], header))
    assert sm.bai(b, at, off, [0, 1], 2, sm.level0_blk_off(u_len)) == want
    moved = sm.bai(b, at, off, [0, 1], 2, [5000, 9000])            # another block table: every offset moves by blk_off[0] << 16
    refs, n_no_coor = sm.parse_bai(moved)
    assert n_no_coor == 1 and refs[0]["bins"][4681] == [((5000 << 16) | a0, (5000 << 16) | a1)] and refs[0]["linear"] == [(5000 << 16) | a0, (5000 << 16) | a1]
    assert refs[1] == {"bins": {}, "linear": []}
    assert sm.query(want, 0, 16385, 16386) == [(a1, b1)] and sm.query(want, 0, 0, 16384) == [(a1, b1), (a0, a1)][::-1]
    assert sm.query(want, 0, 40000, 40001) == [] and sm.query(want, 1, 0, 5) == []


def test_what_the_index_refuses():
    header = bm.header_bytes([("a", 1 << 29), ("b", 5)], "")
    ok = [sm.rec(0, 5), sm.rec(0, 5), sm.rec(1, 0), sm.rec(-1, 7, 4), sm.rec(-1, 3, 4)]
    b, at, off = sm.stream(ok, header)
    sm.bai(b, at, off, [1, 1, 1], 2, [0, 70000])
    for recs, code, kind, bad in (([sm.rec(0, 5), sm.rec(0, 4)], sm.ARG, sm.ORDER, 1), ([sm.rec(1, 0), sm.rec(0, 9)], sm.ARG, sm.ORDER, 1),
                                  ([sm.rec(-1, 0, 4), sm.rec(0, 9)], sm.ARG, sm.ORDER, 1), ([sm.rec(0, -1)], sm.ARG, sm.PLACED, 0),
                                  ([sm.rec(2, 1)], sm.ARG, sm.REF, 0), ([sm.rec(0, (1 << 29) - 3, n=4)], sm.LIMIT, sm.END, 0)):
        b, at, off = sm.stream(recs, header)
        n_al = sum(1 for r in recs if not r[18] & 4)
        with pytest.raises(sm.SortError) as e:
            sm.bai(b, at, off, [1] * n_al, 2, [0, 70000])
        assert (e.value.code, e.value.kind, e.value.bad_record) == (code, kind, bad)
    b, at, off = sm.stream([sm.rec(0, (1 << 29) - 4, n=4)], header)
    refs, _ = sm.parse_bai(sm.bai(b, at, off, [1], 2, [0, 70000]))
    assert list(refs[0]["bins"]) == [37448, 37450] and len(refs[0]["linear"]) == 32768, "a record that ends exactly at 2^29"
    with pytest.raises(sm.SortError) as e:
        sm.bai(b, at, off, [1], 2, [0, 1 << 48])
    assert e.value.code == sm.LIMIT


@pytest.fixture(scope="module")
def golden_files():
    """per file of the golden pair: (the sorted stream, its header's length, the compressed file, its .bai)"""
    out = []
    lens = {}
    for ln in open(os.path.join(GOLDEN, "case.fasta")).read().split(">")[1:]:
        name, seq = ln.split("\n", 1)
        lens[name.split()[0]] = len(seq.replace("\n", ""))
    for f in (1, 2):
        text = open(os.path.join(GOLDEN, f"case_{f}.sam")).read()
        names = [ln.split("\t")[1][3:] for ln in text.split("\n") if ln.startswith("@SQ")]
        enc = bm.encode(text, names, [lens[n] for n in names])
        b, at, off = enc["header"] + enc["records"], len(enc["header"]), enc["rec_off"] + np.uint64(len(enc["header"]))
        s = sm.sort(b, at, off)
        n_al = int(((s["flag"] & 4) == 0).sum())
        passed = (np.arange(n_al) % 5 != 0).astype(np.uint8)
        v = sm.carry_pass(s["flag"], s["perm"], passed)
        u = sm.tagged_head(b, at, s["rec_off"], v, s["head"])
        z, blk_off, _ = dm.deflate_file(u)
        out.append((u, len(s["head"]), z, sm.bai(b, len(s["head"]), s["rec_off"], v, len(names), blk_off), len(names)))
    return out


def overlapping(u, n_head, tid, beg, end):
    """brute force: the stream offsets of the records of reference tid that overlap [beg, end)"""
    out = []
    for o in bm.walk(u, n_head)[0]:
        pos, e, _, ref_id = sm.ref_end(u, o)
        if ref_id == tid and pos < end and e > beg:
            out.append(o)
    return out


def test_region_queries_through_the_index_find_what_a_scan_finds(golden_files):
    rng = np.random.default_rng(2024)
    for u, n_head, z, bai, n_ref in golden_files:
        starts = bm.walk(u, n_head)[0]
        assert len(starts) > 200
        ref_len = bm.header(u)["ref_len"]
        regions = []
        for o in starts:                                             # every record's own interval
            pos, e, _, ref_id = sm.ref_end(u, o)
            if ref_id >= 0:
                regions.append((ref_id, pos, e))
        for _ in range(200):
            tid = int(rng.integers(0, n_ref))
            beg = int(rng.integers(0, ref_len[tid]))
            regions.append((tid, beg, beg + int(rng.integers(1, 3000))))
        seen = {}
        for tid, beg, end in regions:
            chunks = sm.query(bai, tid, beg, end)
            key = tuple(chunks)
            if key not in seen:                                       # (decoding is the slow part: once per chunk list)
                seen[key] = set(sm.read_chunks(z, chunks))
            want = overlapping(u, n_head, tid, beg, end)
            assert set(want) <= seen[key], (tid, beg, end)
        refs, n_no_coor = sm.parse_bai(bai)
        assert n_no_coor == sum(1 for o in starts if sm.fields(u, o)[0] < 0)
        for R in refs:                                                # every chunk of every bin lies between two records
            for bin_, chunks in R["bins"].items():
                if bin_ != sm.PSEUDO_BIN:
                    sm.read_chunks(z, chunks)


def test_the_binding_has_the_new_symbols():
    import polypolish_amd as pp
    L = pp.lib()
    for name in ("pp_bam_tagged_head", "pp_bam_sort", "pp_bam_sorted_perm", "pp_bam_sorted_rec_off", "pp_bam_sorted_head", "pp_bam_sorted_counts",
                 "pp_bam_sorted_pass", "pp_bam_sorted_kernel_ms", "pp_bam_sorted_free", "pp_bam_index", "pp_ctx_set_sort_out"):
        assert name in pp.SIGNATURES and hasattr(L, name), name
    assert list(pp.SIGNATURES).index("pp_bam_tagged_head") == list(pp.SIGNATURES).index("pp_bam_tagged") + 1
    assert "pp_bam_sorted_stage_ms_" in pp.HOOKS and callable(pp.BamSorted.close) and pp.BamSorted.__doc__
    assert callable(pp.BamIndex.close) and pp.BamIndex.__doc__ and callable(pp.Context.set_sort_out)
