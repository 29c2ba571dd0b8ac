"""tests/tabix_model.py, the definition of pp_tabix_index's bytes, held to what can be checked without the library and without a GPU:
the raw bytes of a hand-written two-contig BED and of a five-line VCF against bytes written out by hand; reg2bin at every level
boundary; and the model's own reader -- the bins of reg2bins cut by the linear index, the chunks read out of the text and out of a
real BGZF file (tests/bgzf_deflate_model.py) with zlib started at each chunk's block -- against a plain scan of the text, for random
texts of both presets and for the model's VCF, BED and bedGraph of the golden pair (tests/golden/derived_e2e), 200 random regions
each, with regions that touch nothing and names that are absent.  No `tabix` binary and no pysam are at hand, so that reader is the
check of the index, as bam_sort_model's was for the .bai.  Then every refusal with its code and line, and the binding's new rows."""
import os
import struct

import pytest

import bgzf_deflate_model as dfm
import tabix_model as tx

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "derived_e2e")


def test_a_hand_written_two_contig_bed():
    text = b"chrA\t10\t20\nchrA\t15\t16400\nchrB\t0\t5\n"      # lines at [0, 11), [11, 25), [25, 34)
    assert [(s, e) for s, e, _ in tx.cut(text)] == [(0, 11), (11, 25), (25, 34)]
    want = b"".join([
        b"TBI\1", struct.pack("<8i", 2, 0x10000, 1, 2, 3, 35, 0, 10), b"chrA\0chrB\0",
        # chrA: [10, 20) in bin 4681, [15, 16400) crosses a 16 kb boundary: bin 585; the bins in ascending number, then the pseudo-bin
        struct.pack("<i", 3),
        struct.pack("<IiQQ", 585, 1, 11, 25),
        struct.pack("<IiQQ", 4681, 1, 0, 11),
        struct.pack("<IiQQQQ", 37450, 2, 0, 25, 2, 0),
        struct.pack("<iQQ", 2, 0, 11),                          # window 0: the first line; window 1: only the second reaches it
        # chrB
        struct.pack("<i", 2),
        struct.pack("<IiQQ", 4681, 1, 25, 34),
        struct.pack("<IiQQQQ", 37450, 2, 25, 34, 1, 0),
        struct.pack("<iQ", 1, 25),
        struct.pack("<Q", 0)])
    assert tx.tbi_raw(text, tx.BED, [0, 65311]) == want
    # the block's place in the file goes into the high 48 bits; an end at the text's end stays in block 0 (34 < 65,280)
    moved = tx.tbi_raw(text, tx.BED, [4096, 70000])
    assert tx.parse_tbi(moved)["refs"][1]["bins"][4681] == [((4096 << 16) | 25, (4096 << 16) | 34)]
    t = tx.parse_tbi(want)
    assert (t["format"], t["col_seq"], t["col_beg"], t["col_end"], t["meta"], t["skip"], t["n_no_coor"]) == (0x10000, 1, 2, 3, 35, 0, 0)
    assert t["names"] == [b"chrA", b"chrB"]


def test_a_hand_written_five_line_vcf():
    lines = [b"##fileformat=VCFv4.2", b"#CHROM\tPOS\tID\tREF\tALT", b"c1\t5\t.\tAC\tA\t.\t.\t.", b"c1\t5\t.\tA\tG\t.\t.\t.", b"c2\t16385\t.\tA\tT\t.\t.\t."]
    text = tx.join(lines)
    assert [(s, e) for s, e, _ in tx.cut(text)] == [(0, 21), (21, 43), (43, 61), (61, 78), (78, 99)]
    want = b"".join([
        b"TBI\1", struct.pack("<8i", 2, 2, 1, 2, 0, 35, 0, 6), b"c1\0c2\0",
        # c1: POS 5 REF AC = [4, 6), POS 5 REF A = [4, 5): one bin, two consecutive lines, one chunk
        struct.pack("<i", 2),
        struct.pack("<IiQQ", 4681, 1, 43, 78),
        struct.pack("<IiQQQQ", 37450, 2, 43, 78, 2, 0),
        struct.pack("<iQ", 1, 43),
        # c2: POS 16385 = [16384, 16385) in window 1; the untouched window 0 takes window 1's value
        struct.pack("<i", 2),
        struct.pack("<IiQQ", 4682, 1, 78, 99),
        struct.pack("<IiQQQQ", 37450, 2, 78, 99, 1, 0),
        struct.pack("<iQQ", 2, 78, 78),
        struct.pack("<Q", 0)])
    assert tx.tbi_raw(text, tx.VCF, [0, 65311]) == want
    assert tx.tbi_raw(text[:-1], tx.VCF, [0, 65311]) == want.replace(struct.pack("<QQ", 78, 99), struct.pack("<QQ", 78, 98)), "a last line without a newline ends at the text's end"


def test_a_text_without_a_data_line():
    empty = b"TBI\1" + struct.pack("<8i", 0, 2, 1, 2, 0, 35, 0, 0) + struct.pack("<Q", 0)
    assert tx.tbi_raw(b"", tx.VCF, [0]) == empty
    assert tx.tbi_raw(b"##a\n#b\n", tx.VCF, [0, 40]) == empty


def test_reg2bin_at_every_level_boundary():
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        edge = 1 << shift
        up = {14: 585, 17: 73, 20: 9, 23: 1, 26: 0}[shift]        # the first bin of the level above
        assert tx.reg2bin(edge - 1, edge) == 4681 + ((edge - 1) >> 14), "ends AT the boundary: still the small bin"
        assert tx.reg2bin(edge, edge + 1) == 4681 + (edge >> 14)
        assert tx.reg2bin(edge - 1, edge + 1) == up, "across the boundary: the level above"
        assert tx.reg2bin(0, edge) == first and tx.reg2bin(0, edge + 1) == up
    assert tx.reg2bin((1 << 29) - 1, 1 << 29) == 37448 and tx.reg2bin(0, 1 << 29) == 0
    for beg, end in ((0, 1), (16383, 16385), (1 << 20, (1 << 20) + 5), (5, 1 << 28)):
        assert tx.reg2bin(beg, end) in tx.reg2bins(beg, end)


def _golden_texts(orc):
    import bed_model as bm
    import depth_model as dm
    import fasta_model as fm
    import vcf_model as vm
    fa = os.path.join(GOLDEN, "case.fasta")
    res = orc.polish_files(fa, [os.path.join(GOLDEN, f"case_{i}.sam") for i in (1, 2)], debug=True, positions=True)
    names, _, off, bases = fm.parse(open(fa, "rb").read())
    off = [int(x) for x in off]
    return [(tx.VCF, vm.from_debug_tsv(names, off, bases, res["debug"], "0")), (tx.BED, bm.bed(res["positions"]["status"], off, names, bm.ALL)),
            (tx.BED, dm.bedgraph(res["positions"]["depth"], off, names))]


def _reader_finds_what_the_scan_finds(text, preset, seed, file_and_blocks=None):
    f, blk = file_and_blocks if file_and_blocks else (None, tx.level0_blk_off(len(text)))
    raw = tx.tbi_raw(text, preset, blk)
    if f is None:                                             # the level-0 file: stored blocks, made here
        import bam_tag_model as tm
        f = tm.frame(text)
    rs = tx.rows(text, preset)
    hits = 0
    for name, beg, end in tx.random_regions(text, preset, seed):
        want = tx.scan(text, preset, name, beg, end, rs)
        assert tx.fetch(f, raw, preset, name, beg, end) == want, (name, beg, end)
        hits += bool(want)
    return hits


@pytest.mark.parametrize("preset", [tx.VCF, tx.BED])
def test_the_reader_finds_what_a_scan_finds_on_random_texts(preset):
    hits = 0
    for seed in range(20):
        text = tx.random_text(preset, seed)
        hits += _reader_finds_what_the_scan_finds(text, preset, seed)
    assert hits > 1000, "most regions touch a line: the test cannot pass on empty answers"


def test_the_reader_finds_what_a_scan_finds_on_the_golden_pairs_tracks(orc):
    for k, (preset, text) in enumerate(_golden_texts(orc)):
        assert len(tx.rows(text, preset)) > (3 if k < 2 else 500), k
        assert _reader_finds_what_the_scan_finds(text, preset, 100 + k) > 20, k


@pytest.mark.parametrize("preset", [tx.VCF, tx.BED])
def test_the_same_through_a_real_bgzf_file(preset):
    text = tx.random_text(preset, 7, n_lines=1500 if preset == tx.VCF else 4000, n_names=3)
    if preset == tx.VCF:                                      # one record longer than a block: the next line starts two blocks on
        lines = text.split(b"\n")
        at = next(i for i, ln in enumerate(lines) if ln[:1] != b"#")
        name, pos = lines[at].split(b"\t")[:2]
        lines.insert(at + 1, tx.vcf_line(name, int(pos), b"ACGT" * 17_500, b"<DEL>"))
        text = b"\n".join(lines)
    assert len(text) > tx.PAYLOAD
    f, blk, _ = dfm.deflate_file(text)
    assert len(blk) >= 3 and blk[1] != 65311
    assert _reader_finds_what_the_scan_finds(text, preset, 5, (f, blk)) > 50


def _refused(text, preset, code, line, kind, blk=None):
    with pytest.raises(tx.TabixError) as e:
        tx.tbi_raw(text, preset, tx.level0_blk_off(len(text)) if blk is None else blk)
    assert (e.value.code, e.value.bad_line, e.value.kind) == (code, line, kind), (text[:60], e.value)


def test_every_refusal_with_its_code_and_line():
    ok_b, ok_v = b"c\t1\t2\n", tx.vcf_line(b"c", 7) + b"\n"
    for bad, kind in ((b"\n", tx.EMPTY), (b"\t1\t2\n", tx.NAME), (b"c\t1\n", tx.COLUMN), (b"c\n", tx.COLUMN), (b"c\t1x\t2\n", tx.NUMBER), (b"c\t\t2\n", tx.NUMBER),
                      (b"c\t1\t\n", tx.NUMBER), (b"c\t1\t-2\n", tx.NUMBER), (b"c\t12345678901\t12345678902\n", tx.NUMBER), (b"c\t5\t4\n", tx.ENDBEG),
                      (b"c\t0\t3\n", tx.ORDER), (b"c\t1\t2 \n", tx.NUMBER)):
        _refused(b"#m\n" + ok_b + bad + ok_b, tx.BED, tx.ARG, 2, kind)
    for bad, kind in ((b"\n", tx.EMPTY), (b"\t1\t.\tA\tC\n", tx.NAME), (b"c\t9\t.\tA\n", tx.COLUMN), (b"c\t9\n", tx.COLUMN), (b"c\t0\t.\tA\tC\n", tx.POS0),
                      (b"c\t9\t.\t\tC\n", tx.REF), (b"c\t+9\t.\tA\tC\n", tx.NUMBER), (b"c\t6\t.\tA\tC\n", tx.ORDER)):
        _refused(b"##m\n#n\n" + ok_v + bad + ok_v, tx.VCF, tx.ARG, 3, kind)
    _refused(b"a\t1\t2\nb\t1\t2\n#x\na\t5\t6\n", tx.BED, tx.ARG, 3, tx.BACK)
    _refused(b"a\t1\t2\nb\t1\t2\na\t5\t6\nb\t0\tx\n", tx.BED, tx.ARG, 2, tx.BACK)     # the first of two offenders, in line order
    _refused(b"a\t1\t2\nb\t1\tx\na\t5\t6\n", tx.BED, tx.ARG, 1, tx.NUMBER)
    _refused(b"c\t5\t%d\n" % ((1 << 29) + 1), tx.BED, tx.LIMIT, 0, tx.END)
    _refused(tx.vcf_line(b"c", (1 << 29), b"AC") + b"\n", tx.VCF, tx.LIMIT, 0, tx.END)
    assert tx.tbi_raw(b"c\t5\t%d\n" % (1 << 29), tx.BED, [0, 30]) and tx.tbi_raw(tx.vcf_line(b"c", 1 << 29) + b"\n", tx.VCF, [0, 30])
    _refused(ok_b, 2, tx.ARG, None, tx.PRESET)
    _refused(ok_b, tx.BED, tx.ARG, None, tx.N_BLK, [0, 10, 20])
    _refused(ok_b, tx.BED, tx.ARG, None, tx.N_BLK, [0])
    _refused(ok_b, tx.BED, tx.LIMIT, None, tx.BLK, [0, 1 << 48])
    # what is NOT refused: end == beg, equal begs, a ninth column, a carriage return behind column 4
    t = tx.index_tables(b"c\t4\t4\nc\t4\t9\tx\ty\n", tx.BED, [0, 30])
    assert t[0]["lines"] == 2 and list(t[0]["bins"]) == [4681]


def test_the_binding_has_the_new_rows():
    import ctypes as C
    import inspect

    import polypolish_amd as pp
    assert len(pp.SIGNATURES["pp_tabix_index"][1]) == 11 and pp.SIGNATURES["pp_tabix_index"][0] is C.c_int
    order = list(pp.SIGNATURES)
    assert order.index("pp_tabix_index") == order.index("pp_bam_index") + 1
    assert "pp_tabix_stage_ms_" in pp.HOOKS and hasattr(pp.lib(), "pp_tabix_index")
    assert (pp.TBX_VCF, pp.TBX_BED, pp.TBX_LANE_BYTES) == (tx.VCF, tx.BED, tx.LANE_BYTES)
    head = open(os.path.join(pp.ROOT, "include", "polypolish_hip.h")).read()
    assert "#define PP_TBX_VCF 0" in head and "#define PP_TBX_BED 1" in head and "#define PP_TBX_LANE_BYTES %d" % tx.LANE_BYTES in head
    assert {"text", "preset", "blk_off", "mem"} <= set(inspect.signature(pp.tabix_index).parameters)
