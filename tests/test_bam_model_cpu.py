"""tests/bam_model.py -- the plain model of the BAM front end -- pinned from both sides, without a GPU:
  * decode(encode(text)) is gate_model.raw_from_text(text), the model of Alignment::new per SAM line, field by field: on
    synth.rich_dataset (both files, ZP:Z:fail on some lines) and on every named case of ingest_model's table, over the lines that
    have an equivalent BAM record (encode RAISES on the others: no SEQ character is mapped to N to make a case pass);
  * the two host helpers of the library, pp_bam_header and pp_bam_walk, are the model's header() / walk() on the same bytes and on
    every prefix of a small file: a cut either is PP_ERR_ARG or stops the walk cleanly at the cut, and no record runs past it;
  * the generated inputs of tests/test_bam_records_gpu.py have the shape that test relies on."""
import numpy as np
import pytest

import bam_model as bm
import gate_model as gm
import ingest_model as im
import synth

MAX_LINES = 20_000      # of a case's text: the long cases repeat their lines, and the two models are plain Python


def lines_that_encode(text, ref_names):
    """the text without the alignment lines that have no equivalent BAM record -> (text, lines kept, lines dropped)"""
    index = {n: i for i, n in enumerate(ref_names)}
    kept, dropped, out = 0, 0, []
    for ln in im._lines(text)[:MAX_LINES]:
        if ln and ln[0] != "@":
            try:
                bm.encode_line(ln, index)
            except bm.NotBam:
                dropped += 1
                continue
            kept += 1
        out.append(ln)
    return ("\n".join(out) + "\n").encode("ascii"), kept, dropped


def compare_with_the_text(contigs, text):
    """decode(encode(text)) against raw_from_text(text), record by record, by CONTENT (the rooms are pinned apart)"""
    names = [n for n, _ in contigs]
    enc = bm.encode(text, names, [len(s) for _, s in contigs])
    try:
        raw, zp = gm.raw_from_text(contigs, text)
    except gm.NotRaw as e:
        # Alignment::new refuses a line: the decode refuses the file, with the code of the reference's exit
        want = {"missing_NM_tag": bm.QUIT, "nm": bm.PANIC}
        assert e.args[0] in want, e.args[0]
        with pytest.raises(bm.BamError) as err:
            bm.decode(enc["records"], enc["rec_off"])
        assert err.value.code == want[e.args[0]]
        return 0
    got = bm.decode(enc["records"], enc["rec_off"])
    for k in ("flag", "contig", "ref_start", "nm", "seq_len", "n_cig"):
        assert got[k].dtype == raw[k].dtype and np.array_equal(got[k], raw[k]), k
    assert np.array_equal(got["zp"], zp)
    lines = [ln.split("\t") for ln in im._lines(text) if ln and ln[0] != "@"]
    assert len(lines) == len(got["flag"])
    b = enc["records"]
    for r, cols in enumerate(lines):
        so, sl, co, nc = int(got["seq_off"][r]), int(got["seq_len"][r]), int(got["cig_off"][r]), int(got["n_cig"][r])
        assert got["seq"][so:so + sl].tobytes() == (b"" if cols[9] == "*" else cols[9].upper().encode()), r
        ro = int(raw["cig_off"][r])
        assert np.array_equal(got["cigar"][co:co + nc], raw["cigar"][ro:ro + nc]), r
        no, nl = int(got["name_off"][r]), int(got["name_len"][r])
        assert b[no:no + nl] == cols[0].encode() and b[no + nl] == 0, r
    return len(lines)


def test_rich_dataset_through_bam_equals_the_text(tmp_path):
    ds = synth.rich_dataset(str(tmp_path), seed=23, contig_lens=(4000, 2500), coverage=30, repeat_len=400, repeat_copies=3, zp_frac=0.02)
    contigs = [(c.name, c.assembly) for c in ds["contigs"]]
    fails = 0
    for path in (ds["sam1"], ds["sam2"]):
        text = open(path, "rb").read()
        kept_text, kept, dropped = lines_that_encode(text, [n for n, _ in contigs])
        assert dropped == 0 and kept > 500, "every line of the dataset has a BAM record"
        assert compare_with_the_text(contigs, text) == kept
        fails += text.count(b"ZP:Z:fail")
    assert fails > 0


@pytest.mark.parametrize("name", sorted(im.CASES))
def test_named_cases_through_bam_equal_the_text(name):
    c = im.case(name)
    for text in c.texts:
        kept_text, kept, _ = lines_that_encode(text, [n for n, _ in c.contigs])
        if kept:
            compare_with_the_text(c.contigs, kept_text)


def test_most_of_the_table_encodes():
    kept = dropped = 0
    for name in ("details", "names", "seq_bytes", "stage_S_crlf", "files_MSL", "error_missing_NM_tag", "error_nm"):
        for text in im.case(name).texts:
            _, k, d = lines_that_encode(text, [n for n, _ in im.case(name).contigs])
            kept, dropped = kept + k, dropped + d
    assert kept > 1000 and kept > dropped


def test_encode_raises_instead_of_mapping():
    for seq in ("ACG.T", "ACGU", "ac-gt", "ACGX"):
        with pytest.raises(bm.NotBam):
            bm.pack_seq(seq)
    assert bm.pack_seq("acgtn=") == bytes([0x12, 0x48, 0xF0])
    line = "q\t0\tc\t1\t60\t0M4M\t*\t0\t0\tACGT\t*\tNM:i:0"
    with pytest.raises(bm.NotBam):
        bm.encode_line(line, {"c": 0})
    with pytest.raises(bm.NotBam):
        bm.encode_line(line.replace("0M4M", "4M").replace("\tc\t", "\tother\t"), {"c": 0})


def test_the_models_rooms():
    recs = [bm.record(b"a", 0, 0, 0, [(33 << 4)], "ACGTN" * 6 + "ACG", bm.aux("NM", "C", 0), seq_pad_nibble=0xF),
            bm.record(b"b", 256, 0, 0, [(33 << 4)], "", bm.aux("NM", "C", 0)),
            bm.record(b"c", 0, -1, -1, [(32 << 4)], "=" * 32, bm.aux("NM", "C", 0)),
            bm.record(b"d", 4, -1, -1, [], "N", b"")]
    b, off = bm.lay_out(recs, lead=3, pad=lambda i: i)
    d = bm.decode(b, off)
    assert d["seq_off"].tolist() == [0, 64, 64, 96] and d["seq_len"].tolist() == [33, 0, 32, 1] and len(d["seq"]) == 128
    assert d["seq"][:33].tobytes() == b"ACGTN" * 6 + b"ACG" and not d["seq"][33:64].any(), "the unused nibble does not get through"
    assert d["seq"][64:96].tobytes() == b"=" * 32 and d["seq"][96:].tobytes() == b"N" + bytes(31)
    assert d["contig"].tolist() == [0, 0, bm.NO_CONTIG, bm.NO_CONTIG] and d["ref_start"].tolist() == [0, 0, 0, 0]
    assert d["zp"].tolist() == [1, 1, 1] and d["cig_off"].tolist() == [0, 1, 2, 3]
    m = bm.decode(b, off[::-1], ref_map=[7, 5])      # one reference; entry 1 answers refID -1
    assert m["contig"].tolist() == [5, 5, 7, 7] and m["seq_len"].tolist() == [1, 32, 0, 33]


def test_defects_and_their_order():
    good = bm.record(b"g", 0, 0, 0, [(4 << 4)], "ACGT", bm.aux("NM", "C", 0))
    no_nm = bm.record(b"g", 0, 0, 0, [(4 << 4)], "ACGT", b"")
    neg = bm.record(b"g", 4, 0, 0, [(4 << 4)], "ACGT", bm.aux("NM", "c", -1) + bm.aux("NM", "C", 3))
    umax = bm.record(b"g", 0, 0, 0, [(4 << 4)], "ACGT", bm.aux("NM", "I", 0xFFFFFFFF))
    for kind, rec in bm.defect_records():
        b, off = bm.lay_out([good, no_nm, rec, good])
        with pytest.raises(bm.BamError) as e:
            bm.decode(b, off, ref_map=[0, 1, 2, 9])
        assert (e.value.code, e.value.kind, e.value.bad_record) == (bm.ARG, kind, 2), "a defect wins over an earlier refusal"
    for recs, want in (([good, no_nm, neg], (bm.QUIT, bm.MISSING_NM, 1)), ([good, neg, no_nm], (bm.PANIC, bm.PANIC_NM, 1)),
                       ([umax], (bm.QUIT, bm.MISSING_NM, 0))):
        b, off = bm.lay_out(recs)
        with pytest.raises(bm.BamError) as e:
            bm.decode(b, off)
        assert (e.value.code, e.value.kind, e.value.bad_record) == want
    b, off = bm.lay_out([good, good])
    for cut, o in ((0, len(b) + 1), (0, len(b) - 3), (0, 1 << 63), (1, int(off[1]))):      # ... and a last record one byte short
        with pytest.raises(bm.BamError) as e:
            bm.decode(b[:len(b) - cut], [0, o])
        assert (e.value.kind, e.value.bad_record) == (bm.RANGE, 1)
    assert bm.decode(bm.defect_records()[7][1], [0])["contig"].tolist() == [3], "without a ref_map a refID has no upper bound"


def test_generated_inputs_have_the_shape_the_gpu_test_relies_on():
    recs = bm.seam_records()
    assert len(recs) == len(bm.SEAM_LENS) * 8
    for lead in (0, 1):
        b, off = bm.lay_out(recs, lead, lambda i: (3 * i) % 7 if i + 1 < len(recs) else 0)
        d = bm.decode(b, off)
        assert int(off[0]) == lead and off[-1] + len(recs[-1]) == len(b), "the last record ends at the last byte"
        cig_at = d["name_off"] + d["name_len"] + 1
        seq_at = cig_at + 4 * d["n_cig"].astype(np.uint64)
        has = d["seq_len"] > 0
        assert set((cig_at % 8).tolist()) == set(range(8)) and set((seq_at[has] % 8).tolist()) == set(range(8))
        assert set(zip(d["seq_len"].tolist(), (d["name_len"] + 1).tolist())) == {(a, n) for a in bm.SEAM_LENS for n in range(2, 10)}
        assert set(d["seq"].tolist()) == set(bm.NIBBLE.encode()) | {0}, "all 16 codes"
    kinds = [k for k, _ in bm.defect_records()]
    assert set(kinds) == {bm.BLOCK, bm.NAME, bm.CIGAR_OP, bm.REF_ID, bm.AUX}
    b, off = bm.lay_out(bm.mixed_records())
    d = bm.decode(b, off)
    assert len(off) > 4 * bm.BAM_BLOCK and (d["zp"] == 0).sum() > 100 and (d["flag"] & 4).sum() > 100 and (d["seq_len"] == 0).sum() > 100


# ---- the library's host helpers (no device) ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pp():
    import polypolish_amd
    polypolish_amd.lib()
    return polypolish_amd


def small_file():
    refs = [("contig_1", 4000), ("c2", 2500), ("", 7)]
    recs = [r for _, r, _, _ in bm.aux_records()[:9]] + bm.seam_records()[:12]
    body, off = bm.lay_out(recs)
    head = bm.header_bytes(refs, "@HD\tVN:1.6\n@SQ\tSN:contig_1\tLN:4000\n")
    return head, body, off, refs


def test_header_and_walk_equal_the_model(pp):
    head, body, off, refs = small_file()
    data = head + body
    got, want = pp.bam_header(data), bm.header(data)
    assert got["names"] == want["names"] == [n.encode() for n, _ in refs] and got["records_at"] == want["records_at"] == len(head)
    for k in ("name_off", "name_len", "ref_len"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    rec_off, end = pp.bam_walk(data, got["records_at"])
    assert np.array_equal(rec_off, off + np.uint64(len(head))) and end == len(data)
    assert (bm.walk(data, len(head))[0], bm.walk(data, len(head))[1]) == (rec_off.tolist(), end)
    rec_off, end = pp.bam_walk(body)
    assert np.array_equal(rec_off, off) and end == len(body)
    assert pp.bam_walk(b"")[0].size == 0 and pp.bam_walk(data, len(data)) [1] == len(data)
    with pytest.raises(pp.PolypolishError) as e:
        pp.bam_walk(body, len(body) + 1)
    assert e.value.code == pp.ERR_ARG and "behind" in e.value.msg


def test_header_cap_and_filling_by_pieces(pp):
    import ctypes as C
    head, body, off, refs = small_file()
    L = pp.lib()
    b = np.frombuffer(head + body, np.uint8)
    n_ref, at = C.c_uint32(0), C.c_uint64(0)
    no, nl, rl = np.zeros(2, np.uint64), np.zeros(2, np.uint32), np.zeros(2, np.uint32)
    rc = L.pp_bam_header(b.ctypes.data, len(b), 2, C.byref(n_ref), no.ctypes.data, nl.ctypes.data, rl.ctypes.data, C.byref(at))
    assert rc == pp.ERR_ARG and n_ref.value == 3 and nl.tolist() == [8, 2] and rl.tolist() == [4000, 2500]
    assert b"room for 2" in L.pp_bam_last_error()
    # the walk in pieces of five records: every call goes on where the one before stopped
    got, start = [], len(head)
    while True:
        piece, n, end = np.zeros(5, np.uint64), C.c_uint64(0), C.c_uint64(0)
        assert L.pp_bam_walk(b.ctypes.data, len(b), start, piece.ctypes.data, 5, C.byref(n), C.byref(end)) == pp.OK
        got += piece[:n.value].tolist()
        if n.value < 5:
            break
        start = end.value
    assert got == (off + np.uint64(len(head))).tolist() and end.value == len(b)


def test_every_truncation_is_refused_or_stops_at_the_cut(pp):
    head, body, off, _ = small_file()
    data = head + body[:int(off[4])]        # the header and four records: every prefix of it
    ends = set((off[:5] + np.uint64(len(head))).tolist())
    for cut in range(len(data) + 1):
        piece = data[:cut]
        try:
            want = bm.header(piece)
        except bm.BamError:
            want = None
        try:
            got = pp.bam_header(piece)
        except pp.PolypolishError as e:
            assert e.code == pp.ERR_ARG and e.msg and want is None, cut
            continue
        assert want is not None and got["records_at"] == want["records_at"] == len(head) and cut >= len(head), cut
        w_off, w_end, w_ok = bm.walk(piece, len(head))
        try:
            rec_off, end = pp.bam_walk(piece, len(head))
        except pp.PolypolishError as e:
            assert e.code == pp.ERR_ARG and not w_ok and (e.n_rec, e.end) == (len(w_off), w_end) and cut not in ends, cut
            assert e.end + 4 > cut or e.end + 4 + bm._le32(piece, e.end) > cut, "the refused record does run past the cut"
            continue
        assert w_ok and cut in ends and end == cut and rec_off.tolist() == w_off, cut
        assert all(int(o) + 4 + bm._le32(piece, int(o)) <= cut for o in rec_off), "no record runs past the cut"
    # a block_size below the fixed part, among good records
    bad = bytearray(body)
    bad[int(off[2]):int(off[2]) + 4] = (31).to_bytes(4, "little")
    with pytest.raises(pp.PolypolishError) as e:
        pp.bam_walk(bytes(bad))
    assert (e.value.code, e.value.n_rec, e.value.end) == (pp.ERR_ARG, 2, int(off[2])) and "block_size" in e.value.msg
    bad[int(off[2]):int(off[2]) + 4] = (0xFFFFFFFF).to_bytes(4, "little")      # ... and one no sum may wrap over
    with pytest.raises(pp.PolypolishError) as e:
        pp.bam_walk(bytes(bad))
    assert (e.value.n_rec, e.value.end) == (2, int(off[2]))
