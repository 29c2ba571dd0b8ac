"""tests/sam_records_model.py -- the plain model of pp_sam_records -- pinned without a GPU:
  * on mutated SAM texts (synth.mutate_sam over a small synth.rich_dataset text) its per-record arrays are those of
    gate_model.raw_from_text -- the only way to raw records from text so far -- and, over the lines that have a BAM record, those of
    bam_model.decode(bam_model.encode(text)): the two front ends of the record chain make one batch;
  * every refusal: the kinds of ingest_model._parse with code and line, the three LIMIT lines and their neighbours that fit, the
    first-line-wins order, bytes >= 0x80;
  * the generated inputs of tests/test_sam_records_gpu.py have the shape that test relies on."""
import numpy as np
import pytest

import bam_model as bm
import gate_model as gm
import ingest_model as im
import sam_records_model as sm
import synth

N_TEXTS, MUTATE_SEED = 60, 5


@pytest.fixture(scope="module")
def base(tmp_path_factory):
    ds = synth.rich_dataset(str(tmp_path_factory.mktemp("sam_model")), seed=31, contig_lens=(1200, 700), coverage=6, zp_frac=0.05,
                            unaligned_frac=0.05)
    return [(c.name, c.assembly) for c in ds["contigs"]], open(ds["sam1"], "rb").read().decode("ascii")


@pytest.fixture(scope="module")
def texts(base):
    rng = np.random.default_rng(MUTATE_SEED)
    return [base[1].encode()] + [synth.mutate_sam(base[1], rng, n_mut=int(rng.integers(1, 4))).encode("ascii") for _ in range(N_TEXTS)]


def same_as_raw(dec, raw, zp, upper=False):
    """the model's arrays against a raw batch whose SEQ bytes lie elsewhere: by value, SEQ and CIGAR gathered"""
    for k in ("flag", "ref_start", "nm", "n_cig", "seq_len"):
        assert dec[k].dtype == raw[k].dtype and np.array_equal(dec[k], raw[k]), k
    assert np.array_equal(dec["cigar"], raw["cigar"]) and np.array_equal(dec["cig_off"], raw["cig_off"])
    assert dec["zp"].dtype == np.uint8 and np.array_equal(dec["zp"], zp)
    theirs = raw["seq"].tobytes()
    for r, mine in enumerate(sm.seq_bytes(dec)):
        so, sl = int(raw["seq_off"][r]), int(raw["seq_len"][r])
        assert (mine.upper() if upper else mine) == theirs[so:so + sl], r


def test_mutated_texts_against_raw_from_text(base, texts):
    contigs, _ = base
    taken = refused = 0
    for text in texts:
        try:
            raw, zp = gm.raw_from_text(contigs, text)
        except gm.NotRaw:
            with pytest.raises(sm.SamError):
                sm.decode(text)
            refused += 1
            continue
        try:
            dec = sm.decode(text)
        except sm.SamError as e:       # the one thing raw_from_text takes and a raw batch cannot tell: an aligned line with an empty SEQ
            assert (e.code, e.kind) == (sm.LIMIT, "empty_seq")
            refused += 1
            continue
        same_as_raw(dec, raw, zp)
        assert np.array_equal(dec["seq"], np.frombuffer(text, np.uint8)) and not dec["read_id"].any() and not dec["contig"].any()
        lines = im._lines(text)
        assert sm.column(dec, "name") == [lines[li].split("\t")[0].encode() for li in dec["line"]]
        assert sm.column(dec, "rname") == [lines[li].split("\t")[2].encode() for li in dec["line"]]
        taken += 1
    assert 3 * taken >= len(texts) and 3 * refused >= len(texts), (taken, refused)


def lines_with_a_bam_record(text, ref_names):
    """the text without the alignment lines that have no BAM record of their own (an empty SEQ column has none: l_seq 0 is "*")"""
    index = {n: i for i, n in enumerate(ref_names)}
    out, kept = [], 0
    for ln in im._lines(text):
        if ln and ln[0] != "@":
            try:
                bm.encode_line(ln, index)
            except bm.NotBam:
                continue
            if ln.split("\t")[9] == "":
                continue
            kept += 1
        out.append(ln)
    return ("\n".join(out) + "\n").encode("ascii"), kept


def test_mutated_texts_against_the_bam_front_end(base, texts):
    contigs, _ = base
    names = [n for n, _ in contigs]
    taken = refused = 0
    for text in texts:
        kept, n = lines_with_a_bam_record(text, names)
        assert n > 40
        enc = bm.encode(kept, names, [len(s) for _, s in contigs])
        try:
            want = bm.decode(enc["records"], enc["rec_off"])
        except bm.BamError as e:        # Alignment::new's refusals that survive the encoding: the same code, the same record
            with pytest.raises(sm.SamError) as mine:
                sm.decode(kept)
            before = sum(1 for ln in im._lines(kept)[:mine.value.bad_line] if ln and ln[0] != "@")
            assert (mine.value.code, before) == (e.code, e.bad_record)
            refused += 1
            continue
        same_as_raw(sm.decode(kept), want, want["zp"], upper=True)
        taken += 1
    assert taken > 10 and refused > 5, (taken, refused)


def test_every_error_kind_of_the_parse_with_its_code_and_line():
    cases = sm.error_texts()
    assert set(cases) == {"too_few_columns", "missing_NM_tag", "invalid_cigar", "flag", "pos", "nm", "cigar_overflow"}
    for kind, (text, code, line) in cases.items():
        with pytest.raises(sm.SamError) as e:
            sm.decode(text)
        assert (e.value.code, e.value.bad_line, e.value.kind) == (code, line, kind)
        with pytest.raises(im.ModelError) as m:     # ... and the same line, alone, is what ingest_model's parse refuses
            im._parse(im._lines(text)[line], "text", line + 1)
        assert (m.value.code, m.value.kind) == (code, kind)


def test_the_limit_lines_and_their_neighbours():
    cases = sm.limit_texts()
    for kind in ("flag_above_u16", "pos_above_u32", "empty_seq"):
        text, line = cases[kind]
        with pytest.raises(sm.SamError) as e:
            sm.decode(text)
        assert (e.value.code, e.value.bad_line, e.value.kind) == (sm.LIMIT, line, kind)
        im._parse(im._lines(text)[line], "text", line + 1)      # the reference takes the line
    fits = sm.decode(cases["fits"][0])
    assert fits["flag"].tolist() == [65531, 0, 4, 0] and fits["ref_start"].tolist()[1] == (1 << 32) - 2
    assert fits["seq_len"].tolist() == [24, 24, 0, 0] and len(fits["zp"]) == 3


def test_the_first_refused_line_wins_whatever_its_kind():
    got = []
    for text, code, line in sm.two_bad_lines():
        with pytest.raises(sm.SamError) as e:
            sm.decode(text)
        assert (e.value.code, e.value.bad_line) == (code, line)
        got.append(code)
    assert got == [sm.PANIC, sm.QUIT, sm.LIMIT, sm.QUIT]
    # a line that is refused by the parse AND beyond a limit: the parse's refusal (the reference never takes the line)
    g = im.Gen(1)
    with pytest.raises(sm.SamError) as e:
        sm.decode((g.line(flag=70000, cigar="5Q") + "\n").encode())
    assert e.value.code == sm.QUIT


def test_a_byte_outside_ascii_refuses_the_text_as_pp_dev_ingest_sam_does():
    """pp_dev_ingest_sam answers PP_ERR_NOT_ASCII for a byte >= 0x80 anywhere in the file -- a header, QUAL, behind a refused line --
    before it parses a line (newline_index's flag, pp_devtext.h): so does this decode, and it names no line"""
    g, T = im.Gen(2), im.Text()
    T.add("@CO\tcomment")
    T.add("x\t0")           # too few columns: refused, if anybody parsed it
    T.add(g.line())
    plain = T.bytes()
    with pytest.raises(sm.SamError) as e:
        sm.decode(plain)
    assert (e.value.code, e.value.bad_line) == (sm.QUIT, 1)
    for at in (5, len(plain) - 2):      # in the header in front of the refused line, and in the last line
        odd = bytearray(plain)
        odd[at] = 0xC3
        with pytest.raises(sm.SamError) as e:
            sm.decode(bytes(odd))
        assert (e.value.code, e.value.bad_line) == (sm.NOT_ASCII, None)
    sm.decode(plain.replace(b"x\t0\n", b"").replace(b"comment", b"\x7f\x01\x7e"))   # 0x7F and control bytes are ASCII


# ---- the generated inputs of tests/test_sam_records_gpu.py ------------------------------------------------------------------------
def test_the_record_count_texts():
    assert sm.RECORD_COUNTS == (1, 63, 64, 65, 1023, 1024, 1025, 2049)
    for n in sm.RECORD_COUNTS:
        dec = sm.decode(sm.count_text(n))
        assert len(dec["flag"]) == n and (dec["flag"][0::2] & 4 == 0).all() and (dec["flag"][1::2] & 4 == 4).all()
        assert len(dec["zp"]) == (n + 1) // 2 and (n < 3 or not dec["zp"].all())
        assert dec["line"][0] == 1 and (n < 3 or dec["line"][-1] > n), "header and empty lines in between"
        assert n < 64 or (set(dec["n_cig"].tolist()) == {0, 1, 2, 3, 4, 5} and dec["cig_off"][-1] > n)
    for n in (sm.SAM_BLOCK - 1, sm.SAM_BLOCK, sm.SAM_BLOCK + 1):
        dec = sm.decode(sm.count_text(n, plain=True))
        assert dec["line"].tolist() == list(range(n)), "a line per record: the workgroup's edge is a record's"


def test_the_cigar_text():
    text, n_cig = sm.cigar_text()
    dec = sm.decode(text)
    assert dec["n_cig"].tolist() == n_cig == [1, 0, 1, 2, 1, 0, 1, 2, 4, 9, 1, 40, 1]
    runs = [dec["cigar"][int(o):int(o) + int(n)].tolist() for o, n in zip(dec["cig_off"], dec["n_cig"])]
    M = sm.MAX_RUN << 4
    assert runs[6:9] == [[M], [M, 1 << 4], [M, M, M, 1 << 4]] and runs[9] == [(1 << 4) | op for op in range(9)]
    assert runs[3] == [15 << 4, 15 << 4] and runs[2] == runs[4] == [30 << 4]


def test_the_tag_text():
    text, nm, zp = sm.tag_text()
    dec = sm.decode(text)
    assert dec["nm"].tolist() == nm and dec["zp"].tolist() == zp
    assert zp.count(0) == 6 and nm.count(sm.NO_NM) == 5 and 7 in nm and 8 in nm
    lines = im._lines(text)
    assert lines[0].count("\t") == 10 and lines[1].endswith("\t") and lines[2].endswith("\t")


def test_the_array_end_cases():
    for name, whole, n in sm.array_end_cases():
        assert whole[n:n + len(sm.HOSTILE)] == sm.HOSTILE and whole.endswith(b"\n")
        if name in ("behind_lf", "behind_cr"):  # the hostile bytes are a refused line of their own, or make the last line's NM "0\r"
            with pytest.raises(sm.SamError) as e:
                sm.decode(whole)
            assert (e.value.code, e.value.bad_line) == ((sm.QUIT, 70) if name == "behind_lf" else (sm.PANIC, 69))
        else:
            beyond = sm.decode(whole)
            assert len(beyond["flag"]) == 71
        if name == "inside_a_line":
            with pytest.raises(sm.SamError) as e:
                sm.decode(whole[:n])
            assert (e.value.code, e.value.bad_line) == (sm.QUIT, 69)
            continue
        dec = sm.decode(whole[:n])
        assert len(dec["flag"]) == 70 and dec["zp"].all()
        assert whole[n - 1:n] == {"line_end": b"0", "behind_cr": b"\r", "behind_lf": b"\n"}[name]
        if name == "line_end":      # the hostile bytes would change the last record
            assert beyond["nm"][69] == 7 and dec["nm"][69] == 0 and beyond["zp"][69] == 0
