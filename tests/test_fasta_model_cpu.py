"""tests/fasta_model.py, the plain model pp_fasta_records is held against on the GPU (tests/test_fasta_records_gpu.py), pinned to the
two loaders that exist without one: pp_assembly_load (the product's host loader) and the oracle's orc_load_fasta, on the model's own
generated texts -- LF and CRLF, a lone '\\r' inside a line and at the end of a last line without a newline, runs of empty lines,
every Unicode White_Space form directly behind '>' and behind the name, unnamed headers in front of a header and at the end, lower
case and IUPAC bases, blanks inside sequence lines, every refusal with its code and words, and two refusals in one text in either
order.  This pins the model; it passes without the device link, and that is its purpose.  No GPU."""
import ctypes as C

import pytest

import fasta_model as fm


class OrcFasta(C.Structure):
    _fields_ = [("n", C.c_size_t), ("name", C.POINTER(C.c_char_p)), ("desc", C.POINTER(C.c_char_p)),
                ("seq", C.POINTER(C.c_void_p)), ("len", C.POINTER(C.c_size_t))]


def product(path):
    """pp_assembly_load on a file -> the model's tuple, or (code, words)"""
    import polypolish_amd as pp
    L = pp.lib()
    a, err = C.c_void_p(), C.create_string_buffer(1024)
    rc = L.pp_assembly_load(path.encode(), C.byref(a), err, 1024)
    if rc:
        return rc, fm.words_of(err.value.decode(), path)
    try:
        n = L.pp_assembly_n_contigs(a)
        off = [int(L.pp_assembly_offsets(a)[i]) for i in range(n + 1)]
        bases = C.string_at(L.pp_assembly_bases(a), off[-1])
        return [L.pp_assembly_name(a, i) for i in range(n)], [L.pp_assembly_description(a, i) for i in range(n)], off, bases
    finally:
        L.pp_assembly_free(a)


def oracle(orc, path):
    """orc_load_fasta on a file -> the model's tuple, or (code, words)"""
    L = orc.lib()
    f, err = OrcFasta(), C.create_string_buffer(1024)
    rc = L.orc_load_fasta(path.encode(), C.byref(f), err, C.c_size_t(1024))
    if rc:
        return rc, fm.words_of(err.value.decode(), path)
    try:
        seqs = [C.string_at(f.seq[i], f.len[i]) for i in range(f.n)]
        off = [0]
        for s in seqs:
            off.append(off[-1] + len(s))
        return [f.name[i] for i in range(f.n)], [f.desc[i] for i in range(f.n)], off, b"".join(seqs)
    finally:
        L.orc_fasta_free(C.byref(f))


def modelled(text):
    try:
        return fm.parse(text)
    except fm.FastaError as e:
        return e


@pytest.mark.parametrize("name", sorted(fm.CASES))
def test_model_against_both_loaders(orc, tmp_path, name):
    text = fm.CASES[name]
    want = modelled(text)
    assert isinstance(want, fm.FastaError) == name.startswith("r_"), "the case's name says whether it is refused"
    p = tmp_path / "a.fasta"
    p.write_bytes(text)
    got = product(str(p))
    if len(text) < 2:  # is_file_gzipped refuses such a FILE before any loader reads a line; the model speaks of texts
        assert got == oracle(orc, str(p)) == (fm.QUIT, "is too small")
        return
    if isinstance(want, fm.FastaError):
        assert got == (want.code, want.words)
    else:
        assert got == want
    # the oracle: the reference's loader takes a sequence line with a byte >= 0x80 that is valid UTF-8 (the product's documented limit)
    if isinstance(want, fm.FastaError) and want.code == fm.LIMIT:
        return
    ref = oracle(orc, str(p))
    if isinstance(want, fm.FastaError):
        assert ref == (want.code, want.words)
    else:
        assert ref == want


def test_bad_line_counts_every_line():
    """bad_line is the 0-based index among ALL lines, empty ones and headers included; refusals behind the walk name none"""
    for name, line in (("r_no_header", 0), ("r_no_header_after_empty", 2), ("r_bases_behind_unnamed", 3), ("r_header_truncated_utf8", 2),
                       ("r_sequence_non_ascii", 1), ("r_non_ascii_then_bad_header", 1), ("r_bad_header_then_non_ascii", 0),
                       ("r_headless_then_non_ascii", 0), ("r_non_ascii_then_headless", 1), ("r_limit_then_not_utf8", 1),
                       ("r_duplicate", None), ("r_empty_text", None), ("r_empty_sequence_last", None)):
        with pytest.raises(fm.FastaError) as e:
            fm.parse(fm.CASES[name])
        assert e.value.bad_line == line, name


def test_the_words_of_every_refusal_occur():
    seen = {(e.code, e.words) for e in map(modelled, fm.CASES.values()) if isinstance(e, fm.FastaError)}
    assert seen == {(fm.QUIT, fm.NOT_FORMATTED), (fm.QUIT, fm.UNABLE), (fm.LIMIT, fm.NOT_ASCII), (fm.QUIT, fm.NO_SEQUENCES),
                    (fm.QUIT, fm.EMPTY_SEQUENCE), (fm.QUIT, fm.DUPLICATED)}
