"""The plain model of the ingest (tests/ingest_model.py) pinned on the CPU, on every named case the GPU tests of the device
tokenizer use (tests/test_tokenizer_seam_gpu.py: the same table, the same seeds): the model's arrays are the host ingest's
(pp_ingest_* needs no GPU) -- array by array in file order, the same records when window-grouped --, its error is the host
ingest's and the oracle's, and for the cases that are valid jobs the oracle polishing the model's records gives the bytes of
the oracle polishing the files.  Every case's declared shape is checked here as well: the staging instance each file takes, how
many of its lines are not staged, the blocks of the window split, the windows of the assembly, QNAME and read lengths -- a case
that was meant to straddle a boundary and does not fails here, before a GPU sees it."""
import numpy as np
import pytest

import ingest_model as im
from layout_check import check_seq_layout, check_window_order_mirror, same_records

# what the host ingest says where the reference panics (the panic's own text is the Rust runtime's)
PANIC_TEXT = {"flag": "could not parse the FLAG column", "pos": "could not parse the POS column", "nm": "could not parse the NM tag",
              "cigar_overflow": "CIGAR run length does not fit u32", "empty_cigar": "has an empty CIGAR",
              "start_past_u32": "starts past the end of", "empty_group": "no aligned records to process",
              "verdict_count": "filter verdicts for the"}


@pytest.fixture(scope="module")
def pp():
    import polypolish_amd
    return polypolish_amd


def check_shape(c, m):
    """what the case declares about itself, against the restated staging and split of ingest_model and the model's records"""
    sh = dict(c.shape)
    stagings = [im.staging(t) for t in c.texts]
    if "stage" in sh:
        assert [s[0] for s in stagings] == sh.pop("stage")
    if "unstaged" in sh:
        assert [int((~s[1]).sum()) for s in stagings] == sh.pop("unstaged")
    if "unstaged_min" in sh:
        assert all(int((~s[1]).sum()) >= n for s, n in zip(stagings, sh.pop("unstaged_min")))
    if "size" in sh:
        assert [len(t) for t in c.texts] == sh.pop("size")
    if "n_win" in sh:
        assert im.n_windows(c.contigs) == sh.pop("n_win")
    if "nb" in sh:
        assert [im.split_blocks(a) for a, _, _ in m["counts"]] == sh.pop("nb")
    if "name_lens" in sh:
        assert sh.pop("name_lens") <= m["name_lens"]
    if "read_lens" in sh:
        assert sh.pop("read_lens") <= set(m["recs"]["seq_len"].tolist())
    if "max_k" in sh:
        assert int(m["recs"]["k"].max()) == sh.pop("max_k")
    assert not sh, ("a declared shape nobody checks", sh)


@pytest.mark.parametrize("name", list(im.CASES))
def test_model_is_the_host_ingest_and_the_oracle(orc, pp, tmp_path, name):
    c = im.case(name)
    fa, sams = im.write_case(c, tmp_path)
    try:
        m, merr = c.model(sams), None
    except im.ModelError as e:
        m, merr = None, e
    assert (None if merr is None else (merr.code, merr.kind)) == c.error, merr
    kw = dict(max_errors=c.max_errors, careful=c.careful, verdicts=c.verdicts)
    try:
        host, herr = pp.ingest(fa, sams, seq_layout=0, **kw), None
    except pp.PolypolishError as e:
        host, herr = None, e
    if c.verdicts is None:
        try:
            want, oerr = orc.polish_files(fa, sams, max_errors=c.max_errors, careful=c.careful), None
        except orc.OrcError as e:
            want, oerr = None, e
    if merr is not None:
        assert herr is not None and herr.code == merr.code, (herr, merr)
        if merr.msg is not None:
            assert herr.msg == merr.msg
        else:
            assert PANIC_TEXT[merr.kind] in herr.msg, herr.msg
        if c.verdicts is None:
            assert oerr is not None and oerr.code == merr.code, (oerr, merr)
            if merr.msg is not None:
                assert oerr.msg == merr.msg
        return
    assert herr is None, herr
    check_shape(c, m)
    names, _, off, bases, recs, counts = host
    assert names == [n for n, _ in c.contigs]
    assert bases.tobytes() == "".join(s for _, s in c.contigs).encode()
    assert counts == m["counts"], (counts, m["counts"])
    for k, want_arr in m["recs"].items():
        assert recs[k].dtype == want_arr.dtype and np.array_equal(recs[k], want_arr), (k, np.flatnonzero(recs[k] != want_arr)[:5]
                                                                                 if len(recs[k]) == len(want_arr) else (len(recs[k]), len(want_arr)))
    used = [cnt[1] for cnt in counts]
    grouped = pp.ingest(fa, sams, seq_layout=1, **kw)
    same_records(m["recs"], grouped[4])
    check_seq_layout(grouped[4], off, used, grouped=True, file_order_inside=True)
    if len(recs["contig"]):
        check_window_order_mirror(grouped[4], off, used, file_order_inside=True)
    if c.verdicts is None:
        if not c.valid_job:
            assert oerr is not None, "the case says the oracle refuses this job"
            return
        assert oerr is None, (oerr.code, oerr.msg)
        assert want["counts"] == tuple(sum(cnt[i] for cnt in counts) for i in range(3))
        assert orc.polish_records(off, bases, m["recs"])["polished"] == im.seqs(want["fasta"])


def test_every_family_has_the_cases_it_was_given():
    """the counts the GPU tests rely on, for the model alone: every family has cases, the error family has quits and panics, the
    cases that run end to end are valid jobs, one per family that has one"""
    fam = {}
    for name in im.CASES:
        fam.setdefault(im.case(name).family, []).append(name)
    assert set(fam) == set(im.FAMILIES)
    for f in ("stage_S", "stage_M", "stage_L"):
        assert len(fam[f]) >= 7
    codes = [im.case(n).error for n in fam["errors"]]
    assert sum(c is not None and c[0] == im.QUIT for c in codes) >= 6 and sum(c is not None and c[0] == im.PANIC for c in codes) >= 6
    assert sum(im.case(n).error is None for n in im.CASES) >= 45
    assert all(im.case(n).valid_job and im.case(n).verdicts is None for n in im.END_TO_END)
    assert {im.case(n).family for n in im.END_TO_END} == set(im.FAMILIES) - {"details", "errors"}
    assert sum(im.case(n).filter_pair for n in im.CASES) >= 20


def test_mate_texts_have_the_shape_of_their_first_files():
    """the second file of a pair for the filter (the same lines on the other strand): same sizes, same line ends, so the same
    staging instance and the same unstaged lines"""
    for name in im.CASES:
        c = im.case(name)
        if not c.filter_pair:
            continue
        mate = im.case(name, mate=True)
        for a, b in zip(c.texts, mate.texts):
            assert len(a) == len(b) and a != b, name
            assert np.array_equal(im.line_spans(a)[1], im.line_spans(b)[1]), name


def test_the_restated_staging_on_hand_made_texts():
    """tok_stage_for and the staged predicate on texts small enough to check by hand"""
    assert im.tok_stage_for(220 * 100, 100) == "S" and im.tok_stage_for(221 * 100, 100) == "M"
    assert im.tok_stage_for(359 * 100, 100) == "M" and im.tok_stage_for(360 * 100, 100) == "L"
    assert im.tok_stage_for(0, 0) == "S"
    one = b"x" * 16327 + b"\n"                       # end 16327: 16327 + 8 <= 16320 + 16 is false
    assert im.staging(one)[0] == "L"                 # (a single long line picks L, where it fits)
    text = (b"y" * 9 + b"\n") * 2000 + b"x" * (16328 - 8) + b"\n"     # 2000 lines: wave 31 starts at line 1984, byte 19840
    inst, staged = im.staging(text)
    assert inst == "S" and staged[:2000].all()
    # a0 = 19840; the long line ends at 20000 + 16320 = 36320: 36320 - 19840 + 8 = 16488 > 16336
    assert not staged[2000]
    assert im.split_blocks(16384) == 1 and im.split_blocks(16385) == 2 and im.split_blocks(64 * 16384 + 1) == 65
