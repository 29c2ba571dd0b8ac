"""tests/text_chain_model.py pinned to ingest_model's line splitting, and pp_aln_file_kind_text (host code, no device): what
pp_aln_file_kind answers, except that BGZF which does not hold BAM is bgzipped SAM text."""
import gzip
import os

import pytest

import bgzf_model as zm
import ingest_model as im
import polypolish_amd as pp
import text_chain_model as tm
from test_aln_file_kind_cpu import BAM, OTHER_SUBFIELD, SAM, put

REC = b"r1\t0\tctg\t1\t60\t4M\t*\t0\t0\tACGT\t*\tNM:i:0"
TEXTS = {
    "lf": b"@HD\tVN:1.6\n" + (REC + b"\n") * 3,
    "crlf": b"@HD\tVN:1.6\r\n" + (REC + b"\r\n") * 3,
    "no_final_newline": (REC + b"\n") * 2 + REC,
    "no_final_newline_cr": (REC + b"\r\n") * 2 + REC + b"\r",
    "runs_of_empty_lines": REC + b"\n\n\n\n" + REC + b"\n\r\n\r\n" + REC + b"\n\n",
    "empty_first": b"\n" + REC + b"\n",
    "cr_only_first": b"\r\n" + REC + b"\n",
    "header_behind_a_record": REC + b"\n@CO\tlate\n" + REC + b"\n",
    "one_line": REC,
    "only_a_newline": b"\n",
    "nothing": b"",
}


@pytest.mark.parametrize("name", sorted(TEXTS))
def test_prefix_is_the_first_lines_of_ingest_model(name):
    text = TEXTS[name]
    lines = im._lines(text)
    assert tm.n_lines(text) == len(lines)
    for n in range(len(lines) + 3):
        p = tm.prefix(text, n)
        assert text.startswith(p) and im._lines(p) == lines[:n], (name, n)
        assert n >= len(lines) or p == b"" or p.endswith(b"\n"), "a cut lies behind a newline"
    assert tm.prefix(text, 1 << 40) == text and tm.prefix(text, 0) == b""


@pytest.mark.parametrize("name", sorted(TEXTS))
def test_first_empty_line_is_ingest_model_s_first_line_without_a_byte(name):
    lines = im._lines(TEXTS[name])
    want = next((i for i, ln in enumerate(lines) if ln == ""), None)
    assert tm.first_empty_line(TEXTS[name]) == want
    for n in range(len(lines) + 1):         # an empty line behind the limit is not seen
        assert tm.first_empty_line(tm.prefix(TEXTS[name], n)) == (want if want is not None and want < n else None)


def test_the_cases_hold_what_they_are_named_after():
    assert tm.first_empty_line(TEXTS["runs_of_empty_lines"]) == 1 and tm.first_empty_line(TEXTS["cr_only_first"]) == 0
    assert tm.first_empty_line(TEXTS["lf"]) is None and tm.first_empty_line(TEXTS["no_final_newline_cr"]) is None
    assert tm.prefix(TEXTS["crlf"], 2).endswith(b"\r\n") and tm.prefix(TEXTS["no_final_newline"], 2) == (REC + b"\n") * 2


# ---- pp_aln_file_kind_text ----------------------------------------------------------------------------------------------------

def refused(path, *words):
    with pytest.raises(pp.PolypolishError) as e:
        pp.aln_file_kind_text(path)
    assert e.value.code == pp.ERR_QUIT, e.value
    for w in words:
        assert w in e.value.msg, (w, e.value.msg)
    assert os.path.basename(str(path)) in e.value.msg, "the message names the path"


def test_the_new_kind_is_the_header_s():
    text = open(os.path.join(pp.ROOT, "include", "polypolish_hip.h")).read()
    assert "enum { PP_ALN_SAM_BGZF = 3 };" in text and pp.ALN_SAM_BGZF == 3


def test_what_both_calls_answer_alike(tmp_path):
    one = zm.block(BAM, 6, extra_front=OTHER_SUBFIELD) + zm.EOF_BLOCK
    for name, data, kind in (("a.sam", SAM, pp.ALN_SAM), ("empty.sam", b"", pp.ALN_SAM), ("a.bam", one, pp.ALN_BAM),
                             ("spread.bam", zm.EOF_BLOCK + zm.block(BAM[:1], 0) + zm.block(BAM[1:], 6) + zm.EOF_BLOCK, pp.ALN_BAM),
                             ("cut.bam", one[:len(OTHER_SUBFIELD) + 18 + 12], pp.ALN_BAM), ("raw.bam", BAM, pp.ALN_BAM_RAW)):
        path = put(tmp_path, name, data)
        assert pp.aln_file_kind_text(path) == pp.aln_file_kind(path) == kind, name


def test_bgzipped_sam_is_its_own_kind_and_the_old_call_still_refuses_it(tmp_path):
    for name, data in (("a.sam.gz", zm.block(SAM, 6) + zm.EOF_BLOCK), ("only_eof.sam.gz", zm.EOF_BLOCK),
                       ("three_bytes.sam.gz", zm.block(b"BAM", 6) + zm.EOF_BLOCK),
                       ("spread.sam.gz", zm.block(SAM[:2], 0) + zm.EOF_BLOCK + zm.block(SAM[2:], 6) + zm.EOF_BLOCK)):
        path = put(tmp_path, name, data)
        assert pp.aln_file_kind_text(path) == pp.ALN_SAM_BGZF, name
        with pytest.raises(pp.PolypolishError) as e:
            pp.aln_file_kind(path)
        assert "is BGZF-compressed but does not hold BAM" in e.value.msg


def test_plain_gzip_and_a_cut_header_stay_refused(tmp_path):
    refused(put(tmp_path, "plain.sam.gz", gzip.compress(SAM)), "is gzip-compressed but not BGZF")
    refused(put(tmp_path, "plain.bam.gz", gzip.compress(BAM)), "is gzip-compressed but not BGZF")
    whole = zm.block(SAM, 6, extra_front=OTHER_SUBFIELD)
    header = 12 + len(OTHER_SUBFIELD) + 6
    for n in range(2, header):
        refused(put(tmp_path, f"cut_{n}.sam.gz", whole[:n]), "ends before a whole gzip header")
    refused(os.path.join(str(tmp_path), "nothing_here.sam"), "unable to load alignments from")


def test_the_one_process_per_gpu_launcher_refuses_the_flag_before_it_touches_a_device(tmp_path):
    from polypolish_amd import distributed
    fasta = put(tmp_path, "asm.fasta", b">ctg\n" + b"ACGT" * 25 + b"\n")
    with pytest.raises(SystemExit) as e:
        distributed.main(["polish", "--text_chain", fasta, put(tmp_path, "a.sam", SAM)])
    assert "runs on one GPU" in str(e.value.code) and "--text_chain" in str(e.value.code)
