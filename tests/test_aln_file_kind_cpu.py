"""pp_aln_file_kind: SAM text, BAM behind BGZF or uncompressed BAM, told by the head of a file -- and the inputs it refuses with their
words.  The helper is host code and needs no device.  The BGZF files are the model's (tests/bgzf_model.py), the BAM bytes the BAM
model's (tests/bam_model.py)."""
import gzip
import os
import struct

import pytest

import bam_model as bm
import bgzf_model as zm
import polypolish_amd as pp

SAM = b"@SQ\tSN:ctg\tLN:100\nr1\t0\tctg\t1\t60\t4M\t*\t0\t0\tACGT\t*\tNM:i:0\n"
BAM = (bm.header_bytes([("ctg", 100)], "@SQ\tSN:ctg\tLN:100\n")
       + bm.record(b"r1", 0, 0, 0, [4 << 4], "ACGT", bm.aux("NM", "C", 0)))
OTHER_SUBFIELD = b"XY" + struct.pack("<H", 3) + b"abc"          # a subfield in front of BC: BC is not the first


def put(tmp_path, name, data):
    p = os.path.join(str(tmp_path), name)
    with open(p, "wb") as f:
        f.write(data)
    return p


def refused(path, *words):
    with pytest.raises(pp.PolypolishError) as e:
        pp.aln_file_kind(path)
    assert e.value.code == pp.ERR_QUIT, e.value
    for w in words:
        assert w in e.value.msg, (w, e.value.msg)
    assert os.path.basename(str(path)) in e.value.msg, "the message names the path"


def test_the_kind_constants_are_the_header_s():
    text = open(os.path.join(pp.ROOT, "include", "polypolish_hip.h")).read()
    assert "enum { PP_ALN_SAM = 0, PP_ALN_BAM = 1, PP_ALN_BAM_RAW = 2 };" in text
    assert (pp.ALN_SAM, pp.ALN_BAM, pp.ALN_BAM_RAW) == (0, 1, 2)


def test_sam_text_and_an_empty_file_are_text(tmp_path):
    assert pp.aln_file_kind(put(tmp_path, "a.sam", SAM)) == pp.ALN_SAM
    assert pp.aln_file_kind(put(tmp_path, "empty.sam", b"")) == pp.ALN_SAM
    assert pp.aln_file_kind(put(tmp_path, "one.sam", b"\x1f")) == pp.ALN_SAM, "a lone 1f is no gzip magic: the text route says what it is"
    assert pp.aln_file_kind(put(tmp_path, "bam_without_its_01.sam", b"BAM")) == pp.ALN_SAM


def test_bgzf_bam_whose_bc_subfield_is_not_the_first(tmp_path):
    one = zm.block(BAM, 6, extra_front=OTHER_SUBFIELD) + zm.EOF_BLOCK
    assert pp.aln_file_kind(put(tmp_path, "a.bam", one)) == pp.ALN_BAM
    # the four bytes spread over several blocks, an empty block in front, stored and compressed blocks
    spread = zm.EOF_BLOCK + zm.block(BAM[:1], 0) + zm.block(BAM[1:3], 6) + zm.block(BAM[3:], 6) + zm.EOF_BLOCK
    assert pp.aln_file_kind(put(tmp_path, "spread.bam", spread)) == pp.ALN_BAM
    # a file that ends inside its first block is still BAM by its head: the inflate names the truncation
    assert pp.aln_file_kind(put(tmp_path, "cut.bam", one[:len(OTHER_SUBFIELD) + 18 + 12])) == pp.ALN_BAM


def test_raw_bam(tmp_path):
    assert pp.aln_file_kind(put(tmp_path, "raw.bam", BAM)) == pp.ALN_BAM_RAW
    assert pp.aln_file_kind(put(tmp_path, "magic_only.bam", b"BAM\1")) == pp.ALN_BAM_RAW


def test_gzip_that_is_not_bgzf_is_refused(tmp_path):
    refused(put(tmp_path, "plain.bam.gz", gzip.compress(BAM)), "is gzip-compressed but not BGZF")
    refused(put(tmp_path, "plain.sam.gz", gzip.compress(SAM)), "is gzip-compressed but not BGZF")
    # FEXTRA with subfields, none of them BC
    raw = zm.deflate(BAM)
    head = struct.pack("<4BI2BH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, len(OTHER_SUBFIELD)) + OTHER_SUBFIELD
    refused(put(tmp_path, "extra_no_bc.gz", head + raw + struct.pack("<II", 0, len(BAM))), "is gzip-compressed but not BGZF")


def test_bgzipped_sam_is_refused(tmp_path):
    refused(put(tmp_path, "a.sam.gz", zm.block(SAM, 6) + zm.EOF_BLOCK), "is BGZF-compressed but does not hold BAM")
    refused(put(tmp_path, "only_eof.bam", zm.EOF_BLOCK), "is BGZF-compressed but does not hold BAM")


def test_a_gzip_file_cut_inside_its_header_is_refused_at_every_length(tmp_path):
    whole = zm.block(BAM, 6, extra_front=OTHER_SUBFIELD)
    header = 12 + len(OTHER_SUBFIELD) + 6
    for n in range(2, header):
        refused(put(tmp_path, f"cut_{n}.bam", whole[:n]), "ends before a whole gzip header")
    assert pp.aln_file_kind(put(tmp_path, "header_only.bam", whole[:header])) == pp.ALN_BAM, "a whole header: BGZF, the rest is the inflate's to judge"


def test_a_missing_path_is_refused_in_the_drivers_words(tmp_path):
    missing = os.path.join(str(tmp_path), "nothing_here.bam")
    refused(missing, "unable to load alignments from")


def test_the_one_process_per_gpu_launcher_refuses_bam_before_it_touches_a_device(tmp_path):
    from polypolish_amd import distributed
    fasta = put(tmp_path, "asm.fasta", b">ctg\n" + b"ACGT" * 25 + b"\n")
    bam = put(tmp_path, "a.bam", zm.block(BAM, 6) + zm.EOF_BLOCK)
    with pytest.raises(SystemExit) as e:
        distributed.main(["polish", fasta, put(tmp_path, "a.sam", SAM), bam])
    assert "runs on one GPU" in str(e.value.code) and bam in str(e.value.code)
    with pytest.raises(SystemExit) as e:
        distributed.main(["polish", fasta, put(tmp_path, "plain.gz", gzip.compress(SAM))])
    assert "is gzip-compressed but not BGZF" in str(e.value.code)


def test_a_path_that_is_no_regular_file_is_not_opened(tmp_path):
    fifo = os.path.join(str(tmp_path), "pipe.sam")
    os.mkfifo(fifo)
    assert pp.aln_file_kind(fifo) == pp.ALN_SAM, "a pipe is text, and nobody has read a byte of it"
