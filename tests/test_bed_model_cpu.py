"""tests/bed_model.py pinned without a GPU: every word against hand-written bytes; on the golden pair (tests/golden/derived_e2e) the BED
built from the status column of the ORACLE's --debug TSV equals the BED built from its per-position records, the summed record
lengths per status are the counts of that status, and masked().upper() gives the oracle's polished bytes back; the hand-built jobs of
tests/bed_jobs.py are what they are built to be; the parser of the status list; the binding has the new rows."""
import os

import numpy as np
import pytest

import bed_jobs as bj
import bed_model as bm
import fasta_model as fm
import fasta_text_model as tm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "derived_e2e")


def test_hand_written_bytes_for_every_word():
    #                0  1  2  3  4  5  6  7  8  9 10 11 | 12 13 14
    status = bytes([0, 0, 1, 2, 2, 2, 3, 4, 4, 5, 0, 5, 5, 5, 2])
    off, names = [0, 12, 12, 15], [b"one", b"empty", b"two two;=<>"]
    assert bm.bed(status, off, names, bm.ALL) == (b"one\t0\t2\tkept\none\t2\t3\tchanged\none\t3\t6\tlow_depth\none\t6\t7\tnone\none\t7\t9\tmultiple\n"
                                                  b"one\t9\t10\ttoo_close\none\t10\t11\tkept\none\t11\t12\ttoo_close\n"
                                                  b"two two;=<>\t0\t2\ttoo_close\ntwo two;=<>\t2\t3\tlow_depth\n")
    # the default mask: the four undecided ones; the run 11..14 of too_close is split at the contig boundary
    assert bm.bed(status, off, names) == (b"one\t3\t6\tlow_depth\none\t6\t7\tnone\none\t7\t9\tmultiple\none\t9\t10\ttoo_close\none\t11\t12\ttoo_close\n"
                                          b"two two;=<>\t0\t2\ttoo_close\ntwo two;=<>\t2\t3\tlow_depth\n")
    assert bm.UNDECIDED == 0b111100 and bm.bed(status, off, names, 1 << bm.CHANGED) == b"one\t2\t3\tchanged\n"
    # an unselected status between two runs of one selected status keeps them apart; two selected ones side by side are two records
    assert bm.bed(bytes([2, 0, 2, 3]), [0, 4], ["c"], bm.UNDECIDED) == b"c\t0\t1\tlow_depth\nc\t2\t3\tlow_depth\nc\t3\t4\tnone\n"
    assert bm.bed(b"", [0], [], bm.ALL) == b"" and bm.bed(b"", [0, 0], [b"c"], bm.ALL) == b"" and bm.bed(bytes([0, 1]), [0, 2], [b"c"]) == b""
    assert bm.counts(status, off, bm.ALL) == (3, 1, 4, 1, 2, 4) and bm.counts(status, off) == (0, 0, 4, 1, 2, 4)
    assert bm.parse(bm.bed(status, off, names))[5] == (b"two two;=<>", 0, 2, b"too_close")
    assert bm.bed(bytes([3]) * 1_000_001, [0, 1_000_001], [b"c"]) == b"c\t0\t1000001\tnone\n"


def test_hand_written_masked_bytes():
    #  position      0     1    2     3    4    5
    emit_len = [1, 0, 3, 1, 1, 2]
    status = [bm.KEPT, bm.CHANGED, bm.MULTIPLE, bm.LOW_DEPTH, bm.KEPT, bm.CHANGED]
    pol = b"A" + b"" + b"CgT" + b"N" + b"*" + b"GA"
    assert bm.masked(pol, emit_len, status) == b"Acgtn*GA"
    assert bm.masked(pol, emit_len, status, 1 << bm.CHANGED) == b"ACgTN*ga"  # (a position that emits nothing changes nothing)
    assert bm.masked(pol, emit_len, status, bm.ALL) == b"acgtn*ga"
    assert bm.masked(b"", [], []) == b""


def test_the_parser_of_the_status_list():
    assert bm.parse_status_list("low_depth,none,multiple,too_close") == bm.UNDECIDED
    assert bm.parse_status_list(b"kept") == 1 and bm.parse_status_list("changed,kept,changed") == 3
    for bad in ("", ",", "kept,", ",kept", "kept,,none", "Kept", "kept ", "low-depth", "all"):
        with pytest.raises(ValueError):
            bm.parse_status_list(bad)
    import polypolish_amd as pp
    assert pp.STATUS_WORDS == tuple(w.decode() for w in bm.WORDS) and pp.BED_UNDECIDED == bm.UNDECIDED
    for ok in ("low_depth,none", "kept", "too_close,changed,multiple"):
        assert pp.bed_status_mask(ok) == bm.parse_status_list(ok)
    assert pp.bed_status_mask(None) == bm.UNDECIDED and pp.bed_status_mask(5) == 5 and pp.bed_status_mask(["kept", "none"]) == 9
    for bad in ("", "kept,", "Kept", []):
        with pytest.raises(pp.PolypolishError):
            pp.bed_status_mask(bad)


@pytest.fixture(scope="module")
def golden(orc):
    fa = os.path.join(GOLDEN, "case.fasta")
    res = orc.polish_files(fa, [os.path.join(GOLDEN, f"case_{i}.sam") for i in (1, 2)], debug=True, positions=True)
    names, _, off, bases = fm.parse(open(fa, "rb").read())
    return names, off, res


def test_the_debug_tsv_and_the_positions_give_the_same_bed_on_the_golden_pair(golden):
    names, off, res = golden
    st_tsv, st_pos = bm.status_of_debug_tsv(res["debug"]), res["positions"]["status"]
    assert np.array_equal(st_tsv, st_pos)
    for mask in (bm.UNDECIDED, bm.ALL, 1 << bm.CHANGED):
        text = bm.bed(st_tsv, off, names, mask)
        assert text == bm.bed(st_pos, off, names, mask)
        recs = bm.parse(text)
        assert len(recs) >= 1, "the golden pair has records: the test cannot pass empty"
        for s in range(6):  # per status, the summed record lengths are the count of that status
            n = sum(b - a for _, a, b, w in recs if w == bm.WORDS[s])
            assert n == (int((st_pos == s).sum()) if (mask >> s) & 1 else 0) == bm.counts(st_pos, off, mask)[s]
        assert all(0 <= a < b for _, a, b, _ in recs) and [r[0] for r in recs] == sorted((r[0] for r in recs), key=names.index)


def test_masked_upper_is_the_oracles_polished_bytes(golden):
    names, off, res = golden
    pos = res["positions"]
    polished = b"".join(tm.parse_headers(res["fasta"])[1])
    assert int(pos["emit_len"].sum()) == len(polished)
    for mask in (bm.UNDECIDED, bm.ALL, 1 << bm.KEPT):
        m = bm.masked(polished, pos["emit_len"], pos["status"], mask)
        assert m.upper() == polished.upper() and len(m) == len(polished)
    assert bm.masked(polished, pos["emit_len"], pos["status"], bm.ALL) == polished.lower()
    assert bm.masked(polished, pos["emit_len"], pos["status"]) != polished, "the golden pair has undecided positions that emit a base"


@pytest.mark.parametrize("which", [0, 1])
def test_the_hand_built_job_is_what_it_is_built_to_be(orc, which):
    """tests/bed_jobs.py (the GPU tests' jobs): the oracle reports exactly the built statuses, every status is there"""
    job = bj.job(T=2048, which=which)
    res = orc.polish_records(job["off"], job["bases"], job["recs"], min_depth=1, positions=True)
    bj.check_oracle_made(job, res)
    assert set(np.unique(job["status"]).tolist()) == set(range(6))


def test_the_binding_has_the_new_rows():
    import ctypes as C
    import polypolish_amd as pp
    rows = (("pp_status_bed", 9), ("pp_polish_bed", 4), ("pp_bed_out_bytes", 4), ("pp_bed_out_counts", 2), ("pp_bed_out_write", 2),
            ("pp_bed_out_kernel_ms", 2), ("pp_bed_out_free", 1), ("pp_polish_masked", 3), ("pp_masked_bytes", 3), ("pp_masked_kernel_ms", 2),
            ("pp_masked_free", 1), ("pp_ctx_set_bed", 4), ("pp_ctx_bed", 2), ("pp_ctx_set_soft_mask", 2))
    for name, n_args in rows:
        assert name in pp.SIGNATURES and len(pp.SIGNATURES[name][1]) == n_args, name
    order = list(pp.SIGNATURES)
    assert [n for n in order if n in dict(rows)] == [n for n, _ in rows], "in the header's order"
    assert order.index("pp_status_bed") == order.index("pp_vcf_out_free") + 1 and order.index("pp_ctx_set_bed") == order.index("pp_ctx_vcf") + 1
    assert pp.SIGNATURES["pp_status_bed"][0] is C.c_int and pp.SIGNATURES["pp_bed_out_free"][0] is None and pp.SIGNATURES["pp_masked_free"][0] is None
    assert "pp_bed_out_stage_ms_" in pp.HOOKS and "pp_bed_geometry_" in pp.HOOKS
    assert issubclass(pp.StatusBed, pp._Owned) and pp.StatusBed._free == "pp_bed_out_free"
    assert issubclass(pp.Masked, pp._Owned) and pp.Masked._free == "pp_masked_free"
    assert callable(pp.Context.set_bed) and callable(pp.Context.bed) and callable(pp.Context.set_soft_mask) and callable(pp.bed_geometry)
    import inspect
    for fn in (pp.Context.polish_files, pp.Context.filter_polish_files, pp.polish):
        assert {"bed", "bed_bgzf", "bed_status", "soft_mask"} <= set(inspect.signature(fn).parameters)
