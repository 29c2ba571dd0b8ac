"""The jobs of tests/long_sites.py are what they claim to be -- with the oracle and the plain models alone, no GPU.  Every check here is a
condition of a test in tests/test_long_winner_outputs_gpu.py: an input that stops meeting it fails here."""
import numpy as np
import pytest

import long_sites as ls
import vcf_jobs as vj
import vcf_model as vm
from debug_tsv_util import HEADER


@pytest.fixture(scope="module")
def geometry():
    import polypolish_amd
    ppt, tile, lane, text_wg = polypolish_amd.vcf_geometry()  # (the library's own report: no GPU is touched)
    return ppt, tile, lane, text_wg


def _oracle(orc, job):
    res = orc.polish_records(job["off"], job["bases"], job["recs"], positions=True, **job["kw"])
    nb = vj.new_bases(res)
    if job["spec"] is not None:
        vj.check_oracle_made(job["bases"], job["spec"], nb)
    return res, nb


def _files_oracle(orc, tmp_path, job, name):
    fa, sam = ls.write_files(str(tmp_path), job, name)
    w = orc.polish_files(fa, [sam], debug=True, **job["kw"])
    return w, b"".join(ln for ln in w["fasta"].split(b"\n") if ln[:1] != b">")


@pytest.mark.parametrize("which", ["small", "coarse"])
def test_l1_emits_every_length_a_code_holds_and_the_first_it_does_not(orc, which):
    res, _ = _oracle(orc, ls.l1_job(which))
    assert set(res["positions"]["emit_len"].tolist()) >= {0, 2, 3, 126, 127}


def test_the_dashed_winners_emit_less_than_they_hold(orc, tmp_path):
    job = ls.dashed_job()
    res, nb = _oracle(orc, job)
    w, seq = _files_oracle(orc, tmp_path, job, "job")
    assert seq == res["polished"]
    raw = vm.new_bases_of_debug_tsv(w["debug"])
    assert [x.replace(b"-", b"") for x in raw] == nb
    long = sorted((len(nb[p]), len(raw[p])) for p in range(len(nb)) if len(nb[p]) > 3)
    assert long == [(126, 128), (127, 129), (202, 205)], "(emitted, raw) bytes: the winners' list holds both, and they differ"


def test_l2_holds_every_placement(orc, geometry):
    ppt, tile, _, _ = geometry
    job = ls.l2_job(tile, ppt)
    res, nb = _oracle(orc, job)  # (check_oracle_made: exactly the wanted positions are edited, to the wanted bytes)
    el = res["positions"]["emit_len"].astype(np.int64)
    assert sorted(set(el[el >= 100].tolist())) == [n + 1 for n in ls.INSERTS], "the oracle emits exactly these long winners"
    s = ls.l2_sites(tile, ppt)
    ff = {int(p) for p in np.nonzero(el >= 127)[0]}  # the positions whose emit code is 0xFF
    assert set(s["adjacent"]) <= ff and s["adjacent"][1] == s["adjacent"][0] + 1
    a, b = s["one_thread"]
    assert {a, b} <= ff and a // ppt == b // ppt and a != b
    assert s["tile_seam"] == (tile - 1, tile) and set(s["tile_seam"]) <= ff
    p = s["between_subs"][0]
    assert p in ff and all(len(nb[q]) == 1 and nb[q] != bytes(job["bases"][q:q + 1]) for q in (p - 1, p + 1))
    names = job["names"]
    recs = vm.records(names, job["off"], bytes(job["bases"]), nb)
    assert (0, p, bytes(job["bases"][p - 1:p + 2]), nb[p - 1] + nb[p] + nb[p + 1]) in recs, "one record with a 3-base REF"
    p = s["before_deletion"][0]
    assert p in ff and all(el[q] == 0 for q in range(p + 1, p + 6)) and el[p + 6] == 1
    p = s["third_last"][0]
    G, total = int(job["off"][-1]), len(res["polished"])
    cum = np.concatenate([[0], np.cumsum(el)])
    assert p == G - 3 and p in ff and 0 <= total - int(cum[p + 1]) < 16, "its bytes end within 16 bytes of the output's end"
    assert all(el[q] == 126 for q in s["code_fe"]), "the last length an emit code holds"
    p = s["case"][0]
    assert nb[p][1:] == ls.CASE_BYTES and {ord("A") - 1, ord("A"), ord("Z"), ord("Z") + 1, ord("a") - 1, ord("z") + 1} <= set(nb[p])
    assert int(job["off"][1]) < s["contig_2"][0] and s["contig_2"][0] in ff
    assert set(res["positions"]["status"].tolist()) >= {0, 1, 2}, "kept, changed and low_depth: the masks select differently"


def test_l3_puts_long_alts_on_the_text_seams(orc, geometry):
    _, _, lane, text_wg = geometry
    job = ls.l3_job()
    res, nb = _oracle(orc, job)
    assert set(res["positions"]["emit_len"].tolist()) == {1, 301}
    import polypolish_amd
    version = polypolish_amd.lib().pp_version()
    starts, tile_hit, wg_hit = set(), 0, 0
    for n in range(1, 17):
        vcf = vm.vcf_from_positions(ls.l3_names(n), job["off"], bytes(job["bases"]), nb, version)
        assert len(vcf) > text_wg, "more than one text workgroup"
        starts |= {a % lane for a, _ in ls.alt_fields(vcf)}
        tile_hit += ls.strictly_inside_a_long_alt(vcf, 4096)
        wg_hit += ls.strictly_inside_a_long_alt(vcf, text_wg)
    assert tile_hit >= 1 and wg_hit >= 1, "text offsets 4096 and 16384 lie strictly inside an ALT of 127 bytes or more"
    assert len(starts) >= 8, "the ALT fields begin at 8 and more offsets modulo a lane's 16 bytes"


@pytest.mark.parametrize("make", [lambda g: ls.l1_job("small"), lambda g: ls.l2_job(g[1], g[0], ls.CASE_BYTES_UPPER), lambda g: ls.no_multi_job(),
                                  lambda g: ls.one_contig_job()],
                         ids=["l1_small", "l2_upper", "no_multi", "one_contig"])
def test_the_sequence_jobs_as_files_are_the_same_jobs(orc, tmp_path, geometry, make):
    """the job-after-job test takes its TSVs from the oracle on FASTA / SAM files: they hold the same job as the records"""
    job = make(geometry)
    res, nb = _oracle(orc, job)
    w, seq = _files_oracle(orc, tmp_path, job, "job")
    assert seq == res["polished"]
    assert [x.replace(b"-", b"") for x in vm.new_bases_of_debug_tsv(w["debug"])] == nb


def test_l1_small_has_a_winner_that_keeps_a_dash_in_the_tsv(orc, tmp_path):
    """the key ref + "-" wins at one site: the polish drops the '-' (one byte is left, the emit code is that byte and the winners' list
    has no entry), the TSV's new_base shows the winner as the reads have it; and new_base of 126 and 127 bytes"""
    w, _ = _files_oracle(orc, tmp_path, ls.l1_job("small"), "job")
    nb = vm.new_bases_of_debug_tsv(w["debug"])
    assert any(len(x) == 2 and x[1:] == b"-" and x[:1] in (b"A", b"C", b"G", b"T") for x in nb)
    assert {len(x) for x in nb} >= {126, 127}


def test_the_sequence_jobs_differ_where_it_matters(orc, geometry):
    el = _oracle(orc, ls.no_multi_job())[0]["positions"]["emit_len"]
    assert int(el.max()) == 1 and int(el.min()) == 0, "no multi-byte winner"
    job = ls.one_contig_job()
    assert len(job["off"]) == 2 and int(job["off"][-1]) < geometry[1]
    assert int(_oracle(orc, job)[0]["positions"]["emit_len"].max()) >= 127


def test_t1_fills_more_than_one_window_per_block(orc, tmp_path):
    fa, sams = ls.t1_files(str(tmp_path))
    body = orc.polish_files(fa, sams, debug=True)["debug"][len(HEADER):]
    names = {ln.split(b"\t")[0] for ln in ls.tsv_lines(body)}
    assert names == {n.encode() for n in ls.T1_NAMES} and sorted(len(n) for n in names) == [90, 97, 103]
    blocks = ls.blocks(body)
    assert len(blocks) >= 4 and min(blocks) > ls.WIN, blocks
    assert max(blocks) > 2 * ls.WIN, "a block with a third window"


def test_t2_holds_the_long_line_the_long_winners_and_the_item_counts(orc, tmp_path):
    fa, sam = ls.t2_files(str(tmp_path))
    body = orc.polish_files(fa, [sam], debug=True)["debug"][len(HEADER):]
    lines = [ln.split(b"\t") for ln in ls.tsv_lines(body)]
    assert len(lines) == 1000
    long = ls.tsv_lines(body)[ls.T2["long"]]
    assert len(long) + 1 > ls.WIN, "one line longer than a staging window"
    items = lines[ls.T2["long"]][6].split(b",")
    assert len(items) == ls.T2["n_long"] + 1 and sum(len(i) == 127 + 2 for i in items) == ls.T2["n_long"], "140 items of 127-byte keys"
    for p, n in ls.T2["winners"].items():
        assert lines[p][7] == b"changed" and len(lines[p][8]) == n + 1, (p, lines[p][7:])
    assert sorted(len(lines[p][8]) for p in ls.T2["winners"]) == [126, 127, 128, 201]
    assert lines[ls.T2["items12"]][6].count(b",") == ls.HEAVY - 1, "12 items: the thread places them"
    assert lines[ls.T2["items13"]][6].count(b",") == ls.HEAVY, "13 items: the workgroup places them"
    lo = ls.comma_cut(body, ls.T2["long"])
    assert lo is not None, "a chunk whose second staging window begins with a comma of the long line"
    assert b"\n".join(ls.tsv_lines(body)[lo:])[ls.WIN:ls.WIN + 1] == b","
