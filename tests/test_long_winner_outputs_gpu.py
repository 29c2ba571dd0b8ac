"""The device-made --debug TSV (pp_k_debug.h), VCF (pp_k_vcf.h) and soft mask (k_bed_mask, pp_k_bed.h) on jobs whose winners and lines
are LONG (tests/long_sites.py; tests/test_long_sites_cpu.py proves what the jobs hold).  Each of the three passes works out again how
many bytes a position emits and where they lie; from 127 bytes on the emit code is 0xFF and the length comes from the multi-byte
winners' list.  Everything expected comes from the CPU oracle and the plain models (vcf_model, bed_model, the oracle's own TSV), never
from the device; the device's polished bytes are the oracle's (asserted first: the precondition); every comparison is byte for byte.

  gap                                                    the tests that cover it
  code 0xFF in the VCF and the mask (k_vcf_multi, mlen)  test_vcf_*, test_mask_* on L1 / L2, test_job_after_job_on_one_context; which field of
                                                         the winners' list it is (emitted, not raw bytes): the same tests on the dashed job
  an ALT longer than a lane's 16 bytes (k_vcf_text)      test_vcf_* on L2 (the output's end), test_vcf_on_l3_under_16_name_lengths
  the second staging window of k_dfmt_write              test_tsv_whole, test_tsv_into_device_memory, test_tsv_t2_*
  long keys and long new_base, the DFMT_HEAVY seam       test_tsv_* on T2, test_t2_ties_the_outputs_together

Needs an MI355X: `-m gpu`."""
import numpy as np
import pytest

import bed_model as bm
import long_sites as ls
import vcf_jobs as vj
import vcf_model as vm
from debug_tsv_util import HEADER, _diff, _raw

pytestmark = pytest.mark.gpu

MASKS = (bm.ALL, bm.UNDECIDED, 1 << bm.CHANGED)


@pytest.fixture(scope="module")
def pp():
    import polypolish_amd
    return polypolish_amd


@pytest.fixture(scope="module")
def ctx(pp):
    c = pp.Context(0)
    yield c
    c.close()


# ---- the jobs and what the oracle and the models say of them, made once ---------------------------------------------------------------
def _expected(pp, orc, job):
    res = orc.polish_records(job["off"], job["bases"], job["recs"], positions=True, **job["kw"])
    nb = vj.new_bases(res)
    if job["spec"] is not None:
        vj.check_oracle_made(job["bases"], job["spec"], nb)
    return {"res": res, "nb": nb, "vcf": vm.vcf_from_positions(job["names"], job["off"], bytes(job["bases"]), nb, pp.lib().pp_version())}


def _with_tsv(orc, tmp, job, exp, name):
    """... and the oracle's TSV of the same job as files (the same job: test_long_sites_cpu.py, and the polished bytes here)"""
    fa, sam = ls.write_files(tmp, job, name)
    w = orc.polish_files(fa, [sam], debug=True, **job["kw"])
    assert b"".join(ln for ln in w["fasta"].split(b"\n") if ln[:1] != b">") == exp["res"]["polished"]
    assert w["debug"].startswith(HEADER)
    exp["tsv"] = w["debug"][len(HEADER):]
    return exp


@pytest.fixture(scope="module")
def jobs(pp, orc):
    ppt, tile, _, _ = pp.vcf_geometry()
    out = {"l1_small": ls.l1_job("small"), "l1_coarse": ls.l1_job("coarse"), "dashed": ls.dashed_job(), "l2": ls.l2_job(tile, ppt)}
    return {k: (j, _expected(pp, orc, j)) for k, j in out.items()}


def _first_diff(got, want):
    i = next((k for k, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    return len(got), len(want), i, got[max(0, i - 40):i + 40], want[max(0, i - 40):i + 40]


def _polish(pp, ctx, job, exp, path="plain", debug=True):
    off, bases, recs = job["off"], job["bases"], job["recs"]
    if path == "plain":
        got = ctx.polish_records(off, bases, recs, debug=debug, **job["kw"])["polished"]
        assert not ctx.took_direct_path()
    else:
        prep = pp.prepare_records(ctx, off, recs)
        try:
            pp.lib().pp_polish_set_debug(ctx._h, int(debug))
            ctx.polish_begin(off, bases.ctypes.data, pp.MEM_HOST, **job["kw"])
            ctx.polish_add_ptrs(prep.n_aln, prep.ptrs(), prep.seq_bytes, prep.n_cig_total, pp.MEM_DEVICE)
            ctx.polish_finish()
            assert ctx.took_direct_path()
            got = ctx.result()[0]
        finally:
            pp.lib().pp_polish_set_debug(ctx._h, 0)
            prep.close()
    assert got == exp["res"]["polished"], "the device's job is the oracle's"


def _vcf(pp, ctx, job, exp, names=None, want=None):
    names = names or job["names"]
    want = exp["vcf"] if want is None else want
    v = pp.Vcf(ctx, names)
    try:
        got = v.bytes()
        assert got == want, _first_diff(got, want)
        assert v.n_records == len(vm.records(names, job["off"], bytes(job["bases"]), exp["nb"])) and v.n_bytes == len(want)
    finally:
        v.close()
    return got


def _applies_back(job, exp, vcf):
    off, out_off, pol = job["off"], exp["res"]["offsets"], exp["res"]["polished"]
    contigs = [(n, bytes(job["bases"][int(off[i]):int(off[i + 1])])) for i, n in enumerate(job["names"])]
    assert [s for _, s in vm.apply(contigs, vcf)] == [pol[int(out_off[i]):int(out_off[i + 1])] for i in range(len(contigs))]


def _mask(pp, ctx, exp, mask):
    pos, pol = exp["res"]["positions"], exp["res"]["polished"]
    want = bm.masked(pol, pos["emit_len"], pos["status"], mask)
    m = pp.Masked(ctx, mask)
    try:
        got = m.bytes()
        assert got == want, (mask, _first_diff(got, want))
        assert m.n_bytes == ctx.result_size() == len(pol)
    finally:
        m.close()
    assert ctx.result()[0] == pol, "the job's own bytes stay as they are"
    return got


def _bed(pp, ctx, job, exp, mask):
    st = exp["res"]["positions"]["status"]
    want = bm.bed(st, job["off"], job["names"], mask)
    b = pp.StatusBed(ctx, job["names"], mask)
    try:
        got = b.bytes()
        assert got == want, (mask, _first_diff(got, want))
        assert b.n_records == want.count(b"\n") and b.counts == bm.counts(st, job["off"], mask)
    finally:
        b.close()


# ---- VCF, mask and BED on L1 and L2 ---------------------------------------------------------------------------------------------------
PATHS = pytest.mark.parametrize("path", ["plain", "direct"])
JOBS = pytest.mark.parametrize("which", ["l1_small", "l1_coarse", "dashed", "l2"])


@PATHS
@JOBS
def test_vcf_where_the_length_comes_from_the_winners_list(pp, ctx, jobs, which, path):
    """k_vcf_multi's store and vcf_len's J.mlen[p]: a wrong length there moves every output offset behind it, and with it every ALT
    and every decision "this position emits its own base"; on L2 one ALT ends two bytes in front of the polished output's end (wide
    loads only where the 16-byte piece lies wholly inside the array)"""
    job, exp = jobs[which]
    assert int(exp["res"]["positions"]["emit_len"].max()) >= 127
    _polish(pp, ctx, job, exp, path, debug=False)  # (the VCF needs no per-position records)
    got = _vcf(pp, ctx, job, exp)
    _applies_back(job, exp, got)
    if which == "l2":
        tile = pp.vcf_geometry()[1]
        b, nb = job["bases"], exp["nb"]
        assert (b"contig_1", tile, bytes(b[tile - 1:tile + 1]), nb[tile - 1] + nb[tile]) in vm.parse(got)[1], "one ALT of 428 bytes across the workgroups"
        assert got.endswith(nb[-3] + b"\t.\t.\t.\n") and len(nb[-3]) == 127, "the last record's ALT: the winner at the third-last position"


@PATHS
@JOBS
def test_mask_where_the_length_comes_from_the_winners_list(pp, ctx, jobs, which, path):
    """k_bed_mask lower-cases a winner whole, from the offset the emitted lengths in front of it give"""
    job, exp = jobs[which]
    _polish(pp, ctx, job, exp, path)
    got = {mask: _mask(pp, ctx, exp, mask) for mask in MASKS}
    assert len({got[m] for m in MASKS}) == 3, "the three masks select differently"
    if which == "l2":
        at = got[bm.ALL].index(b"@az[`az{n*")  # the case winner: only 'A'..'Z' change
        assert got[bm.UNDECIDED][at:at + 10] == ls.CASE_BYTES and got[1 << bm.CHANGED][at:at + 10] == b"@az[`az{n*"


@PATHS
@JOBS
def test_bed_beside_the_long_winners(pp, ctx, jobs, which, path):
    job, exp = jobs[which]
    _polish(pp, ctx, job, exp, path)
    for mask in MASKS:
        _bed(pp, ctx, job, exp, mask)
    _vcf(pp, ctx, job, exp)  # ... and the VCF of the same finished context, behind the BED


# ---- VCF on L3: a text beyond one text workgroup ---------------------------------------------------------------------------------------
def test_vcf_on_l3_under_16_name_lengths(pp, ctx, orc):
    """ALT fields of 301 bytes behind a one-byte REF: k_vcf_text's wide path with REF and ALT of different lengths, the ALT beginning
    at every offset modulo a lane's 16 bytes, across the text tiles' (4096) and the text workgroups' (16384) boundaries"""
    job = ls.l3_job()
    exp = _expected(pp, orc, job)
    _polish(pp, ctx, job, exp, debug=False)
    starts = set()
    for n in range(1, 17):
        names = ls.l3_names(n)
        want = vm.vcf_from_positions(names, job["off"], bytes(job["bases"]), exp["nb"], pp.lib().pp_version())
        assert len(want) > pp.vcf_geometry()[3]
        got = _vcf(pp, ctx, job, exp, names, want)
        starts |= {a % 16 for a, _ in ls.alt_fields(got)}
    assert len(starts) >= 8


# ---- the TSV on T1 and T2 -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tsv_jobs(pp, orc, tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("long_tsv"))
    out = {}
    fa2, sam2 = ls.t2_files(tmp)
    for key, (fa, sams) in (("t1", ls.t1_files(tmp)), ("t2", (fa2, [sam2]))):
        w = orc.polish_files(fa, sams, debug=True)
        assert w["debug"].startswith(HEADER)
        names, _, off, bases, recs, _ = pp.ingest(fa, sams)
        out[key] = {"names": names, "off": off, "bases": bases, "recs": recs, "body": w["debug"][len(HEADER):],
                    "polished": b"".join(ln for ln in w["fasta"].split(b"\n") if ln[:1] != b">")}
    assert min(ls.blocks(out["t1"]["body"])) > ls.WIN and len(ls.tsv_lines(out["t2"]["body"])[ls.T2["long"]]) + 1 > ls.WIN
    return out


def _polish_tsv_job(ctx, t):
    res = ctx.polish_records(t["off"], t["bases"], t["recs"], debug=True)
    assert res["polished"] == t["polished"], "the device's job is the oracle's"
    return int(t["off"][-1])


@pytest.mark.parametrize("which", ["t1", "t2"])
def test_tsv_whole(ctx, tsv_jobs, which):
    """every workgroup of T1 stages its 256 lines in two or three windows; T2's first line alone fills more than one"""
    t = tsv_jobs[which]
    _polish_tsv_job(ctx, t)
    got = ctx.debug_tsv(t["names"])
    assert got == t["body"], _diff(got, t["body"])


@pytest.mark.parametrize("which", ["t1", "t2"])
def test_tsv_into_device_memory_at_every_alignment(pp, ctx, tsv_jobs, which):
    """the destination's alignment is the windows' `shift`, derived again per window"""
    import torch
    t = tsv_jobs[which]
    G = _polish_tsv_job(ctx, t)
    body = t["body"]
    dev = torch.empty(len(body) + 96, dtype=torch.uint8, device="cuda:0")
    assert dev.data_ptr() % 16 == 0
    want = np.frombuffer(body, np.uint8)
    for k in range(16):
        dev.fill_(0xEE)
        torch.cuda.synchronize()
        at = 16 + k
        rc, _, n, nxt = _raw(pp, ctx, t["names"], 0, G, len(body) + 8, mem=pp.MEM_DEVICE, out=dev.data_ptr() + at)
        assert rc == 0 and n == len(body) and nxt == G, (k, rc, n, nxt)
        host = dev.cpu().numpy()
        assert np.array_equal(host[at:at + n], want), (k, _diff(host[at:at + n].tobytes(), body))
        assert (host[:at] == 0xEE).all() and (host[at + n:] == 0xEE).all(), (k, "bytes around the text were written")


def test_tsv_t2_a_room_one_byte_short_of_the_long_line(pp, ctx, tsv_jobs):
    t = tsv_jobs["t2"]
    G = _polish_tsv_job(ctx, t)
    p, line = ls.T2["long"], ls.tsv_lines(t["body"])[ls.T2["long"]] + b"\n"
    rc, buf, n, nxt = _raw(pp, ctx, t["names"], p, G, len(line) - 1)
    assert rc == pp.ERR_ARG and n == 0 and nxt == 0 and (buf == 0xEE).all()


def test_tsv_t2_a_room_of_exactly_the_long_line(pp, ctx, tsv_jobs):
    t = tsv_jobs["t2"]
    G = _polish_tsv_job(ctx, t)
    p, line = ls.T2["long"], ls.tsv_lines(t["body"])[ls.T2["long"]] + b"\n"
    rc, buf, n, nxt = _raw(pp, ctx, t["names"], p, G, len(line))
    assert rc == 0 and n == len(line) and nxt == p + 1, (rc, n, nxt)
    assert buf[:n].tobytes() == line, _diff(buf[:n].tobytes(), line)


def test_tsv_t2_the_comma_at_a_windows_first_byte(pp, ctx, tsv_jobs):
    t = tsv_jobs["t2"]
    _polish_tsv_job(ctx, t)
    lo = ls.comma_cut(t["body"], ls.T2["long"])
    assert lo is not None
    want = b"".join(x + b"\n" for x in ls.tsv_lines(t["body"])[lo:])
    assert want[ls.WIN:ls.WIN + 1] == b","
    got = ctx.debug_tsv(t["names"], lo=lo)
    assert got == want, _diff(got, want)


def test_tsv_t2_in_chunks_of_one_to_three_long_lines(pp, ctx, tsv_jobs):
    t = tsv_jobs["t2"]
    G = _polish_tsv_job(ctx, t)
    body = t["body"]
    longest = max(len(x) for x in ls.tsv_lines(body)) + 1
    rng = np.random.default_rng(51)
    for _ in range(3):
        cuts = np.unique(np.concatenate([[0, G], rng.integers(0, G, 6)]))
        parts = []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            p = int(lo)
            while p < int(hi):
                cap = int(longest + rng.integers(0, 2 * longest + 1))
                rc, buf, n, nxt = _raw(pp, ctx, t["names"], p, int(hi), cap)
                assert rc == 0 and 0 < n <= cap and p < nxt <= int(hi), (rc, n, cap, p, nxt)
                assert (buf[n:] == 0xEE).all()  # nothing behind the lines written
                parts.append(buf[:n].tobytes())
                p = nxt
        got = b"".join(parts)
        assert got == body, _diff(got, body)


def test_tsv_t1_in_chunks(pp, ctx, tsv_jobs):
    """rooms of a few lines to a few windows over random cuts: blocks that begin anywhere, windows that end in any line"""
    t = tsv_jobs["t1"]
    G = _polish_tsv_job(ctx, t)
    body = t["body"]
    longest = max(len(x) for x in ls.tsv_lines(body)) + 1
    rng = np.random.default_rng(52)
    cuts = np.unique(np.concatenate([[0, G], rng.integers(0, G, 8)]))
    parts = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        p = int(lo)
        while p < int(hi):
            cap = int(rng.integers(longest, 3 * ls.WIN))
            rc, buf, n, nxt = _raw(pp, ctx, t["names"], p, int(hi), cap)
            assert rc == 0 and 0 < n <= cap and p < nxt <= int(hi), (rc, n, cap, p, nxt)
            assert (buf[n:] == 0xEE).all()
            parts.append(buf[:n].tobytes())
            p = nxt
    got = b"".join(parts)
    assert got == body, _diff(got, body)


def test_t2_ties_the_outputs_together(pp, ctx, tsv_jobs):
    """the records route with debug records: the VCF of the same finished context is the model's on the ORACLE's TSV (new_base of 126,
    127, 128 and 201 bytes from J.multi in the TSV, from the polished output in the VCF), before and behind the TSV"""
    t = tsv_jobs["t2"]
    _polish_tsv_job(ctx, t)
    names = [n.encode() for n in t["names"]]
    want = vm.from_debug_tsv(names, t["off"], bytes(t["bases"]), HEADER + t["body"], pp.lib().pp_version())
    assert sorted(len(r[3]) for r in vm.parse(want)[1]) == [126, 127, 128, 201]
    for _ in range(2):
        v = pp.Vcf(ctx, names)
        got = v.bytes()
        v.close()
        assert got == want, _first_diff(got, want)
        tsv = ctx.debug_tsv(t["names"])
        assert tsv == t["body"], _diff(tsv, t["body"])


# ---- the TSV of the records jobs: new_base from the winners' list at 126 bytes and beyond, and from a key where the list has no entry ------
@pytest.mark.parametrize("path", ["plain", "direct"])
@pytest.mark.parametrize("which", ["l1_small", "dashed", "l2_upper", "one_contig"])
def test_tsv_new_base_of_long_winners_and_of_a_winner_with_a_dash(pp, ctx, orc, tmp_path, which, path):
    """L1 small: winners of 126 and 127 bytes, and the key ref + "-" as a winner -- one byte is left of it, its emit code is that byte
    and the winners' list has no entry: new_base is the key as the reads have it ("C-").  L2 (without lower-case letters: the TSV's
    oracle reads the job as SAM text) and the one-contig job: new_base of 126 to 301 bytes, two of them in consecutive lines.  The dashed
    job: winners whose raw bytes (new_base) are more than they emit."""
    ppt, tile, _, _ = pp.vcf_geometry()
    job = {"l1_small": lambda: ls.l1_job("small"), "dashed": ls.dashed_job, "l2_upper": lambda: ls.l2_job(tile, ppt, ls.CASE_BYTES_UPPER), "one_contig": ls.one_contig_job}[which]()
    exp = _with_tsv(orc, str(tmp_path), job, _expected(pp, orc, job), which)
    nb = vm.new_bases_of_debug_tsv(HEADER + exp["tsv"])
    assert max(len(x) for x in nb) >= 127 and (which != "l1_small" or any(len(x) == 2 and x[1:] == b"-" for x in nb))
    _polish(pp, ctx, job, exp, path)
    got = ctx.debug_tsv([n.decode() for n in job["names"]])
    assert got == exp["tsv"], _diff(got, exp["tsv"])


# ---- job after job on one fresh context ---------------------------------------------------------------------------------------------------
def test_job_after_job_on_one_context(pp, orc, tmp_path):
    """L2, a job without any multi-byte winner (J.mlen stays null), L1 small, L2 again, a one-contig job of less than a workgroup's
    positions: nothing of a job's winners' list, lengths table or formatter tables outlives it.  The outputs are taken in another
    order from step to step, and the one taken first is taken again last: the same bytes."""
    ppt, tile, _, _ = pp.vcf_geometry()
    l2 = ls.l2_job(tile, ppt, ls.CASE_BYTES_UPPER)  # (without lower-case letters: the TSV's oracle reads the job as SAM text)
    made = {}
    for key, job in (("l2", l2), ("no_multi", ls.no_multi_job()), ("l1_small", ls.l1_job("small")), ("one_contig", ls.one_contig_job())):
        made[key] = (job, _with_tsv(orc, str(tmp_path), job, _expected(pp, orc, job), key))
    assert int(made["no_multi"][1]["res"]["positions"]["emit_len"].max()) == 1
    assert len(made["one_contig"][0]["off"]) == 2 and int(made["one_contig"][0]["off"][-1]) < tile
    c = pp.Context(0)
    try:
        for step, key in enumerate(("l2", "no_multi", "l1_small", "l2", "one_contig")):
            job, exp = made[key]
            _polish(pp, c, job, exp, "plain" if step % 2 == 0 else "direct")
            names = [n.decode() for n in job["names"]]
            take = {"vcf": lambda: _vcf(pp, c, job, exp), "mask": lambda: _mask(pp, c, exp, bm.ALL),
                    "tsv": lambda: c.debug_tsv(names)}
            order = [("vcf", "mask", "tsv"), ("tsv", "vcf", "mask"), ("mask", "tsv", "vcf")][step % 3]
            got = {}
            for what in order + order[:1]:
                out = take[what]()
                assert got.setdefault(what, out) == out, (key, what, "taken again: other bytes")
            assert got["tsv"] == exp["tsv"], (key, _diff(got["tsv"], exp["tsv"]))
    finally:
        c.close()
