"""The chain a polish's tracks take to an indexed file, on the device end to end: pp_polish_vcf, pp_polish_bed and pp_polish_depth (in
the runs form and under a bin) on hand-built jobs (tests/bed_jobs.py, tests/long_sites.py), each text through pp_bgzf_deflate and then
pp_tabix_index with the text and the block table where they lie in device memory.  The index is the model's (tests/tabix_model.py),
byte for byte, and the model's reader over the DEVICE's file and the DEVICE's index returns exactly the lines a plain scan of the text
finds -- for every contig as a whole, for regions around every record's ends, for a region behind everything and for a name that is
absent.  The tracks' own bytes are what they were before the call.  Needs an MI355X: `-m gpu`."""
import gzip

import pytest

import bed_jobs as bj
import bed_model as bm
import long_sites as ls
import tabix_model as tx

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pp():
    import polypolish_amd
    return polypolish_amd


@pytest.fixture(scope="module")
def ctx(pp):
    c = pp.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def jobs(pp, orc):
    T = pp.depth_geometry()[1]
    ppt, tile, _, _ = pp.vcf_geometry()
    out = {"bed0": dict(bj.job(T, 0), kw=ls.MIN1), "bed1": dict(bj.job(T, 1), kw=ls.MIN1), "l1_small": ls.l1_job("small"), "dashed": ls.dashed_job(),
           "l2": ls.l2_job(tile, ppt)}
    return {name: (job, orc.polish_records(job["off"], job["bases"], job["recs"], **job["kw"])["polished"]) for name, job in out.items()}


def _regions(text, preset, names):
    rs = tx.rows(text, preset)
    out = [(n if isinstance(n, bytes) else n.encode(), 0, tx.MAX_END) for n in names] + [(b"absent", 0, 1000)]
    step = max(1, len(rs) // 150)                              # (around the ends of every record, of every step-th one in a long track)
    for _, _, _, name, b, e in rs[::step] + rs[-3:]:
        for at in (b - 1, b, b + 1, e - 1, e, e + 1):
            if at >= 0:
                out += [(name, at, at + 1), (name, at, at + 70)]
        out.append((name, e + (1 << 20), e + (1 << 20) + 5))
    return rs, out


def _indexed(pp, ctx, track, preset, names):
    """one track through pp_bgzf_deflate and pp_tabix_index; -> its number of data lines"""
    text = track.bytes()
    z = track.deflate()
    try:
        tbi, raw = pp.tabix_index(ctx, track.dev(), preset, (z.blk_off_ptr, z.n_blocks), pp.MEM_DEVICE)
        assert raw == tx.tbi_raw(text, preset, z.blk_off()) and gzip.decompress(tbi) == raw
        assert track.bytes() == text, "the track's own bytes are unchanged by the call"
        f = z.host().tobytes()
        rs, regions = _regions(text, preset, names)
        for name, beg, end in regions:
            assert tx.fetch(f, raw, preset, name, beg, end) == tx.scan(text, preset, name, beg, end, rs), (name, beg, end)
        listed = tx.parse_tbi(raw)["names"]
        assert listed == [n for i, n in enumerate(r[3] for r in rs) if i == 0 or rs[i - 1][3] != n], "the names with a line, in the order of their first"
        return len(rs)
    finally:
        z.close()


@pytest.mark.parametrize("name", ["bed0", "bed1", "l1_small", "dashed", "l2"])
def test_every_track_of_a_job_indexed_on_the_device(pp, ctx, jobs, name):
    job, polished = jobs[name]
    names = job["names"]
    got = ctx.polish_records(job["off"], job["bases"], job["recs"], debug=True, **job["kw"])["polished"]
    assert got == polished, "the device's job is the oracle's"
    lines = {}
    for what, make, preset in (("vcf", lambda: pp.Vcf(ctx, names), tx.VCF), ("bed", lambda: pp.StatusBed(ctx, names, bm.ALL), tx.BED),
                               ("runs", lambda: ctx.polish_depth(names, 0), tx.BED), ("bins", lambda: ctx.polish_depth(names, 100), tx.BED)):
        track = make()
        try:
            lines[what] = _indexed(pp, ctx, track, preset, names)
        finally:
            track.close()
    assert lines["bed"] > 0 and lines["runs"] > 0 and lines["bins"] > 0, lines
    assert ctx.result()[0] == polished, "the job's own bytes stay as they are"


def test_the_jobs_have_edits_to_index(pp, ctx, jobs):
    total = 0
    for name in ("l1_small", "dashed", "l2"):
        job, _ = jobs[name]
        ctx.polish_records(job["off"], job["bases"], job["recs"], **job["kw"])
        v = pp.Vcf(ctx, job["names"])
        total += v.n_records
        v.close()
    assert total > 5, "the long-winner jobs change positions: the VCF tracks above are not headers alone"
