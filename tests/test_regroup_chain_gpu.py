"""The record chain on COORDINATE-SORTED BAM, with the regroup added: Bgzf (pp_bgzf_inflate) -> bam_header -> Names (the reference map)
-> .bam_walk -> BamRecords -> Names (read_id) -> regroup_records -> gate_records -> (prepare) -> polish, against the oracle on
regroup_text of the sorted SAM (tests/regroup_model.py) -- the sorted text itself the oracle refuses, as the gate refuses the sorted
records (tests/test_regroup_model_cpu.py).  The dataset is that of tests/test_bam_chain_gpu.py, each file sorted by (contig, POS);
BGZF blocks as in tests/test_bgzf_chain_gpu.py.  With the filter, the filter runs on the sorted records as they lie and its verdicts
go through carry_pass.  (tests/test_bam_chain_gpu.py checks no --debug positions, so none are checked here.)  Needs an MI355X:
`-m gpu`."""
import os

import numpy as np
import pytest

import bam_model as bm
import filter_model as fm
import ingest_model as im
import regroup_model as rm
from test_bgzf_chain_gpu import MAX_ERRORS, bgzf_file, cut_points

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pp():
    import polypolish_amd
    return polypolish_amd


@pytest.fixture(scope="module")
def dataset(tmp_path_factory, orc):
    d = str(tmp_path_factory.mktemp("regroup_chain"))
    ds = rm.sorted_dataset(d)
    # the oracle's filter on the sorted text (it joins a read's records wherever they lie), its polish on regroup_text of the outputs
    outs = [os.path.join(d, f"filtered_sorted_{i}.sam") for i in (1, 2)]
    ds["report"] = orc.filter_files(ds["sorted_paths"][0], ds["sorted_paths"][1], outs[0], outs[1])
    ds["verdicts"] = [fm.failed_lines(open(p, "rb").read()) for p in outs]
    again = []
    for f, p in enumerate(outs):
        again.append(os.path.join(d, f"filtered_regrouped_{f + 1}.sam"))
        with open(again[-1], "wb") as fh:
            fh.write(rm.regroup_text(open(p, "rb").read())[0])
    ds["want_filtered"] = orc.polish_files(ds["fasta"], again, max_errors=MAX_ERRORS)
    ds["oracle"] = lambda **kw: orc.polish_files(ds["fasta"], ds["regrouped_paths"], **kw)
    return ds


class Chain:
    """the links in front of the regroup for both files of a dataset: .recs[f] are the decoded records, read_id filled in"""

    def __init__(self, pp, ctx, contigs, texts):
        self.pp, self.ctx, self.owned, self.recs = pp, ctx, [], []
        n_contigs = len(contigs)
        header_order = [name for name, _ in contigs][::-1]
        self.rnames, self.qnames = pp.Names(ctx, n_contigs), pp.Names(ctx)
        self.owned += [self.rnames, self.qnames]
        assert self.rnames.ids([name for name, _ in contigs]).tolist() == list(range(n_contigs))
        for text in texts:
            enc = bm.encode(text, header_order, [len(dict(contigs)[n]) for n in header_order])
            data = enc["header"] + enc["records"]
            starts = set((enc["rec_off"] + np.uint64(len(enc["header"]))).tolist())
            z = pp.Bgzf(ctx, bgzf_file(data, cut_points(len(data), starts)))
            self.owned.append(z)
            hdr = pp.bam_header(z.host(0, len(enc["header"])))
            ref_map = self.rnames.ids(hdr["names"] + [b"*"]).astype(np.uint32)
            rec_off_ptr, n_rec, end = z.bam_walk(hdr["records_at"])
            assert end == len(data) and n_rec == len(enc["rec_off"])
            rec = pp.BamRecords(ctx, (z.bytes_ptr, z.n_bytes), (rec_off_ptr, n_rec), ref_map, mem=pp.MEM_DEVICE)
            self.owned.append(rec)
            self.recs.append(rec)
            self.qnames.ids(**rec.names(), mem=pp.MEM_DEVICE, out=rec.read_id_ptr)

    def close(self):
        for o in self.owned[::-1]:
            o.close()


def polish(pp, ctx, contigs, batches):
    off = np.concatenate([[0], np.cumsum([len(s) for _, s in contigs])]).astype(np.uint64)
    bases = np.frombuffer("".join(s for _, s in contigs).upper().encode(), np.uint8)
    ctx.polish_begin(off, bases.ctypes.data, pp.MEM_HOST)
    for b in batches:
        if b.n_aln:
            ctx.polish_add_ptrs(b.n_aln, b.ptrs(), b.seq_bytes, b.n_cig_total, pp.MEM_DEVICE)
    ctx.polish_finish()
    return ctx.result()[0], off


@pytest.fixture(scope="module")
def chain(pp, dataset):
    ctx = pp.Context(0)
    c = Chain(pp, ctx, dataset["contigs"], dataset["sorted"])
    yield c
    c.close()
    ctx.close()


def test_the_sorted_records_as_they_lie_are_refused_by_the_gate(pp, chain):
    with pytest.raises(pp.PolypolishError) as e:
        pp.gate_records(chain.ctx, chain.recs[0].raw(), MAX_ERRORS, False, chain.recs[0].zp, mem=pp.MEM_DEVICE)
    assert e.value.code == im.QUIT and "contain sequence" in str(e.value)


@pytest.mark.parametrize("kw", [dict(), dict(careful=True), dict(max_errors=2)], ids=["plain", "careful", "max_errors_2"])
def test_regroup_in_front_of_the_gate_gives_the_oracle_s_fasta_and_counts(pp, chain, dataset, kw):
    ctx = chain.ctx
    want = dataset["oracle"](**dict(dict(max_errors=MAX_ERRORS), **kw))
    made = []
    try:
        gated = []
        for f, rec in enumerate(chain.recs):
            g = pp.regroup_records(ctx, rec.raw(), mem=pp.MEM_DEVICE)
            made.append(g)
            assert np.array_equal(g.perm(), dataset["moved"][f]), "the records' perm is the model's perm of the lines"
            n_groups, n_moved = g.counts()
            assert 3 * n_moved > rec.n_rec and n_groups == len(set(ln.split(b"\t")[0] for ln in dataset["sorted"][f].split(b"\n") if ln and ln[:1] != b"@"))
            gated.append(pp.gate_records(ctx, g.raw(), kw.get("max_errors", MAX_ERRORS), kw.get("careful", False), g.carry_pass(rec.zp), mem=pp.MEM_DEVICE))
            made.append(gated[-1])
        assert tuple(map(sum, zip(*[g.counts for g in gated]))) == tuple(want["counts"])
        polished, _ = polish(pp, ctx, dataset["contigs"], gated)
        assert polished == im.seqs(want["fasta"])
        assert not ctx.took_direct_path()
        if not kw:      # ... and with pp_batch_prepare in between
            off = np.concatenate([[0], np.cumsum([len(s) for _, s in dataset["contigs"]])]).astype(np.uint64)
            prepared = [pp.prepare_batch(ctx, off, g.n_aln, g.ptrs(), g.seq_bytes, g.n_cig_total, pp.MEM_DEVICE) for g in gated]
            made += prepared
            polished, _ = polish(pp, ctx, dataset["contigs"], prepared)
            assert polished == im.seqs(want["fasta"]) and ctx.took_direct_path()
    finally:
        for o in made[::-1]:
            o.close()


def test_the_filter_on_the_sorted_records_and_its_verdicts_carried_over(pp, chain, dataset):
    ctx = chain.ctx
    got = pp.filter_records(ctx, chain.recs[0].raw(), chain.recs[1].raw(), mem=pp.MEM_DEVICE)
    assert got["report"] == dataset["report"]
    made = []
    try:
        gated = []
        for f, rec in enumerate(chain.recs):
            passed = got["pass"][f] & rec.zp
            assert np.array_equal(passed, dataset["verdicts"][f] & rec.zp) and (passed == 0).any(), f
            g = pp.regroup_records(ctx, rec.raw(), mem=pp.MEM_DEVICE)
            made.append(g)
            carried = g.carry_pass(passed)
            assert not np.array_equal(carried, passed) and carried.sum() == passed.sum()
            gated.append(pp.gate_records(ctx, g.raw(), MAX_ERRORS, False, carried, mem=pp.MEM_DEVICE))
            made.append(gated[-1])
        want = dataset["want_filtered"]
        assert tuple(map(sum, zip(*[g.counts for g in gated]))) == tuple(want["counts"])
        polished, _ = polish(pp, ctx, dataset["contigs"], gated)
        assert polished == im.seqs(want["fasta"])
    finally:
        for o in made[::-1]:
            o.close()


def test_polish_raw_with_regroup_takes_host_records(pp, chain, dataset):
    ctx = chain.ctx
    want = dataset["oracle"](max_errors=MAX_ERRORS)
    contigs = dataset["contigs"]
    off = np.concatenate([[0], np.cumsum([len(s) for _, s in contigs])]).astype(np.uint64)
    bases = np.frombuffer("".join(s for _, s in contigs).upper().encode(), np.uint8)
    raws = [{k: v for k, v in rec.host().items() if k in dict(pp.RAW_FIELDS)} for rec in chain.recs]
    res = ctx.polish_raw(off, bases, raws, MAX_ERRORS, passed=[rec.zp for rec in chain.recs], regroup=True)
    assert res["polished"] == im.seqs(want["fasta"]) and tuple(map(sum, zip(*res["counts"]))) == tuple(want["counts"])
    with pytest.raises(pp.PolypolishError):
        ctx.polish_raw(off, bases, raws, MAX_ERRORS, passed=[rec.zp for rec in chain.recs])


def test_a_read_of_nothing_but_star_records_is_named_by_its_first_record_in_the_file(pp, dataset):
    """one read of the sorted file loses every SEQ: the gate's QUIT, taken through perm, is the file's own record of the read's first line"""
    lines = dataset["sorted"][0].split(b"\n")
    recs = [i for i, ln in enumerate(lines) if ln and ln[:1] != b"@"]
    names = [lines[i].split(b"\t")[0] for i in recs]
    aligned = [not int(lines[i].split(b"\t")[1]) & 4 for i in recs]
    moved = dataset["moved"][0]
    # a read with two aligned records or more that do not stand together, none of them the file's first group
    pick = next(n for j, n in enumerate(names) if j > 50 and aligned[j] and sum(1 for k, m in enumerate(names) if m == n and aligned[k]) >= 2
                and names[j + 1] != n and names.index(n) == j and int(np.flatnonzero(moved == j)[0]) != j)
    first = names.index(pick)
    for j, n in enumerate(names):
        if n == pick:
            col = lines[recs[j]].split(b"\t")
            col[9] = col[10] = b"*"
            lines[recs[j]] = b"\t".join(col)
    text = b"\n".join(lines)
    ctx = pp.Context(0)
    c = Chain(pp, ctx, dataset["contigs"], [text])
    g = None
    try:
        rec = c.recs[0]
        g = pp.regroup_records(ctx, rec.raw(), mem=pp.MEM_DEVICE)
        assert np.array_equal(g.perm(), moved)
        with pytest.raises(pp.PolypolishError) as e:
            pp.gate_records(ctx, g.raw(), MAX_ERRORS, False, g.carry_pass(rec.zp), mem=pp.MEM_DEVICE)
        assert e.value.code == im.QUIT and "contain sequence" in str(e.value)
        at = e.value.bad_record
        assert int(g.perm()[at]) == first and at != first, "the view's record, through perm, is the file's"
        assert c.qnames.name(int(g.host()["read_id"][at])) == pick
    finally:
        if g is not None:
            g.close()
        c.close()
        ctx.close()
