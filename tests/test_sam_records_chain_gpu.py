"""The record chain FROM SAM TEXT against the oracle: SamRecords (pp_sam_records) -> Names twice (RNAME -> contig on a table seeded with
the FASTA names, QNAME -> read_id) -> (filter_records) -> (regroup_records) -> gate_records -> (prepare_batch) -> polish.  The dataset
is that of tests/test_regroup_chain_gpu.py (regroup_model.sorted_dataset): its name-grouped texts go straight to the gate, its
coordinate-sorted texts are refused by the gate as they lie and go through the regroup; options as there.  The name-grouped chain
takes its texts from host memory, the sorted chain from device memory.  Needs an MI355X: `-m gpu`."""
import os

import numpy as np
import pytest

import filter_model as fm
import ingest_model as im
import regroup_model as rm
from test_bgzf_chain_gpu import MAX_ERRORS
from test_regroup_chain_gpu import polish

pytestmark = pytest.mark.gpu
OPTIONS = [dict(), dict(careful=True), dict(max_errors=2)]
IDS = ["plain", "careful", "max_errors_2"]


@pytest.fixture(scope="module")
def pp():
    import polypolish_amd
    return polypolish_amd


@pytest.fixture(scope="module")
def dataset(tmp_path_factory, orc):
    d = str(tmp_path_factory.mktemp("sam_chain"))
    ds = rm.sorted_dataset(d)
    ds["texts"] = [open(p, "rb").read() for p in ds["sams"]]
    outs = [os.path.join(d, f"filtered_sorted_{i}.sam") for i in (1, 2)]
    ds["report"] = orc.filter_files(ds["sorted_paths"][0], ds["sorted_paths"][1], outs[0], outs[1])
    ds["verdicts"] = [fm.failed_lines(open(p, "rb").read()) for p in outs]
    again = []
    for f, p in enumerate(outs):
        again.append(os.path.join(d, f"filtered_regrouped_{f + 1}.sam"))
        with open(again[-1], "wb") as fh:
            fh.write(rm.regroup_text(open(p, "rb").read())[0])
    ds["want_filtered"] = orc.polish_files(ds["fasta"], again, max_errors=MAX_ERRORS)
    ds["oracle_grouped"] = lambda **kw: orc.polish_files(ds["fasta"], ds["sams"], **kw)
    ds["oracle_regrouped"] = lambda **kw: orc.polish_files(ds["fasta"], ds["regrouped_paths"], **kw)
    return ds


class Chain:
    """the links in front of the gate for the texts of a dataset: .recs[f] are the decoded records, contig and read_id filled in"""

    def __init__(self, pp, ctx, contigs, texts, mem):
        self.pp, self.ctx, self.owned, self.recs = pp, ctx, [], []
        self.rnames, self.qnames = pp.Names(ctx, len(contigs)), pp.Names(ctx)
        self.owned += [self.rnames, self.qnames]
        assert self.rnames.ids([name for name, _ in contigs]).tolist() == list(range(len(contigs)))
        for text in texts:
            if mem == pp.MEM_HOST:
                rec = pp.SamRecords(ctx, text)
            else:
                import torch
                t = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).to("cuda:0")
                torch.cuda.synchronize()
                rec = pp.SamRecords(ctx, (t.data_ptr(), len(text)), pp.MEM_DEVICE)
                del t           # the object keeps its own copy
            self.owned.append(rec)
            self.recs.append(rec)
            self.rnames.ids(**rec.rnames(), mem=pp.MEM_DEVICE, out32=rec.contig_ptr)
            self.qnames.ids(**rec.names(), mem=pp.MEM_DEVICE, out=rec.read_id_ptr)

    def close(self):
        for o in self.owned[::-1]:
            o.close()


@pytest.fixture(scope="module")
def grouped(pp, dataset):
    ctx = pp.Context(0)
    c = Chain(pp, ctx, dataset["contigs"], dataset["texts"], pp.MEM_HOST)
    yield c
    c.close()
    ctx.close()


@pytest.fixture(scope="module")
def sorted_chain(pp, dataset):
    ctx = pp.Context(0)
    c = Chain(pp, ctx, dataset["contigs"], dataset["sorted"], pp.MEM_DEVICE)
    yield c
    c.close()
    ctx.close()


def offsets(contigs):
    return np.concatenate([[0], np.cumsum([len(s) for _, s in contigs])]).astype(np.uint64)


@pytest.mark.parametrize("kw", OPTIONS, ids=IDS)
def test_name_grouped_texts_equal_the_oracle_s_fasta_and_counts(pp, grouped, dataset, kw):
    ctx = grouped.ctx
    want = dataset["oracle_grouped"](**dict(dict(max_errors=MAX_ERRORS), **kw))
    made = []
    try:
        gated = [pp.gate_records(ctx, rec.raw(), kw.get("max_errors", MAX_ERRORS), kw.get("careful", False), rec.zp, mem=pp.MEM_DEVICE)
                 for rec in grouped.recs]
        made += gated
        assert tuple(map(sum, zip(*[g.counts for g in gated]))) == tuple(want["counts"])
        assert any(not rec.zp.all() for rec in grouped.recs), "ZP:Z:fail lines are among them"
        polished, _ = polish(pp, ctx, dataset["contigs"], gated)
        assert polished == im.seqs(want["fasta"])
        if not kw:      # ... and once more with pp_batch_prepare in between: the direct path
            prepared = [pp.prepare_batch(ctx, offsets(dataset["contigs"]), g.n_aln, g.ptrs(), g.seq_bytes, g.n_cig_total, pp.MEM_DEVICE) for g in gated]
            made += prepared
            polished, _ = polish(pp, ctx, dataset["contigs"], prepared)
            assert polished == im.seqs(want["fasta"]) and ctx.took_direct_path()
    finally:
        for o in made[::-1]:
            o.close()


def test_the_sorted_records_as_they_lie_are_refused_by_the_gate(pp, sorted_chain):
    rec = sorted_chain.recs[0]
    with pytest.raises(pp.PolypolishError) as e:
        pp.gate_records(sorted_chain.ctx, rec.raw(), MAX_ERRORS, False, rec.zp, mem=pp.MEM_DEVICE)
    assert e.value.code == im.QUIT and "contain sequence" in str(e.value)


@pytest.mark.parametrize("kw", OPTIONS, ids=IDS)
def test_sorted_texts_through_the_regroup_equal_the_oracle_on_regroup_text(pp, sorted_chain, dataset, kw):
    ctx = sorted_chain.ctx
    want = dataset["oracle_regrouped"](**dict(dict(max_errors=MAX_ERRORS), **kw))
    made = []
    try:
        gated = []
        for f, rec in enumerate(sorted_chain.recs):
            g = pp.regroup_records(ctx, rec.raw(), mem=pp.MEM_DEVICE)
            made.append(g)
            assert np.array_equal(g.perm(), dataset["moved"][f]), "the records' perm is the model's perm of the lines"
            gated.append(pp.gate_records(ctx, g.raw(), kw.get("max_errors", MAX_ERRORS), kw.get("careful", False), g.carry_pass(rec.zp), mem=pp.MEM_DEVICE))
            made.append(gated[-1])
        assert tuple(map(sum, zip(*[g.counts for g in gated]))) == tuple(want["counts"])
        polished, _ = polish(pp, ctx, dataset["contigs"], gated)
        assert polished == im.seqs(want["fasta"])
    finally:
        for o in made[::-1]:
            o.close()


def test_the_filter_on_the_sorted_pair_and_its_verdicts_carried_over(pp, sorted_chain, dataset):
    ctx = sorted_chain.ctx
    got = pp.filter_records(ctx, sorted_chain.recs[0].raw(), sorted_chain.recs[1].raw(), mem=pp.MEM_DEVICE)
    assert got["report"] == dataset["report"]
    made = []
    try:
        gated = []
        for f, rec in enumerate(sorted_chain.recs):
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


def test_a_read_of_nothing_but_star_records_is_named_by_its_own_line_of_the_file(pp, dataset):
    """one read of the sorted file loses every SEQ: the gate's bad_record, taken through .perm() and .lines(), is the line of the
    read's first record in the file"""
    lines = dataset["sorted"][0].split(b"\n")
    recs = [i for i, ln in enumerate(lines) if ln and ln[:1] != b"@"]
    names = [lines[i].split(b"\t")[0] for i in recs]
    aligned = [not int(lines[i].split(b"\t")[1]) & 4 for i in recs]
    moved = dataset["moved"][0]
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
    c = Chain(pp, ctx, dataset["contigs"], [text], pp.MEM_DEVICE)
    g = None
    try:
        rec = c.recs[0]
        g = pp.regroup_records(ctx, rec.raw(), mem=pp.MEM_DEVICE)
        assert np.array_equal(g.perm(), moved)
        with pytest.raises(pp.PolypolishError) as e:
            pp.gate_records(ctx, g.raw(), MAX_ERRORS, False, g.carry_pass(rec.zp), mem=pp.MEM_DEVICE)
        assert e.value.code == im.QUIT and "contain sequence" in str(e.value)
        at = e.value.bad_record
        line = int(rec.lines()[int(g.perm()[at])])
        assert line == recs[first] and line != at and lines[line].split(b"\t")[0] == pick, "the file's own line, header lines counted"
        assert c.qnames.name(int(g.host()["read_id"][at])) == pick
    finally:
        if g is not None:
            g.close()
        c.close()
        ctx.close()
