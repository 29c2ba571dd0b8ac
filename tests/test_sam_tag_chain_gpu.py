"""The reference's two-command workflow on SAM TEXT, on the device from the upload of the text to the FASTA: `filter` = SamRecords x2 ->
Names (one QNAME table for both files, the RNAMEs on a table seeded with the FASTA names) -> filter_records -> SamRecords.tagged
(pp_sam_tagged_records) x2, whose outputs must be the ORACLE's filtered files byte for byte; each output through pp_bgzf_deflate and
pp_bgzf_inflate gives itself again; then `polish` = that inflated device text through SamRecords -> Names -> gate_records with the ZP
tags alone -> polish, against the oracle's polish of its own filtered files.  The dataset is that of tests/test_bam_tag_chain_gpu.py, the
links in front of the gate those of tests/test_sam_records_chain_gpu.py.  Needs an MI355X: `-m gpu`."""
import numpy as np
import pytest

import ingest_model as im
import sam_tag_model as sm
from test_bam_tag_chain_gpu import dataset, pp  # noqa: F401 (fixtures)
from test_bgzf_chain_gpu import MAX_ERRORS
from test_regroup_chain_gpu import polish
from test_sam_records_chain_gpu import Chain


@pytest.mark.gpu
def test_filter_to_sam_text_then_polish_from_it_equals_the_oracle_s_two_commands(pp, dataset):  # noqa: F811
    ctx = pp.Context(0)
    texts = [open(p, "rb").read() for p in dataset["sams"]]
    want_files = [open(p, "rb").read() for p in dataset["outs"]]
    chain = Chain(pp, ctx, dataset["contigs"], texts, pp.MEM_HOST)
    made = []
    try:
        # ---- `filter`: text in, tagged text out
        got = pp.filter_records(ctx, chain.recs[0].raw(), chain.recs[1].raw(), mem=pp.MEM_DEVICE)
        assert got["report"] == dataset["report"]
        tagged = []
        for f, rec in enumerate(chain.recs):
            verdict = got["pass"][f]                                    # the filter's own: NOT ANDed with rec.zp
            t = rec.tagged(verdict)
            made.append(t)
            tagged.append(t)
            assert t.bytes() == want_files[f], f
            assert t.counts() == (int(verdict.sum()), int((verdict == 0).sum()), want_files[f].count(b"\n")) == sm.tagged(texts[f], verdict)[1:]
            assert got["counts"][f][0] == len(verdict) == sm.n_aligned(texts[f])
            assert (verdict == 0).any() and (rec.zp == 0).any()
        # ---- each output compressed and read back: itself again, in device memory
        inflated = []
        for f, t in enumerate(tagged):
            z = t.deflate()
            made.append(z)
            assert 0 < z.n_bytes < t.n_bytes // 2 and z.n_blocks == (t.n_bytes + 65279) // 65280
            back = pp.Bgzf(ctx, (z.bytes_ptr, z.n_bytes), (z.blk_off_ptr, z.n_blocks), mem=pp.MEM_DEVICE)
            made.append(back)
            assert back.n_bytes == t.n_bytes and back.host().tobytes() == want_files[f], f
            inflated.append(back)
        # ---- `polish`: the inflated device text through the front end, gated with the ZP tags alone
        gated = []
        for f, back in enumerate(inflated):
            rec = pp.SamRecords(ctx, (back.bytes_ptr, back.n_bytes), pp.MEM_DEVICE)
            made.append(rec)
            chain.rnames.ids(**rec.rnames(), mem=pp.MEM_DEVICE, out32=rec.contig_ptr)
            chain.qnames.ids(**rec.names(), mem=pp.MEM_DEVICE, out=rec.read_id_ptr)
            assert np.array_equal(rec.zp, got["pass"][f] & chain.recs[f].zp), "a line carries the tag where the filter failed it or it came with it"
            g = pp.gate_records(ctx, rec.raw(), MAX_ERRORS, False, rec.zp, mem=pp.MEM_DEVICE)
            made.append(g)
            gated.append(g)
        want = dataset["want"]
        assert tuple(map(sum, zip(*[g.counts for g in gated]))) == tuple(want["counts"])
        polished, _ = polish(pp, ctx, dataset["contigs"], gated)
        assert polished == im.seqs(want["fasta"])
    finally:
        for o in made[::-1]:
            o.close()
        chain.close()
        ctx.close()
