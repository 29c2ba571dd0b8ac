"""The reference's two-command workflow on BAM, every byte in device memory between the upload of the compressed input and the FASTA:
`filter` = Bgzf -> bam_header -> .bam_walk -> BamRecords -> Names -> filter_records -> BamTagged (pp_bam_tagged), whose files must be
the model's frame(tagged(...)) and whose uncompressed stream the encoding of the ORACLE's filtered SAM files; then `polish` = the
tagged files read back through the same front end (Bgzf with blk_off[b] = b * 65,311, MEM_DEVICE), gated with the ZP tags alone,
prepared and polished, against the oracle's polish of its own filtered SAM files.  Dataset and construction are those of
tests/test_bgzf_chain_gpu.py.  Needs an MI355X: `-m gpu`."""
import os

import numpy as np
import pytest

import bam_model as bm
import bam_tag_model as tm
import ingest_model as im
from test_bgzf_chain_gpu import MAX_ERRORS, bgzf_file, cut_points


@pytest.fixture(scope="module")
def dataset(tmp_path_factory, orc):
    import synth
    d = str(tmp_path_factory.mktemp("bam_tag_chain"))
    ds = synth.rich_dataset(d, seed=23, contig_lens=(4000, 2500), coverage=30, repeat_len=400, repeat_copies=3, zp_frac=0.02)
    contigs = [(c.name, c.assembly) for c in ds["contigs"]]
    sams = [ds["sam1"], ds["sam2"]]
    outs = [os.path.join(d, f"filtered_{i}.sam") for i in (1, 2)]
    report = orc.filter_files(sams[0], sams[1], outs[0], outs[1])
    want = orc.polish_files(ds["fasta"], outs, max_errors=MAX_ERRORS)
    return {"sams": sams, "outs": outs, "contigs": contigs, "report": report, "want": want}


@pytest.fixture(scope="module")
def pp():
    import polypolish_amd
    return polypolish_amd


def front_end(pp, ctx, z, rnames, qnames, made):
    """header -> walk -> BamRecords -> QNAME ids of inflated bytes `z`; -> (header, (rec_off_ptr, n_rec), records)"""
    first = pp.bam_header(z.host(0, min(z.n_bytes, 4096)))
    rec_off_ptr, n_rec, end = z.bam_walk(first["records_at"])
    assert end == z.n_bytes
    ref_map = rnames.ids(first["names"] + [b"*"]).astype(np.uint32)
    rec = pp.BamRecords(ctx, (z.bytes_ptr, z.n_bytes), (rec_off_ptr, n_rec), ref_map, mem=pp.MEM_DEVICE)
    made.append(rec)
    qnames.ids(**rec.names(), mem=pp.MEM_DEVICE, out=rec.read_id_ptr)
    return first, (rec_off_ptr, n_rec), rec


@pytest.mark.gpu
def test_filter_to_bam_files_then_polish_from_them_equals_the_oracle_s_two_commands(pp, dataset):
    import torch
    ctx = pp.Context(0)
    contigs = dataset["contigs"]
    n_contigs = len(contigs)
    header_order = [name for name, _ in contigs][::-1]
    lens = [len(dict(contigs)[n]) for n in header_order]
    rnames, qnames = pp.Names(ctx, n_contigs), pp.Names(ctx)
    made, keep = [], []
    try:
        assert rnames.ids([name for name, _ in contigs]).tolist() == list(range(n_contigs))
        # ---- `filter`: BGZF bytes in, tagged BAM files out
        inflated, recs, walked, datas, heads = [], [], [], [], []
        for path in dataset["sams"]:
            enc = bm.encode(open(path, "rb").read(), header_order, lens)
            data = enc["header"] + enc["records"]
            starts = set((enc["rec_off"] + np.uint64(len(enc["header"]))).tolist())
            z = pp.Bgzf(ctx, bgzf_file(data, cut_points(len(data), starts)))
            made.append(z)
            hdr, offs, rec = front_end(pp, ctx, z, rnames, qnames, made)
            assert hdr["records_at"] == len(enc["header"]) and offs[1] == len(enc["rec_off"])
            inflated.append(z), recs.append(rec), walked.append(offs), datas.append((data, enc)), heads.append(hdr)
        got = pp.filter_records(ctx, recs[0].raw(), recs[1].raw(), mem=pp.MEM_DEVICE)
        assert got["report"] == dataset["report"]
        tagged = []
        for f in range(2):
            data, enc = datas[f]
            at = heads[f]["records_at"]
            verdict = got["pass"][f]                                     # the filter's own: NOT ANDed with recs[f].zp
            t = pp.BamTagged(ctx, (inflated[f].bytes_ptr, inflated[f].n_bytes), at, walked[f], verdict, mem=pp.MEM_DEVICE)
            made.append(t)
            tagged.append(t)
            u = tm.tagged(data, at, enc["rec_off"] + np.uint64(at), verdict)
            assert t.host().tobytes() == tm.frame(u), f
            filtered = bm.encode(open(dataset["outs"][f], "rb").read(), header_order, lens)
            assert u == filtered["header"] + filtered["records"], "the uncompressed stream is the encoding of the oracle's filtered SAM file"
            assert t.counts == (int(verdict.sum()), int((verdict == 0).sum()), (len(u) + tm.PAYLOAD - 1) // tm.PAYLOAD)
            assert (verdict == 0).any() and (recs[f].zp == 0).any()
        # ---- `polish`: the tagged files through the same front end, from device memory
        gated, prepared = [], []
        for f in range(2):
            t = tagged[f]
            n_blocks = t.counts[2]
            blk = torch.from_numpy(tm.blk_off(n_blocks).view(np.int64).copy()).to("cuda:0")
            torch.cuda.synchronize()
            keep.append(blk)
            z = pp.Bgzf(ctx, (t.bytes_ptr, t.n_bytes), (blk.data_ptr(), n_blocks), mem=pp.MEM_DEVICE)
            made.append(z)
            assert z.n_bytes == t.n_bytes - 31 * n_blocks - 28
            _, _, rec = front_end(pp, ctx, z, rnames, qnames, made)
            assert np.array_equal(rec.zp, got["pass"][f] & recs[f].zp), "a record carries the tag where the filter failed it or it came with it"
            g = pp.gate_records(ctx, rec.raw(), MAX_ERRORS, False, rec.zp, mem=pp.MEM_DEVICE)      # the tags alone
            made.append(g)
            gated.append(g)
        want = dataset["want"]
        assert tuple(map(sum, zip(*[g.counts for g in gated]))) == tuple(want["counts"])
        off = np.concatenate([[0], np.cumsum([len(s) for _, s in contigs])]).astype(np.uint64)
        bases = np.frombuffer("".join(s for _, s in contigs).upper().encode(), np.uint8)
        prepared = [pp.prepare_batch(ctx, off, g.n_aln, g.ptrs(), g.seq_bytes, g.n_cig_total, pp.MEM_DEVICE) for g in gated]
        made += prepared
        ctx.polish_begin(off, bases.ctypes.data, pp.MEM_HOST)
        for b in prepared:
            if b.n_aln:
                ctx.polish_add_ptrs(b.n_aln, b.ptrs(), b.seq_bytes, b.n_cig_total, pp.MEM_DEVICE)
        ctx.polish_finish()
        polished, _, _ = ctx.result()
        assert polished == im.seqs(want["fasta"])
    finally:
        for o in made[::-1] + [rnames, qnames]:
            o.close()
        ctx.close()
