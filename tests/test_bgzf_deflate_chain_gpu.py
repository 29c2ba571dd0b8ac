"""The reference's two-command workflow on BAM with COMPRESSED files between the commands: `filter` = Bgzf -> ... -> filter_records ->
BamTagged -> .deflate() -> .write(); then `polish` = the files read back FROM DISK through Bgzf -> BamRecords -> the gate -> prepare ->
polish, against the oracle's polish of its own filtered SAM files.  gzip reads every written file back to the level-0 file's
uncompressed stream.  Dataset and helpers are those of tests/test_bam_tag_chain_gpu.py.  Needs an MI355X: `-m gpu`."""
import gzip
import os

import numpy as np
import pytest

import bam_model as bm
import bam_tag_model as tm
import bgzf_deflate_model as D
import ingest_model as im
from test_bam_tag_chain_gpu import dataset, front_end, pp  # noqa: F401 (fixtures)
from test_bgzf_chain_gpu import MAX_ERRORS, bgzf_file, cut_points


@pytest.mark.gpu
def test_filter_to_compressed_bam_files_then_polish_from_disk_equals_the_oracle(pp, dataset, tmp_path):  # noqa: F811
    ctx = pp.Context(0)
    contigs = dataset["contigs"]
    header_order = [name for name, _ in contigs][::-1]
    lens = [len(dict(contigs)[n]) for n in header_order]
    rnames, qnames = pp.Names(ctx, len(contigs)), pp.Names(ctx)
    made = []
    try:
        assert rnames.ids([name for name, _ in contigs]).tolist() == list(range(len(contigs)))
        # ---- `filter`: BGZF bytes in, compressed tagged BAM files on disk
        inflated, recs, walked, datas, heads = [], [], [], [], []
        for path in dataset["sams"]:
            enc = bm.encode(open(path, "rb").read(), header_order, lens)
            data = enc["header"] + enc["records"]
            starts = set((enc["rec_off"] + np.uint64(len(enc["header"]))).tolist())
            z = pp.Bgzf(ctx, bgzf_file(data, cut_points(len(data), starts)))
            made.append(z)
            hdr, offs, rec = front_end(pp, ctx, z, rnames, qnames, made)
            inflated.append(z), recs.append(rec), walked.append(offs), datas.append((data, enc)), heads.append(hdr)
        got = pp.filter_records(ctx, recs[0].raw(), recs[1].raw(), mem=pp.MEM_DEVICE)
        assert got["report"] == dataset["report"]
        paths = []
        for f in range(2):
            data, enc = datas[f]
            at = heads[f]["records_at"]
            t = pp.BamTagged(ctx, (inflated[f].bytes_ptr, inflated[f].n_bytes), at, walked[f], got["pass"][f], mem=pp.MEM_DEVICE)
            made.append(t)
            c = t.deflate()
            made.append(c)
            u = tm.tagged(data, at, enc["rec_off"] + np.uint64(at), got["pass"][f])
            assert t.host().tobytes() == tm.frame(u)
            path = os.path.join(str(tmp_path), f"filtered_{f + 1}.bam")
            c.write(path)
            on_disk = open(path, "rb").read()
            assert gzip.decompress(on_disk) == u, "gzip reads the written file back to the level-0 file's uncompressed stream"
            assert on_disk == D.deflate_file(u)[0] and len(on_disk) < t.n_bytes / 2 and c.counts[2] == c.n_blocks
            paths.append(path)
        # ---- `polish`: the files from disk through the front end
        gated = []
        for f in range(2):
            z = pp.Bgzf(ctx, open(paths[f], "rb").read())
            made.append(z)
            _, _, rec = front_end(pp, ctx, z, rnames, qnames, made)
            assert np.array_equal(rec.zp, got["pass"][f] & recs[f].zp)
            g = pp.gate_records(ctx, rec.raw(), MAX_ERRORS, False, rec.zp, mem=pp.MEM_DEVICE)
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
