"""The record chain from a BAM file's own bytes: Bgzf (pp_bgzf_inflate) -> .host() prefix -> bam_header -> .bam_walk -> BamRecords(mem =
MEM_DEVICE) -> Names -> filter_records -> gate_records -> (prepare) -> polish, against the oracle's filter + polish on the SAM text.
The dataset is that of tests/test_bam_chain_gpu.py, header in REVERSE FASTA order.  Each file's BAM bytes are cut into BGZF blocks
every 4,093 bytes (a byte later where that would be a record boundary) at level 6, with one stored block, one Z_FIXED block and the EOF block
mixed in.  The compressed bytes are uploaded once; every later byte is produced and consumed in device memory.  Needs an MI355X:
`-m gpu`."""
import os
import zlib

import numpy as np
import pytest

import bam_model as bm
import bgzf_model as zm
import filter_model as fm
import ingest_model as im

MAX_ERRORS = 10
CUT = 4093


def cut_points(n, avoid):
    """0, then every CUT bytes -- one byte later where that would be a record boundary"""
    cuts, at = [0], CUT
    while at < n:
        at += at in avoid
        cuts.append(at)
        at += CUT
    return cuts


def bgzf_file(data, cuts):
    """the bytes cut at `cuts`: level 6, block 1 stored, block 2 Z_FIXED, an EOF block in the middle and one at the end"""
    blocks = []
    for i, (lo, hi) in enumerate(zip(cuts, cuts[1:] + [len(data)])):
        piece = data[lo:hi]
        blocks.append(zm.block(piece, 0) if i == 1 else zm.block(piece, 6, zlib.Z_FIXED) if i == 2 else zm.block(piece, 6))
        if i == 3:
            blocks.append(zm.EOF_BLOCK)
    return b"".join(blocks) + zm.EOF_BLOCK


@pytest.fixture(scope="module")
def dataset(tmp_path_factory, orc):
    import synth
    d = str(tmp_path_factory.mktemp("bgzf_chain"))
    ds = synth.rich_dataset(d, seed=23, contig_lens=(4000, 2500), coverage=30, repeat_len=400, repeat_copies=3, zp_frac=0.02)
    contigs = [(c.name, c.assembly) for c in ds["contigs"]]
    sams = [ds["sam1"], ds["sam2"]]
    outs = [os.path.join(d, f"filtered_{i}.sam") for i in (1, 2)]
    report = orc.filter_files(sams[0], sams[1], outs[0], outs[1])
    verdicts = [fm.failed_lines(open(p, "rb").read()) for p in outs]
    want = orc.polish_files(ds["fasta"], outs, max_errors=MAX_ERRORS)
    return {"sams": sams, "contigs": contigs, "report": report, "verdicts": verdicts, "want": want}


@pytest.fixture(scope="module")
def pp():
    import polypolish_amd
    return polypolish_amd


@pytest.mark.gpu
def test_chain_from_bgzf_bytes_equals_the_oracle_s_filter_and_polish(pp, dataset):
    ctx = pp.Context(0)
    contigs = dataset["contigs"]
    n_contigs = len(contigs)
    header_order = [name for name, _ in contigs][::-1]
    rnames, qnames = pp.Names(ctx, n_contigs), pp.Names(ctx)
    recs, gated, prepared, inflated = [], [], [], []
    try:
        assert rnames.ids([name for name, _ in contigs]).tolist() == list(range(n_contigs))      # FASTA order: the contig indices
        for path in dataset["sams"]:
            enc = bm.encode(open(path, "rb").read(), header_order, [len(dict(contigs)[n]) for n in header_order])
            data = enc["header"] + enc["records"]
            starts = set((enc["rec_off"] + np.uint64(len(enc["header"]))).tolist())
            cuts = cut_points(len(data), starts)
            assert len(cuts) > 8 and not set(cuts[1:]) & starts, "no cut at a record boundary"
            z = pp.Bgzf(ctx, bgzf_file(data, cuts))
            inflated.append(z)
            assert z.n_bytes == len(data) and z.host().tobytes() == data, "the inflated bytes are the uncompressed encoding"
            hdr = pp.bam_header(z.host(0, len(enc["header"])))
            assert hdr["names"] == [n.encode() for n in header_order] and hdr["records_at"] == len(enc["header"])
            ref_map = rnames.ids(hdr["names"] + [b"*"]).astype(np.uint32)
            assert ref_map.tolist() == list(range(n_contigs))[::-1] + [n_contigs], "the header's order is not the FASTA's: the map matters"
            rec_off_ptr, n_rec, end = z.bam_walk(hdr["records_at"])
            assert end == len(data) and n_rec == len(enc["rec_off"])
            rec = pp.BamRecords(ctx, (z.bytes_ptr, z.n_bytes), (rec_off_ptr, n_rec), ref_map, mem=pp.MEM_DEVICE)
            recs.append(rec)
            qnames.ids(**rec.names(), mem=pp.MEM_DEVICE, out=rec.read_id_ptr)                       # one table serves both files
        assert any((r.zp == 0).any() for r in recs) and any((v == 0).any() for v in dataset["verdicts"])

        got = pp.filter_records(ctx, recs[0].raw(), recs[1].raw(), mem=pp.MEM_DEVICE)
        assert got["report"] == dataset["report"]
        passed = []
        for f in range(2):
            # (a line that came with ZP:Z:fail keeps its tag in the oracle's output: its verdict is the caller's zp, not the filter's)
            zp = recs[f].zp
            assert np.array_equal(got["pass"][f] & zp, dataset["verdicts"][f] & zp), f
            passed.append(got["pass"][f] & zp)
        want = dataset["want"]
        off = np.concatenate([[0], np.cumsum([len(s) for _, s in contigs])]).astype(np.uint64)
        bases = np.frombuffer("".join(s for _, s in contigs).upper().encode(), np.uint8)
        gated = [pp.gate_records(ctx, recs[f].raw(), MAX_ERRORS, False, passed[f], mem=pp.MEM_DEVICE) for f in range(2)]
        assert tuple(map(sum, zip(*[g.counts for g in gated]))) == tuple(want["counts"])
        for prepare in (False, True):
            batches = gated
            if prepare:
                prepared = [pp.prepare_batch(ctx, off, g.n_aln, g.ptrs(), g.seq_bytes, g.n_cig_total, pp.MEM_DEVICE) for g in gated]
                batches = prepared
            ctx.polish_begin(off, bases.ctypes.data, pp.MEM_HOST)
            for b in batches:
                if b.n_aln:
                    ctx.polish_add_ptrs(b.n_aln, b.ptrs(), b.seq_bytes, b.n_cig_total, pp.MEM_DEVICE)
            ctx.polish_finish()
            polished, offs, _ = ctx.result()
            assert polished == im.seqs(want["fasta"]), prepare
            assert ctx.took_direct_path() == prepare
    finally:
        for o in prepared + gated + recs + inflated + [rnames, qnames]:
            o.close()
        ctx.close()
