"""pp_sam_bam inside the record chain, on the dataset of tests/test_bam_chain_gpu.py (its QUAL columns made as long as their SEQ, see
sam_bam_model.with_fitting_qual: the dataset's own lines with an indel are no valid SAM and the encoder refuses them; nothing the
filter or the polish read is touched, and the oracle's report and verdicts are checked to be those of the untouched files):
  * pp_bam_records(pp_sam_bam(text)) is pp_sam_records(text) array by array, SEQ after upper-casing, the contig through one name table;
  * pp_bam_walk_device over the encoded bytes from records_at yields rec_off;
  * `filter` = SamRecords -> filter_records -> .bam() -> .tagged(verdicts) -> .deflate(): the file is, byte for byte, the models'
    deflate_file(tagged(sam_bam_model(text), verdicts)); read back through Bgzf and the BAM front end and polished, the FASTA is the
    oracle's for its two commands.
Needs an MI355X: `-m gpu`."""
import os

import numpy as np
import pytest

import bam_tag_model as tm
import bgzf_deflate_model as D
import filter_model as fm
import ingest_model as im
import sam_bam_model as sb
from test_bam_tag_chain_gpu import front_end
from test_bgzf_chain_gpu import MAX_ERRORS
from test_regroup_chain_gpu import polish
from test_sam_records_chain_gpu import Chain


@pytest.fixture(scope="module")
def pp():
    import polypolish_amd
    return polypolish_amd


@pytest.fixture(scope="module")
def dataset(tmp_path_factory, orc):
    import synth
    d = str(tmp_path_factory.mktemp("sam_bam_chain"))
    ds = synth.rich_dataset(d, seed=23, contig_lens=(4000, 2500), coverage=30, repeat_len=400, repeat_copies=3, zp_frac=0.02)
    contigs = [(c.name, c.assembly) for c in ds["contigs"]]
    texts, sams = [], []
    for f, p in enumerate((ds["sam1"], ds["sam2"])):
        texts.append(sb.with_fitting_qual(open(p, "rb").read()))
        sams.append(os.path.join(d, f"fitting_{f + 1}.sam"))
        with open(sams[-1], "wb") as fh:
            fh.write(texts[-1])
    outs = [os.path.join(d, f"filtered_{i}.sam") for i in (1, 2)]
    plain = [os.path.join(d, f"filtered_plain_{i}.sam") for i in (1, 2)]
    report = orc.filter_files(sams[0], sams[1], outs[0], outs[1])
    assert report == orc.filter_files(ds["sam1"], ds["sam2"], plain[0], plain[1]), "the QUAL column changes nothing the filter reads"
    verdicts = [fm.failed_lines(open(p, "rb").read()) for p in outs]
    assert all(np.array_equal(v, fm.failed_lines(open(p, "rb").read())) for v, p in zip(verdicts, plain))
    want = orc.polish_files(ds["fasta"], outs, max_errors=MAX_ERRORS)
    return {"texts": texts, "contigs": contigs, "report": report, "verdicts": verdicts, "want": want}


@pytest.fixture(scope="module")
def chain(pp, dataset):
    ctx = pp.Context(0)
    c = Chain(pp, ctx, dataset["contigs"], dataset["texts"], pp.MEM_HOST)
    yield c
    c.close()
    ctx.close()


@pytest.mark.gpu
def test_bam_records_of_the_encoded_text_are_the_sam_records(pp, chain, dataset):
    ctx = chain.ctx
    for f, rec in enumerate(chain.recs):
        enc = rec.bam()
        walked = back = None
        try:
            want = sb.encode(dataset["texts"][f])
            assert enc.bytes() == want["bytes"] and enc.records_at == want["records_at"] and np.array_equal(enc.rec_off(), want["rec_off"])
            hdr = pp.bam_header(want["bytes"][:want["records_at"]] + bytes(4))
            assert hdr["names"] == [n.encode() for n, _ in dataset["contigs"]] and hdr["records_at"] == enc.records_at
            ref_map = chain.rnames.ids(hdr["names"] + [b"*"]).astype(np.uint32)
            back = enc.records(ref_map)
            a, b = rec.host(), back.host()
            assert rec.n_rec == back.n_rec == enc.n_rec
            for k in ("flag", "ref_start", "nm", "n_cig", "cigar", "seq_len", "contig"):
                assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
            assert np.array_equal(rec.zp, back.zp) and (rec.zp == 0).any()
            for r in range(rec.n_rec):
                n = int(a["seq_len"][r])
                x, y = int(a["seq_off"][r]), int(b["seq_off"][r])
                assert a["seq"][x:x + n].tobytes().upper() == b["seq"][y:y + n].tobytes(), r
            walked = pp.bam_walk_device(ctx, enc.dev(), enc.records_at, mem=pp.MEM_DEVICE)
            assert np.array_equal(walked.host(), want["rec_off"])
        finally:
            for o in (walked, back, enc):
                if o is not None:
                    o.close()


@pytest.mark.gpu
def test_filter_to_compressed_bam_from_text_then_polish_equals_the_oracle(pp, chain, dataset):
    ctx = chain.ctx
    made = []
    try:
        got = pp.filter_records(ctx, chain.recs[0].raw(), chain.recs[1].raw(), mem=pp.MEM_DEVICE)
        assert got["report"] == dataset["report"]
        gated = []
        for f, rec in enumerate(chain.recs):
            verdict = got["pass"][f]                                    # the filter's own: NOT ANDed with rec.zp
            assert np.array_equal(verdict & rec.zp, dataset["verdicts"][f] & rec.zp) and (verdict == 0).any()
            enc = rec.bam()
            made.append(enc)
            t = enc.tagged(verdict)
            made.append(t)
            z = t.deflate()
            made.append(z)
            model = sb.encode(dataset["texts"][f])
            u = tm.tagged(model["bytes"], model["records_at"], model["rec_off"], verdict)
            assert z.host().tobytes() == D.deflate_file(u)[0], f
            assert z.n_bytes < len(dataset["texts"][f]) // 2
            back = pp.Bgzf(ctx, (z.bytes_ptr, z.n_bytes), (z.blk_off_ptr, z.n_blocks), mem=pp.MEM_DEVICE)
            made.append(back)
            assert back.n_bytes == len(u)
            _, _, again = front_end(pp, ctx, back, chain.rnames, chain.qnames, made)
            assert np.array_equal(again.zp, verdict & rec.zp), "a record carries the tag where the filter failed it or it came with it"
            g = pp.gate_records(ctx, again.raw(), MAX_ERRORS, False, again.zp, mem=pp.MEM_DEVICE)
            made.append(g)
            gated.append(g)
        want = dataset["want"]
        assert tuple(map(sum, zip(*[g.counts for g in gated]))) == tuple(want["counts"])
        polished, _ = polish(pp, ctx, dataset["contigs"], gated)
        assert polished == im.seqs(want["fasta"])
    finally:
        for o in made[::-1]:
            o.close()
