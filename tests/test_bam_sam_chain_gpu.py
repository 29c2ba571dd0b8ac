"""pp_bam_sam inside the record chain, on the canonical form of the dataset of tests/test_sam_bam_chain_gpu.py (QUAL columns as long as
their SEQ, SEQ upper-cased: tests/test_bam_sam_model_cpu.py pins that this is all that keeps the dataset from being canonical):
  * pp_bam_sam_encoded(pp_sam_bam(T)) == T, byte for byte, and the model's decode of the encoder's bytes;
  * pp_sam_records of the output is pp_bam_records of the input, record for record;
  * the output with the oracle's verdicts is the oracle's filtered file; through pp_bgzf_deflate -> pp_bgzf_inflate -> pp_sam_records ->
    names -> gate -> polish the FASTA is the oracle's for its two commands.
Needs an MI355X: `-m gpu`."""
import os

import numpy as np
import pytest

import bam_sam_model as bs
import bam_tag_model as tm
import ingest_model as im
import sam_bam_model as sb
from test_bgzf_chain_gpu import MAX_ERRORS
from test_regroup_chain_gpu import polish

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pp():
    import polypolish_amd
    return polypolish_amd


def canonical_texts(ds):
    out = []
    for p in (ds["sam1"], ds["sam2"]):
        lines = sb.with_fitting_qual(open(p, "rb").read()).split(b"\n")
        for i, ln in enumerate(lines):
            if ln and ln[:1] != b"@":
                cols = ln.split(b"\t")
                cols[9] = cols[9].upper()
                lines[i] = b"\t".join(cols)
        out.append(b"\n".join(lines))
    return out


@pytest.fixture(scope="module")
def dataset(tmp_path_factory, orc):
    import synth
    d = str(tmp_path_factory.mktemp("bam_sam_chain"))
    ds = synth.rich_dataset(d, seed=23, contig_lens=(4000, 2500), coverage=30, repeat_len=400, repeat_copies=3, zp_frac=0.02)
    contigs = [(c.name, c.assembly) for c in ds["contigs"]]
    texts, sams = canonical_texts(ds), []
    for f, t in enumerate(texts):
        sams.append(os.path.join(d, f"canonical_{f + 1}.sam"))
        with open(sams[-1], "wb") as fh:
            fh.write(t)
    outs = [os.path.join(d, f"filtered_{i}.sam") for i in (1, 2)]
    orc.filter_files(sams[0], sams[1], outs[0], outs[1])
    filtered = [open(p, "rb").read() for p in outs]
    verdicts = [tm.own_verdicts(t, o) for t, o in zip(texts, filtered)]
    return {"texts": texts, "contigs": contigs, "filtered": filtered, "verdicts": verdicts, "want": orc.polish_files(ds["fasta"], outs, max_errors=MAX_ERRORS)}


@pytest.fixture(scope="module")
def ctx(pp):
    c = pp.Context(0)
    yield c
    c.close()


def test_decode_of_the_encoded_text_is_the_text_and_its_records_are_the_input_s(pp, ctx, dataset):
    contigs = dataset["contigs"]
    rnames = pp.Names(ctx, len(contigs))
    made = [rnames]
    try:
        assert rnames.ids([name for name, _ in contigs]).tolist() == list(range(len(contigs)))
        for f, text in enumerate(dataset["texts"]):
            assert bs.canonical(text) == text
            enc = pp.BamEncoded(ctx, text)
            made.append(enc)
            out = enc.sam()
            made.append(out)
            assert out.bytes() == text, f
            n_al = int(len(dataset["verdicts"][f]))
            assert out.counts() == (n_al, 0, text.count(b"\n"))
            # the text read back by pp_sam_records against the BAM bytes read by pp_bam_records
            s = pp.SamRecords(ctx, out.dev(), pp.MEM_DEVICE)
            made.append(s)
            rnames.ids(**s.rnames(), mem=pp.MEM_DEVICE, out32=s.contig_ptr)
            hdr = pp.bam_header(enc.bytes()[:enc.records_at] + bytes(4))
            b = enc.records(rnames.ids(hdr["names"] + [b"*"]).astype(np.uint32))
            made.append(b)
            x, y = s.host(), b.host()
            assert s.n_rec == b.n_rec == enc.n_rec
            for k in ("flag", "ref_start", "nm", "n_cig", "cigar", "seq_len", "contig"):
                assert x[k].dtype == y[k].dtype and np.array_equal(x[k], y[k]), k
            assert np.array_equal(s.zp, b.zp) and (s.zp == 0).any()
            for r in range(s.n_rec):
                n = int(x["seq_len"][r])
                i, j = int(x["seq_off"][r]), int(y["seq_off"][r])
                assert x["seq"][i:i + n].tobytes() == y["seq"][j:j + n].tobytes(), r
    finally:
        for o in made[::-1]:
            o.close()


def test_tagged_text_is_the_oracle_s_file_and_polishes_to_the_oracle_s_fasta(pp, ctx, dataset):
    contigs = dataset["contigs"]
    rnames, qnames = pp.Names(ctx, len(contigs)), pp.Names(ctx)
    made, gated = [rnames, qnames], []
    try:
        assert rnames.ids([name for name, _ in contigs]).tolist() == list(range(len(contigs)))
        for f, text in enumerate(dataset["texts"]):
            enc = pp.BamEncoded(ctx, text)
            made.append(enc)
            out = enc.sam(dataset["verdicts"][f])
            made.append(out)
            assert out.bytes() == dataset["filtered"][f], "the oracle's filtered file of the same text"
            z = out.deflate()
            made.append(z)
            assert z.n_bytes < out.n_bytes // 2
            back = pp.Bgzf(ctx, (z.bytes_ptr, z.n_bytes), (z.blk_off_ptr, z.n_blocks), mem=pp.MEM_DEVICE)
            made.append(back)
            assert back.n_bytes == out.n_bytes
            s = pp.SamRecords(ctx, (back.bytes_ptr, back.n_bytes), pp.MEM_DEVICE)
            made.append(s)
            rnames.ids(**s.rnames(), mem=pp.MEM_DEVICE, out32=s.contig_ptr)
            qnames.ids(**s.names(), mem=pp.MEM_DEVICE, out=s.read_id_ptr)
            g = pp.gate_records(ctx, s.raw(), MAX_ERRORS, False, s.zp, mem=pp.MEM_DEVICE)
            made.append(g)
            gated.append(g)
        want = dataset["want"]
        assert tuple(map(sum, zip(*[g.counts for g in gated]))) == tuple(want["counts"])
        polished, _ = polish(pp, ctx, contigs, gated)
        assert polished == im.seqs(want["fasta"])
    finally:
        for o in made[::-1]:
            o.close()
