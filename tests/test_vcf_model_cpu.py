"""tests/vcf_model.py pinned without a GPU: every kind of record against hand-written bytes; on the synthetic datasets apply() of the
model's VCF -- made from the ORACLE's --debug TSV -- on the assembly gives the oracle's FASTA, contig by contig; the hand-built jobs of
tests/vcf_jobs.py are what they are built to be; the binding has the new rows."""
import os

import numpy as np
import pytest

import fasta_model as fm
import fasta_text_model as tm
import synth
import vcf_jobs as vj
import vcf_model as vm

HEAD = b"##fileformat=VCFv4.2\n##source=v1\n"
COLS = b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"


def one(bases, edits, name=b"c"):
    nb = [bytes([b]) for b in bases]
    for p, e in edits.items():
        nb[p] = e
    return vm.vcf_from_positions([name], [0, len(bases)], bases, nb, "v1"), nb


def body(vcf, contigs=((b"c", 4),)):
    head = HEAD + b"".join(b"##contig=<ID=%s,length=%d>\n" % c for c in contigs) + COLS
    assert vcf.startswith(head)
    return vcf[len(head):]


@pytest.mark.parametrize("edits, want", [
    ({1: b"T"}, b"c\t2\t.\tC\tT\t.\t.\t.\n"),                      # a substitution
    ({1: b"CA"}, b"c\t2\t.\tC\tCA\t.\t.\t.\n"),                    # an insertion anchors itself
    ({2: b"-"}, b"c\t2\t.\tCG\tC\t.\t.\t.\n"),                     # a deletion inside a contig: the base in front is the anchor
    ({0: b"-"}, b"c\t1\t.\tAC\tC\t.\t.\t.\n"),                     # a deletion at position 0: the base behind it
    ({0: b"", 1: b"-", 2: b"-"}, b"c\t1\t.\tACGT\tT\t.\t.\t.\n"),  # positions 0..k deleted
    ({0: b"-", 1: b"-", 2: b"-", 3: b""}, b"c\t1\t.\tACGT\t<DEL>\t.\t.\t.\n"),  # a whole contig deleted
    ({1: b"T", 2: b"A"}, b"c\t2\t.\tCG\tTA\t.\t.\t.\n"),           # two adjacent edits: one record
    ({1: b"-", 2: b"GT"}, b"c\t2\t.\tCG\tGT\t.\t.\t.\n"),          # a deletion next to an insertion: ALT is not empty
    ({1: b"-C"}, b""),                                             # a winner that leaves the assembly's byte: no edit
    ({1: b"-T", 3: b"T-"}, b"c\t2\t.\tC\tT\t.\t.\t.\n"),           # '-' is dropped wherever it stands
    ({0: b"C", 3: b"TT"}, b"c\t1\t.\tA\tC\t.\t.\t.\nc\t4\t.\tT\tTT\t.\t.\t.\n"),
    ({}, b""),                                                     # a job without edits: the header alone
])
def test_hand_written_records(edits, want):
    vcf, nb = one(b"ACGT", edits)
    assert body(vcf) == want
    (_, got), = vm.apply([(b"c", b"ACGT")], vcf)
    assert got == b"".join(nb).replace(b"-", b"")


def test_runs_never_join_across_a_contig_boundary():
    names, off, bases = [b"one", b"two two"], [0, 3, 6], b"ACGTTA"
    nb = [b"A", b"C", b"T", b"", b"T", b"A"]  # the last position of `one` and the first of `two two`
    vcf = vm.vcf_from_positions(names, off, bases, nb, "v1")
    assert body(vcf, ((b"one", 3), (b"two two", 3))) == b"one\t3\t.\tG\tT\t.\t.\t.\ntwo two\t1\t.\tTT\tT\t.\t.\t.\n"
    assert vm.apply([(b"one", b"ACG"), (b"two two", b"TTA")], vcf) == [(b"one", b"ACT"), (b"two two", b"TA")]
    # contigs of one base: deleted, edited, kept
    vcf = vm.vcf_from_positions([b"a", b"b", b"c"], [0, 1, 2, 3], b"-GT", [b"", b"GA", b"T"], "v1")
    assert body(vcf, ((b"a", 1), (b"b", 1), (b"c", 1))) == b"a\t1\t.\t-\t<DEL>\t.\t.\t.\nb\t1\t.\tG\tGA\t.\t.\t.\n"
    assert vm.apply([(b"a", b"-"), (b"b", b"G"), (b"c", b"T")], vcf) == [(b"a", b""), (b"b", b"GA"), (b"c", b"T")]


def test_bytes_are_written_as_they_are():
    vcf, _ = one(b"acgN", {1: b"n", 3: b"*x"}, name=b"odd;name=<1>")
    assert body(vcf, ((b"odd;name=<1>", 4),)) == b"odd;name=<1>\t2\t.\tc\tn\t.\t.\t.\nodd;name=<1>\t4\t.\tN\t*x\t.\t.\t.\n"


def _contigs_of(fasta_bytes):
    names, _, off, bases = fm.parse(fasta_bytes)
    return names, off, bytes(bases)


def _check_files(orc, fasta, sams, **kw):
    res = orc.polish_files(fasta, sams, debug=True, **kw)
    names, off, bases = _contigs_of(open(fasta, "rb").read())
    vcf = vm.from_debug_tsv(names, off, bases, res["debug"], "v1")
    contigs = [(n, bases[int(off[i]):int(off[i + 1])]) for i, n in enumerate(names)]
    _, want = tm.parse_headers(res["fasta"])
    assert [s for _, s in vm.apply(contigs, vcf)] == want
    return vm.parse(vcf)[1]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_apply_gives_the_oracles_fasta_on_rich_datasets(orc, tmp_path, seed):
    ds = synth.rich_dataset(str(tmp_path), seed=seed, contig_lens=(3000, 1500), coverage=30)
    recs = _check_files(orc, ds["fasta"], [ds["sam1"], ds["sam2"]])
    assert len(recs) > 3, "a dataset with planted assembly errors has records"
    _check_files(orc, ds["fasta"], [ds["sam1"], ds["sam2"]], min_depth=2, fraction_invalid=0.1)


@pytest.mark.parametrize("seed", [5, 6, 7, 8])
def test_apply_gives_the_oracles_fasta_on_random_cigars(orc, tmp_path, seed):
    off, bases, recs = synth.random_cigar_records(seed=seed, k_choices=(1,))
    fa, sam = str(tmp_path / "r.fasta"), str(tmp_path / "r.sam")
    synth.records_to_sam(off, bases, recs, path_fasta=fa, path_sam=sam)
    # (reads whose random differences never agree rarely outvote the assembly: few records or none -- the walk over every position,
    # the contig split and an empty record list are what this holds; the edits are the rich datasets' and the hand-built jobs')
    _check_files(orc, fa, [sam], min_depth=1, max_errors=1000)


@pytest.mark.parametrize("kind", ["sub", "ins", "del", "delins"])
def test_the_hand_built_jobs_are_what_they_are_built_to_be(orc, kind):
    """tests/vcf_jobs.py (the GPU tests' jobs): the oracle edits exactly the wanted positions, and the model's text applies back"""
    off, bases = vj.assembly([700, 300], 9, dash=(699, 700))
    spec = {}
    for p in list(range(1, 600, 3)) + list(range(705, 900, 7)):
        b = int(bases[p])
        spec[p] = {"sub": vj.other(b), "ins": bytes([b]) + vj.other(b, 2), "del": b"-", "delins": b"-" + vj.other(b)}[kind]
    res = orc.polish_records(off, bases, vj.reads(off, bases, spec), min_depth=1, positions=True)
    nb = vj.new_bases(res)
    vj.check_oracle_made(bases, spec, nb)
    vcf = vm.vcf_from_positions([b"a", b"b"], off, bytes(bases), nb, "v1")
    got = vm.apply([(b"a", bytes(bases[:700])), (b"b", bytes(bases[700:]))], vcf)
    o = res["offsets"]
    assert [s for _, s in got] == [res["polished"][int(o[0]):int(o[1])], res["polished"][int(o[1]):int(o[2])]]


def test_the_binding_has_the_new_rows():
    import ctypes as C
    import polypolish_amd as pp
    for name, n_args in (("pp_polish_vcf", 3), ("pp_vcf_out_bytes", 4), ("pp_vcf_out_write", 2), ("pp_vcf_out_kernel_ms", 2),
                         ("pp_vcf_out_free", 1), ("pp_ctx_set_vcf", 3), ("pp_ctx_vcf", 2)):
        assert name in pp.SIGNATURES and len(pp.SIGNATURES[name][1]) == n_args, name
    assert pp.SIGNATURES["pp_polish_vcf"][0] is C.c_int and pp.SIGNATURES["pp_vcf_out_free"][0] is None
    assert "pp_vcf_out_stage_ms_" in pp.HOOKS and "pp_vcf_geometry_" in pp.HOOKS
    assert issubclass(pp.Vcf, pp._Owned) and pp.Vcf._free == "pp_vcf_out_free"
    assert callable(pp.Context.set_vcf) and callable(pp.Context.vcf)
