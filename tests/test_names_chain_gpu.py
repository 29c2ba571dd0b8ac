"""The record chain filter_records -> gate_records -> (prepare) -> polish with NO host dictionary anywhere: pp_raw_batch.contig
comes from a pp_names seeded with the assembly's contig names, .read_id from one pp_names shared by both SAM files, against the
oracle's filter + polish on the equivalent text.  The dataset is the one of tests/test_filter_records_gpu.py plus, in each file, one
aligned line whose RNAME is not in the FASTA -- two different unknown names.  A record that passes the gate with an unknown contig is
an error from pp_polish_finish (as the reference quits over it), so the two lines carry an NM above max_errors: the first test shows
on the CPU that the oracle takes the text that way (and quits without the NM).  The GPU tests need an MI355X: `-m gpu`."""
import os

import numpy as np
import pytest

import filter_model as fm
import gate_model as gm
import ingest_model as im
import names_model as nm
import synth

UNKNOWN = ("plasmid_A", "plasmid_B")
MAX_ERRORS = 10


def stray_line(rname, nm_tag):
    return f"stray\t0\t{rname}\t101\t60\t100M\t*\t0\t0\t{'ACGT' * 25}\t{'I' * 100}\tNM:i:{nm_tag}\n"


@pytest.fixture(scope="module")
def dataset(tmp_path_factory, orc):
    d = str(tmp_path_factory.mktemp("names_chain"))
    ds = synth.rich_dataset(d, seed=23, contig_lens=(4000, 2500), coverage=30, repeat_len=400, repeat_copies=3, zp_frac=0.02)
    contigs = [(c.name, c.assembly) for c in ds["contigs"]]
    sams, quitting = [], []
    for f, src in enumerate((ds["sam1"], ds["sam2"])):
        text = open(src).read()
        for nm_tag, into in ((MAX_ERRORS + 40, sams), (0, quitting)):
            into.append(os.path.join(d, f"stray_nm{nm_tag}_{f + 1}.sam"))
            with open(into[-1], "w") as out:
                out.write(text + stray_line(UNKNOWN[f], nm_tag))
    outs = [os.path.join(d, f"filtered_{i}.sam") for i in (1, 2)]
    report = orc.filter_files(sams[0], sams[1], outs[0], outs[1])
    verdicts = [fm.failed_lines(open(p, "rb").read()) for p in outs]
    return {"fasta": ds["fasta"], "plain": [ds["sam1"], ds["sam2"]], "sams": sams, "quitting": quitting, "filtered": outs, "contigs": contigs,
            "report": report, "verdicts": verdicts, "dir": d}


def test_the_oracle_takes_the_two_unknown_references_as_the_chain_expects(orc, dataset):
    # the filter knows no assembly: the two lines are records like any other, and its output carries them
    for f in range(2):
        assert nm.sam_column(open(dataset["filtered"][f], "rb").read(), column=2)[-1] == UNKNOWN[f].encode()
        assert len(dataset["verdicts"][f]) == len(nm.sam_column(open(dataset["sams"][f], "rb").read()))
    # the polish: above max_errors the lines are counted and dropped before anybody asks for their contig ...
    want = orc.polish_files(dataset["fasta"], dataset["filtered"], max_errors=MAX_ERRORS)
    plain = orc.polish_files(dataset["fasta"], dataset["plain"], max_errors=MAX_ERRORS)
    assert want["counts"][0] == plain["counts"][0] + 2
    # ... and with an NM that passes, the reference quits over the name
    with pytest.raises(orc.OrcError):
        orc.polish_files(dataset["fasta"], dataset["quitting"], max_errors=MAX_ERRORS)


@pytest.fixture(scope="module")
def pp():
    import polypolish_amd
    return polypolish_amd


@pytest.mark.gpu
def test_chain_with_interned_names_equals_the_oracle_s_filter_and_polish(pp, orc, dataset):
    ctx = pp.Context(0)
    contigs = dataset["contigs"]
    n_contigs = len(contigs)
    rnames, qnames = pp.Names(ctx, n_contigs), pp.Names(ctx)
    try:
        assert rnames.ids([name for name, _ in contigs]).tolist() == list(range(n_contigs))      # FASTA order: the contig indices
        raws, zps, unknown_ids, seen = [], [], [], set()
        for f, path in enumerate(dataset["sams"]):
            text = open(path, "rb").read()
            raw, zp = gm.raw_from_text(contigs, text)                      # everything but the two ids comes from here
            lines = [ln.split("\t") for ln in im._lines(text) if ln and ln[0] != "@"]
            assert len(lines) == len(raw["flag"]) and all(cols[0] != "" for cols in lines)     # no empty QNAME: its rule changes nothing here
            contig = rnames.ids([cols[2] for cols in lines]).astype(np.uint32)
            known = raw["contig"] != gm.NO_CONTIG
            aligned = (raw["flag"] & 4) == 0
            assert np.array_equal(contig[known], raw["contig"][known]) and (~known & aligned).sum() == 1
            unknown_ids.append(int(contig[~known & aligned][0]))
            raw["contig"] = contig
            read_id = qnames.ids([cols[0] for cols in lines])              # one table over both files
            raw["read_id"] = nm.empty_qname_rule(read_id, [cols[0] for cols in lines], raw["flag"])
            assert np.array_equal(raw["read_id"], read_id)                 # (no empty QNAME: the rule changes nothing)
            seen |= {cols[0] for cols in lines}
            raws.append(raw)
            zps.append(zp)
        # the two unknown references: distinct ids behind the contigs', and the table knows their names ("*" of unaligned lines is a name, too)
        assert unknown_ids[0] != unknown_ids[1] and min(unknown_ids) >= n_contigs
        assert [rnames.name(i) for i in unknown_ids] == [u.encode() for u in UNKNOWN]
        assert qnames.count == len(seen) and rnames.count == n_contigs + 3

        got = pp.filter_records(ctx, raws[0], raws[1])
        assert got["report"] == dataset["report"]
        assert any((v == 0).any() for v in dataset["verdicts"])
        passed = []
        for f in range(2):
            # (a line that came with ZP:Z:fail keeps its tag in the oracle's output: its verdict is the caller's zp, not the filter's)
            assert np.array_equal(got["pass"][f] & zps[f], dataset["verdicts"][f] & zps[f]), f
            passed.append(got["pass"][f] & zps[f])
        want = orc.polish_files(dataset["fasta"], dataset["filtered"], max_errors=MAX_ERRORS)
        off = np.concatenate([[0], np.cumsum([len(s) for _, s in contigs])]).astype(np.uint64)
        bases = np.frombuffer("".join(s for _, s in contigs).upper().encode(), np.uint8)
        for prepare in (False, True):
            res = ctx.polish_raw(off, bases, raws, max_errors=MAX_ERRORS, passed=passed, prepare=prepare)
            assert res["polished"] == im.seqs(want["fasta"]), prepare
            assert tuple(map(sum, zip(*res["counts"]))) == tuple(want["counts"])
            assert ctx.took_direct_path() == prepare
    finally:
        rnames.close()
        qnames.close()
        ctx.close()
