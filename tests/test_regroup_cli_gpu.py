"""`polypolish polish --regroup` and `filter-polish --regroup` on COORDINATE-SORTED BAM files, against the oracle on regroup_text of the
sorted SAM text (tests/regroup_model.py); `filter` needs no flag and writes in file order.  The dataset is that of
tests/test_bam_cli_gpu.py, each file sorted by (contig, POS), header in REVERSE FASTA order, BGZF blocks that straddle the records.
Every test but the last runs bin/polypolish as a child process.  Needs an MI355X: `-m gpu`."""
import os
import subprocess

import numpy as np
import pytest

import bam_model as bm
import bam_tag_model as tm
import bgzf_deflate_model as D
import regroup_model as rm
from test_bgzf_chain_gpu import MAX_ERRORS, bgzf_file, cut_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "polypolish")
pytestmark = pytest.mark.gpu


def run(*argv, env=None):
    r = subprocess.run([EXE, *map(str, argv)], capture_output=True, env=dict(os.environ, **(env or {})), timeout=300)
    if r.returncode < 0 or r.returncode in (134, 139) or b"illegal memory access" in r.stderr:  # a crash is a finding: nothing more is started on the device
        pytest.exit(f"polypolish {' '.join(map(str, argv))} ended with {r.returncode}: {r.stderr.decode()[-600:]}", returncode=3)
    return r


def put(path, data):
    with open(path, "wb") as f:
        f.write(data)
    return str(path)


def bam_of(text, contigs, path):
    """SAM bytes as a BGZF file whose blocks straddle the records; -> (path, uncompressed bytes, header length, record offsets)"""
    header_order = [name for name, _ in contigs][::-1]
    enc = bm.encode(text, header_order, [len(dict(contigs)[n]) for n in header_order])
    data = enc["header"] + enc["records"]
    at = len(enc["header"])
    starts = set((enc["rec_off"] + np.uint64(at)).tolist())
    return put(path, bgzf_file(data, cut_points(len(data), starts))), data, at, enc["rec_off"] + np.uint64(at)


@pytest.fixture(scope="module")
def ds(tmp_path_factory, orc):
    d = str(tmp_path_factory.mktemp("regroup_cli"))
    s = rm.sorted_dataset(d)
    s["dir"] = d
    s["bams"], s["grouped_bams"], s["want_filtered_bam"] = [], [], []
    outs = [os.path.join(d, f"oracle_filtered_{i}.sam") for i in (1, 2)]
    orc.filter_files(s["sorted_paths"][0], s["sorted_paths"][1], outs[0], outs[1])
    again = []
    for f in range(2):
        path, data, at, rec_off = bam_of(s["sorted"][f], s["contigs"], os.path.join(d, f"sorted_{f + 1}.bam"))
        s["bams"].append(path)
        s["grouped_bams"].append(bam_of(open(s["sams"][f], "rb").read(), s["contigs"], os.path.join(d, f"grouped_{f + 1}.bam"))[0])
        filtered = open(outs[f], "rb").read()
        verdict = tm.own_verdicts(s["sorted"][f], filtered)
        assert (verdict == 0).any()
        s["want_filtered_bam"].append(D.deflate_file(tm.tagged(data, at, rec_off, verdict))[0])     # file order
        again.append(put(os.path.join(d, f"oracle_filtered_regrouped_{f + 1}.sam"), rm.regroup_text(filtered)[0]))
    s["polish"] = orc.polish_files(s["fasta"], s["regrouped_paths"], max_errors=MAX_ERRORS)
    s["per_file"] = [orc.polish_files(s["fasta"], [p], max_errors=MAX_ERRORS)["counts"] for p in s["regrouped_paths"]]
    s["polish_filtered"] = orc.polish_files(s["fasta"], again, max_errors=MAX_ERRORS)["fasta"]
    return s


def test_polish_regroup_on_the_sorted_pair_is_the_oracle_s_fasta_and_counts(ds):
    r = run("polish", "--regroup", ds["fasta"], *ds["bams"])
    log = r.stderr.decode()
    assert r.returncode == 0 and r.stdout == ds["polish"]["fasta"], log[-800:]
    for path, (alignments, _, reads) in zip(ds["bams"], ds["per_file"]):
        assert f"{path}: {alignments:,} alignments from {reads:,} reads\n" in log
    total, used, _ = ds["polish"]["counts"]
    assert f"  {used:,} alignments kept\n  {total - used:,} alignments discarded\n" in log
    r = run("polish", "--regroup", ds["fasta"], *ds["bams"], env=dict(PP_BAM_PREPARE="1"))
    assert r.returncode == 0 and r.stdout == ds["polish"]["fasta"], r.stderr.decode()[-800:]


def test_polish_without_the_flag_still_refuses_the_sorted_pair(ds):
    r = run("polish", ds["fasta"], *ds["bams"])
    err = r.stderr.decode()
    assert r.returncode == 1 and r.stdout == b"", err[-600:]
    assert "no alignments for read r114 contain sequence" in err.split("Error: ")[-1] and ds["bams"][0] in err.split("Error: ")[-1]


@pytest.fixture(scope="module")
def filtered(ds):
    """`polypolish filter` on the sorted pair, once: it needs no flag"""
    outs = [os.path.join(ds["dir"], f"filtered_{i}.bam") for i in (1, 2)]
    r = run("filter", "--in1", ds["bams"][0], "--in2", ds["bams"][1], "--out1", outs[0], "--out2", outs[1])
    assert r.returncode == 0 and r.stdout == b"", r.stderr.decode()[-800:]
    return outs


def test_filter_and_then_polish_regroup_is_the_oracle_s_two_commands(ds, filtered):
    for f in range(2):
        assert open(filtered[f], "rb").read() == ds["want_filtered_bam"][f], f
    r = run("polish", "--regroup", ds["fasta"], *filtered)
    assert r.returncode == 0 and r.stdout == ds["polish_filtered"], r.stderr.decode()[-800:]


def test_filter_polish_regroup_and_its_outputs_in_file_order(ds, tmp_path):
    r = run("filter-polish", "--regroup", "--in1", ds["bams"][0], "--in2", ds["bams"][1], ds["fasta"])
    assert r.returncode == 0 and r.stdout == ds["polish_filtered"], r.stderr.decode()[-800:]
    outs = [str(tmp_path / f"fused_{i}.bam") for i in (1, 2)]
    r = run("filter-polish", "--in1", ds["bams"][0], "--in2", ds["bams"][1], "--out1", outs[0], "--out2", outs[1], "--regroup", ds["fasta"])
    assert r.returncode == 0 and r.stdout == ds["polish_filtered"], r.stderr.decode()[-800:]
    for f in range(2):
        assert open(outs[f], "rb").read() == ds["want_filtered_bam"][f], f
    r = run("filter-polish", "--in1", ds["bams"][0], "--in2", ds["bams"][1], ds["fasta"])       # without the flag: as before
    assert r.returncode == 1 and b"contain sequence" in r.stderr


def test_polish_regroup_on_the_name_grouped_pair_changes_nothing(ds):
    plain = run("polish", ds["fasta"], *ds["grouped_bams"])
    flagged = run("polish", "--regroup", ds["fasta"], *ds["grouped_bams"])
    assert plain.returncode == 0 and flagged.returncode == 0 and plain.stdout == flagged.stdout and len(plain.stdout) > 6000
    assert plain.stdout == ds["polish"]["fasta"], "on this dataset the regrouped text polishes to the name-grouped original's FASTA"


def test_regroup_on_sam_text_is_refused_by_name(ds, tmp_path):
    for argv in (["polish", "--regroup", ds["fasta"], ds["sorted_paths"][0]],
                 ["filter-polish", "--regroup", "--in1", ds["sorted_paths"][0], "--in2", ds["sorted_paths"][1], "--out1", tmp_path / "o1.sam",
                  "--out2", tmp_path / "o2.sam", ds["fasta"]]):
        r = run(*argv)
        err = r.stderr.decode().split("Error: ")[-1]
        assert r.returncode == 1 and r.stdout == b"", err
        assert ds["sorted_paths"][0] in err and "--regroup takes BAM input" in err
    assert not (tmp_path / "o1.sam").exists(), "refused before the filter wrote anything"


def test_the_flag_takes_no_value_and_filter_has_none(ds):
    r = run("polish", "--regroup=1", ds["fasta"], *ds["bams"])
    assert r.returncode == 2 and b"unexpected value '1' for '--regroup' found; no more were expected" in r.stderr
    r = run("filter-polish", "--regroup=yes", "--in1", ds["bams"][0], "--in2", ds["bams"][1], ds["fasta"])
    assert r.returncode == 2 and b"unexpected value 'yes' for '--regroup'" in r.stderr
    r = run("filter", "--regroup", "--in1", ds["bams"][0], "--in2", ds["bams"][1], "--out1", "x", "--out2", "y")
    assert r.returncode == 2 and b"unexpected argument '--regroup' found" in r.stderr
    assert b"--regroup" in run("polish", "--help").stdout and b"--regroup" in run("filter-polish", "--help").stdout


def test_a_read_of_nothing_but_star_records_is_named_with_the_file_s_own_record(ds):
    """the gate's QUIT under --regroup: the read's name and the 1-based number, counting all records, of its first record in the file"""
    lines = ds["sorted"][0].split(b"\n")
    recs = [i for i, ln in enumerate(lines) if ln and ln[:1] != b"@"]
    names = [lines[i].split(b"\t")[0] for i in recs]
    aligned = [not int(lines[i].split(b"\t")[1]) & 4 for i in recs]
    moved = ds["moved"][0]
    # a read of two aligned records or more that do not stand together, whose first record does not stay where it is
    pick = next(n for j, n in enumerate(names) if j > 50 and aligned[j] and names.index(n) == j and names[j + 1] != n
                and sum(1 for k, m in enumerate(names) if m == n and aligned[k]) >= 2 and int(np.flatnonzero(moved == j)[0]) != j)
    first = names.index(pick)
    for j, n in enumerate(names):
        if n == pick:
            col = lines[recs[j]].split(b"\t")
            col[9] = col[10] = b"*"
            lines[recs[j]] = b"\t".join(col)
    hollow = bam_of(b"\n".join(lines), ds["contigs"], os.path.join(ds["dir"], "hollow.bam"))[0]
    r = run("polish", "--regroup", ds["fasta"], hollow, ds["bams"][1])
    err = r.stderr.decode().split("Error: ")[-1]
    assert r.returncode == 1 and r.stdout == b"", err
    assert f"no alignments for read {pick.decode()} contain sequence" in err and hollow in err and f"(record {first + 1})" in err, err


def test_the_python_face(ds):
    import polypolish_amd as pp
    assert pp.polish(ds["fasta"], ds["bams"], max_errors=MAX_ERRORS, regroup=True) == ds["polish"]["fasta"]
    ctx = pp.Context(0)
    try:
        with pytest.raises(pp.PolypolishError) as e:
            ctx.polish_files(ds["fasta"], ds["bams"])
        assert e.value.code == pp.ERR_QUIT
        assert ctx.polish_files(ds["fasta"], ds["bams"], regroup=True) == ds["polish"]["fasta"]
        with pytest.raises(pp.PolypolishError):      # the keyword holds for its call alone
            ctx.polish_files(ds["fasta"], ds["bams"])
        ctx.set_regroup(True)
        fasta, rep = ctx.filter_polish_files(ds["fasta"], ds["bams"][0], ds["bams"][1])
        assert fasta == ds["polish_filtered"] and rep["after"] < rep["before"]
        ctx.set_regroup(False)
    finally:
        ctx.close()
