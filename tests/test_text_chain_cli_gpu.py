"""`polypolish polish / filter / filter-polish --text_chain`: SAM text, plain or bgzipped, through the record chain on the device, against
the oracle and against the run without the flag.  The dataset is that of tests/test_regroup_cli_gpu.py (regroup_model.sorted_dataset):
its name-grouped texts, its coordinate-sorted texts (which only this route takes as text: --regroup) and the oracle's regroup_text of
them; the seams and the errors are hand-built pairs of a dozen reads.  Every test but the last runs bin/polypolish as a child process.
Needs an MI355X: `-m gpu`."""
import gzip
import os
import re

import pytest

import bgzf_deflate_model as D
import ingest_model as im
import regroup_model as rm
import sam_bam_model as sb
from test_bgzf_chain_gpu import MAX_ERRORS, bgzf_file, cut_points
from test_regroup_cli_gpu import bam_of, put, run

pytestmark = pytest.mark.gpu


def tail(r):
    """what stands behind the last "Error: " of a run's log"""
    return r.stderr.decode().split("Error: ")[-1]


def log_of(r):
    """the log without its one line that differs from run to run"""
    return re.sub(r"Time to run: [^\n]*\n", "", r.stderr.decode())


@pytest.fixture(scope="module")
def ds(tmp_path_factory, orc):
    d = str(tmp_path_factory.mktemp("text_chain_cli"))
    s = rm.sorted_dataset(d)
    s["dir"] = d
    s["grouped"] = orc.polish_files(s["fasta"], s["sams"], max_errors=MAX_ERRORS)
    s["grouped_per_file"] = [orc.polish_files(s["fasta"], [p], max_errors=MAX_ERRORS)["counts"] for p in s["sams"]]
    s["polish"] = orc.polish_files(s["fasta"], s["regrouped_paths"], max_errors=MAX_ERRORS)
    s["per_file"] = [orc.polish_files(s["fasta"], [p], max_errors=MAX_ERRORS)["counts"] for p in s["regrouped_paths"]]
    outs = [os.path.join(d, f"oracle_filtered_{i}.sam") for i in (1, 2)]
    orc.filter_files(s["sorted_paths"][0], s["sorted_paths"][1], outs[0], outs[1])
    s["want_filtered"] = [open(p, "rb").read() for p in outs]
    again = [put(os.path.join(d, f"oracle_filtered_regrouped_{f + 1}.sam"), rm.regroup_text(s["want_filtered"][f])[0]) for f in range(2)]
    s["polish_filtered"] = orc.polish_files(s["fasta"], again, max_errors=MAX_ERRORS)["fasta"]
    return s


def counts_in_log(log, paths, per_file, counts):
    for path, (alignments, _, reads) in zip(paths, per_file):
        assert f"{path}: {alignments:,} alignments from {reads:,} reads\n" in log, log[-800:]
    total, used, _ = counts
    assert f"  {used:,} alignments kept\n  {total - used:,} alignments discarded\n" in log, log[-800:]


# ---- the three commands on the dataset ------------------------------------------------------------------------------------------

def test_polish_on_the_name_grouped_pair_is_the_oracle_s_and_the_unflagged_run_s(ds):
    plain = run("polish", ds["fasta"], *ds["sams"])
    r = run("polish", "--text_chain", ds["fasta"], *ds["sams"])
    assert r.returncode == 0 and r.stdout == ds["grouped"]["fasta"] == plain.stdout, tail(r)
    counts_in_log(r.stderr.decode(), ds["sams"], ds["grouped_per_file"], ds["grouped"]["counts"])
    assert log_of(r) == log_of(plain), "the log is the unflagged run's, line for line"
    r = run("polish", "--text_chain", ds["fasta"], *ds["sams"], env=dict(PP_BAM_PREPARE="1"))
    assert r.returncode == 0 and r.stdout == ds["grouped"]["fasta"] and log_of(r) == log_of(plain), tail(r)


def test_polish_regroup_on_the_sorted_texts_is_the_oracle_on_the_regrouped_texts(ds):
    r = run("polish", "--text_chain", "--regroup", ds["fasta"], *ds["sorted_paths"])
    assert r.returncode == 0 and r.stdout == ds["polish"]["fasta"], tail(r)
    counts_in_log(r.stderr.decode(), ds["sorted_paths"], ds["per_file"], ds["polish"]["counts"])


def test_the_sorted_texts_without_regroup_are_refused_with_the_line_of_the_read_s_first_record(ds):
    r = run("polish", "--text_chain", ds["fasta"], *ds["sorted_paths"])
    err = tail(r)
    assert r.returncode == 1 and r.stdout == b"", err
    m = re.search(r'no alignments for read (\S+) contain sequence: "([^"]*)" \(line (\d+)\)', err)
    assert m and m.group(2) == ds["sorted_paths"][0], err
    lines = ds["sorted"][0].split(b"\n")
    assert lines[int(m.group(3)) - 1].split(b"\t")[0] == m.group(1).encode(), "the line, counting the header, is a record of that read"
    plain = run("polish", ds["fasta"], *ds["sorted_paths"])
    assert plain.returncode == 1 and f"no alignments for read {m.group(1)} contain sequence" in tail(plain), "the same read as without the flag"


@pytest.fixture(scope="module")
def filtered(ds):
    """`polypolish filter --text_chain` on the sorted pair, once: it needs no --regroup"""
    outs = [os.path.join(ds["dir"], f"filtered_{i}.sam") for i in (1, 2)]
    r = run("filter", "--text_chain", "--in1", ds["sorted_paths"][0], "--in2", ds["sorted_paths"][1], "--out1", outs[0], "--out2", outs[1])
    assert r.returncode == 0 and r.stdout == b"", tail(r)
    return outs, r


def test_filter_writes_the_oracle_s_outputs_in_file_order_with_the_unflagged_log(ds, filtered, tmp_path):
    outs, r = filtered
    for f in range(2):
        assert open(outs[f], "rb").read() == ds["want_filtered"][f], f
    plain_outs = [str(tmp_path / f"plain_{i}.sam") for i in (1, 2)]
    plain = run("filter", "--in1", ds["sorted_paths"][0], "--in2", ds["sorted_paths"][1], "--out1", plain_outs[0], "--out2", plain_outs[1])
    assert plain.returncode == 0
    assert log_of(r).replace(outs[0], "O1").replace(outs[1], "O2") == log_of(plain).replace(plain_outs[0], "O1").replace(plain_outs[1], "O2")


def test_filter_and_then_polish_regroup_is_the_oracle_s_two_commands(ds, filtered):
    r = run("polish", "--text_chain", "--regroup", ds["fasta"], *filtered[0])
    assert r.returncode == 0 and r.stdout == ds["polish_filtered"], tail(r)


def test_filter_polish_regroup_with_and_without_outputs(ds, tmp_path):
    r = run("filter-polish", "--text_chain", "--regroup", "--in1", ds["sorted_paths"][0], "--in2", ds["sorted_paths"][1], ds["fasta"])
    assert r.returncode == 0 and r.stdout == ds["polish_filtered"], tail(r)
    outs = [str(tmp_path / f"fused_{i}.sam") for i in (1, 2)]
    r = run("filter-polish", "--in1", ds["sorted_paths"][0], "--in2", ds["sorted_paths"][1], "--out1", outs[0], "--out2", outs[1], "--regroup",
            "--text_chain", ds["fasta"])
    assert r.returncode == 0 and r.stdout == ds["polish_filtered"], tail(r)
    for f in range(2):
        assert open(outs[f], "rb").read() == ds["want_filtered"][f], f
    r = run("filter-polish", "--text_chain", "--in1", ds["sorted_paths"][0], "--in2", ds["sorted_paths"][1], ds["fasta"])    # no --regroup: the gate's refusal
    assert r.returncode == 1 and "contain sequence" in tail(r) and "(line " in tail(r)
    # on the name-grouped pair the fused command is the unflagged one's, FASTA and log
    plain = run("filter-polish", "--in1", ds["sams"][0], "--in2", ds["sams"][1], ds["fasta"])
    r = run("filter-polish", "--text_chain", "--in1", ds["sams"][0], "--in2", ds["sams"][1], ds["fasta"])
    assert plain.returncode == 0 and r.returncode == 0 and r.stdout == plain.stdout and log_of(r) == log_of(plain), tail(r)


# ---- bgzipped text --------------------------------------------------------------------------------------------------------------

def text_cuts(text):
    """cuts every 4,093 bytes (inside a line), and three chosen ones: one inside a "\\r\\n" where the text has one, one right behind
    a newline, one a byte behind that; bgzf_file adds the mid-file empty block"""
    cuts = set(cut_points(len(text), set()))
    nl = [i for i in range(20000, min(len(text), 60000)) if text[i:i + 1] == b"\n"]
    cuts.add(nl[0] if text[nl[0] - 1:nl[0]] == b"\r" else nl[0] - 1)    # between "\r" and "\n" (or in front of a lone "\n")
    cuts.add(nl[5] + 1)
    cuts.add(nl[9] + 2)
    return sorted(cuts)


@pytest.fixture(scope="module")
def zipped(ds):
    """the sorted pair bgzipped (what the filter is asked about), and the name-grouped pair with its second file in "\\r\\n" lines"""
    out = {"sorted": [], "grouped": [], "grouped_plain": []}
    for f in range(2):
        text = ds["sorted"][f]
        out["sorted"].append(put(os.path.join(ds["dir"], f"sorted_{f + 1}.sam.gz"), bgzf_file(text, text_cuts(text))))
        text = open(ds["sams"][f], "rb").read()
        if f == 1:
            text = text.replace(b"\n", b"\r\n")
        out["grouped_plain"].append(put(os.path.join(ds["dir"], f"grouped_eol_{f + 1}.sam"), text))
        cuts = text_cuts(text)
        assert f == 0 or any(text[c - 1:c + 1] == b"\r\n" for c in cuts), "a block ends inside a \\r\\n"
        out["grouped"].append(put(os.path.join(ds["dir"], f"grouped_{f + 1}.sam.gz"), bgzf_file(text, cuts)))
    return out


def test_bgzipped_polish_and_filter_polish_match_the_plain_text_runs(ds, zipped):
    plain = run("polish", "--text_chain", ds["fasta"], *zipped["grouped_plain"])
    r = run("polish", "--text_chain", ds["fasta"], *zipped["grouped"])
    assert plain.returncode == 0 and plain.stdout == ds["grouped"]["fasta"], tail(plain)
    assert r.returncode == 0 and r.stdout == plain.stdout, tail(r)
    for a, b in zip(zipped["grouped"], zipped["grouped_plain"]):
        assert log_of(r).count(a) == log_of(plain).count(b) == 2
    r = run("polish", "--text_chain", "--regroup", ds["fasta"], *zipped["sorted"])
    assert r.returncode == 0 and r.stdout == ds["polish"]["fasta"], tail(r)
    r = run("filter-polish", "--text_chain", "--regroup", "--in1", zipped["sorted"][0], "--in2", zipped["sorted"][1], ds["fasta"])
    assert r.returncode == 0 and r.stdout == ds["polish_filtered"], tail(r)
    r = run("polish", ds["fasta"], *zipped["grouped"])                  # without the flag: refused as before
    assert r.returncode == 1 and "is BGZF-compressed but does not hold BAM" in tail(r)


def test_bgzipped_filter_writes_the_model_s_compression_of_the_oracle_s_text(ds, zipped, tmp_path):
    outs = [str(tmp_path / f"filtered_{i}.sam.gz") for i in (1, 2)]
    r = run("filter", "--text_chain", "--in1", zipped["sorted"][0], "--in2", zipped["sorted"][1], "--out1", outs[0], "--out2", outs[1])
    assert r.returncode == 0, tail(r)
    for f in range(2):
        got = open(outs[f], "rb").read()
        assert gzip.decompress(got) == ds["want_filtered"][f], f
        assert got == D.deflate_file(ds["want_filtered"][f])[0], f


def test_a_flipped_crc_names_the_path_and_the_block(ds, zipped, tmp_path):
    data = bytearray(open(zipped["sorted"][0], "rb").read())
    at, k = 0, 0
    while k < 2:                                        # the third block's CRC32: the four bytes in front of its ISIZE
        at += int.from_bytes(data[at + 16:at + 18], "little") + 1
        k += 1
    end = at + int.from_bytes(data[at + 16:at + 18], "little") + 1
    data[end - 8] ^= 0x40
    bad = put(tmp_path / "flipped.sam.gz", bytes(data))
    for argv in (["polish", "--text_chain", "--regroup", ds["fasta"], bad, zipped["sorted"][1]],
                 ["filter", "--text_chain", "--in1", bad, "--in2", zipped["sorted"][1], "--out1", tmp_path / "o1", "--out2", tmp_path / "o2"]):
        r = run(*argv)
        assert r.returncode == 1 and r.stdout == b"" and bad in tail(r) and "(block 3)" in tail(r), tail(r)
    assert not (tmp_path / "o1").exists()


def test_out_bam_writes_the_bytes_of_the_run_without_the_flag(ds, tmp_path):
    """(the dataset's QUAL columns made as long as their SEQ, as in tests/test_out_bam_cli_gpu.py: the encoder refuses the others)"""
    ins = [put(tmp_path / f"fitting_{f + 1}.sam", sb.with_fitting_qual(ds["sorted"][f])) for f in range(2)]
    got, want = [str(tmp_path / f"chain_{i}.bam") for i in (1, 2)], [str(tmp_path / f"fused_{i}.bam") for i in (1, 2)]
    a = run("filter", "--out_bam", "--in1", ins[0], "--in2", ins[1], "--out1", want[0], "--out2", want[1])
    b = run("filter", "--out_bam", "--text_chain", "--in1", ins[0], "--in2", ins[1], "--out1", got[0], "--out2", got[1])
    assert a.returncode == 0 and b.returncode == 0, (tail(a), tail(b))
    for f in range(2):
        assert open(got[f], "rb").read() == open(want[f], "rb").read() and os.path.getsize(got[f]) > 1000, f
    assert log_of(b).replace(got[0], "O1").replace(got[1], "O2") == log_of(a).replace(want[0], "O1").replace(want[1], "O2")
    # a line the encoder refuses: the same sentence either way, the input's path and line, and nothing written
    outs = [str(tmp_path / f"refused_{i}.bam") for i in (1, 2)]
    for flag in ([], ["--text_chain"]):
        r = run("filter", "--out_bam", *flag, "--in1", ds["sorted_paths"][0], "--in2", ds["sorted_paths"][1], "--out1", outs[0], "--out2", outs[1])
        assert r.returncode == 1 and "--out_bam" in tail(r) and "a QUAL that does not fit its SEQ" in tail(r), tail(r)
        assert re.search(r'"%s" \(line \d+\)' % re.escape(ds["sorted_paths"][0]), tail(r)) and not os.path.exists(outs[0])


# ---- seams of a text, on hand-built pairs ---------------------------------------------------------------------------------------

def small_pair(d, name, build, eol="\n", final=True):
    """-> (fasta path, [path1, path2], [text1, text2]): build(g, T) adds the lines; the second file is the mates' (same lines, other strand)"""
    paths, texts = [], []
    for f, mate in enumerate((False, True)):
        g, T = im.Gen(900, (3000,), mate=mate), im.Text(eol)
        T.add("@SQ\tSN:ctg0\tLN:3000")
        build(g, T)
        texts.append(T.bytes(final))
        paths.append(put(os.path.join(d, f"{name}_{f + 1}.sam"), texts[-1]))
    return put(os.path.join(d, name + ".fasta"), im.fasta_text(g.contigs)), paths, texts


def dozen(g, T, n=12):
    for i in range(n):
        T.add(g.line(pos=100 + 150 * i, n=60, nm=0))


def both_ways(argv_of, check=None):
    """the command with and without --text_chain: the same exit code, stdout and error"""
    plain, r = run(*argv_of([])), run(*argv_of(["--text_chain"]))
    assert r.returncode == plain.returncode and r.stdout == plain.stdout, (tail(r), tail(plain))
    if plain.returncode:
        assert tail(r) == tail(plain)
    if check:
        check(plain)
    return r


SEAMS = {
    "no_final_newline": dict(build=dozen, final=False),
    "crlf": dict(build=dozen, eol="\r\n"),
    "crlf_no_final_newline": dict(build=dozen, eol="\r\n", final=False),
    "came_with_zp_fail": dict(build=lambda g, T: [T.add(g.line(pos=100 + 150 * i, n=60, nm=0, tags=("ZP:Z:fail",) if i % 4 == 1 else ())) for i in range(12)]),
    "unaligned_between_a_read_s_records": dict(build=lambda g, T: [T.add(ln) for i in range(6) for ln in (
        g.line(name=f"m{i}", pos=100 + 150 * i, n=60, nm=0), g.line(name=f"u{i}", flag=4, rname="*", cigar="*", nm=None, pos=0),
        g.line(name=f"m{i}", pos=2000, n=60, nm=0, seq="*", cigar="60M", flag=256))] + [T.add(g.line(pos=1000 + 100 * i, n=60, nm=0)) for i in range(8)]),
}


@pytest.mark.parametrize("name", sorted(SEAMS))
def test_a_seam_of_the_text_changes_nothing(tmp_path, name):
    fasta, paths, texts = small_pair(str(tmp_path), name, **SEAMS[name])
    r = both_ways(lambda flag: ["polish", *flag, fasta, *paths])
    assert r.returncode == 0 and len(r.stdout) > 3000
    outs = {flag: [str(tmp_path / f"{flag}_{i}.sam") for i in (1, 2)] for flag in ("plain", "chain")}
    r = both_ways(lambda flag: ["filter", *flag, "--in1", paths[0], "--in2", paths[1], "--out1", outs["chain" if flag else "plain"][0],
                                "--out2", outs["chain" if flag else "plain"][1]])
    assert r.returncode == 0, tail(r)
    for f in range(2):
        assert open(outs["chain"][f], "rb").read() == open(outs["plain"][f], "rb").read(), f
    both_ways(lambda flag: ["filter-polish", *flag, "--in1", paths[0], "--in2", paths[1], fasta])


def test_header_lines_only(tmp_path):
    fasta, paths, _ = small_pair(str(tmp_path), "headers", lambda g, T: T.add("@CO\tnothing else"))
    plain, r = run("polish", fasta, *paths), run("polish", "--text_chain", fasta, *paths)
    assert plain.returncode == 101 and "no aligned records to process" in tail(plain), "the reference panics on its empty read group"
    assert r.returncode == 1 and r.stdout == b"" and tail(r).strip() == f'no alignments in "{paths[0]}"', "the chain's sentence, as for BAM"
    r = both_ways(lambda flag: ["filter", *flag, "--in1", paths[0], "--in2", paths[1], "--out1", tmp_path / "o1", "--out2", tmp_path / "o2"])
    assert r.returncode == 1 and f'no alignments found in "{paths[0]}"' in tail(r)


def test_a_record_whose_qname_is_empty(tmp_path):
    """the reference lets the record behind an empty QNAME join its group (alignment.rs:255), whatever its name: the text front applies
    the rule to the interned ids.  Reads of two alignments around the empty names, so that --careful, which drops them, shows every
    group: FASTA, counts and log are the unflagged run's."""
    def build(g, T):
        for i in range(12):
            T.add(g.line(name="" if i in (3, 7, 8) else None, pos=100 + 150 * i, n=60, nm=0))
            if i in (2, 4, 8, 10):      # ... a second alignment of the same read (or of the nameless one) right behind it
                T.add(g.line(name="" if i == 8 else f"r{g.serial - 1}", pos=2000 + 60 * i, n=60, nm=0, flag=256))
        T.add(g.line(name="r5", pos=2800, n=60, nm=0))      # a name seen before, behind others: its own group again
    fasta, paths, _ = small_pair(str(tmp_path), "empty_qname", build)
    for extra in ([], ["--careful"]):
        plain, r = run("polish", *extra, fasta, *paths), run("polish", "--text_chain", *extra, fasta, *paths)
        assert plain.returncode == 0 and r.returncode == 0 and r.stdout == plain.stdout and log_of(r) == log_of(plain), (extra, tail(r))
        reads = re.findall(r"alignments from (\d+) reads", log_of(r))
        assert reads == ["10", "10"], "17 alignments in 10 groups: the nameless records pull their successors in"
    outs = {flag: [str(tmp_path / f"{flag}_{i}.sam") for i in (1, 2)] for flag in ("plain", "chain")}
    r = both_ways(lambda flag: ["filter", *flag, "--in1", paths[0], "--in2", paths[1], "--out1", outs["chain" if flag else "plain"][0],
                                "--out2", outs["chain" if flag else "plain"][1]])
    assert r.returncode == 0, tail(r)
    for f in range(2):
        assert open(outs["chain"][f], "rb").read() == open(outs["plain"][f], "rb").read(), f
    for extra in ([], ["--careful"]):
        plain = run("filter-polish", *extra, "--in1", paths[0], "--in2", paths[1], fasta)
        r = run("filter-polish", "--text_chain", *extra, "--in1", paths[0], "--in2", paths[1], fasta)
        assert plain.returncode == 0 and r.returncode == 0 and r.stdout == plain.stdout and log_of(r) == log_of(plain), (extra, tail(r))


# ---- errors: the exit code, the reference's sentence, the path and the line --------------------------------------------------------

def with_line(d, name, at, make, n=12):
    """a dozen good lines with make(g) in place of record `at`, in file 2 -> (fasta, paths, the 1-based line of it)"""
    def build(g, T):
        for i in range(n):
            T.add(make(g) if (i == at and g.mate) else g.line(pos=100 + 150 * i, n=60, nm=0))
    fasta, paths, _ = small_pair(d, name, build)
    return fasta, paths, at + 2


def test_a_line_without_nm_in_file_2(tmp_path):
    fasta, paths, line = with_line(str(tmp_path), "no_nm", 7, lambda g: g.line(pos=1150, n=60, nm=None))
    r = both_ways(lambda flag: ["polish", *flag, fasta, *paths])
    assert r.returncode == 1 and tail(r).strip() == f'missing NM tag in "{paths[1]}" (line {line})'
    r = run("polish", "--text_chain", "--regroup", fasta, *paths)
    assert r.returncode == 1 and tail(r).strip() == f'missing NM tag in "{paths[1]}" (line {line})'
    r = run("filter-polish", "--text_chain", "--in1", paths[0], "--in2", paths[1], fasta)      # the chain's filter looks at NM
    assert r.returncode == 1 and tail(r).strip() == f'missing NM tag in "{paths[1]}" (line {line})'


def test_a_negative_nm_is_the_reference_s_panic(tmp_path):
    fasta, paths, line = with_line(str(tmp_path), "neg_nm", 3, lambda g: g.line(pos=550, n=60, nm=-1))
    r = both_ways(lambda flag: ["polish", *flag, fasta, *paths])
    assert r.returncode == 101 and f'"{paths[1]}" (line {line})' in tail(r)


def test_too_few_columns(tmp_path):
    fasta, paths, line = with_line(str(tmp_path), "few", 9, lambda g: "x\t0\tctg0\t1\t60\t24M")
    r = both_ways(lambda flag: ["polish", *flag, fasta, *paths])
    assert r.returncode == 1 and tail(r).strip() == f'too few columns in "{paths[1]}" (line {line})'
    r = both_ways(lambda flag: ["filter", *flag, "--in1", paths[0], "--in2", paths[1], "--out1", tmp_path / "o1", "--out2", tmp_path / "o2"])
    assert r.returncode == 1 and tail(r).strip() == f'too few columns in "{paths[1]}" (line {line})' and not (tmp_path / "o1").exists()


def test_an_rname_the_assembly_lacks(tmp_path):
    fasta, paths, line = with_line(str(tmp_path), "rname", 4, lambda g: g.line(pos=700, n=60, nm=0, rname="elsewhere"))
    plain, r = run("polish", fasta, *paths), run("polish", "--text_chain", fasta, *paths)
    assert plain.returncode == 1 and "query name elsewhere in SAM but not in assembly" in tail(plain)
    assert r.returncode == 1 and r.stdout == b"", tail(r)
    assert tail(r).strip() == f'query name elsewhere in SAM but not in assembly: "{paths[1]}" (line {line})'


def test_a_group_of_star_records_in_front_of_a_malformed_line(tmp_path):
    """the reference streams: the group's error comes first; under --regroup the decode's refusal is reported at once"""
    def build(g, T):
        for i in range(12):
            if i == 3:
                T.add(g.line(name="hollow", pos=550, n=60, nm=0, seq="*"))
                T.add(g.line(name="hollow", pos=900, n=60, nm=0, seq="*", flag=256))
            elif i == 9:
                T.add("x\t0\tctg0\t1\t60\t24M")
            else:
                T.add(g.line(pos=100 + 150 * i, n=60, nm=0))
    fasta, paths, _ = small_pair(str(tmp_path), "hollow", build)
    plain = run("polish", fasta, paths[0])
    assert plain.returncode == 1 and tail(plain).strip() == "no alignments for read hollow contain sequence"
    r = run("polish", "--text_chain", fasta, paths[0])
    assert r.returncode == 1 and r.stdout == b"" and tail(r).strip() == f'no alignments for read hollow contain sequence: "{paths[0]}" (line 5)'
    r = run("polish", "--text_chain", "--regroup", fasta, paths[0])
    assert r.returncode == 1 and tail(r).strip() == f'too few columns in "{paths[0]}" (line 12)'


def test_an_empty_line_is_refused_by_filter_and_skipped_by_polish(tmp_path):
    def build(g, T):
        for i in range(12):
            if i == 6 and g.mate:
                T.add("")
            T.add(g.line(pos=100 + 150 * i, n=60, nm=0))
    fasta, paths, _ = small_pair(str(tmp_path), "empty_line", build)
    r = both_ways(lambda flag: ["polish", *flag, fasta, *paths])
    assert r.returncode == 0
    for argv in (["filter", "--in1", paths[0], "--in2", paths[1], "--out1", tmp_path / "o1", "--out2", tmp_path / "o2"],
                 ["filter-polish", "--in1", paths[0], "--in2", paths[1], fasta]):
        r = both_ways(lambda flag: [argv[0], *flag, *argv[1:]])
        assert r.returncode == 1 and r.stdout == b"" and tail(r).strip() == f'too few columns in "{paths[1]}" (line 8)'
    assert not (tmp_path / "o1").exists()


# ---- refusals with the flag on ----------------------------------------------------------------------------------------------------

def test_a_pipe_is_refused_by_name(ds, tmp_path):
    fifo = str(tmp_path / "pipe.sam")
    os.mkfifo(fifo)
    r = run("polish", "--text_chain", ds["fasta"], fifo)
    assert r.returncode == 1 and r.stdout == b"" and fifo in tail(r) and "reads regular files" in tail(r), tail(r)


def test_refusals_by_name(ds, tmp_path):
    r = run("polish", "--text_chain", ds["fasta"], *ds["sams"], env=dict(PP_GPUS="2"))
    assert r.returncode == 1 and r.stdout == b"" and "runs on one GPU" in tail(r) and ds["sams"][0] in tail(r)
    r = run("polish", "--text_chain", ds["fasta"], *ds["sams"], env=dict(PP_SHARE_GPU="2"))
    assert r.returncode == 1 and "runs on one GPU" in tail(r)
    bam = bam_of(open(ds["sams"][1], "rb").read(), ds["contigs"], str(tmp_path / "two.bam"))[0]
    r = run("polish", "--text_chain", ds["fasta"], ds["sams"][0], bam)
    assert r.returncode == 1 and "must all be SAM text or all be BAM" in tail(r) and ds["sams"][0] in tail(r) and bam in tail(r)
    r = run("filter", "--text_chain", "--in1", ds["sams"][0], "--in2", bam, "--out1", tmp_path / "o1", "--out2", tmp_path / "o2")
    assert r.returncode == 1 and "must both be SAM text or both be BAM" in tail(r)
    gz = put(tmp_path / "plain.sam.gz", gzip.compress(open(ds["sams"][0], "rb").read()))
    r = run("polish", "--text_chain", ds["fasta"], gz)
    assert r.returncode == 1 and "is gzip-compressed but not BGZF" in tail(r) and gz in tail(r)


def test_a_byte_outside_ascii(ds, tmp_path):
    text = open(ds["sams"][0], "rb").read()
    at = text.index(b"\n", len(text) // 2)
    odd = put(tmp_path / "odd.sam", text[:at] + b"\tXX:Z:\xc3\xa9" + text[at:])
    plain = run("polish", ds["fasta"], odd, ds["sams"][1])
    r = run("polish", "--text_chain", ds["fasta"], odd, ds["sams"][1], env=dict(PP_TIMING="1"))
    assert plain.returncode == 0 and r.returncode == 0 and r.stdout == plain.stdout == ds["grouped"]["fasta"], tail(r)
    assert "text chain: bytes outside ASCII" in r.stderr.decode() and odd in r.stderr.decode()
    r = run("polish", "--text_chain", "--regroup", ds["fasta"], odd, ds["sams"][1])
    assert r.returncode == 1 and r.stdout == b"" and odd in tail(r) and "outside ASCII" in tail(r)
    zipped = put(tmp_path / "odd.sam.gz", bgzf_file(open(odd, "rb").read(), cut_points(os.path.getsize(odd), set())))
    r = run("polish", "--text_chain", ds["fasta"], zipped, ds["sams"][1])
    assert r.returncode == 1 and zipped in tail(r) and "outside ASCII" in tail(r)
    outs = [[str(tmp_path / f"{k}_{i}.sam") for i in (1, 2)] for k in ("plain", "chain")]
    a = run("filter", "--in1", odd, "--in2", ds["sams"][1], "--out1", outs[0][0], "--out2", outs[0][1])
    b = run("filter", "--text_chain", "--in1", odd, "--in2", ds["sams"][1], "--out1", outs[1][0], "--out2", outs[1][1])
    assert a.returncode == 0 and b.returncode == 0, tail(b)
    for f in range(2):
        assert open(outs[0][f], "rb").read() == open(outs[1][f], "rb").read()
    a = run("filter-polish", "--in1", odd, "--in2", ds["sams"][1], ds["fasta"])
    b = run("filter-polish", "--text_chain", "--in1", odd, "--in2", ds["sams"][1], ds["fasta"])
    assert a.returncode == 0 and b.returncode == 0 and a.stdout == b.stdout and log_of(a) == log_of(b), tail(b)


# ---- grammar, and the Python face ---------------------------------------------------------------------------------------------------

def test_the_flag_takes_no_value_and_stands_in_the_three_helps(ds):
    r = run("polish", "--text_chain=1", ds["fasta"], *ds["sams"])
    assert r.returncode == 2 and b"unexpected value '1' for '--text_chain' found; no more were expected" in r.stderr
    r = run("filter", "--text_chain=1", "--in1", ds["sams"][0], "--in2", ds["sams"][1], "--out1", "x", "--out2", "y")
    assert r.returncode == 2 and b"unexpected value '1' for '--text_chain'" in r.stderr
    for cmd in ("polish", "filter", "filter-polish"):
        out = run(cmd, "--help").stdout
        line = next(ln for ln in out.split(b"\n") if b"--text_chain" in ln)
        assert b"not in the reference" in line, cmd


def test_the_python_face(ds):
    import polypolish_amd as pp
    assert pp.polish(ds["fasta"], ds["sorted_paths"], max_errors=MAX_ERRORS, text_chain=True, regroup=True) == ds["polish"]["fasta"]
    ctx = pp.Context(0)
    try:
        with pytest.raises(pp.PolypolishError) as e:
            ctx.polish_files(ds["fasta"], ds["sorted_paths"], regroup=True)
        assert e.value.code == pp.ERR_QUIT and "--regroup takes BAM input" in e.value.msg
        assert ctx.polish_files(ds["fasta"], ds["sorted_paths"], regroup=True, text_chain=True) == ds["polish"]["fasta"]
        with pytest.raises(pp.PolypolishError):     # the keyword holds for its call alone
            ctx.polish_files(ds["fasta"], ds["sorted_paths"], regroup=True)
        ctx.set_text_chain(True)
        fasta, rep = ctx.filter_polish_files(ds["fasta"], ds["sorted_paths"][0], ds["sorted_paths"][1], regroup=True)
        assert fasta == ds["polish_filtered"] and rep["after"] < rep["before"]
        assert ctx.polish_files(ds["fasta"], ds["sams"]) == ds["grouped"]["fasta"]
        ctx.set_text_chain(False)
        with pytest.raises(pp.PolypolishError):
            ctx.polish_files(ds["fasta"], ds["sorted_paths"], regroup=True)
        # pp_polish_files_multi with the flag on: several contexts are refused by name
        import ctypes as C
        other = pp.Context(0)
        try:
            for c in (ctx, other):
                c.set_text_chain(True)
            hs = (C.c_void_p * 2)(ctx._h, other._h)
            sams = (C.c_char_p * 2)(*[p.encode() for p in ds["sams"]])
            opt, out = pp.PolishOptions(0.2, 0.5, 10, 5, 0, None, 1), pp.Bytes()
            rc = pp.lib().pp_polish_files_multi(hs, 2, ds["fasta"].encode(), sams, 2, C.byref(opt), C.byref(out))
            said = pp.lib().pp_last_error(ctx._h).decode()
            assert rc == pp.ERR_QUIT and "runs on one GPU" in said and ds["sams"][0] in said, said
        finally:
            other.close()
            ctx.set_text_chain(False)
    finally:
        ctx.close()
