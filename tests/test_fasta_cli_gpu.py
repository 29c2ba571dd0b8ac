"""`polypolish polish` and `filter-polish` with PP_DEVICE_FASTA=1 (the assembly through pp_assembly_load_device: pp_fasta_records on the
mapped file, or on the bytes pp_bgzf_inflate made of a BGZF file) against the same commands without it and against the oracle: stdout,
the --debug file, the exit code, and for every refusal of the loader stderr byte for byte.  The assembly comes wrapped with LF and with
CRLF, on one line per contig, as BGZF (written with the tests' own BGZF model, blocks cut every 4,093 bytes, a stored, a Z_FIXED and a
mid-file EOF block among them) and as plain gzip, which stays with the host loader.  One run takes BAM input: its RNAME table is seeded
from the assembly.  pp_assembly_load_device itself is held against pp_assembly_load on every form.  Every command runs bin/polypolish
as a child process.  Needs an MI355X: `-m gpu`."""
import ctypes as C
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import bam_model as bm
import fasta_model as fm
from test_bgzf_chain_gpu import MAX_ERRORS, bgzf_file, cut_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "polypolish")
pytestmark = pytest.mark.gpu
ON = dict(PP_DEVICE_FASTA="1")
FORMS = ["lf60", "crlf70", "one_line", "bgzf", "gzip"]


def run(*argv, env=None):
    base = {k: v for k, v in os.environ.items() if k != "PP_DEVICE_FASTA"}
    r = subprocess.run([EXE, *map(str, argv)], capture_output=True, env=dict(base, **(env or {})), timeout=300)
    if r.returncode < 0 or r.returncode in (134, 139) or b"illegal memory access" in r.stderr:  # a crash is a finding: nothing more is started on the device
        pytest.exit(f"polypolish {' '.join(map(str, argv))} ended with {r.returncode}: {r.stderr.decode()[-600:]}", returncode=3)
    return r


def put(path, data):
    with open(path, "wb") as f:
        f.write(data)
    return str(path)


def log_of(r):
    """stderr without what differs from run to run: the durations"""
    return re.sub(rb"(Time to run: )[^\n]*", rb"\1-", r.stderr)


def wrapped(records, width, end):
    out = []
    for head, seq in records:
        out.append(head + end)
        out += [seq[i:i + width] + end for i in range(0, len(seq), width)] if width else [seq + end]
    return b"".join(out)


def bgzf(data):
    return bgzf_file(data, cut_points(len(data), set()))


@pytest.fixture(scope="module")
def ds(tmp_path_factory, orc):
    import synth
    d = str(tmp_path_factory.mktemp("fasta_cli"))
    s = synth.rich_dataset(d, seed=23, contig_lens=(4000, 2500), coverage=30, repeat_len=400, repeat_copies=3, zp_frac=0.02)
    text = open(s["fasta"], "rb").read()
    names, descs, off, b = fm.parse(text)
    records = [(b">" + n + (b" " + dsc if dsc else b""), b[off[i]:off[i + 1]].lower() if i % 2 else b[off[i]:off[i + 1]])
               for i, (n, dsc) in enumerate(zip(names, descs))]
    assert fm.parse(wrapped(records, 60, b"\n")) == (names, descs, off, b)
    lf = wrapped(records, 60, b"\n")
    forms = {"lf60": put(os.path.join(d, "lf60.fasta"), lf),
             "crlf70": put(os.path.join(d, "crlf70.fasta"), wrapped(records, 70, b"\r\n")),
             "one_line": put(os.path.join(d, "one_line.fasta"), wrapped(records, 0, b"\n")[:-1]),  # no final newline
             "bgzf": put(os.path.join(d, "bgzf.fasta.gz"), bgzf(lf)),
             "gzip": put(os.path.join(d, "plain.fasta.gz"), gzip.compress(lf))}
    assert gzip.decompress(open(forms["bgzf"], "rb").read()) == lf
    sams = [s["sam1"], s["sam2"]]
    outs = [os.path.join(d, f"oracle_filtered_{i}.sam") for i in (1, 2)]
    orc.filter_files(sams[0], sams[1], outs[0], outs[1])
    # the BAM pair of the chain tests: header in REVERSE FASTA order, records that straddle the blocks
    order = [n.decode() for n in names][::-1]
    lens = [off[i + 1] - off[i] for i in range(len(names))][::-1]
    bams = []
    for f, path in enumerate(sams):
        enc = bm.encode(open(path, "rb").read(), order, lens)
        data = enc["header"] + enc["records"]
        starts = set((enc["rec_off"] + np.uint64(len(enc["header"]))).tolist())
        bams.append(put(os.path.join(d, f"reads_{f + 1}.bam"), bgzf_file(data, cut_points(len(data), starts))))
    return {"dir": d, "forms": forms, "sams": sams, "bams": bams, "parsed": (names, descs, off, b),
            "polish": orc.polish_files(s["fasta"], sams, max_errors=MAX_ERRORS, debug=True),
            "polish_filtered": orc.polish_files(s["fasta"], outs, max_errors=MAX_ERRORS)["fasta"]}


@pytest.mark.parametrize("form", FORMS)
def test_polish_is_the_same_with_and_without_the_switch(ds, orc, tmp_path, form):
    fa = ds["forms"][form]
    assert orc.polish_files(fa, ds["sams"], max_errors=MAX_ERRORS)["fasta"] == ds["polish"]["fasta"], "the oracle on this form of the assembly"
    got = []
    for tag, env in (("off", None), ("on", ON)):
        tsv = str(tmp_path / f"debug_{tag}.tsv")
        r = run("polish", "--debug", tsv, fa, *ds["sams"], env=env)
        assert r.returncode == 0 and r.stdout == ds["polish"]["fasta"], (tag, r.stderr.decode()[-800:])
        assert open(tsv, "rb").read() == ds["polish"]["debug"], tag
        got.append(log_of(r).replace(tsv.encode(), b"TSV"))
    assert got[0] == got[1], "stderr differs"


@pytest.mark.parametrize("form", FORMS)
def test_filter_polish_is_the_same_with_and_without_the_switch(ds, form):
    fa = ds["forms"][form]
    got = []
    for tag, env in (("off", None), ("on", ON)):
        r = run("filter-polish", "--in1", ds["sams"][0], "--in2", ds["sams"][1], fa, env=env)
        assert r.returncode == 0 and r.stdout == ds["polish_filtered"], (tag, r.stderr.decode()[-800:])
        got.append(log_of(r))
    assert got[0] == got[1], "stderr differs"


@pytest.mark.parametrize("form", ["crlf70", "bgzf"])
def test_bam_input_seeds_its_rname_table_from_the_device_assembly(ds, form):
    fa = ds["forms"][form]
    got = []
    for tag, env in (("off", None), ("on", ON)):
        r = run("filter-polish", "--in1", ds["bams"][0], "--in2", ds["bams"][1], fa, env=env)
        assert r.returncode == 0 and r.stdout == ds["polish_filtered"], (tag, r.stderr.decode()[-800:])
        got.append(log_of(r))
        r = run("polish", fa, *ds["bams"], env=env)
        assert r.returncode == 0 and r.stdout == ds["polish"]["fasta"], (tag, r.stderr.decode()[-800:])
        got.append(log_of(r))
    assert got[:2] == got[2:], "stderr differs"


def damaged(data, at=40):
    return data[:at] + bytes([data[at] ^ 0x55]) + data[at + 1:]


REFUSALS = {
    "not_formatted": (fm.CASES["r_no_header_after_empty"], 1, fm.NOT_FORMATTED),
    "bases_behind_unnamed": (fm.CASES["r_bases_behind_unnamed"], 1, fm.NOT_FORMATTED),
    "header_not_utf8": (fm.CASES["r_header_truncated_utf8"], 1, fm.UNABLE),
    "sequence_not_utf8": (fm.CASES["r_sequence_not_utf8"], 1, fm.UNABLE),
    "non_ascii": (fm.CASES["r_sequence_non_ascii"], 5, fm.NOT_ASCII),
    "no_sequences": (fm.CASES["r_only_unnamed"], 1, fm.NO_SEQUENCES),
    "empty_sequence": (fm.CASES["r_empty_sequence_last"], 1, fm.EMPTY_SEQUENCE),
    "duplicated": (fm.CASES["r_duplicate"], 1, fm.DUPLICATED),
    "too_small": (b">", 1, "is too small"),
    "bgzf_duplicated": (bgzf(fm.CASES["r_duplicate"]), 1, fm.DUPLICATED),
    "bgzf_not_formatted": (bgzf(b">a\nAC\n" * 1 + b"\n" * 9000 + b">\nAC\n"), 1, fm.NOT_FORMATTED),
    "bgzf_damaged": (damaged(bgzf(b">a\n" + b"ACGT" * 3000 + b"\n")), 1, fm.UNABLE),  # a chain that walks, a block that does not inflate
    "gzip_duplicated": (gzip.compress(fm.CASES["r_duplicate"]), 1, fm.DUPLICATED),
}


@pytest.mark.parametrize("name", sorted(REFUSALS) + ["missing"])
def test_every_refusal_of_the_loader_reads_the_same(ds, tmp_path, name):
    if name == "missing":
        fa, words = str(tmp_path / "no_such.fasta"), "unable to open"
    else:
        data, _, words = REFUSALS[name]
        fa = put(tmp_path / "bad.fasta", data)
    for command in (("polish", fa, ds["sams"][0]), ("filter-polish", "--in1", ds["bams"][0], "--in2", ds["bams"][1], fa)):
        off, on = run(*command), run(*command, env=ON)
        assert (on.returncode, on.stdout, on.stderr) == (off.returncode, off.stdout, off.stderr), command[0]
        # (a path that is not there: `polish` looks for its inputs before any loader runs, check_inputs_exist of the reference, and
        # says so in its own words; the fused command on BAM input meets it in the loader)
        want = "file does not exist" if name == "missing" and command[0] == "polish" else words
        assert off.returncode != 0 and off.stdout == b"" and want.encode() in off.stderr and fa.encode() in off.stderr, off.stderr.decode()[-600:]


# ---- pp_assembly_load_device against pp_assembly_load, in this process ------------------------------------------------------------
@pytest.fixture(scope="module")
def pp():
    import polypolish_amd
    return polypolish_amd


@pytest.fixture(scope="module")
def ctx(pp):
    c = pp.Context(0)
    yield c
    c.close()


def loaded(pp, ctx, path, device):
    """(code, message) or (names, descriptions, offsets, bases through pp_assembly_bases, has device bases)"""
    L = pp.lib()
    a, err = C.c_void_p(), C.create_string_buffer(1024)
    rc = L.pp_assembly_load_device(ctx._h, path.encode(), C.byref(a), err, 1024) if device else L.pp_assembly_load(path.encode(), C.byref(a), err, 1024)
    if rc:
        return rc, err.value
    try:
        n = L.pp_assembly_n_contigs(a)
        off = [int(L.pp_assembly_offsets(a)[i]) for i in range(n + 1)]
        dev = L.pp_assembly_bases_device(a)
        on_dev = ctx.download(dev, off[-1], np.uint8).tobytes() if dev else None
        host = C.string_at(L.pp_assembly_bases(a), off[-1])  # (a device assembly: downloaded on this first use)
        assert on_dev is None or on_dev == host
        assert C.string_at(L.pp_assembly_bases(a), off[-1]) == host
        return [L.pp_assembly_name(a, i) for i in range(n)], [L.pp_assembly_description(a, i) for i in range(n)], off, host, bool(dev)
    finally:
        L.pp_assembly_free(a)


@pytest.mark.parametrize("form", FORMS)
def test_assembly_load_device_makes_the_same_assembly(pp, ctx, ds, form):
    names, descs, off, b = ds["parsed"]
    host, dev = loaded(pp, ctx, ds["forms"][form], False), loaded(pp, ctx, ds["forms"][form], True)
    assert host == (names, descs, off, b, False)
    assert dev == (names, descs, off, b, form != "gzip"), "plain gzip stays with the host loader"


@pytest.mark.parametrize("name", sorted(REFUSALS) + ["missing"])
def test_assembly_load_device_refuses_in_the_host_loaders_words(pp, ctx, tmp_path, name):
    fa = str(tmp_path / "no_such.fasta") if name == "missing" else put(tmp_path / "bad.fasta", REFUSALS[name][0])
    host, dev = loaded(pp, ctx, fa, False), loaded(pp, ctx, fa, True)
    assert len(host) == 2 and dev == host
    if name != "missing":
        assert host[0] == REFUSALS[name][1] and REFUSALS[name][2].encode() in host[1]
