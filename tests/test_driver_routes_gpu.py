"""The command drivers' input routes, pinned: every route a `polish`, `filter` or `filter-polish` command can take through
pp_driver*.cpp and pp_filter_host.cpp gives the oracle's bytes and -- word for word -- the stderr log of its command's default
route.  One tiny job (two contigs, one with a description in its FASTA header; two SAM files of a few hundred records with unaligned
records, reads with several alignments, reads with indels and ZP:Z:fail records), the same records as a BGZF BAM pair and as an
uncompressed BAM pair.  Every case runs bin/polypolish as a child process in a directory of its own, where the inputs carry the same
relative names whatever their kind (a file's kind is told by its head): the logs are compared as they are, less the `Time to run:`
line and the `[timing]` lines.  The orders of errors are pinned by test_gpu_parity.py and test_bam_cli_gpu.py.  Needs an MI355X:
`-m gpu`."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import bam_model as bm
import bam_tag_model as tm
import bgzf_deflate_model as D
from test_bgzf_chain_gpu import bgzf_file, cut_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "polypolish")
ORC_EXE = os.path.join(ROOT, "oracle", "_build", "pp_oracle")
pytestmark = pytest.mark.gpu

INPUTS = ("asm.fasta", "reads_1", "reads_2")
COMMANDS = {
    "polish": ["polish", *INPUTS],
    "polish-debug": ["polish", "--debug", "debug.tsv", *INPUTS],
    "filter": ["filter", "--in1", "reads_1", "--in2", "reads_2", "--out1", "out_1", "--out2", "out_2"],
    "fused-outputs": ["filter-polish", "--in1", "reads_1", "--in2", "reads_2", "--out1", "out_1", "--out2", "out_2", "asm.fasta"],
    "fused": ["filter-polish", "--in1", "reads_1", "--in2", "reads_2", "asm.fasta"],
}
# (command, the inputs' kind, environment); the default route of a command is its first case: SAM text, nothing set
ROUTES = [
    ("polish", "sam", {}),
    ("polish", "sam", {"PP_DEVICE_INGEST": "0"}),
    ("polish", "sam", {"PP_DEVICE_INGEST": "0", "PP_STREAM_ADDS": "0"}),
    ("polish", "sam", {"PP_SHARE_GPU": "3"}),
    ("polish", "sam", {"PP_SHARE_GPU": "3", "PP_DEVICE_INGEST": "0"}),
    ("polish", "bgzf", {}),
    ("polish", "raw", {}),
    ("polish", "bgzf", {"PP_BAM_PREPARE": "1"}),
    ("polish-debug", "sam", {}),
    ("polish-debug", "sam", {"PP_SHARE_GPU": "3"}),
    ("polish-debug", "bgzf", {}),
    ("filter", "sam", {}),
    ("filter", "bgzf", {}),
    ("fused-outputs", "sam", {}),
    ("fused", "sam", {}),
    ("fused-outputs", "bgzf", {}),
    ("fused", "bgzf", {}),
    # SAM text that the device tokenizer hands back to the host ingest at the second file: a QNAME there has one character outside
    # ASCII ("é"; a lone byte of 0x80 and more is not UTF-8, and the reference refuses such a file)
    ("polish", "handed-back", {}),
]


def put(path, data):
    with open(path, "wb") as f:
        f.write(data)


@pytest.fixture(scope="module")
def job(tmp_path_factory, orc):
    import synth
    d = str(tmp_path_factory.mktemp("driver_routes"))
    s = synth.rich_dataset(d, seed=29, contig_lens=(4000, 2500), coverage=12, repeat_len=400, repeat_copies=3, zp_frac=0.03)
    sams = [s["sam1"], s["sam2"]]
    texts = [open(p, "rb").read() for p in sams]
    records = [[l.split(b"\t") for l in t.splitlines() if not l.startswith(b"@")] for t in texts]
    for recs in records:
        assert 200 < len(recs) < 1000
        assert any(int(r[1]) & 4 for r in recs), "an unaligned record"
        assert any(int(r[1]) & 256 for r in recs), "a read with several alignments"
        assert any(b"I" in r[5] or b"D" in r[5] for r in recs), "a read with an indel"
        assert any(b"ZP:Z:fail" in r for r in recs), "a ZP:Z:fail record"
    assert open(s["fasta"]).readline().strip() == ">contig_1 some description"
    contigs = [(c.name, c.assembly) for c in s["contigs"]]
    header_order = [name for name, _ in contigs][::-1]
    lens = [len(dict(contigs)[n]) for n in header_order]
    filtered = [os.path.join(d, f"oracle_filtered_{i}.sam") for i in (1, 2)]
    orc.filter_files(sams[0], sams[1], filtered[0], filtered[1])
    kinds = {k: os.path.join(d, k) for k in ("sam", "bgzf", "raw", "handed-back")}
    for p in kinds.values():
        os.mkdir(p)
        shutil.copy(s["fasta"], os.path.join(p, "asm.fasta"))
    want_bam = []
    for f, text in enumerate(texts):
        name = f"reads_{f + 1}"
        put(os.path.join(kinds["sam"], name), text)
        enc = bm.encode(text, header_order, lens)
        data = enc["header"] + enc["records"]
        at = len(enc["header"])
        starts = set((enc["rec_off"] + np.uint64(at)).tolist())
        cuts = cut_points(len(data), starts)
        assert len(cuts) > 8 and not set(cuts[1:]) & starts, "records straddle the blocks"
        put(os.path.join(kinds["bgzf"], name), bgzf_file(data, cuts))
        put(os.path.join(kinds["raw"], name), data)
        verdict = tm.own_verdicts(text, open(filtered[f], "rb").read())
        assert (verdict == 0).any()
        want_bam.append(D.deflate_file(tm.tagged(data, at, enc["rec_off"] + np.uint64(at), verdict))[0])
    # the same records, one read of the second file under a name outside ASCII: the groups, and with them every count, stay
    qname = next(r[0] for r in records[1][len(records[1]) // 2:] if not int(r[1]) & 4)
    renamed = b"".join((b"caf\xc3\xa9" + l[len(qname):] if l.startswith(qname + b"\t") else l) for l in texts[1].splitlines(True))
    assert renamed != texts[1]
    put(os.path.join(kinds["handed-back"], "reads_1"), texts[0])
    put(os.path.join(kinds["handed-back"], "reads_2"), renamed)
    tsv = os.path.join(d, "oracle_debug.tsv")
    r = subprocess.run([ORC_EXE, "polish", "--debug", tsv, s["fasta"], *sams], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-600:]
    fused = subprocess.run([ORC_EXE, "polish", s["fasta"], *filtered], capture_output=True, timeout=120)
    assert fused.returncode == 0, fused.stderr.decode()[-600:]
    return {"dir": d, "kinds": kinds, "fasta": r.stdout, "debug": open(tsv, "rb").read(), "fasta_filtered": fused.stdout,
            "filtered_sam": [open(p, "rb").read() for p in filtered], "filtered_bam": want_bam, "ran": {}}


def log_of(stderr):
    return [l for l in stderr.decode().splitlines() if not l.startswith("Time to run:") and not l.startswith("[timing]")]


def run_route(job, command, kind, env):
    """the command on the inputs of `kind`, in a fresh directory (once per route: the default routes are every other's yardstick)"""
    key = (command, kind, tuple(sorted(env.items())))
    if key not in job["ran"]:
        cwd = os.path.join(job["dir"], f"case_{len(job['ran'])}")
        shutil.copytree(job["kinds"][kind], cwd)
        r = subprocess.run([EXE, *COMMANDS[command]], cwd=cwd, capture_output=True, env=dict(os.environ, **env), timeout=120)
        if r.returncode < 0 or r.returncode in (134, 139) or b"illegal memory access" in r.stderr:  # a crash is a finding: nothing more is started on the device
            pytest.exit(f"polypolish {command} ({kind}, {env}) ended with {r.returncode}: {r.stderr.decode()[-600:]}", returncode=3)
        job["ran"][key] = (r, cwd)
    return job["ran"][key]


@pytest.mark.parametrize("command, kind, env", ROUTES, ids=[f"{c}-{k}" + "".join(f"-{n}={v}" for n, v in e.items()) for c, k, e in ROUTES])
def test_route_gives_the_oracle_s_bytes_and_the_default_route_s_log(job, command, kind, env):
    r, cwd = run_route(job, command, kind, env)
    log = r.stderr.decode()
    assert r.returncode == 0, log[-800:]
    if command in ("polish", "polish-debug"):
        assert r.stdout == job["fasta"]
    elif command == "filter":
        assert r.stdout == b""
    else:
        assert r.stdout == job["fasta_filtered"]
    if command == "polish-debug":
        assert open(os.path.join(cwd, "debug.tsv"), "rb").read() == job["debug"]
    if command in ("filter", "fused-outputs"):
        want = job["filtered_sam"] if kind == "sam" else job["filtered_bam"]
        for f in range(2):
            assert open(os.path.join(cwd, f"out_{f + 1}"), "rb").read() == want[f], f
    else:
        assert not os.path.exists(os.path.join(cwd, "out_1")) and not os.path.exists(os.path.join(cwd, "out_2"))
    default, _ = run_route(job, command, "sam", {})
    assert default.returncode == 0
    assert log_of(r.stderr) == log_of(default.stderr)
    if kind == "handed-back":  # the host ingest's second look resumes the log where the first one stopped
        for line in ("Loading assembly", "Loading alignments", "Polishing assembly sequences", "Finished!"):
            assert log.count(line + "\n") == 1, line
        for name in INPUTS[1:]:
            assert log.count(f"{name}: ") == 1, name
