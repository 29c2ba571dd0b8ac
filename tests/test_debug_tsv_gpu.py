"""The --debug TSV formatted on the device (pp_polish_debug_tsv, pp_k_debug.h) on every route `polish` takes: the C ABI
whole and in chunks, the depth's one decimal, the order of a position's items, every ingest route of the CLI, several
contexts in one process, the one-process-per-GPU launcher and a full-size job.  Byte for byte against the oracle's TSV
(oracle/pp_oracle.c, the reference's src/polish.rs:230-266 and src/pileup.rs:137-166).  Needs an MI355X: `-m gpu`."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import synth
from debug_tsv_util import HEADER, _diff, _raw, _write_job

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "polypolish")
OPTION_SETS = (dict(), dict(min_depth=2, fraction_invalid=0.1, max_errors=3), dict(careful=True))


@pytest.fixture(scope="module")
def pp():
    import polypolish_amd
    return polypolish_amd


@pytest.fixture(scope="module")
def ctx(pp):
    c = pp.Context(0)
    yield c
    c.close()


def _device_tsv(pp, ctx, fasta, sams, **kw):
    """ingest on the host, polish with the debug records kept on the device, the TSV through Context.debug_tsv"""
    names, _, off, bases, recs, _ = pp.ingest(fasta, sams, max_errors=kw.get("max_errors", 10), careful=kw.get("careful", False))
    res = ctx.polish_records(off, bases, recs, min_depth=kw.get("min_depth", 5), fraction_valid=kw.get("fraction_valid", 0.5),
                             fraction_invalid=kw.get("fraction_invalid", 0.2), debug=True)
    return names, off, res


# ---- 1. the ABI, whole and chunked ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [dict(seed=31, contig_lens=(4000, 2500), coverage=40),
                                  dict(seed=32, contig_lens=(6000, 1200, 900), coverage=30, repeat_len=400, repeat_copies=3)],
                         ids=["seed31", "seed32"])
def test_abi_whole_and_chunked(pp, ctx, orc, tmp_path, case):
    import torch
    ds = synth.rich_dataset(str(tmp_path), **case)
    sams = [ds["sam1"], ds["sam2"]]
    rng = np.random.default_rng(case["seed"])
    for kw in OPTION_SETS:
        want = orc.polish_files(ds["fasta"], sams, debug=True, **kw)["debug"]
        assert want.startswith(HEADER)
        body = want[len(HEADER):]
        names, off, res = _device_tsv(pp, ctx, ds["fasta"], sams, **kw)
        G = int(off[-1])
        got = ctx.debug_tsv(names)
        assert got == body, (kw, _diff(got, body))
        # the same into device memory
        dev = torch.empty(len(body) + 64, dtype=torch.uint8, device="cuda:0")
        rc, _, n, nxt = _raw(pp, ctx, names, 0, G, len(body) + 64, mem=pp.MEM_DEVICE, out=dev.data_ptr())
        assert rc == 0 and n == len(body) and nxt == G
        assert dev[:n].cpu().numpy().tobytes() == body
        # a tiny room (one to a few lines a call) over random splits of the positions: the same bytes
        lines = body.split(b"\n")[:-1]
        longest = max(len(l) for l in lines) + 1
        cuts = np.unique(np.concatenate([[0, G], rng.integers(0, G, 12)]))
        parts = []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            p = int(lo)
            while p < int(hi):
                cap = int(longest + rng.integers(0, 2 * longest))
                rc, buf, n, nxt = _raw(pp, ctx, names, p, int(hi), cap)
                assert rc == 0 and 0 < n <= cap and p < nxt <= int(hi), (rc, n, cap, p, nxt)
                assert (buf[n:] == 0xEE).all()  # nothing behind the lines written
                parts.append(buf[:n].tobytes())
                p = nxt
        assert b"".join(parts) == body, kw
        # a room below one line: PP_ERR_ARG, nothing written
        first = len(lines[0]) + 1
        rc, buf, n, nxt = _raw(pp, ctx, names, 0, G, first - 1)
        assert rc == pp.ERR_ARG and n == 0 and nxt == 0 and (buf == 0xEE).all()
        rc, buf, n, nxt = _raw(pp, ctx, names, 0, G, first)
        assert rc == 0 and n == first and nxt == 1 and buf[:n].tobytes() == lines[0] + b"\n"


# ---- hand-built jobs ---------------------------------------------------------------------------------------------------
def _check_hand_job(pp, ctx, orc, fa, sam, **kw):
    want = orc.polish_files(fa, [sam], debug=True, **kw)
    body = want["debug"][len(HEADER):]
    names, off, res = _device_tsv(pp, ctx, fa, [sam], **kw)
    got = ctx.debug_tsv(names)
    assert got == body, _diff(got, body)
    return body


def _rand_dna(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


# ---- 2. the depth's one decimal ----------------------------------------------------------------------------------------
def test_depth_is_printed_correctly_rounded(pp, ctx, orc, tmp_path):
    rng = np.random.default_rng(7)
    zone, L = 60, 30
    d = _rand_dna(rng, 6 * zone)
    sink = _rand_dna(rng, 4000)
    alns, q = [], [0]
    sink_at = [0]

    def group(k, zone_idx):  # one read: one record in the zone, k - 1 in the sink
        q[0] += 1
        s = zone_idx * zone + 10
        alns.append((f"r{q[0]}", "d", s, f"{L}M", d[s:s + L]))
        for _ in range(k - 1):
            p = sink_at[0] % (len(sink) - L)
            sink_at[0] += 37
            alns.append((f"r{q[0]}", "sink", p, f"{L}M", sink[p:p + L]))

    group(4, 0)                                   # 0.25 -> "0.2"
    for _ in range(3):
        group(4, 1)                               # 0.75 -> "0.8"
    for _ in range(9):
        group(4, 2)                               # 2.25 -> "2.2"
    for _ in range(1000):
        group(1, 3)
    group(4, 3)                                   # 1000.25 -> "1000.2"
    for k in (3, 5, 3, 6, 7, 5, 7, 7, 5, 7, 6, 3):
        group(k, 4)                               # 1/3, 1/5, 1/6, 1/7 summed in file order
    for _ in range(10001):
        group(1, 5)
    group(3, 5)                                   # above 10,000
    fa, sam = _write_job(str(tmp_path), [("d", d), ("sink", sink)], alns)
    body = _check_hand_job(pp, ctx, orc, fa, sam)
    depths = {l.split(b"\t")[3] for l in body.split(b"\n") if l.startswith(b"d\t")}
    assert {b"0.2", b"0.8", b"2.2", b"1000.2", b"10001.3"} <= depths, sorted(depths)


# ---- 3. the order of a position's items --------------------------------------------------------------------------------
def test_items_sorted_as_whole_strings(pp, ctx, orc, tmp_path):
    rng = np.random.default_rng(11)
    c = list(_rand_dna(rng, 600))
    # anchors: an 'A' at 100 (insertions A/AC/ACG, the byte x), 200 (N, lowercase, x, y), 300 (more than 64 distinct keys),
    # 400 (a multi-byte winner), 460 (a deletion wins), '-' in the assembly at 520 and 540
    for p in (100, 200, 300, 400, 460):
        c[p] = "A"
    c[520] = "-"
    c[540] = "-"
    ref = "".join(c)
    alns, q = [], [0]

    def read(s, cig, seq):
        q[0] += 1
        alns.append((f"r{q[0]}", "ctg", s, cig, seq))

    def ins_read(p, ins, left=15, right=15):  # the read's base at p, then `ins`
        s = p - left + 1
        read(s, f"{left}M{len(ins)}I{right}M", ref[s:p + 1] + ins + ref[p + 1:p + 1 + right])

    def sub_read(p, b, n=30):
        s = p - 12
        read(s, f"{n}M", ref[s:p] + b + ref[p + 1:s + n])

    for ins in ("C", "CG", "C", "x", "CG", "CGT", "x"):
        ins_read(100, ins)
    for _ in range(3):
        sub_read(100, "A")
    s = 100 - 10
    read(s, "10M1D20M", ref[s:100] + ref[101:121])  # a deletion at 100: the key "-"
    for b in ("N", "a", "x", "y", "N", "c", "x", "X", "n"):
        sub_read(200, b)
    for k in (1, 2, 3):
        for i in range(4 ** k):
            ins = "".join("ACGT"[(i >> (2 * j)) & 3] for j in range(k))
            ins_read(300, ins)
    for _ in range(3):
        ins_read(300, "TT")
    for _ in range(12):
        ins_read(400, "GT")                         # "AGT" wins: a multi-byte new_base
    for _ in range(12):
        s = 460 - 10
        read(s, "10M1D20M", ref[s:460] + ref[461:481])  # "-" wins
    for _ in range(8):
        sub_read(520, "C")                          # an assembly '-' polished to C
    fa, sam = _write_job(str(tmp_path), [("ctg", ref)], alns)
    for kw in (dict(), dict(min_depth=2, fraction_invalid=0.1)):
        body = _check_hand_job(pp, ctx, orc, fa, sam, **kw)
    line = {int(l.split(b"\t")[1]): l.split(b"\t") for l in body.split(b"\n") if l}
    assert len(line[300][6].split(b",")) > 64
    assert line[400][8] == b"AGT" and line[460][8] == b"-" and line[520][2] == b"-"


# ---- 4. every ingest route of the CLI ---------------------------------------------------------------------------------
def test_cli_debug_on_every_ingest_route(orc, tmp_path):
    ds = synth.rich_dataset(str(tmp_path), seed=33, contig_lens=(5000,), coverage=50, repeat_len=300, repeat_copies=5,
                            inverted=False, n_rate=0.01)
    sams = [ds["sam1"], ds["sam2"]]
    want = orc.polish_files(ds["fasta"], sams, debug=True)
    tsv = str(tmp_path / "d.tsv")
    for env in (dict(PP_TIMING="1"), dict(PP_DEVICE_INGEST="0"), dict(PP_SEQ_LAYOUT="window"), dict(PP_SEQ_LAYOUT="file"),
                dict(PP_SEQ4="0")):
        if os.path.exists(tsv):
            os.remove(tsv)
        r = subprocess.run([EXE, "polish", "--debug", tsv, ds["fasta"], *sams], capture_output=True,
                           env=dict(os.environ, **env), timeout=300)
        assert r.returncode == 0, (env, r.stderr.decode()[-2000:])
        assert r.stdout == want["fasta"], env
        got = open(tsv, "rb").read()
        assert got == want["debug"], (env, _diff(got, want["debug"]))
        if "PP_TIMING" in env:  # the default run went through the device tokenizer
            assert b"[timing] device ready, tokenizer created" in r.stderr, r.stderr.decode()[-2000:]


# ---- 5. several contexts in one process --------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ctx", [2, 3])
def test_debug_on_several_contexts_in_one_process(orc, tmp_path, n_ctx):
    ds = synth.rich_dataset(str(tmp_path), seed=83, contig_lens=(140_000, 900, 2_000, 30_000), coverage=12, repeat_len=300,
                            repeat_copies=3)
    sams = [ds["sam1"], ds["sam2"]]
    want = orc.polish_files(ds["fasta"], sams, debug=True)
    tsv = str(tmp_path / "d.tsv")
    for ingest in ("1", "0"):
        r = subprocess.run([EXE, "polish", "--debug", tsv, ds["fasta"], *sams], capture_output=True, timeout=600,
                           env=dict(os.environ, PP_SHARE_GPU=str(n_ctx), PP_DEVICE_INGEST=ingest, PP_TIMING="1"))
        assert r.returncode == 0, (ingest, r.stderr.decode()[-2000:])
        assert b"[timing] uploaded + polished on the devices" in r.stderr, ingest
        assert r.stdout == want["fasta"], ingest
        got = open(tsv, "rb").read()
        assert got == want["debug"], (ingest, _diff(got, want["debug"]))
    # filter-polish --debug (the fused command) under the same environment
    o1, o2 = str(tmp_path / "o1.sam"), str(tmp_path / "o2.sam")
    orc.filter_files(ds["sam1"], ds["sam2"], o1, o2)
    want = orc.polish_files(ds["fasta"], [o1, o2], debug=True)
    r = subprocess.run([EXE, "filter-polish", "--in1", ds["sam1"], "--in2", ds["sam2"], "--debug", tsv, ds["fasta"]],
                       capture_output=True, timeout=600, env=dict(os.environ, PP_SHARE_GPU=str(n_ctx)))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert r.stdout == want["fasta"]
    got = open(tsv, "rb").read()
    assert got == want["debug"], _diff(got, want["debug"])


def test_debug_file_that_cannot_be_created_on_several_contexts(tmp_path):
    """create_debug_file (polish.rs:230-245) fails after the alignments are loaded: with two contexts the command leaves
    then with the tokenizers of both still alive -- the reference's message, exit code 1, nothing on stdout."""
    ds = synth.rich_dataset(str(tmp_path), seed=84, contig_lens=(30_000, 900), coverage=12, repeat_len=300, repeat_copies=3)
    bad = str(tmp_path / "no" / "such" / "dir.tsv")
    for ingest in ("1", "0"):
        r = subprocess.run([EXE, "polish", "--debug", bad, ds["fasta"], ds["sam1"], ds["sam2"]], capture_output=True,
                           timeout=300, env=dict(os.environ, PP_SHARE_GPU="2", PP_DEVICE_INGEST=ingest))
        assert r.returncode == 1 and r.stdout == b"", (ingest, r.stderr.decode()[-2000:])
        assert f'unable to create "{bad}"'.encode() in r.stderr, (ingest, r.stderr.decode()[-2000:])


# ---- 6. the one-process-per-GPU launcher -------------------------------------------------------------------------------
def test_debug_through_the_distributed_launcher(orc, tmp_path):
    ds = synth.rich_dataset(str(tmp_path), seed=81, contig_lens=(140_000, 900, 2_000), coverage=12, repeat_len=300,
                            repeat_copies=3)
    sams = [ds["sam1"], ds["sam2"]]
    want = orc.polish_files(ds["fasta"], sams, debug=True)
    tsv = str(tmp_path / "d.tsv")
    env = dict(os.environ, PP_SHARE_GPU="1", PYTHONPATH=ROOT)
    port = 37000 + os.getpid() % 2000
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                        "127.0.0.1", "--master-port", str(port), "-m", "polypolish_amd.distributed", "polish", "--debug", tsv,
                        ds["fasta"], *sams], capture_output=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert r.stdout == want["fasta"]
    got = open(tsv, "rb").read()
    assert got == want["debug"], _diff(got, want["debug"])
    # a file that cannot be created: the reference's error, from rank 0
    bad = str(tmp_path / "no" / "such" / "dir.tsv")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                        "127.0.0.1", "--master-port", str(port + 1), "-m", "polypolish_amd.distributed", "polish", "--debug", bad,
                        ds["fasta"], *sams], capture_output=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode != 0 and f'unable to create "{bad}"'.encode() in r.stderr


# ---- 7. full size ------------------------------------------------------------------------------------------------------
def test_full_size_config1_from_sam_text(orc, tmp_path):
    """configs[1] (5 Mbp, 200x) as SAM text: the TSV's sha256 is the oracle's."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import debug_tsv_e2e as e2e
    fa, sams, _ = e2e.write_config(1, str(tmp_path))
    tsv = str(tmp_path / "d.tsv")
    _, _, fsha, tsha = e2e.run_debug(EXE, fa, sams, tsv, timeout=600)
    _, _, wfsha, wtsha = e2e.run_debug(os.path.join(ROOT, "oracle", "_build", "pp_oracle"), fa, sams, tsv, timeout=1500)
    assert (fsha, tsha) == (wfsha, wtsha)
