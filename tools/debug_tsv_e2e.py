"""`polypolish polish --debug` end to end on SAM text of BASELINE.json configs[N]'s shape: wall time of the command and the
sha256 of its FASTA and TSV, optionally against the oracle's CLI (one core) and against another build of the command
(`--before DIR`: a checkout's bin/polypolish, e.g. the one with the host TSV writer).  Prints one JSON line.

    python tools/debug_tsv_e2e.py --config 1 [--genome 5000000] [--oracle] [--before /path/to/old/checkout]
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _sha(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for b in iter(lambda: f.read(1 << 24), b""):
            h.update(b)
    return h.hexdigest()


def write_config(config, outdir, genome=None, coverage=None, seed=1):
    """FASTA + two SAM files of configs[config]'s shape under outdir (made on the GPU, tools/samgen.c writes the text)."""
    import torch
    import bench
    from synthjob import make_job, write_sam_pair
    lens, cov, repeat, label = bench.config_shape(config, genome, coverage)
    job = make_job(torch.device("cuda"), contig_lens=lens, coverage=cov, seed=seed, pairs=True, unaligned_frac=1e-3, repeat=repeat)
    torch.cuda.synchronize()
    fa, sams = write_sam_pair(job, outdir, qual=True)
    del job
    torch.cuda.empty_cache()
    return fa, sams, label


def run_debug(exe, fa, sams, tsv, env=None, timeout=1800):
    """(wall seconds, completed process, sha256 of the FASTA, sha256 of the TSV)"""
    t0 = time.perf_counter()
    r = subprocess.run([exe, "polish", "--debug", tsv, fa] + list(sams), capture_output=True, env=env, timeout=timeout)
    t = time.perf_counter() - t0
    if r.returncode != 0:
        raise RuntimeError(f"{exe} failed ({r.returncode}): {r.stderr.decode(errors='replace')[-1000:]}")
    return t, r, hashlib.sha256(r.stdout).hexdigest(), _sha(tsv)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=1)
    ap.add_argument("--genome", type=int, default=None)
    ap.add_argument("--coverage", type=int, default=None)
    ap.add_argument("--dir", default=None, help="where the inputs and outputs go (default: a fresh temporary directory)")
    ap.add_argument("--oracle", action="store_true", help="also run the oracle's CLI and compare the hashes")
    ap.add_argument("--before", default=None, help="a checkout whose bin/polypolish is timed on the same files")
    ap.add_argument("--repeat", type=int, default=2)
    a = ap.parse_args()
    d = a.dir or tempfile.mkdtemp(prefix="pp_dbg_", dir=os.environ.get("TMPDIR", "/tmp"))
    os.makedirs(d, exist_ok=True)
    t0 = time.perf_counter()
    fa, sams, label = write_config(a.config, d, a.genome, a.coverage)
    out = {"config": label, "text_bytes": sum(os.path.getsize(s) for s in sams), "generated_s": round(time.perf_counter() - t0, 1)}
    exe = os.path.join(ROOT, "bin", "polypolish")
    tsv = os.path.join(d, "debug.tsv")
    times = []
    for _ in range(a.repeat):
        t, r, fsha, tsha = run_debug(exe, fa, sams, tsv)
        times.append(t)
    out["after"] = {"wall_s": [round(t, 3) for t in times], "fasta_sha256": fsha, "tsv_sha256": tsha, "tsv_bytes": os.path.getsize(tsv)}
    _, r, _, _ = run_debug(exe, fa, sams, tsv, env=dict(os.environ, PP_TIMING="1"))
    out["after"]["stages"] = [l for l in r.stderr.decode(errors="replace").splitlines() if l.startswith("[timing]")]
    if a.before:
        old = os.path.join(a.before, "bin", "polypolish")
        times = []
        for _ in range(a.repeat):
            t, r, ofsha, otsha = run_debug(old, fa, sams, tsv)
            times.append(t)
        out["before"] = {"wall_s": [round(t, 3) for t in times], "fasta_sha256": ofsha, "tsv_sha256": otsha,
                         "same_bytes": ofsha == fsha and otsha == tsha}
    if a.oracle:
        t, r, wfsha, wtsha = run_debug(os.path.join(ROOT, "oracle", "_build", "pp_oracle"), fa, sams, tsv, timeout=3600)
        out["oracle"] = {"wall_s": round(t, 2), "cores": 1, "fasta_sha256": wfsha, "tsv_sha256": wtsha,
                         "parity": wfsha == fsha and wtsha == tsha}
    if not a.dir:
        for p in [fa, tsv] + list(sams):
            os.remove(p)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
