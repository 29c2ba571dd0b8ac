#!/usr/bin/env python3
"""What the commands cost END TO END with --text_chain, next to the same build's commands without it, on configs[1]'s SAM pair
(tools/synthjob.py, make_job(pairs=True); every record, QUAL included: the recipe of tools/sam_bam_timing.py) -- plain, and bgzipped
(level 6, blocks of 0xff00 bytes, as bgzip writes them; only --text_chain reads those).  bin/polypolish runs as a child process on files
in a warm page cache, outputs under --tmp (tmpfs by default): per command one warm-up run of each variant, then --runs rounds in which
the variants ALTERNATE.  Prints one JSON line and writes it to profiles/text_chain_timing.json (--out); per command (polish, filter,
filter_polish, filter_out_bam) and per variant (fused = without the flag, chain = with it, chain_bgzf = with it on the bgzipped pair):
  wall_s         every run's wall seconds (process start to exit), and their median
  laps           the PP_TIMING lines of one more run: seconds since the driver was entered, per stage
  same           polish, filter_polish: the FASTA is the fused run's (sha256); filter: the outputs are the fused run's bytes (chain), or
                 inflate to them (chain_bgzf); filter_out_bam: the BAM files are the fused run's bytes
Measurement only: no threshold is attached to any of it, and no default depends on it."""
import argparse
import gzip
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
EXE = os.path.join(ROOT, "bin", "polypolish")


def log(msg):
    print(f"[text_chain_timing] {msg}", file=sys.stderr, flush=True)


def timed(argv, stdout_path, timing=False):
    """one run of the CLI: (wall seconds, the PP_TIMING laps); the FASTA goes to stdout_path"""
    env = dict(os.environ, **({"PP_TIMING": "1"} if timing else {}))
    with open(stdout_path, "wb") as out:
        t0 = time.perf_counter()
        r = subprocess.run([EXE, *argv], stdout=out, stderr=subprocess.PIPE, env=env)
        dt = time.perf_counter() - t0
    if r.returncode != 0:
        raise RuntimeError(f"polypolish {' '.join(argv)} ended with {r.returncode}: {r.stderr.decode()[-800:]}")
    laps = [[re.sub(r"\s*\(process$", "", m.group(1).strip()), float(m.group(2))]
            for m in re.finditer(r"^\[timing\] (.*?)\s+([0-9.]+) s", r.stderr.decode(), re.M)]
    return dt, laps


def sha(path, inflate=False):
    data = open(path, "rb").read()
    return hashlib.sha256(gzip.decompress(data) if inflate else data).hexdigest()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mbp", type=float, default=5.0, help="assembly size (configs[1]: 5)")
    ap.add_argument("--coverage", type=int, default=200)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--tmp", default="/dev/shm" if os.path.isdir("/dev/shm") else None, help="where the files go (a directory made there is removed afterwards)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "text_chain_timing.json"))
    a = ap.parse_args()
    import torch

    import bgzf_timing
    import synthjob
    tmp = tempfile.mkdtemp(prefix="text_chain_timing_", dir=a.tmp)
    try:
        job = synthjob.make_job(torch.device("cuda:0"), contig_lens=(int(a.mbp * 1e6),), coverage=a.coverage, seed=a.seed, pairs=True,
                                unaligned_frac=1e-3)
        torch.cuda.synchronize()
        n_rec = job["sam"]["n"]
        fasta, sams = synthjob.write_sam_pair(job, tmp, qual=True)
        del job
        torch.cuda.empty_cache()  # (the child processes are the only users of the device from here on)
        zipped = []
        for f, p in enumerate(sams):
            z, _, _ = bgzf_timing.compress(np.fromfile(p, np.uint8), 6)
            zipped.append(os.path.join(tmp, f"reads_{f + 1}.sam.gz"))
            z.tofile(zipped[-1])
            log(f"{p}: {os.path.getsize(p)} bytes of text, {len(z)} bgzipped")
        size = os.path.getsize
        out = {"input": f"{a.mbp:g} Mbp x {a.coverage}, {n_rec} records in two files (seed {a.seed}); bgzipped: level 6, blocks of 0xff00 bytes",
               "runs": a.runs, "file_bytes": {"sam": [size(p) for p in sams], "sam_bgzf": [size(p) for p in zipped]}}
        variants = {"fused": ([], sams), "chain": (["--text_chain"], sams), "chain_bgzf": (["--text_chain"], zipped)}
        outs = {v: [os.path.join(tmp, f"{v}_filtered_{i}") for i in (1, 2)] for v in variants}
        commands = {
            "polish": lambda flag, ins, o: ["polish", *flag, fasta, *ins],
            "filter": lambda flag, ins, o: ["filter", *flag, "--in1", ins[0], "--in2", ins[1], "--out1", o[0], "--out2", o[1]],
            "filter_polish": lambda flag, ins, o: ["filter-polish", *flag, "--in1", ins[0], "--in2", ins[1], fasta],
            "filter_out_bam": lambda flag, ins, o: ["filter", "--out_bam", *flag, "--in1", ins[0], "--in2", ins[1], "--out1", o[0], "--out2", o[1]],
        }
        for cmd, argv_of in commands.items():
            names = [v for v in variants if not (cmd == "filter_out_bam" and v == "chain_bgzf")]
            res = {v: {"wall_s": []} for v in names}
            stdout = {v: os.path.join(tmp, f"{cmd}_{v}.stdout") for v in names}
            for v in names:  # warm-up
                timed(argv_of(*variants[v], outs[v]), stdout[v])
            for _ in range(a.runs):  # the variants alternate
                for v in names:
                    res[v]["wall_s"].append(round(timed(argv_of(*variants[v], outs[v]), stdout[v])[0], 3))
            for v in names:
                res[v]["median_s"] = sorted(res[v]["wall_s"])[len(res[v]["wall_s"]) // 2]
                res[v]["laps"] = [[what.replace(tmp + os.sep, ""), s] for what, s in timed(argv_of(*variants[v], outs[v]), stdout[v], timing=True)[1]]
                if v != "fused":
                    if cmd in ("polish", "filter_polish"):
                        res[v]["same"] = sha(stdout[v]) == sha(stdout["fused"])
                    else:
                        res[v]["same"] = all(sha(x, inflate=v == "chain_bgzf") == sha(y) for x, y in zip(outs[v], outs["fused"]))
                log(f"{cmd} {v}: {res[v]['wall_s']}")
            if cmd in ("filter", "filter_out_bam"):
                res["out_bytes"] = {v: [size(p) for p in outs[v]] for v in names}
            out[cmd] = res
        line = json.dumps(out)
        print(line)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
