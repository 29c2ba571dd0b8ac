#!/usr/bin/env python3
"""What the commands cost END TO END on BAM files, next to the same build's commands on the same records as SAM text: the records of
configs[1] (tools/synthjob.py, make_job(pairs=True)) written once as a SAM pair (tools/samgen.c) and once as the equivalent BAM pair
(tools/bam_timing.py's encoder behind a header; level 6, blocks of 0xff00 bytes, as htslib writes them).  bin/polypolish runs as a
child process on files in a warm page cache: one warm-up run, then --repeat runs.  Prints one JSON line; per command (polish, filter,
filter-polish) and per kind (sam, bam):
  wall_s         median and best of the runs (process start to exit)
  sha_equal      polish, filter-polish: the FASTA of the BAM run is the FASTA of the SAM run (sha256)
  laps           the PP_TIMING lines of one more BAM run: seconds since the driver was entered, per stage
and for polish also bam_prepared: the BAM route through pp_batch_prepare (PP_BAM_PREPARE=1), the direct path.
file_bytes has the sizes of the inputs and of filter's outputs.  --out FILE writes the line to FILE as well.  Measurement only: no
threshold is attached to any of it."""
import argparse
import hashlib
import json
import os
import re
import shutil
import struct
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
    print(f"[bam_cli_timing] {msg}", file=sys.stderr, flush=True)


def bam_header(names, lens):
    out = b"BAM\1" + struct.pack("<ii", 0, len(names))
    for name, ln in zip(names, lens):
        out += struct.pack("<i", len(name) + 1) + name + b"\0" + struct.pack("<i", int(ln))
    return out


def timed(argv, env, stdout_path):
    """one run of the CLI: (wall seconds, stderr text); the FASTA goes to stdout_path"""
    with open(stdout_path, "wb") as out:
        t0 = time.perf_counter()
        r = subprocess.run([EXE, *argv], stdout=out, stderr=subprocess.PIPE, env=dict(os.environ, **env))
        dt = time.perf_counter() - t0
    if r.returncode != 0:
        raise RuntimeError(f"polypolish {' '.join(argv)} ended with {r.returncode}: {r.stderr.decode()[-800:]}")
    return dt, r.stderr.decode()


def sha(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for piece in iter(lambda: f.read(1 << 24), b""):
            h.update(piece)
    return h.hexdigest()


def measure(argv, repeat, tmp, tag, env=None):
    env = env or {}
    out = os.path.join(tmp, f"{tag}.stdout")
    timed(argv, env, out)  # warm-up
    walls = sorted(timed(argv, env, out)[0] for _ in range(repeat))
    res = {"wall_s": {"median": round(walls[len(walls) // 2], 3), "best": round(walls[0], 3)}, "sha256": sha(out)}
    _, err = timed(argv, dict(env, PP_TIMING="1"), out)
    res["laps"] = [[re.sub(r"\s*\(process$", "", m.group(1).strip()).replace(tmp + os.sep, ""), float(m.group(2))] for m in re.finditer(r"^\[timing\] (.*?)\s+([0-9.]+) s", err, re.M)]
    log(f"{tag}: {res['wall_s']}")
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mbp", type=float, default=5.0, help="assembly size (configs[1]: 5)")
    ap.add_argument("--coverage", type=int, default=200)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--dir", help="where the files go (default: a temporary directory, removed afterwards)")
    ap.add_argument("--out", help="also write the JSON line to this file")
    a = ap.parse_args()
    import torch

    import bam_timing
    import bgzf_timing
    import synthjob
    tmp = a.dir or tempfile.mkdtemp(prefix="bam_cli_timing_")
    os.makedirs(tmp, exist_ok=True)
    try:
        job = synthjob.make_job(torch.device("cuda:0"), contig_lens=(int(a.mbp * 1e6),), coverage=a.coverage, seed=a.seed, pairs=True,
                                unaligned_frac=1e-3)
        torch.cuda.synchronize()
        fasta, sams = synthjob.write_sam_pair(job, tmp)
        S = job["sam"]
        n, half = S["n"], S["half"]
        off = job["contig_off"]
        head = bam_header([b"contig_%d" % (i + 1) for i in range(len(off) - 1)], np.diff(off.astype(np.int64)))
        bams = []
        for f, (lo, hi) in enumerate(((0, half), (half, n))):
            b, _ = bam_timing.encode_bam(S, lo, hi)
            z, _, _ = bgzf_timing.compress(np.concatenate([np.frombuffer(head, np.uint8), b]), 6)
            p = os.path.join(tmp, f"reads_{f + 1}.bam")
            z.tofile(p)
            bams.append(p)
            log(f"records [{lo}, {hi}): {len(b)} BAM bytes, {len(z)} in the file")
        del job, S
        torch.cuda.empty_cache()  # (the child processes are the only users of the device from here on)
        size = os.path.getsize
        out = {"input": f"{a.mbp:g} Mbp x {a.coverage}, {n} records in two files (seed {a.seed}); BAM: level 6, blocks of 0xff00 bytes",
               "repeat": a.repeat, "file_bytes": {"sam": [size(p) for p in sams], "bam": [size(p) for p in bams]}}
        o = {k: [os.path.join(tmp, f"filtered_{i}.{k}") for i in (1, 2)] for k in ("sam", "bam")}
        ins = {"sam": sams, "bam": bams}
        for kind in ("sam", "bam"):
            i1, i2 = ins[kind]
            o1, o2 = o[kind]
            out.setdefault("polish", {})[kind] = measure(["polish", fasta, i1, i2], a.repeat, tmp, f"polish_{kind}")
            out.setdefault("filter", {})[kind] = measure(["filter", "--in1", i1, "--in2", i2, "--out1", o1, "--out2", o2], a.repeat, tmp, f"filter_{kind}")
            out.setdefault("filter_polish", {})[kind] = measure(["filter-polish", "--in1", i1, "--in2", i2, fasta], a.repeat, tmp, f"fused_{kind}")
            out["file_bytes"][f"filtered_{kind}"] = [size(o1), size(o2)]
        out["polish"]["bam_prepared"] = measure(["polish", fasta, *bams], a.repeat, tmp, "polish_bam_prepared", env={"PP_BAM_PREPARE": "1"})
        for cmd in ("polish", "filter_polish"):
            out[cmd]["sha_equal"] = out[cmd]["sam"]["sha256"] == out[cmd]["bam"]["sha256"]
        out["polish"]["sha_equal"] = out["polish"]["sha_equal"] and out["polish"]["bam_prepared"]["sha256"] == out["polish"]["sam"]["sha256"]
        for cmd in ("polish", "filter", "filter_polish"):
            for v in out[cmd].values():
                if isinstance(v, dict):
                    v.pop("sha256", None)
            out[cmd].get("sam", {}).pop("laps", None)  # (the laps of the BAM runs are what this tool is about)
        line = json.dumps(out)
        print(line)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
    finally:
        if not a.dir:
            shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
