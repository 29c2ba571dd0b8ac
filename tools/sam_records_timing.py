#!/usr/bin/env python3
"""What pp_sam_records costs on configs[1]'s SAM text: the two files tools/synthjob.py writes for make_job(pairs=True) (every record,
QUAL included), each resident in HBM in an allocation of exactly its length and decoded with mem = MEM_DEVICE.  One warm-up pass,
then --repeat passes; every figure is the sum over the two files, given as the median of the passes with their minimum and maximum.
Writes one JSON line to profiles/sam_records_timing.json (--out) and prints it:
  stages_ms      HIP-event time by stage: copy (the device-to-device copy of the text, and the zeros behind it) | newline_index | scan
                 (k_sam_scan) | place (k_sam_place x 2 + k_colscan<3>) | cigar (k_sam_cigar)
  text_bytes, records, scan_gbps = text_bytes over the scan's time, copy_share = copy over the sum of the five stages
  tokenizer      pp_dev_ingest_sam on the same two files at the same commit (the command, PP_DEVICE_INGEST=1):
                   k_tok_parse       kernel time of k_tok_parse (ms, over both files) from a `rocprofv3 --kernel-trace --stats` run of
                                     its own -- the tokenizer records no events -- and text bytes per second over it (gbps)
                   lines_parsed_ms   the tokenizer's PP_TIMING lap "lines parsed": a host clock around k_tok_parse, its scan and a
                                     synchronising read-back, from a run without the profiler
  bam            pp_bam_records on the same records as uncompressed BAM (tools/bam_timing.py's encoder): pass_a | scans | pass_b
Measurement only: no threshold is attached to any of it."""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import polypolish_amd as pp  # noqa: E402
import bam_timing  # noqa: E402
import gate_timing  # noqa: E402
import synthjob  # noqa: E402

STAGES = ("copy", "newline_index", "scan", "place", "cigar")


def spread(values):
    return {"median": round(statistics.median(values), 4), "min": round(min(values), 4), "max": round(max(values), 4)}


CHILD = """import sys
sys.path.insert(0, sys.argv[1])
import polypolish_amd as pp
ctx = pp.Context(0)
pp.ingest_device(ctx, sys.argv[2], sys.argv[3:])
ctx.close()
"""


def k_tok_parse_kernel_ms(fa, sams, tmp):
    """kernel time of k_tok_parse from rocprofv3's kernel statistics of a Python process of its own that runs pp_dev_ingest_sam over
    the files (ingest_device; under the command itself the profiler wrote no statistics)"""
    prof = shutil.which("rocprofv3")
    if not prof:
        return {"skipped": "no rocprofv3 on PATH"}
    out = os.path.join(tmp, "trace")
    r = subprocess.run([prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable, "-c", CHILD, ROOT, fa] + sams,
                       capture_output=True)
    if r.returncode:
        return {"error": r.stderr.decode(errors="replace")[-300:]}
    total, calls = 0.0, 0
    for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                if "k_tok_parse" in row.get("Name", ""):
                    total += float(row["TotalDurationNs"])
                    calls += int(row["Calls"])
    if not calls:
        found = [os.path.relpath(q, out) for q in glob.glob(os.path.join(out, "**", "*"), recursive=True) if os.path.isfile(q)]
        return {"error": "no k_tok_parse row in rocprofv3's kernel statistics", "files": found[:12]}
    return {"ms": round(total / 1e6, 4), "calls": calls}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mbp", type=float, default=5.0, help="assembly size (configs[1]: 5)")
    ap.add_argument("--coverage", type=int, default=200)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--no-bam", action="store_true", help="leave pp_bam_records out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sam_records_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sam_records_timing: no GPU (nothing is measured without one)")
    if synthjob.samgen_lib() is None:
        sys.exit("sam_records_timing: tools/_build/libsamgen.so is missing (make)")
    dev = torch.device("cuda:0")
    job = synthjob.make_job(dev, contig_lens=(int(a.mbp * 1e6),), coverage=a.coverage, seed=a.seed, pairs=True, unaligned_frac=1e-3)
    torch.cuda.synchronize()
    out = {"input": f"{a.mbp:g} Mbp x {a.coverage}, {job['sam']['n']} records in two SAM files with QUAL (seed {a.seed})", "repeat": a.repeat}
    with tempfile.TemporaryDirectory(prefix="pp_sam_", dir=os.environ.get("TMPDIR", "/tmp")) as tmp:
        fa, sams = synthjob.write_sam_pair(job, tmp, qual=True)
        texts = [torch.from_numpy(np.fromfile(p, np.uint8)).to(dev) for p in sams]
        torch.cuda.synchronize()
        ctx = pp.Context(0)
        ctx.set_profiling(1)
        runs, records = [], 0
        for i in range(a.repeat + 1):       # (the first pass warms up: code objects, the allocator)
            ms, records = dict.fromkeys(STAGES, 0.0), 0
            for t in texts:
                rec = pp.SamRecords(ctx, (t.data_ptr(), t.numel()), pp.MEM_DEVICE)
                for k, v in rec.stage_ms().items():
                    ms[k] += v
                records += rec.n_rec
                rec.close()
            if i:
                runs.append(ms)
        text_bytes = sum(t.numel() for t in texts)
        out.update(text_bytes=text_bytes, records=records, stages_ms={k: spread([r[k] for r in runs]) for k in STAGES},
                   total_ms=spread([sum(r.values()) for r in runs]),
                   scan_gbps=spread([text_bytes / 1e9 / (r["scan"] / 1e3) for r in runs]),
                   copy_share=spread([r["copy"] / sum(r.values()) for r in runs]))
        del texts
        kernel = k_tok_parse_kernel_ms(fa, sams, tmp)
        if "ms" in kernel:
            kernel["gbps"] = round(text_bytes / 1e9 / (kernel["ms"] / 1e3), 1)
        laps = gate_timing.tokenizer_stages(job, tmp)
        out["tokenizer"] = {"k_tok_parse": kernel, "lines_parsed_ms": laps.get("lines parsed", laps), "laps_ms": laps}
        if not a.no_bam:
            S, n, half = job["sam"], job["sam"]["n"], job["sam"]["half"]
            files = []
            for lo, hi in ((0, half), (half, n)):
                b, off = bam_timing.encode_bam(S, lo, hi)
                files.append((torch.from_numpy(b).to(dev), torch.from_numpy(off.view(np.int64)).to(dev), len(b), len(off)))
            torch.cuda.synchronize()
            runs = []
            for i in range(a.repeat + 1):
                ms = dict.fromkeys(("pass_a", "scans", "pass_b"), 0.0)
                for tb, to, n_bytes, n_rec in files:
                    rec = pp.BamRecords(ctx, (tb.data_ptr(), n_bytes), (to.data_ptr(), n_rec), None, pp.MEM_DEVICE)
                    for k, v in rec._stage_ms("pp_bam_stage_ms_", tuple(ms)).items():
                        ms[k] += v
                    rec.close()
                if i:
                    runs.append(ms)
            out["bam"] = {"bam_bytes": sum(f[2] for f in files), "stages_ms": {k: spread([r[k] for r in runs]) for k in runs[0]},
                          "total_ms": spread([sum(r.values()) for r in runs])}
        ctx.close()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
