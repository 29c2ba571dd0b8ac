#!/usr/bin/env python3
"""What the device reduction of the filter's samples buys, and what the record grouping costs, on the filter input of
BASELINE.json configs[1] (5 Mbp, 200x, 2 x 150 bp; tools/synthjob.py's SAM pair).  Prints one JSON line:
  file_drivers    the laps of `polypolish filter` with PP_TIMING=1 for the step the file drivers do on the host: "samples from the
                  device" and "thresholds" (host loader), and "names interned" / "groups built" of PP_DEVICE_FILTER=1.  --exe PATH
                  takes them from another build's binary (default bin/polypolish)
  new_thresholds  pp_filter_thresholds right after pp_filter_begin on the same input: wall time of the call, HIP-event time of its
                  kernels (3 warm-ups, 10 runs)
  records         pp_filter_records on the same records in device memory: HIP-event time of rec_compact / rec_intern / rec_groups
--out FILE writes the line to FILE as well.  Measurement only: no threshold is attached to any of it."""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import synthjob  # noqa: E402
import polypolish_amd as pp  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--exe", default=os.path.join(ROOT, "bin", "polypolish"), help="the polypolish binary whose PP_TIMING laps are taken")
ap.add_argument("--out", default=None)
args = ap.parse_args()
EXE = args.exe
res = {}


def save():
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh)


dev = torch.device("cuda:0")
tmp = tempfile.mkdtemp(prefix="pp_meas_", dir=os.environ.get("TMPDIR", "/tmp"))
t0 = time.perf_counter()
job = synthjob.make_job(dev, contig_lens=[5_000_000], coverage=200, seed=4243, pairs=True, unaligned_frac=1e-3, repeat=None, recipe="survey")
torch.cuda.synchronize()
fa, sams = synthjob.write_sam_pair(job, tmp, qual=True)
del job
torch.cuda.empty_cache()
res["files"] = {"text_bytes": sum(os.path.getsize(p) for p in sams), "generated_s": round(time.perf_counter() - t0, 1)}
save()

# ---- the file drivers' own laps ----
outs = [os.path.join(tmp, f"out_{i}.sam") for i in (1, 2)]


def exe_run(extra_env):
    env = dict(os.environ, PP_TIMING="1", **extra_env)
    r = subprocess.run([EXE, "filter", "--in1", sams[0], "--in2", sams[1], "--out1", outs[0], "--out2", outs[1]], capture_output=True, env=env, timeout=170)
    if r.returncode != 0:
        raise RuntimeError(r.stderr.decode(errors="replace")[-600:])
    return r.stderr.decode(errors="replace")


def laps_cumulative(text):
    out = {}
    for m in re.finditer(r"\[timing\] (.{28}) +([0-9.]+) s", text):
        out[m.group(1).strip()] = float(m.group(2))
    return out


def laps_device_load(text):
    return {m.group(1).strip(): float(m.group(2)) for m in re.finditer(r"\[timing\]   device load: (.{18}) ([0-9.]+) s", text)}


if os.path.exists(EXE):
    host_runs, dev_runs = [], []
    for rep in range(4):
        text = exe_run({})
        lp = laps_cumulative(text)
        if rep:
            host_runs.append({"samples from the device": round(lp["samples from the device"] - lp["alignments loaded"], 4),
                              "thresholds": round(lp["thresholds"] - lp["samples from the device"], 4)})
        m = re.search(r"Low threshold:\s+(\d+).*\nHigh threshold:\s+(\d+)", text)
        res["file_driver_thresholds"] = [int(m.group(1)), int(m.group(2))] if m else None
        cnt = re.findall(r"^(fr|rf|ff|rr): ([0-9,]+) pairs", text, re.M)
        res["file_driver_counts"] = [int(c.replace(",", "")) for _, c in cnt]
    for rep in range(3):
        text = exe_run({"PP_DEVICE_FILTER": "1"})
        if rep:
            dev_runs.append(laps_device_load(text))
    res["file_drivers"] = {"exe": EXE, "host_loader_laps_s": host_runs, "device_loader_laps_s": dev_runs, "note": "lap resolution 1 ms; first run of each kind left out"}
    save()
else:
    res["file_drivers"] = {"skipped": EXE + " is missing"}

# ---- new path: pp_filter_thresholds on the same input ----
L = pp.lib()
ctx = pp.Context(0)
loaded = pp.FilterLoaded(sams[0], sams[1])
res["input"] = {"n_reads": loaded.n_reads, "n_aln": [len(f["ref_id"]) for f in loaded.files], "counts": loaded.counts}


def one_thresholds(profile):
    ctx.set_profiling(profile)
    assert L.pp_filter_begin(ctx._h, C.byref(loaded.input), pp.MEM_HOST) == 0
    ctx.sync()
    t = time.perf_counter()
    rep = ctx.filter_thresholds("auto", 0.1, 99.9)
    wall = time.perf_counter() - t
    ms = None
    if profile:
        kt = pp.KernelTimes()
        L.pp_filter_kernel_times(ctx._h, C.byref(kt))
        ms = kt.as_dict()["ms"]
    return wall, rep, ms


for _ in range(3):
    one_thresholds(False)
walls, kms = [], []
for _ in range(10):
    w, rep, _ = one_thresholds(False)
    walls.append(w * 1e3)
for _ in range(10):
    w, rep, ms = one_thresholds(True)
    kms.append(ms)
res["new_thresholds"] = {"report": rep, "wall_ms_no_profiling": {"median": round(statistics.median(walls), 4), "min": round(min(walls), 4), "max": round(max(walls), 4)},
                         "kernel_ms_median": {k: round(statistics.median(m[k] for m in kms), 4) for k in kms[0]},
                         "note": "the call runs the pass over the reads ('samples') too, as the drivers' 'samples from the device' lap does; 3 warm-ups, 10 runs"}
# (the same call when the pass over the reads has already run: the reduction alone)
walls2 = []
for _ in range(10):
    ctx.set_profiling(False)
    assert L.pp_filter_begin(ctx._h, C.byref(loaded.input), pp.MEM_HOST) == 0
    o, i = np.zeros(loaded.n_reads, np.uint8), np.zeros(loaded.n_reads, np.uint32)
    t = time.perf_counter()
    assert L.pp_filter_samples(ctx._h, o.ctypes.data, i.ctypes.data) == 0
    ts = time.perf_counter() - t
    t = time.perf_counter()
    ctx.filter_thresholds("auto", 0.1, 99.9)
    walls2.append(((time.perf_counter() - t) * 1e3, ts * 1e3))
res["new_thresholds"]["wall_ms_after_samples"] = round(statistics.median(w for w, _ in walls2), 4)
res["new_thresholds"]["pp_filter_samples_wall_ms"] = round(statistics.median(s for _, s in walls2), 4)
save()

# ---- grouping: pp_filter_records on the same records, device memory ----
raws, keep = [], []
for f in loaded.files:
    n = len(f["ref_id"])
    rid = (f["read"].astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15))  # (wraps: any 64-bit value is an id)
    host = {"flag": f["flags"].astype(np.uint16), "read_id": rid, "contig": f["ref_id"], "ref_start": f["ref_start"], "cig_off": f["cig_off"],
            "n_cig": f["n_cig"], "cigar": f["cigar"]}
    signed = {2: np.int16, 4: np.int32, 8: np.int64}
    t = {k: torch.from_numpy(np.ascontiguousarray(v).view(signed[v.dtype.itemsize])).to(dev) for k, v in host.items()}
    keep.append(t)
    p = {k: v.data_ptr() for k, v in t.items()}
    p.update(n_rec=n, seq_bytes=0, n_cig_total=len(f["cigar"]))
    raws.append(p)
torch.cuda.synchronize()
rec_ms, rec_wall = [], []
for it in range(7):
    ctx.set_profiling(it >= 2)
    t = time.perf_counter()
    got = pp.filter_records(ctx, raws[0], raws[1], mem=pp.MEM_DEVICE)
    w = time.perf_counter() - t
    if it >= 2:
        kt = pp.KernelTimes()
        L.pp_filter_kernel_times(ctx._h, C.byref(kt))
        rec_ms.append(kt.as_dict()["ms"])
        rec_wall.append(w * 1e3)
res["records"] = {"report": got["report"], "counts": got["counts"], "kernel_ms_median": {k: round(statistics.median(m[k] for m in rec_ms), 4) for k in rec_ms[0]},
                  "wall_ms_median_with_profiling": round(statistics.median(rec_wall), 3), "note": "2 warm-ups, 5 runs"}
res["agree"] = {"thresholds_vs_file_drivers": res.get("file_driver_thresholds") == [rep["low"], rep["high"]],
                "records_vs_thresholds": (got["report"]["low"], got["report"]["high"], got["report"]["counts"]) == (rep["low"], rep["high"], rep["counts"])}
save()
print(json.dumps(res))
loaded.close()
ctx.close()
for p in sams + outs + [fa]:
    if os.path.exists(p):
        os.remove(p)
