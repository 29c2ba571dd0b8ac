#!/usr/bin/env python3
"""What pp_polish_depth and pp_depth_bedgraph cost on bench.py's configs[1] job (5 Mbp / 200x, resident in HBM), stage by stage, next
to what else moves as many bytes.  One warm-up pass, then --repeat passes; every figure is the median of the passes with their minimum
and maximum.  Writes one JSON line to profiles/depth_timing.json (--out) and prints it.
  job_runs / job_bin1000      pp_polish_depth on the job's own depth plane with bin 0 (runs) and bin 1000: records, text_bytes, the
                              summary, stage_ms (HIP-event spans on the context's stream: values | records | lengths | text -- a span holds
                              the host's work between its launches too: the read-backs, the allocations and the uploads), kernel_ms
                              (their sum), call_ms (wall time of the whole call)
  flat_runs / flat_bin1000    pp_depth_bedgraph on a flat device array of G doubles: one run
  bed_all                     pp_polish_bed with every status selected on the same job: kernel_ms, call_ms
  d2d_copy_8G_ms              HIP-event time of a device-to-device copy of 8 G bytes (the depth plane); d2d_copy_text_ms: of each text's bytes
  runs_over_copy              the runs form's kernel_ms over the copies of the bytes it reads and writes: the plane twice, the text once
  polish_e2e_s                `polypolish polish` on a SAM pair (--e2e_mbp / --e2e_coverage: smaller than configs[1], the files are written
                              and read here) with and without --depth, the runs alternating: wall seconds
Measurement only: no threshold is attached to any of it."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import polypolish_amd as pp  # noqa: E402

STAGES = ("values", "records", "lengths", "text")


def spread(values):
    return {"median": round(statistics.median(values), 4), "min": round(min(values), 4), "max": round(max(values), 4)}


def wall_ms(f):
    t = time.perf_counter()
    f()
    return (time.perf_counter() - t) * 1e3


def d2d_ms(n, repeat, dev):
    src = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    out = []
    for i in range(repeat + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        if i:
            out.append(e0.elapsed_time(e1))
    return spread(out)


def track_times(make, repeat):
    """make() -> DepthTrack, repeat + 1 times (the first pass warms up)"""
    stages, call = {k: [] for k in STAGES}, []
    for i in range(repeat + 1):
        box = []
        ms = wall_ms(lambda: box.append(make()))
        t = box[0]
        if i:
            call.append(ms)
            for k, x in t.stage_ms().items():
                stages[k].append(x)
        rec, nb, summ = t.n_records, t.n_bytes, t.summary()
        t.close()
    kernel = [sum(x) for x in zip(*stages.values())]
    return {"records": rec, "text_bytes": nb, "summary": summ, "stage_ms": {k: spread(x) for k, x in stages.items()}, "kernel_ms": spread(kernel),
            "call_ms": spread(call)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mbp", type=float, default=5.0, help="assembly size (configs[1]: 5)")
    ap.add_argument("--coverage", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--runs", type=int, default=3, help="end-to-end runs per variant (0: none)")
    ap.add_argument("--e2e_mbp", type=float, default=1.0)
    ap.add_argument("--e2e_coverage", type=int, default=50)
    ap.add_argument("--tmp", default="/dev/shm" if os.path.isdir("/dev/shm") else None, help="where the files go (a directory made there is removed afterwards)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("depth_timing: no GPU (nothing is measured without one)")
    import synthjob
    dev = torch.device("cuda:0")
    G0 = int(a.mbp * 1e6)
    # bench.py's configs[1] job, seed included (config 1, rank 0), as tools/bed_timing.py makes it
    job = synthjob.with_wo(synthjob.with_seq4(synthjob.make_job(dev, contig_lens=[G0], coverage=a.coverage, read_len=150, seed=42 + 1 + 1,
                                                                indel_read_frac=synthjob.SURVEY_INDEL_READ_FRAC, recipe="survey")))
    torch.cuda.synchronize()
    G = int(job["contig_off"][-1])
    ptrs = {k: v.data_ptr() for k, v in job["recs"].items()}
    ptrs.update(seq4=job["seq4"].data_ptr(), wo=job["wo"].data_ptr(), wo_runs=job["wo_runs"])
    L = pp.lib()
    ctx = pp.Context(0)
    ctx.trust_mirrors(True)
    names = [b"chr1"]
    out = {"tool": "tools/depth_timing.py", "workload": f"configs[1]: {G / 1e6:g} Mbp / {a.coverage}x, {job['n_aln']} records resident in HBM",
           "repeat": a.repeat, "geometry": dict(zip(("pos_per_thread", "pos_per_workgroup", "bytes_per_store", "bytes_per_workgroup"), pp.depth_geometry()))}
    run = ctx.prepared_job(job["contig_off"], job["bases"].data_ptr(), pp.MEM_DEVICE, job["n_aln"], ptrs, job["recs"]["seq"].numel(),
                           job["recs"]["cigar"].numel(), pp.MEM_DEVICE, 5, 0.5, 0.2)
    L.pp_polish_set_debug(ctx._h, 1)
    try:
        run()
        ctx.sync()
    finally:
        L.pp_polish_set_debug(ctx._h, 0)
    ctx.set_profiling(1)
    flat = torch.full((G,), 30.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    off = [0, G]
    for key, W in (("runs", 0), ("bin1000", 1000)):
        out["job_" + key] = track_times(lambda: ctx.polish_depth(names, W), a.repeat)
        out["flat_" + key] = track_times(lambda: ctx.depth_bedgraph(flat.data_ptr(), off, names, W, mem=pp.MEM_DEVICE), a.repeat)
    kernel, call = [], []
    for i in range(a.repeat + 1):
        box = []
        ms = wall_ms(lambda: box.append(pp.StatusBed(ctx, names, 63)))
        b = box[0]
        if i:
            call.append(ms)
            kernel.append(b.kernel_ms())
        rec, nb = b.n_records, b.n_bytes
        b.close()
    out["bed_all"] = {"records": rec, "text_bytes": nb, "kernel_ms": spread(kernel), "call_ms": spread(call)}
    ctx.set_profiling(0)
    ctx.close()
    del flat, job
    torch.cuda.empty_cache()
    out["d2d_copy_8G_ms"] = d2d_ms(8 * G, a.repeat, dev)
    out["d2d_copy_text_ms"] = {}
    for key in ("job_runs", "job_bin1000", "flat_runs", "flat_bin1000"):
        out["d2d_copy_text_ms"][key] = d2d_ms(out[key]["text_bytes"], a.repeat, dev)
        out[key]["kernel_over_d2d_8G"] = round(out[key]["kernel_ms"]["median"] / out["d2d_copy_8G_ms"]["median"], 2)
    for key in ("job_runs", "flat_runs"):  # the runs form reads the plane twice and writes the text once
        moved = 2 * out["d2d_copy_8G_ms"]["median"] + out["d2d_copy_text_ms"][key]["median"]
        out.setdefault("runs_over_copy", {})[key] = round(out[key]["kernel_ms"]["median"] / moved, 2)
    # ---- `polish` end to end with and without --depth, the runs alternating ----
    if a.runs > 0:
        import text_chain_timing as tct
        tmp = tempfile.mkdtemp(prefix="depth_timing_", dir=a.tmp)
        try:
            pairs = synthjob.make_job(dev, contig_lens=(int(a.e2e_mbp * 1e6),), coverage=a.e2e_coverage, seed=42, pairs=True, unaligned_frac=1e-3)
            torch.cuda.synchronize()
            fasta, sams = synthjob.write_sam_pair(pairs, tmp, qual=True)
            del pairs
            torch.cuda.empty_cache()  # (the child processes are the only users of the device from here on)
            track = os.path.join(tmp, "depth.bedgraph")
            variants = {"plain": [], "depth": ["--depth", track], "depth_bin1000_bgzf": ["--depth", track + ".gz", "--depth_bin", "1000", "--depth_bgzf"]}
            res = {v: [] for v in variants}
            for v, flags in variants.items():  # warm-up
                tct.timed(["polish", *flags, fasta, *sams], os.path.join(tmp, f"{v}.stdout"))
            for _ in range(a.runs):
                for v, flags in variants.items():
                    res[v].append(round(tct.timed(["polish", *flags, fasta, *sams], os.path.join(tmp, f"{v}.stdout"))[0], 3))
            out["polish_e2e_s"] = {v: {"wall_s": x, "median_s": statistics.median(x)} for v, x in res.items()}
            out["polish_e2e_s"]["workload"] = f"{a.e2e_mbp:g} Mbp / {a.e2e_coverage}x as a SAM pair"
            out["polish_e2e_s"]["same_fasta"] = tct.sha(os.path.join(tmp, "depth.stdout")) == tct.sha(os.path.join(tmp, "plain.stdout"))
            out["polish_e2e_s"]["depth_file_bytes"] = {"runs_text": os.path.getsize(track), "bin1000_bgzf": os.path.getsize(track + ".gz")}
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
