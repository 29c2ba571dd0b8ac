#!/usr/bin/env python3
"""What pp_polish_bed and pp_polish_masked cost on bench.py's configs[1] job (5 Mbp / 200x, resident in HBM), next to what else reads or
writes as many bytes, and what switching the per-position debug records on costs the step.  One warm-up pass, then --repeat passes; every
figure is the median of the passes with their minimum and maximum.  Writes one JSON line to profiles/bed_timing.json (--out) and prints
it.
  bed_undecided / bed_all     pp_polish_bed with the default mask and with every status selected: records, text_bytes, positions per
                              status, stage_ms (HIP-event spans on the context's stream: runs | records | text -- a span holds the host's
                              work between its launches too: the read-backs, the allocations and the uploads), kernel_ms (their sum),
                              call_ms (wall time of the whole call)
  masked_undecided / _all     pp_polish_masked: kernel_ms (the copy of the polished bytes and the mask pass, HIP events), call_ms
  vcf                         pp_polish_vcf on the same job: kernel_ms, call_ms
  d2d_copy_G_ms / _out_ms     HIP-event time of a device-to-device copy of G bytes and of the polished bytes
  step_ms                     wall time of the polish step (begin + add + finish on the resident records) with and without
                              pp_polish_set_debug(ctx, 1), the runs alternating: what keeping the status costs a run today, which
                              decides whether the status gets a plane of its own
Measurement only: no threshold is attached to any of it."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import polypolish_amd as pp  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mbp", type=float, default=5.0, help="assembly size (configs[1]: 5)")
    ap.add_argument("--coverage", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bed_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bed_timing: no GPU (nothing is measured without one)")
    import synthjob
    dev = torch.device("cuda:0")
    G0 = int(a.mbp * 1e6)
    # bench.py's configs[1] job, seed included (config 1, rank 0), as tools/vcf_timing.py makes it
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
    out = {"tool": "tools/bed_timing.py", "workload": f"configs[1]: {G / 1e6:g} Mbp / {a.coverage}x, {job['n_aln']} records resident in HBM",
           "repeat": a.repeat}
    run = ctx.prepared_job(job["contig_off"], job["bases"].data_ptr(), pp.MEM_DEVICE, job["n_aln"], ptrs, job["recs"]["seq"].numel(),
                           job["recs"]["cigar"].numel(), pp.MEM_DEVICE, 5, 0.5, 0.2)

    def polish(debug):
        L.pp_polish_set_debug(ctx._h, debug)
        try:
            run()
            ctx.sync()
        finally:
            L.pp_polish_set_debug(ctx._h, 0)

    # ---- the step with and without the debug records, the runs alternating ----
    for debug in (0, 1):
        polish(debug)  # warm-up: the buffers of both forms are allocated
    step = {"plain": [], "debug": []}
    for _ in range(a.repeat):
        for key, debug in (("plain", 0), ("debug", 1)):
            step[key].append(wall_ms(lambda: polish(debug)))
    out["step_ms"] = {k: spread(v) for k, v in step.items()}
    out["step_ms"]["debug_over_plain"] = round(out["step_ms"]["debug"]["median"] / out["step_ms"]["plain"]["median"], 3)
    # ---- the post-passes on a job that kept its status ----
    polish(1)
    n_out = ctx.result_size()
    out["polished_bytes"] = n_out
    ctx.set_profiling(1)
    for name, mask in (("undecided", pp.BED_UNDECIDED), ("all", 63)):
        stages, call = {k: [] for k in ("runs", "records", "text")}, []
        for i in range(a.repeat + 1):  # (the first pass warms up)
            box = []
            ms = wall_ms(lambda: box.append(pp.StatusBed(ctx, names, mask)))
            b = box[0]
            if i:
                call.append(ms)
                for k, x in b.stage_ms().items():
                    stages[k].append(x)
            rec, nb, counts = b.n_records, b.n_bytes, b.counts
            b.close()
        kernel = [sum(x) for x in zip(*stages.values())]
        out["bed_" + name] = {"records": rec, "text_bytes": nb, "positions": dict(zip(pp.STATUS_WORDS, counts)),
                              "stage_ms": {k: spread(x) for k, x in stages.items()}, "kernel_ms": spread(kernel), "call_ms": spread(call)}
        kernel, call = [], []
        for i in range(a.repeat + 1):
            box = []
            ms = wall_ms(lambda: box.append(pp.Masked(ctx, mask)))
            m = box[0]
            if i:
                call.append(ms)
                kernel.append(m.kernel_ms())
            m.close()
        out["masked_" + name] = {"kernel_ms": spread(kernel), "call_ms": spread(call)}
    kernel, call = [], []
    for i in range(a.repeat + 1):
        box = []
        ms = wall_ms(lambda: box.append(pp.Vcf(ctx, names)))
        v = box[0]
        if i:
            call.append(ms)
            kernel.append(v.kernel_ms())
        rec = v.n_records
        v.close()
    out["vcf"] = {"records": rec, "kernel_ms": spread(kernel), "call_ms": spread(call)}
    ctx.set_profiling(0)
    ctx.close()
    out["d2d_copy_G_ms"] = d2d_ms(G, a.repeat, dev)
    out["d2d_copy_out_ms"] = d2d_ms(n_out, a.repeat, dev)
    for key in ("bed_undecided", "bed_all", "masked_undecided", "masked_all", "vcf"):
        out[key]["kernel_over_d2d_G"] = round(out[key]["kernel_ms"]["median"] / out["d2d_copy_G_ms"]["median"], 2)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
