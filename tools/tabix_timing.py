#!/usr/bin/env python3
"""What pp_tabix_index costs on the tracks of bench.py's configs[1] job (5 Mbp / 200x, resident in HBM), stage by stage, next to what
else moves as many bytes.  One warm-up pass, then --repeat passes; every figure is the median of the passes with their minimum and
maximum.  Writes one JSON line to profiles/tabix_timing.json (--out) and prints it.
  vcf / bed / depth_runs / depth_bin1000   pp_tabix_index on the job's VCF, its BED, its depth track in the runs form and under bins of
                              1000, the text and the block table of its pp_bgzf_deflate where they lie in device memory: lines,
                              text_bytes, tbi_bytes, stage_ms (HIP-event spans on the context's stream: newlines | rows | names | chunks |
                              linear), kernel_ms (their sum), call_ms (wall time of the whole call), host_ms (call_ms - kernel_ms: the
                              read-backs between the stages, the allocations, the serialiser and the index's own pp_bgzf_deflate)
  ...["deflate_ms"]           pp_bgzf_deflate of the same text: the HIP-event time of its kernels, and its wall time
  ...["d2d_copy_text_ms"]     a device-to-device copy of the text's bytes; kernel_over_copy: kernel_ms over it
  polish_e2e_s                `polypolish polish` on a SAM pair (--e2e_mbp / --e2e_coverage: smaller than configs[1], the files are written
                              and read here) with --depth --depth_bgzf, with and without --depth_tbi, and plain, the runs alternating
pp_bam_index on configs[1]'s records is tools/bam_sort_timing.py's figure (profiles/bam_sort_timing.json) and is not measured again.
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

STAGES = ("newlines", "rows", "names", "chunks", "linear")


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


def index_times(ctx, track, preset, repeat, dev):
    text = track.dev()
    lines = track.n_records
    dk, dw = [], []
    for i in range(repeat + 1):
        box = []
        ms = wall_ms(lambda: box.append(track.deflate()))
        if i:
            dw.append(ms)
            dk.append(box[0].kernel_ms())
        if i < repeat:
            box[0].close()
    z = box[0]
    stages, call = {k: [] for k in STAGES}, []
    for i in range(repeat + 1):
        box = []
        ms = wall_ms(lambda: box.append(pp.tabix_index(ctx, text, preset, (z.blk_off_ptr, z.n_blocks), pp.MEM_DEVICE, raw=False)))
        if i:
            call.append(ms)
            for k, x in pp.tabix_stage_ms(ctx).items():
                stages[k].append(x)
    kernel = [sum(x) for x in zip(*stages.values())]
    out = {"lines": lines, "text_bytes": text[1], "file_bytes": z.n_bytes, "tbi_bytes": len(box[0][0]), "stage_ms": {k: spread(x) for k, x in stages.items()},
           "kernel_ms": spread(kernel), "call_ms": spread(call), "host_ms": spread([c - k for c, k in zip(call, kernel)]),
           "deflate_ms": {"kernel_ms": spread(dk), "call_ms": spread(dw)}}
    z.close()
    out["d2d_copy_text_ms"] = d2d_ms(text[1], repeat, dev)
    out["kernel_over_copy"] = round(out["kernel_ms"]["median"] / max(out["d2d_copy_text_ms"]["median"], 1e-6), 2)
    out["call_over_deflate_call"] = round(out["call_ms"]["median"] / max(out["deflate_ms"]["call_ms"]["median"], 1e-6), 3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mbp", type=float, default=5.0, help="assembly size (configs[1]: 5)")
    ap.add_argument("--coverage", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3, help="end-to-end runs per variant (0: none)")
    ap.add_argument("--e2e_mbp", type=float, default=1.0)
    ap.add_argument("--e2e_coverage", type=int, default=50)
    ap.add_argument("--tmp", default="/dev/shm" if os.path.isdir("/dev/shm") else None, help="where the files go (a directory made there is removed afterwards)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tabix_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tabix_timing: no GPU (nothing is measured without one)")
    import synthjob
    dev = torch.device("cuda:0")
    G0 = int(a.mbp * 1e6)
    # bench.py's configs[1] job, seed included (config 1, rank 0), as tools/depth_timing.py makes it
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
    out = {"tool": "tools/tabix_timing.py", "workload": f"configs[1]: {G / 1e6:g} Mbp / {a.coverage}x, {job['n_aln']} records resident in HBM", "repeat": a.repeat,
           "lane_bytes": pp.TBX_LANE_BYTES}
    run = ctx.prepared_job(job["contig_off"], job["bases"].data_ptr(), pp.MEM_DEVICE, job["n_aln"], ptrs, job["recs"]["seq"].numel(),
                           job["recs"]["cigar"].numel(), pp.MEM_DEVICE, 5, 0.5, 0.2)
    L.pp_polish_set_debug(ctx._h, 1)
    try:
        run()
        ctx.sync()
    finally:
        L.pp_polish_set_debug(ctx._h, 0)
    ctx.set_profiling(1)
    for key, make, preset in (("vcf", lambda: pp.Vcf(ctx, names), pp.TBX_VCF), ("bed", lambda: pp.StatusBed(ctx, names), pp.TBX_BED),
                              ("depth_runs", lambda: ctx.polish_depth(names, 0), pp.TBX_BED), ("depth_bin1000", lambda: ctx.polish_depth(names, 1000), pp.TBX_BED)):
        track = make()
        try:
            out[key] = index_times(ctx, track, preset, a.repeat, dev)
        finally:
            track.close()
    ctx.set_profiling(0)
    ctx.close()
    del job
    torch.cuda.empty_cache()
    # ---- `polish` end to end with and without the index, the runs alternating ----
    if a.runs > 0:
        import text_chain_timing as tct
        tmp = tempfile.mkdtemp(prefix="tabix_timing_", dir=a.tmp)
        try:
            pairs = synthjob.make_job(dev, contig_lens=(int(a.e2e_mbp * 1e6),), coverage=a.e2e_coverage, seed=42, pairs=True, unaligned_frac=1e-3)
            torch.cuda.synchronize()
            fasta, sams = synthjob.write_sam_pair(pairs, tmp, qual=True)
            del pairs
            torch.cuda.empty_cache()  # (the child processes are the only users of the device from here on)
            track = os.path.join(tmp, "depth.bedgraph.gz")
            variants = {"plain": [], "depth_bgzf": ["--depth", track, "--depth_bgzf"], "depth_bgzf_tbi": ["--depth", track, "--depth_bgzf", "--depth_tbi"]}
            res = {v: [] for v in variants}
            for v, flags in variants.items():  # warm-up
                tct.timed(["polish", *flags, fasta, *sams], os.path.join(tmp, f"{v}.stdout"))
            for _ in range(a.runs):
                for v, flags in variants.items():
                    res[v].append(round(tct.timed(["polish", *flags, fasta, *sams], os.path.join(tmp, f"{v}.stdout"))[0], 3))
            out["polish_e2e_s"] = {v: {"wall_s": x, "median_s": statistics.median(x)} for v, x in res.items()}
            out["polish_e2e_s"]["workload"] = f"{a.e2e_mbp:g} Mbp / {a.e2e_coverage}x as a SAM pair"
            out["polish_e2e_s"]["same_fasta"] = tct.sha(os.path.join(tmp, "depth_bgzf_tbi.stdout")) == tct.sha(os.path.join(tmp, "plain.stdout"))
            out["polish_e2e_s"]["file_bytes"] = {"depth_bgzf": os.path.getsize(track), "tbi": os.path.getsize(track + ".tbi")}
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
