#!/usr/bin/env python3
"""What pp_sam_bam costs on configs[1]'s SAM text, and what `filter --out_bam` does to the command: the two files tools/synthjob.py writes
for make_job(pairs=True) (every record, QUAL included; the recipe of tools/sam_tag_timing.py), each resident in HBM in an allocation of
exactly its length.  Prints one JSON line and writes it to profiles/sam_bam_timing.json (--out); device figures are sums over the files:
  stages_ms        HIP-event time of pp_sam_bam by stage: newline_index | pass_a (k_sb_scan) | names (pp_names_ids x 2) | scans (k_sb_off
                   x 2, k_colscan, k_sb_refid) | pass_b (k_sb_emit); per stage the MEDIAN of --repeat passes behind a warm-up, and the
                   spread (max - min) / median of pass_b
  copy_ms          a plain device-to-device copy of the same texts, same run, median: the memory-rate yardstick; pass_b_over_copy
  sam_records_ms   pp_sam_records' kernels on the same texts (median);  sam_tagged_ms  pp_sam_tagged's, every record passing
  bam_bytes        the uncompressed BAM of the two files
  e2e              bin/polypolish filter, plain against --out_bam, alternating, --runs each, outputs under --tmp (tmpfs by default): wall
                   seconds, the PP_TIMING laps of the last run of each, the outputs' sizes; then polish from the text pair against polish
                   from the BAM pair
Measurement only: no threshold is attached to any of it."""
import argparse
import json
import os
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

import polypolish_amd as pp  # noqa: E402
import synthjob  # noqa: E402

EXE = os.path.join(ROOT, "bin", "polypolish")


def medians(passes):
    """[{stage: ms}] -> {stage: median}"""
    return {k: round(statistics.median(p[k] for p in passes), 4) for k in passes[0]}


def encode_passes(ctx, texts, repeat):
    out, n_bytes = [], 0
    for _ in range(repeat + 1):                                          # (the first pass warms up: code objects, the allocator)
        ms, n_bytes = None, 0
        for t in texts:
            e = pp.BamEncoded(ctx, (t.data_ptr(), t.numel()), mem=pp.MEM_DEVICE)
            s = e.stage_ms()
            ms = s if ms is None else {k: ms[k] + s[k] for k in s}
            n_bytes += e.n_bytes
            e.close()
        out.append(ms)
    return out[1:], n_bytes


def run(argv, timing=False):
    t0 = time.perf_counter()
    r = subprocess.run([EXE, *argv], capture_output=True, env=dict(os.environ, **({"PP_TIMING": "1"} if timing else {})), timeout=900)
    took = time.perf_counter() - t0
    if r.returncode:
        sys.exit(f"sam_bam_timing: polypolish {' '.join(argv)} ended with {r.returncode}: {r.stderr.decode()[-600:]}")
    laps = [ln for ln in r.stderr.decode().splitlines() if ln.startswith("[") or " ms" in ln][-24:]
    return took, laps, r.stdout


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mbp", type=float, default=5.0, help="assembly size (configs[1]: 5)")
    ap.add_argument("--coverage", type=int, default=200)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3, help="end-to-end runs of each command")
    ap.add_argument("--tmp", default="/dev/shm" if os.path.isdir("/dev/shm") else None, help="where the outputs go (default: tmpfs)")
    ap.add_argument("--no-e2e", action="store_true", help="leave out the commands")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sam_bam_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sam_bam_timing: no GPU (nothing is measured without one)")
    if synthjob.samgen_lib() is None:
        sys.exit("sam_bam_timing: tools/_build/libsamgen.so is missing (make)")
    dev = torch.device("cuda:0")
    job = synthjob.make_job(dev, contig_lens=(int(a.mbp * 1e6),), coverage=a.coverage, seed=a.seed, pairs=True, unaligned_frac=1e-3)
    torch.cuda.synchronize()
    out = {"input": f"{a.mbp:g} Mbp x {a.coverage}, {job['sam']['n']} records in two SAM files with QUAL (seed {a.seed})", "repeat": a.repeat}

    def emit(final):
        line = json.dumps(out)
        if final:
            print(line)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")

    with tempfile.TemporaryDirectory(prefix="pp_sam_bam_", dir=a.tmp) as tmp:
        fasta, sams = synthjob.write_sam_pair(job, tmp, qual=True)
        del job
        host = [np.fromfile(p, np.uint8) for p in sams]
        texts = [torch.from_numpy(h).to(dev) for h in host]
        torch.cuda.synchronize()
        text_bytes = sum(len(h) for h in host)
        print(f"[sam_bam_timing] texts: {[len(h) for h in host]} bytes", file=sys.stderr, flush=True)
        ctx = pp.Context(0)
        ctx.set_profiling(1)
        passes, bam_bytes = encode_passes(ctx, texts, a.repeat)
        stages = medians(passes)
        b = [p["pass_b"] for p in passes]
        # ---- next to it, same input, same run: pp_sam_records, pp_sam_tagged (every record passing), a device-to-device copy
        rec_ms, tag_ms, tag_b = [], [], []
        for i in range(a.repeat + 1):
            r_ms = t_ms = t_b = 0.0
            for t in texts:
                rec = pp.SamRecords(ctx, (t.data_ptr(), t.numel()), pp.MEM_DEVICE)
                r_ms += rec.kernel_ms()
                o = rec.tagged(np.ones(len(rec.zp), np.uint8))
                t_ms += o.kernel_ms()
                t_b += o.stage_ms()["pass_b"]
                o.close()
                rec.close()
            if i:
                rec_ms.append(r_ms), tag_ms.append(t_ms), tag_b.append(t_b)
        ctx.set_profiling(0)
        copies, dsts = [], [torch.empty_like(t) for t in texts]
        for i in range(a.repeat + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for d, t in zip(dsts, texts):
                d.copy_(t)
            e1.record()
            torch.cuda.synchronize()
            if i:
                copies.append(e0.elapsed_time(e1))
        del dsts
        copy_ms = statistics.median(copies)
        out.update(text_bytes=text_bytes, bam_bytes=bam_bytes, stages_ms=stages, kernels_ms=round(sum(stages.values()), 4),
                   pass_b_spread=round((max(b) - min(b)) / stages["pass_b"], 3), copy_ms=round(copy_ms, 4),
                   pass_b_over_copy=round(stages["pass_b"] / copy_ms, 2), pass_b_gbps=round((text_bytes + bam_bytes) / 1e9 / (stages["pass_b"] / 1e3), 1),
                   sam_records_ms=round(statistics.median(rec_ms), 4), sam_tagged_ms=round(statistics.median(tag_ms), 4),
                   sam_tagged_pass_b_ms=round(statistics.median(tag_b), 4))
        emit(False)             # (the device's figures are on disk before the commands start)
        ctx.close()
        del texts, host
        torch.cuda.empty_cache()
        if not a.no_e2e:
            text_outs = [os.path.join(tmp, f"filtered_{i}.sam") for i in (1, 2)]
            bam_outs = [os.path.join(tmp, f"filtered_{i}.bam") for i in (1, 2)]
            io = lambda outs: ["--in1", sams[0], "--in2", sams[1], "--out1", outs[0], "--out2", outs[1]]      # noqa: E731
            e2e = {"filter_s": [], "filter_out_bam_s": []}
            for i in range(a.runs):
                last = i == a.runs - 1
                took, laps, _ = run(["filter", *io(text_outs)], timing=last)
                e2e["filter_s"].append(round(took, 3))
                if last:
                    e2e["filter_laps"] = laps
                took, laps, _ = run(["filter", "--out_bam", *io(bam_outs)], timing=last)
                e2e["filter_out_bam_s"].append(round(took, 3))
                if last:
                    e2e["filter_out_bam_laps"] = laps
            e2e["text_out_bytes"] = sum(os.path.getsize(p) for p in text_outs)
            e2e["bam_out_bytes"] = sum(os.path.getsize(p) for p in bam_outs)
            e2e["polish_from_text_s"], e2e["polish_from_bam_s"], same = [], [], True
            for i in range(a.runs):
                t1, _, fa1 = run(["polish", fasta, *text_outs])
                t2, _, fa2 = run(["polish", fasta, *bam_outs])
                e2e["polish_from_text_s"].append(round(t1, 3))
                e2e["polish_from_bam_s"].append(round(t2, 3))
                same = same and fa1 == fa2
            e2e["polish_fasta_equal"] = same
            e2e["tmp"] = a.tmp or tempfile.gettempdir()
            out["e2e"] = e2e
    emit(True)


if __name__ == "__main__":
    main()
