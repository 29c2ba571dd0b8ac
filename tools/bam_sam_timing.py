#!/usr/bin/env python3
"""What pp_bam_sam costs on configs[1]'s records as BAM, and what `filter --out_sam` does to the command: the two files tools/synthjob.py
writes for make_job(pairs=True) (every record, QUAL included; the recipe of tools/sam_bam_timing.py), encoded by pp_sam_bam, the BAM bytes
resident in HBM.  Prints one JSON line and writes it to profiles/bam_sam_timing.json (--out); device figures are sums over the files:
  stages_ms        HIP-event time of pp_bam_sam by stage: pass_a (k_bs_scan) | scans (k_colscan, k_bs_off x 2) | pass_b (k_bs_emit);
                   per stage the MEDIAN of --repeat passes behind a warm-up, and the spread (max - min) / median of pass_b
  copy_ms          a plain device-to-device copy of the OUTPUT's size, same run, median: the memory-rate yardstick; pass_b_over_copy
  sam_bam_pass_b_ms   pp_sam_bam's pass B on the same records, same run (profiles/sam_bam_timing.json has 6.0 ms);
  bam_tagged_ms    pp_bam_tagged's kernels on the same BAM bytes, every record passing
  text_equal       the decoded text is the text the BAM came from (the synthetic job's text is canonical), byte for byte
  e2e              bin/polypolish filter on the BAM pair, BAM -> BAM against --out_sam, alternating, --runs each, outputs under --tmp
                   (tmpfs by default): wall seconds, the PP_TIMING laps of the last run of each, the outputs' sizes
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


def run(argv, timing=False, strip=None):
    """-> (wall seconds, the PP_TIMING laps with the directory `strip` taken out of their paths)"""
    t0 = time.perf_counter()
    r = subprocess.run([EXE, *argv], capture_output=True, env=dict(os.environ, **({"PP_TIMING": "1"} if timing else {})), timeout=900)
    took = time.perf_counter() - t0
    if r.returncode:
        sys.exit(f"bam_sam_timing: polypolish {' '.join(argv)} ended with {r.returncode}: {r.stderr.decode()[-600:]}")
    laps = [ln for ln in r.stderr.decode().splitlines() if ln.startswith("[") or " ms" in ln][-24:]
    return took, [ln.replace(strip + os.sep, "") for ln in laps] if strip else laps


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mbp", type=float, default=5.0, help="assembly size (configs[1]: 5)")
    ap.add_argument("--coverage", type=int, default=200)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3, help="end-to-end runs of each command")
    ap.add_argument("--tmp", default="/dev/shm" if os.path.isdir("/dev/shm") else None, help="where the files go (default: tmpfs)")
    ap.add_argument("--no-e2e", action="store_true", help="leave out the commands")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bam_sam_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bam_sam_timing: no GPU (nothing is measured without one)")
    if synthjob.samgen_lib() is None:
        sys.exit("bam_sam_timing: tools/_build/libsamgen.so is missing (make)")
    dev = torch.device("cuda:0")
    job = synthjob.make_job(dev, contig_lens=(int(a.mbp * 1e6),), coverage=a.coverage, seed=a.seed, pairs=True, unaligned_frac=1e-3)
    torch.cuda.synchronize()
    out = {"input": f"{a.mbp:g} Mbp x {a.coverage}, {job['sam']['n']} records of two SAM files with QUAL as BAM (seed {a.seed})", "repeat": a.repeat}

    def emit(final):
        line = json.dumps(out)
        if final:
            print(line)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")

    with tempfile.TemporaryDirectory(prefix="pp_bam_sam_", dir=a.tmp) as tmp:
        _, sams = synthjob.write_sam_pair(job, tmp, qual=True)
        del job
        host = [np.fromfile(p, np.uint8) for p in sams]
        ctx = pp.Context(0)
        ctx.set_profiling(1)
        encs, enc_b = [], 0.0
        for h in host:                                      # the BAM bytes stay resident; the texts do not
            encs.append(pp.BamEncoded(ctx, h))
        for h in host:                                      # (a second, warm encode for pp_sam_bam's pass B)
            e = pp.BamEncoded(ctx, h)
            enc_b += e.stage_ms()["pass_b"]
            e.close()
        bam_bytes = sum(e.n_bytes for e in encs)
        n_rec = sum(e.n_rec for e in encs)
        print(f"[bam_sam_timing] BAM: {[e.n_bytes for e in encs]} bytes, {n_rec} records", file=sys.stderr, flush=True)
        passes, tag_ms, n_al, text_bytes, equal = [], [], [], 0, True
        for i in range(a.repeat + 1):                       # (the first pass warms up: code objects, the allocator)
            ms, text_bytes = None, 0
            for e, h in zip(encs, host):
                o = e.sam()
                s = o.stage_ms()
                ms = s if ms is None else {k: ms[k] + s[k] for k in s}
                text_bytes += o.n_bytes
                if i == 0:
                    equal = equal and o.n_bytes == len(h) and bool(np.array_equal(np.frombuffer(o.bytes(), np.uint8), h))
                    n_al.append(sum(o.counts()[:2]))
                o.close()
            if i:
                passes.append(ms)
        for i in range(a.repeat + 1):                       # pp_bam_tagged on the same bytes, every record passing
            t_ms = 0.0
            for e, k in zip(encs, n_al):
                t = e.tagged(np.ones(k, np.uint8))
                t_ms += t.kernel_ms()
                t.close()
            if i:
                tag_ms.append(t_ms)
        stages = medians(passes)
        stages.pop("newline_index", None)
        b = [p["pass_b"] for p in passes]
        ctx.set_profiling(0)
        src = torch.empty(text_bytes, dtype=torch.uint8, device=dev)
        dst, copies = torch.empty_like(src), []
        for i in range(a.repeat + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(src)
            e1.record()
            torch.cuda.synchronize()
            if i:
                copies.append(e0.elapsed_time(e1))
        del src, dst
        copy_ms = statistics.median(copies)
        out.update(bam_bytes=bam_bytes, text_bytes=text_bytes, records=n_rec, text_equal=equal, stages_ms=stages, kernels_ms=round(sum(stages.values()), 4),
                   pass_b_spread=round((max(b) - min(b)) / stages["pass_b"], 3), copy_ms=round(copy_ms, 4), pass_b_over_copy=round(stages["pass_b"] / copy_ms, 2),
                   pass_b_gbps=round((text_bytes + bam_bytes) / 1e9 / (stages["pass_b"] / 1e3), 1), sam_bam_pass_b_ms=round(enc_b, 4),
                   bam_tagged_ms=round(statistics.median(tag_ms), 4))
        emit(False)             # (the device's figures are on disk before the commands start)
        if not a.no_e2e:
            bams = [os.path.join(tmp, f"reads_{i}.bam") for i in (1, 2)]
            for e, p, k in zip(encs, bams, n_al):           # the inputs: the same records as compressed BAM, no tag appended
                t = e.tagged(np.ones(k, np.uint8))
                z = t.deflate()
                z.write(p)
                z.close()
                t.close()
        for e in encs:
            e.close()
        ctx.close()
        del host
        torch.cuda.empty_cache()
        if not a.no_e2e:
            bam_outs = [os.path.join(tmp, f"filtered_{i}.bam") for i in (1, 2)]
            text_outs = [os.path.join(tmp, f"filtered_{i}.sam") for i in (1, 2)]
            io = lambda outs: ["--in1", bams[0], "--in2", bams[1], "--out1", outs[0], "--out2", outs[1]]      # noqa: E731
            e2e = {"filter_bam_s": [], "filter_out_sam_s": []}
            for i in range(a.runs):
                last = i == a.runs - 1
                took, laps = run(["filter", *io(bam_outs)], timing=last, strip=tmp)
                e2e["filter_bam_s"].append(round(took, 3))
                if last:
                    e2e["filter_bam_laps"] = laps
                took, laps = run(["filter", "--out_sam", *io(text_outs)], timing=last, strip=tmp)
                e2e["filter_out_sam_s"].append(round(took, 3))
                if last:
                    e2e["filter_out_sam_laps"] = laps
            e2e["bam_in_bytes"] = sum(os.path.getsize(p) for p in bams)
            e2e["bam_out_bytes"] = sum(os.path.getsize(p) for p in bam_outs)
            e2e["text_out_bytes"] = sum(os.path.getsize(p) for p in text_outs)
            e2e["tmp"] = a.tmp or tempfile.gettempdir()
            out["e2e"] = e2e
    emit(True)


if __name__ == "__main__":
    main()
