#!/usr/bin/env python3
"""What pp_bam_sort and pp_bam_tagged_head cost on a configs[1]-shaped input: the records of tools/synthjob.py's SAM pair as
uncompressed BAM behind a one-reference header (tools/bam_timing.py's encoder), one byte array per file, resident in HBM.  The reads
come in read order, so every record moves.  Prints one JSON line, sums over the two files, best of --repeat by the stage in bold:
  sort: keys_ms / sort_ms / gather_ms    HIP-event time of k_bs_key | the radix passes | k_bs_gather and the verdict map (**sort_ms**)
  sort_wall_ms                           host clock around pp_bam_sort: its allocations, the header's download and its read-backs
  regroup_sort_ms                        pp_batch_regroup's sort stage on the same number of records (32-bit keys, all distinct ids:
                                         as many passes as the count has bytes) -- the same kernels, the other key
  tagged_sorted: pass_a / scans / pass_b pp_bam_tagged_head through pp_bam_sorted_rec_off, the carried verdicts and the new header
  tagged_file_order: ...                 pp_bam_tagged on the same records in file order (**pass_b_ms** of each)
  index: scans / records / chunks / linear   pp_bam_index on the sorted records over the compressed file's block offsets (device),
                                         stage by stage (**the sum**), index_wall_ms on the host's clock, bai_bytes
  copy_ms                                a plain device-to-device copy of the byte arrays: the memory-rate yardstick
  filter_e2e                             (unless --no-e2e) bin/polypolish filter, BAM pair (level 6) -> BAM pair, as a child process on
                                         files in a warm page cache: one warm-up each, then --e2e-repeat rounds that ALTERNATE plain |
                                         --sort_out | --sort_out --out_bai; wall seconds, median and best of each; the outputs' bytes
--out FILE writes the line to FILE as well (profiles/bam_sort_timing.json).  Measurement only: no threshold is attached to any of it."""
import argparse
import json
import os
import struct
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
from bam_timing import encode_bam  # noqa: E402


def header_for(length):
    text = b"@HD\tVN:1.6\tSO:unsorted\n"
    return b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", 1) + struct.pack("<i", 9) + b"contig_1\0" + struct.pack("<i", length)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mbp", type=float, default=5.0, help="assembly size (configs[1]: 5)")
    ap.add_argument("--coverage", type=int, default=200)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--fail-frac", type=float, default=0.02, help="share of the aligned records that fail, at random")
    ap.add_argument("--no-e2e", action="store_true", help="leave out the filter runs (they compress and write the BAM pair)")
    ap.add_argument("--e2e-repeat", type=int, default=5)
    ap.add_argument("--out", help="also write the JSON line to this file")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    job = synthjob.make_job(dev, contig_lens=(int(a.mbp * 1e6),), coverage=a.coverage, seed=a.seed, pairs=True, unaligned_frac=1e-3)
    torch.cuda.synchronize()
    S = job["sam"]
    n, half = S["n"], S["half"]
    head = header_for(int(a.mbp * 1e6))
    files = []
    tmp = None if a.no_e2e else tempfile.mkdtemp(prefix="bam_sort_timing_", dir=os.environ.get("TMPDIR", "/tmp"))
    bams = []
    for lo, hi in ((0, half), (half, n)):
        b, off = encode_bam(S, lo, hi)
        b = np.concatenate([np.frombuffer(head, np.uint8), b])
        if tmp:      # the same bytes as a BAM file for the command
            import bgzf_timing
            z, _, _ = bgzf_timing.compress(b, 6)
            bams.append(os.path.join(tmp, f"reads_{len(bams) + 1}.bam"))
            z.tofile(bams[-1])
            del z
        off = off + np.uint64(len(head))
        flag = b[off.astype(np.int64) + 18]
        files.append((torch.from_numpy(b).to(dev), torch.from_numpy(off.view(np.int64)).to(dev), len(b), len(off), int(((flag & 4) == 0).sum())))
        print(f"[bam_sort_timing] records [{lo}, {hi}) encoded: {len(b)} bytes", file=sys.stderr, flush=True)
        del b, off
    torch.cuda.synchronize()
    rng = np.random.default_rng(a.seed)
    verdicts = [(rng.random(f[4]) >= a.fail_frac).astype(np.uint8) for f in files]
    ctx = pp.Context(0)
    ctx.set_profiling(1)
    at = len(head)

    def best_of(run, key):
        best = None
        for _ in range(max(1, a.repeat)):
            got = run()
            if best is None or got[key] < best[key]:
                best = got
        return best

    def sort_lap():
        ms, wall, moved, unplaced = [0.0] * 3, 0.0, 0, 0
        for tb, to, n_bytes, n_rec, _ in files:
            t0 = time.perf_counter()
            s = pp.BamSorted(ctx, (tb.data_ptr(), n_bytes), at, (to.data_ptr(), n_rec), pp.MEM_DEVICE)
            wall += time.perf_counter() - t0
            ms = [x + y for x, y in zip(ms, s.stage_ms().values())]
            moved, unplaced = moved + s.counts()[0], unplaced + s.counts()[1]
            s.close()
        return {"keys_ms": round(ms[0], 4), "sort_ms": round(ms[1], 4), "gather_ms": round(ms[2], 4), "sort_wall_ms": round(wall * 1e3, 3), "moved": moved, "unplaced": unplaced}

    def tag_lap(sort_first):
        ms, out_bytes = [0.0] * 3, 0
        for f, (tb, to, n_bytes, n_rec, _) in enumerate(files):
            if sort_first:
                s = pp.BamSorted(ctx, (tb.data_ptr(), n_bytes), at, (to.data_ptr(), n_rec), pp.MEM_DEVICE)
                t = pp.BamTagged(ctx, (tb.data_ptr(), n_bytes), at, (s.rec_off_ptr, s.n_rec), s.carry_pass(verdicts[f]), pp.MEM_DEVICE, head=s.head)
                s.close()
            else:
                t = pp.BamTagged(ctx, (tb.data_ptr(), n_bytes), at, (to.data_ptr(), n_rec), verdicts[f], pp.MEM_DEVICE)
            ms = [x + y for x, y in zip(ms, t.stage_ms().values())]
            out_bytes += t.n_bytes
            t.close()
        return {"pass_a_ms": round(ms[0], 4), "scans_ms": round(ms[1], 4), "pass_b_ms": round(ms[2], 4), "out_bytes": out_bytes}

    def index_lap():
        ms, wall, size = [0.0] * 4, 0.0, 0
        for f, (tb, to, n_bytes, n_rec, _) in enumerate(files):
            s = pp.BamSorted(ctx, (tb.data_ptr(), n_bytes), at, (to.data_ptr(), n_rec), pp.MEM_DEVICE)
            v = s.carry_pass(verdicts[f])
            t = pp.BamTagged(ctx, (tb.data_ptr(), n_bytes), at, (s.rec_off_ptr, s.n_rec), v, pp.MEM_DEVICE, head=s.head)
            z = t.deflate()
            t0 = time.perf_counter()
            x = pp.BamIndex(ctx, (tb.data_ptr(), n_bytes), len(s.head), (s.rec_off_ptr, s.n_rec), v, 1, (z.blk_off_ptr, z.n_blocks), pp.MEM_DEVICE)
            wall += time.perf_counter() - t0
            ms = [p + q for p, q in zip(ms, x.stage_ms().values())]
            size += len(x.bytes)
            for o in (z, t, s):
                o.close()
        return {"scans_ms": round(ms[0], 4), "records_ms": round(ms[1], 4), "chunks_ms": round(ms[2], 4), "linear_ms": round(ms[3], 4),
                "index_ms": round(sum(ms), 4), "index_wall_ms": round(wall * 1e3, 3), "bai_bytes": size}

    def regroup_lap():
        total = 0.0
        for _, _, _, n_rec, _ in files:
            z32, z64 = torch.zeros(n_rec, dtype=torch.int32, device=dev), torch.zeros(n_rec, dtype=torch.int64, device=dev)
            ids = torch.arange(n_rec, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            ptrs = {k: (ids if k == "read_id" else z64 if dt == np.uint64 else z32).data_ptr() for k, dt in pp.RAW_FIELDS}
            ptrs.update(n_rec=n_rec, seq_bytes=0, n_cig_total=0)
            g = pp.regroup_records(ctx, ptrs, mem=pp.MEM_DEVICE)
            total += g.stage_ms()["sort"]
            g.close()
        return {"regroup_sort_ms": round(total, 4)}

    out = {"input": f"{a.mbp:g} Mbp x {a.coverage}, {n} records in two files as uncompressed BAM (seed {a.seed})", "records": int(n),
           "bam_bytes": sum(f[2] for f in files), "fail_frac": a.fail_frac}
    out["sort"] = best_of(sort_lap, "sort_ms")
    out.update(best_of(regroup_lap, "regroup_sort_ms"))
    out["tagged_sorted"] = best_of(lambda: tag_lap(True), "pass_b_ms")
    out["tagged_file_order"] = best_of(lambda: tag_lap(False), "pass_b_ms")
    out["index"] = best_of(index_lap, "index_ms")
    ctx.set_profiling(0)
    copy_ms = None
    dsts = [torch.empty_like(f[0]) for f in files]
    for _ in range(max(2, a.repeat + 1)):      # (the first round warms up)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for d, f in zip(dsts, files):
            d.copy_(f[0])
        e1.record()
        torch.cuda.synchronize()
        took = e0.elapsed_time(e1)
        copy_ms = took if copy_ms is None else min(copy_ms, took)
    out["copy_ms"] = round(copy_ms, 4)
    ctx.close()
    del files, dsts, job, S
    torch.cuda.empty_cache()      # (the child processes are the only users of the device from here on)

    def emit():
        line = json.dumps(out)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return line
    emit()      # (the device's figures are on disk before the command runs start)
    if tmp:
        exe = os.path.join(ROOT, "bin", "polypolish")
        modes = {"plain": [], "sort_out": ["--sort_out"], "sort_out_bai": ["--sort_out", "--out_bai"]}
        outs = {m: [os.path.join(tmp, f"{m}_{i}.bam") for i in (1, 2)] for m in modes}

        def once(m):
            argv = [exe, "filter", *modes[m], "--in1", bams[0], "--in2", bams[1], "--out1", outs[m][0], "--out2", outs[m][1]]
            t0 = time.perf_counter()
            r = subprocess.run(argv, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=600)
            took = time.perf_counter() - t0
            if r.returncode != 0:
                raise RuntimeError(f"{' '.join(argv)} ended with {r.returncode}: {r.stderr.decode()[-600:]}")
            return took
        try:
            for m in modes:
                once(m)      # warm-up
            walls = {m: [] for m in modes}
            for _ in range(max(1, a.e2e_repeat)):      # alternating: a drift of the machine meets every mode alike
                for m in modes:
                    walls[m].append(once(m))
            size = os.path.getsize
            out["filter_e2e"] = {"input_bytes": [size(x) for x in bams], "rounds": max(1, a.e2e_repeat)}
            for m in modes:
                w = sorted(walls[m])
                out["filter_e2e"][m] = {"wall_s": {"median": round(w[len(w) // 2], 3), "best": round(w[0], 3)}, "out_bytes": [size(x) for x in outs[m]]}
            out["filter_e2e"]["sort_out_bai"]["bai_bytes"] = [size(x + ".bai") for x in outs["sort_out_bai"]]
        finally:
            import shutil
            shutil.rmtree(tmp, ignore_errors=True)
    print(emit())


if __name__ == "__main__":
    main()
