#!/usr/bin/env python3
"""What the device walk over the block_size chain costs on the input of tools/bgzf_timing.py: configs[1]'s records as BAM bytes (two
files), deflated at level 6 into BGZF blocks, inflated on the device by pp_bgzf_inflate.  Prints one JSON line:
  walk_ms                HIP-event time of pp_bam_walk_device over the inflated bytes by stage (the chunk tables | the groups, the chain and
                         the replay | the scan and the offsets) and in all, summed over the two files: best and median of --repeat runs
                         behind a warm-up run
  bgzf_bam_walk_wall_ms  wall time around pp_bgzf_bam_walk (the whole call, as tools/bgzf_timing.py takes its bam_walk_wall_ms), summed
                         over the two files: the first call, then best and median of --repeat
  inflate_ms             the inflate's event time on the same run, and walk_over_inflate = walk_ms.total.best / inflate_ms
  stats                  along the true chain, summed: chunks on it, entered through a zone table, on the slow path, passed through;
                         slow_chunks = the third
  equal                  n_rec, end and every offset are pp_bam_walk's on the same bytes
  parent_bam_walk_wall_ms, wall_parent_over_device   with --parent-json FILE: bam_walk_wall_ms of tools/bgzf_timing.py run at the parent
                         commit (its --out file), on the same machine in the same visit, and its ratio to the first call here
--out FILE writes the line to FILE as well.  Measurement only: no threshold is attached to any of it."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def spread(values):
    v = sorted(values)
    return {"best": round(v[0], 3), "median": round(v[len(v) // 2], 3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mbp", type=float, default=5.0, help="assembly size (configs[1]: 5)")
    ap.add_argument("--coverage", type=int, default=200)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--parent-json", help="the --out file of tools/bgzf_timing.py run at the parent commit")
    ap.add_argument("--out", help="also write the JSON line to this file")
    a = ap.parse_args()
    import torch

    import bam_timing
    import bgzf_timing
    import polypolish_amd as pp
    import synthjob
    log = lambda msg: print(f"[bam_walk_timing] {msg}", file=sys.stderr, flush=True)     # noqa: E731
    dev = torch.device("cuda:0")
    job = synthjob.make_job(dev, contig_lens=(int(a.mbp * 1e6),), coverage=a.coverage, seed=a.seed, pairs=True, unaligned_frac=1e-3)
    torch.cuda.synchronize()
    S = job["sam"]
    n, half = S["n"], S["half"]
    plain = [bam_timing.encode_bam(S, lo, hi)[0] for lo, hi in ((0, half), (half, n))]
    del job, S
    torch.cuda.empty_cache()
    log(f"{n} records encoded: {sum(len(b) for b in plain)} bytes")
    ctx = pp.Context(0)
    ctx.set_profiling(1)
    c, z, g = pp.bam_walk_geometry()
    out = {"input": f"{a.mbp:g} Mbp x {a.coverage}, {n} records in two files as BAM bytes (seed {a.seed}), BGZF blocks of {bgzf_timing.BLOCK} bytes, level 6",
           "inflated_bytes": int(sum(len(b) for b in plain)), "records": int(n), "repeat": a.repeat, "geometry": {"chunk": c, "zone": z, "group": g}}
    inflated, inflate_ms = [], 0.0
    for b in plain:
        zb, off, _ = bgzf_timing.compress(b, 6)
        tz, to = torch.from_numpy(zb.copy()).to(dev), torch.from_numpy(off.view(np.int64).copy()).to(dev)
        torch.cuda.synchronize()
        zf = pp.Bgzf(ctx, (tz.data_ptr(), tz.numel()), (to.data_ptr(), to.numel()), mem=pp.MEM_DEVICE)
        inflate_ms += zf.stage_ms()["inflate"]
        inflated.append(zf)
        del tz, to
    log(f"inflated: {inflate_ms:.2f} ms")
    walls, stages = [], []
    for it in range(a.repeat + 1):          # (the first run is reported on its own: it is what a caller's one call costs)
        wall, ms = 0.0, {"tables": 0.0, "chain": 0.0, "offsets": 0.0}
        for zf in inflated:
            t0 = time.perf_counter()
            zf.bam_walk(0)
            wall += (time.perf_counter() - t0) * 1e3
            o = pp.bam_walk_device(ctx, (zf.bytes_ptr, zf.n_bytes), 0, pp.MEM_DEVICE)
            for k, v in o.stage_ms().items():
                ms[k] += v
            o.close()
        walls.append(wall)
        if it:
            stages.append(ms)
    equal, stats, records = True, {"chain": 0, "zone": 0, "slow": 0, "pass": 0}, 0
    for zf, b in zip(inflated, plain):
        want, want_end = pp.bam_walk(b)
        o = pp.bam_walk_device(ctx, (zf.bytes_ptr, zf.n_bytes), 0, pp.MEM_DEVICE)
        equal = equal and (o.n_rec, o.end) == (len(want), want_end) and np.array_equal(o.host(), want)
        for k, v in o.stats().items():
            stats[k] += v
        records += o.n_rec
        o.close()
        zf.close()
    out["walk_ms"] = {k: spread([s[k] for s in stages]) for k in ("tables", "chain", "offsets")}
    out["walk_ms"]["total"] = spread([sum(s.values()) for s in stages])
    out["bgzf_bam_walk_wall_ms"] = dict(spread(walls[1:]), first=round(walls[0], 3))
    out["inflate_ms"] = round(inflate_ms, 3)
    out["walk_over_inflate"] = round(out["walk_ms"]["total"]["best"] / inflate_ms, 3)
    out.update({"stats": stats, "slow_chunks": stats["slow"], "walked_records": int(records), "equal": bool(equal)})
    if a.parent_json:
        with open(a.parent_json) as f:
            parent = json.loads(f.readline())
        out["parent_bam_walk_wall_ms"] = parent["level_6"]["bam_walk_wall_ms"]
        out["wall_parent_over_device"] = round(out["parent_bam_walk_wall_ms"] / out["bgzf_bam_walk_wall_ms"]["first"], 1)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
