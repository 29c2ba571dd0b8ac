#!/usr/bin/env python3
"""What pp_bam_out_deflate costs on a configs[1]-shaped input: the BAM pair of tools/bam_tag_timing.py (decoded, named and filtered on
the device, tagged with the filter's verdicts by pp_bam_tagged), then each level-0 file compressed on the device.  Prints one JSON
line, sums over the two files:
  pieces_ms / scan_ms / place_ms   HIP-event time of k_df_piece | k_colscan | k_df_place: one warm-up run, then best and median of --repeat
  deflate_wall_ms   host clock around pp_bam_out_deflate (best): its allocations and two read-backs included
  in_bytes, out_bytes, ratio, blocks   the uncompressed streams, the compressed files, and the blocks by form (stored, fixed, dynamic)
  deflate_gbps      in_bytes over the best pieces_ms + scan_ms + place_ms
  inflate_ms        pp_bgzf_inflate of the compressed files from device memory with the objects' own blk_off (kernel time, best of 3)
  tagged_pass_b_ms  pp_bam_tagged's pass B, which made the level-0 files, the same visit
  write_level0_ms / write_deflated_ms   pp_bam_out_write of the level-0 files against pp_bgzf_out_write of the compressed ones
  host_zlib         zlib levels 1 and 6 per 65,280-byte piece of file 1's stream on 16 host threads, time and size scaled to both files
--out FILE writes the line to FILE as well.  Measurement only: no threshold is attached to any of it."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import polypolish_amd as pp  # noqa: E402
import synthjob  # noqa: E402
from bam_timing import encode_bam  # noqa: E402

PAYLOAD = 65280


def host_deflate(u, level, threads=16):
    """raw DEFLATE and crc32 per piece of the bytes u on `threads` host threads -> (seconds, bytes of the BGZF file that makes)"""
    def one(at):
        piece = u[at:at + PAYLOAD]
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        zlib.crc32(piece)
        return 26 + len(c.compress(piece)) + len(c.flush())
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as pool:
        made = sum(pool.map(one, range(0, len(u), PAYLOAD), chunksize=64))
    return time.perf_counter() - t0, made + 28


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mbp", type=float, default=5.0, help="assembly size (configs[1]: 5)")
    ap.add_argument("--coverage", type=int, default=200)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--out", help="also write the JSON line to this file")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    job = synthjob.make_job(dev, contig_lens=(int(a.mbp * 1e6),), coverage=a.coverage, seed=a.seed, pairs=True, unaligned_frac=1e-3)
    torch.cuda.synchronize()
    S = job["sam"]
    n, half = S["n"], S["half"]
    files = []
    for lo, hi in ((0, half), (half, n)):
        b, off = encode_bam(S, lo, hi)
        files.append((torch.from_numpy(b).to(dev), torch.from_numpy(off.view(np.int64)).to(dev), len(b), len(off)))
        print(f"[bgzf_deflate_timing] records [{lo}, {hi}) encoded: {len(b)} bytes", file=sys.stderr, flush=True)
        del b, off
    torch.cuda.synchronize()
    ctx = pp.Context(0)
    table, recs = pp.Names(ctx), []
    for tb, to, n_bytes, n_rec in files:
        rec = pp.BamRecords(ctx, (tb.data_ptr(), n_bytes), (to.data_ptr(), n_rec), None, pp.MEM_DEVICE)
        table.ids(**rec.names(), mem=pp.MEM_DEVICE, out=rec.read_id_ptr)
        recs.append(rec)
    verdicts = pp.filter_records(ctx, recs[0].raw(), recs[1].raw(), mem=pp.MEM_DEVICE)["pass"]
    for o in recs + [table]:
        o.close()
    ctx.set_profiling(1)
    tagged = [pp.BamTagged(ctx, (tb.data_ptr(), n_bytes), 0, (to.data_ptr(), n_rec), verdicts[f], pp.MEM_DEVICE) for f, (tb, to, n_bytes, n_rec) in enumerate(files)]
    pass_b = sum(t.stage_ms()["pass_b"] for t in tagged)
    in_bytes = sum(t.n_bytes - 31 * t.counts[2] - 28 for t in tagged)
    print(f"[bgzf_deflate_timing] tagged: {[t.n_bytes for t in tagged]} bytes", file=sys.stderr, flush=True)
    # ---- the compression: one warm-up run, then --repeat runs
    runs, walls, kept = [], [], None
    for it in range(1 + max(1, a.repeat)):
        ms, wall, made = [0.0, 0.0, 0.0], 0.0, []
        for t in tagged:
            t0 = time.perf_counter()
            z = t.deflate()
            wall += time.perf_counter() - t0
            ms = [x + y for x, y in zip(ms, z.stage_ms().values())]
            made.append(z)
        if it:
            runs.append(ms)
            walls.append(wall * 1e3)
        if it == max(1, a.repeat):
            kept = made
        else:
            for z in made:
                z.close()
    totals = [sum(r) for r in runs]
    best = runs[totals.index(min(totals))]
    out = {"input": f"{a.mbp:g} Mbp x {a.coverage}, {n} records in two files as uncompressed BAM (seed {a.seed}), tagged by pp_bam_tagged", "records": int(n),
           "in_bytes": in_bytes, "level0_bytes": sum(t.n_bytes for t in tagged), "out_bytes": sum(z.n_bytes for z in kept),
           "ratio": round(sum(z.n_bytes for z in kept) / in_bytes, 4), "blocks": [sum(z.counts[i] for z in kept) for i in range(3)],
           "repeat": len(runs), "pieces_ms": round(best[0], 3), "scan_ms": round(best[1], 3), "place_ms": round(best[2], 3),
           "kernels_best_ms": round(min(totals), 3), "kernels_median_ms": round(statistics.median(totals), 3),
           "pieces_median_ms": round(statistics.median(r[0] for r in runs), 3),
           "deflate_wall_ms": round(min(walls), 2), "deflate_wall_median_ms": round(statistics.median(walls), 2),
           "deflate_gbps": round(in_bytes / 1e9 / (min(totals) / 1e3), 2), "tagged_pass_b_ms": round(pass_b, 3)}
    # ---- the way back: pp_bgzf_inflate of the compressed files, from device memory
    inflate = None
    for _ in range(3):
        took = 0.0
        for z in kept:
            back = pp.Bgzf(ctx, (z.bytes_ptr, z.n_bytes), (z.blk_off_ptr, z.n_blocks), mem=pp.MEM_DEVICE)
            ms = back.stage_ms()
            took += ms["inflate"] + ms["crc"]
            assert back.n_bytes == z_in(tagged[kept.index(z)])
            back.close()
        inflate = took if inflate is None else min(inflate, took)
    out["inflate_ms"] = round(inflate, 3)
    ctx.set_profiling(0)
    # ---- the files on disk
    with tempfile.TemporaryDirectory(prefix="pp_bgzf_deflate_", dir=os.environ.get("TMPDIR", "/tmp")) as tmp:
        for key, objs in (("write_level0_ms", tagged), ("write_deflated_ms", kept)):
            t0 = time.perf_counter()
            for f, o in enumerate(objs):
                o.write(os.path.join(tmp, f"{key}_{f}.bam"))
            out[key] = round((time.perf_counter() - t0) * 1e3, 1)
    # ---- the host's zlib on the same stream (file 1 measured, scaled to both by their bytes)
    got = tagged[0].host()
    n_blk = tagged[0].counts[2]
    u = np.concatenate([got[b * (PAYLOAD + 31) + 23:min((b + 1) * (PAYLOAD + 31), len(got) - 28) - 8] for b in range(n_blk)]).tobytes()
    del got
    scale = in_bytes / len(u)
    out["host_zlib"] = {}
    for level in (1, 6):
        took, made = host_deflate(u, level)
        out["host_zlib"][f"level_{level}"] = {"ms": round(took * 1e3 * scale, 1), "bytes": int(made * scale)}
    out["host_zlib"]["note"] = "file 1 on 16 threads, scaled to both files by their bytes"
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    for o in kept + tagged:
        o.close()
    ctx.close()


def z_in(t):
    return t.n_bytes - 31 * t.counts[2] - 28


if __name__ == "__main__":
    main()
