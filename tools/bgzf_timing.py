#!/usr/bin/env python3
"""What pp_bgzf_inflate costs on a configs[1]-shaped input: the BAM bytes of tools/bam_timing.py's encoder (two files), cut into
0xff00-byte blocks as htslib cuts them, deflated by zlib at level 6 (and once more at level 1) and wrapped as BGZF, the compressed
bytes resident in HBM (an allocation of exactly their length).  Prints one JSON line; per level:
  inflate_ms / crc_ms    HIP-event time of the stages (headers + scan + k_bgzf_inflate | k_bgzf_crc), summed over the two files: best
                         and median of --repeat runs behind a warm-up run
  compressed_gbps / inflated_gbps    the bytes in and out over inflate + crc (best)
  host_zlib_ms           the same blocks inflated by zlib.decompress in a thread pool (it releases the GIL) of 1 and of 16 threads:
                         wall time, best of two -- the comparison that matters is the device stages against the 16 threads
and once (level 6):
  h2d_ms                 the copy of the compressed bytes from pinned host memory (events), for comparison
  bam_walk_staging_ms    the kernels of pp_bgzf_bam_walk (events; until the device walk existed: the copies of its staging), and
                         bam_walk_wall_ms around the whole call.  tools/bam_walk_timing.py takes the walk apart
  bam_records_ms         pp_bam_records on the inflated bytes and the walked offsets (the next link)
  equal                  the inflated bytes are the encoder's bytes
--out FILE writes the line to FILE as well.  Measurement only: no threshold is attached to any of it."""
import argparse
import json
import os
import struct
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

BLOCK = 0xff00
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def log(msg):
    print(f"[bgzf_timing] {msg}", file=sys.stderr, flush=True)


def bgzf_block(piece, level):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    raw = c.compress(piece) + c.flush()
    total = 18 + len(raw) + 8
    assert total <= 65536
    return struct.pack("<4BI2BH2sHH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6, b"BC", 2, total - 1) + raw + struct.pack("<II", zlib.crc32(piece), len(piece))


def compress(data, level, threads=16):
    """np.uint8 -> (BGZF bytes: np.uint8, blk_off: np.uint64, [raw DEFLATE streams]); the EOF block at the end"""
    view = memoryview(data)
    with ThreadPoolExecutor(threads) as pool:
        blocks = list(pool.map(lambda at: bgzf_block(view[at:at + BLOCK], level), range(0, len(data), BLOCK)))
    blocks.append(EOF_BLOCK)
    off = np.cumsum([0] + [len(b) for b in blocks[:-1]]).astype(np.uint64)
    return np.frombuffer(b"".join(blocks), np.uint8), off, [b[18:-8] for b in blocks]


def host_inflate_ms(raws, threads):
    best = None
    for _ in range(2):
        t0 = time.perf_counter()
        with ThreadPoolExecutor(threads) as pool:
            n = sum(pool.map(lambda r: len(zlib.decompress(r, -15)), raws, chunksize=64))
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
    return round(best, 2), n


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mbp", type=float, default=5.0, help="assembly size (configs[1]: 5)")
    ap.add_argument("--coverage", type=int, default=200)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--out", help="also write the JSON line to this file")
    a = ap.parse_args()
    import torch

    import bam_timing
    import polypolish_amd as pp
    import synthjob
    dev = torch.device("cuda:0")
    job = synthjob.make_job(dev, contig_lens=(int(a.mbp * 1e6),), coverage=a.coverage, seed=a.seed, pairs=True, unaligned_frac=1e-3)
    torch.cuda.synchronize()
    S = job["sam"]
    n, half = S["n"], S["half"]
    plain = []
    for lo, hi in ((0, half), (half, n)):
        b, _ = bam_timing.encode_bam(S, lo, hi)
        plain.append(b)
        log(f"records [{lo}, {hi}) encoded: {len(b)} bytes")
    del job, S
    torch.cuda.empty_cache()
    ctx = pp.Context(0)
    ctx.set_profiling(1)
    out = {"input": f"{a.mbp:g} Mbp x {a.coverage}, {n} records in two files as BAM bytes (seed {a.seed}), BGZF blocks of {BLOCK} bytes",
           "inflated_bytes": int(sum(len(b) for b in plain)), "repeat": a.repeat}
    for level in (6, 1):
        files, raws = [], []
        for b in plain:
            z, off, r = compress(b, level)
            files.append((z, off))
            raws += r
        log(f"level {level}: {sum(len(z) for z, _ in files)} compressed bytes in {sum(len(o) for _, o in files)} blocks")
        res = {"compressed_bytes": int(sum(len(z) for z, _ in files)), "blocks": int(sum(len(o) for _, o in files))}
        on_dev, h2d = [], []
        for z, off in files:
            pinned = torch.from_numpy(z.copy()).pin_memory()
            best = None
            for _ in range(3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                tz = pinned.to(dev, non_blocking=True)
                e1.record()
                torch.cuda.synchronize()
                best = e0.elapsed_time(e1) if best is None else min(best, e0.elapsed_time(e1))
            h2d.append(best)
            on_dev.append((tz, torch.from_numpy(off.view(np.int64).copy()).to(dev)))
            del pinned
        torch.cuda.synchronize()
        runs = []
        for it in range(a.repeat + 1):          # (the first run warms up)
            ms = {"inflate": 0.0, "crc": 0.0}
            for tz, to in on_dev:
                z = pp.Bgzf(ctx, (tz.data_ptr(), tz.numel()), (to.data_ptr(), to.numel()), mem=pp.MEM_DEVICE)
                st = z.stage_ms()
                ms["inflate"] += st["inflate"]
                ms["crc"] += st["crc"]
                z.close()
            if it:
                runs.append(ms)
        for k in ("inflate", "crc"):
            v = sorted(r[k] for r in runs)
            res[f"{k}_ms"] = {"best": round(v[0], 3), "median": round(v[len(v) // 2], 3)}
        both = min(r["inflate"] + r["crc"] for r in runs)
        res["compressed_gbps"] = round(res["compressed_bytes"] / 1e9 / (both / 1e3), 2)
        res["inflated_gbps"] = round(out["inflated_bytes"] / 1e9 / (both / 1e3), 2)
        log(f"level {level}: device {res['inflate_ms']} + {res['crc_ms']} ms")
        res["host_zlib_ms"] = {}
        for threads in (1, 16):
            res["host_zlib_ms"][str(threads)], got = host_inflate_ms(raws, threads)
            assert got == out["inflated_bytes"]
        log(f"level {level}: host zlib {res['host_zlib_ms']} ms")
        if level == 6:
            res["h2d_ms"] = round(sum(h2d), 3)
            walk_ms = walk_wall = rec_ms = 0.0
            equal = True
            for (tz, to), b in zip(on_dev, plain):
                z = pp.Bgzf(ctx, (tz.data_ptr(), tz.numel()), (to.data_ptr(), to.numel()), mem=pp.MEM_DEVICE)
                equal = equal and z.n_bytes == len(b) and np.array_equal(z.host(), b)
                t0 = time.perf_counter()
                ptr, n_rec, end = z.bam_walk(0)
                walk_wall += (time.perf_counter() - t0) * 1e3
                assert end == len(b)
                walk_ms += z.stage_ms()["staging"]
                rec = pp.BamRecords(ctx, (z.bytes_ptr, z.n_bytes), (ptr, n_rec), None, pp.MEM_DEVICE)
                rec_ms += rec.kernel_ms()
                rec.close()
                z.close()
            res.update({"bam_walk_staging_ms": round(walk_ms, 2), "bam_walk_wall_ms": round(walk_wall, 1), "bam_records_ms": round(rec_ms, 3), "equal": bool(equal)})
        out[f"level_{level}"] = res
        del on_dev
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
