#!/usr/bin/env python3
"""What pp_bam_tagged costs on a configs[1]-shaped input: the BAM pair of tools/bam_timing.py (the records of tools/synthjob.py's SAM pair
as uncompressed BAM, one byte array per file, resident in HBM in an allocation of exactly its length), decoded, named and filtered on
the device (BamRecords -> Names -> filter_records), then tagged with the filter's verdicts.  Prints one JSON line, sums over the two files:
  pass_a_ms / scans_ms / pass_b_ms   HIP-event time of k_tag_scan | k_colscan x 2 + k_tag_len x 2 | k_tag_frame (best of --repeat)
  tagged_wall_ms   host clock around pp_bam_tagged: its allocations, the upload of the verdicts and its three read-backs included
  copy_ms          HIP-event time of a plain device-to-device copy of the same arrays, the same visit: the same bytes read once and
                   written once -- the memory-rate yardstick;  pass_b_over_copy = pass_b_ms / copy_ms
  random_verdicts  the three stages once more with --fail-frac of the aligned records failing at random: the job's reads have one
                   alignment each, so the filter itself fails none of them and the appended bytes would go unmeasured
  out_bytes        the two files;  pass_b_gbps = (bam_bytes + out_bytes) over pass B's time
  host_zlib0_ms    the same framing on the host: zlib level 0 and crc32 per 65,280-byte piece of the uncompressed stream, 16 threads
  filter_write_ms  (unless --no-text) pp_filter_write of the equivalent SAM text with the same verdicts, both files, after pp_filter_load
--out FILE writes the line to FILE as well.  Measurement only: no threshold is attached to any of it."""
import argparse
import json
import os
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


def host_frame(u, threads=16):
    """level-0 BGZF of the bytes u on `threads` host threads -> (seconds, bytes made)"""
    def one(at):
        piece = u[at:at + PAYLOAD]
        c = zlib.compressobj(0, zlib.DEFLATED, -15)
        block = b"".join((b"\0" * 18, c.compress(piece), c.flush(), zlib.crc32(piece).to_bytes(4, "little"), len(piece).to_bytes(4, "little")))
        return len(block)
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as pool:
        made = sum(pool.map(one, range(0, len(u), PAYLOAD), chunksize=64))
    return time.perf_counter() - t0, made


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mbp", type=float, default=5.0, help="assembly size (configs[1]: 5)")
    ap.add_argument("--coverage", type=int, default=200)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--low", type=float, default=0.1, help="the filter's low percentile")
    ap.add_argument("--high", type=float, default=99.9, help="the filter's high percentile")
    ap.add_argument("--fail-frac", type=float, default=0.02, help="share of failing records in the second measurement, with random verdicts")
    ap.add_argument("--no-text", action="store_true", help="leave out the pp_filter_write lap (it writes and loads the SAM text)")
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
        print(f"[bam_tag_timing] records [{lo}, {hi}) encoded: {len(b)} bytes", file=sys.stderr, flush=True)
        del b, off
    torch.cuda.synchronize()
    ctx = pp.Context(0)
    # ---- the verdicts: decode, name, filter
    table, recs = pp.Names(ctx), []
    for tb, to, n_bytes, n_rec in files:
        rec = pp.BamRecords(ctx, (tb.data_ptr(), n_bytes), (to.data_ptr(), n_rec), None, pp.MEM_DEVICE)
        table.ids(**rec.names(), mem=pp.MEM_DEVICE, out=rec.read_id_ptr)
        recs.append(rec)
    verdicts = pp.filter_records(ctx, recs[0].raw(), recs[1].raw(), low=a.low, high=a.high, mem=pp.MEM_DEVICE)["pass"]
    for o in recs + [table]:
        o.close()
    print(f"[bam_tag_timing] verdicts: {[int((v == 0).sum()) for v in verdicts]} of {[len(v) for v in verdicts]} fail", file=sys.stderr, flush=True)
    # ---- the tagging
    ctx.set_profiling(1)
    best, u_first = None, None
    for _ in range(max(1, a.repeat)):
        ms, wall, out_bytes, counts = [0.0, 0.0, 0.0], 0.0, 0, []
        for f, (tb, to, n_bytes, n_rec) in enumerate(files):
            t0 = time.perf_counter()
            t = pp.BamTagged(ctx, (tb.data_ptr(), n_bytes), 0, (to.data_ptr(), n_rec), verdicts[f], pp.MEM_DEVICE)
            wall += time.perf_counter() - t0
            ms = [x + y for x, y in zip(ms, t.stage_ms().values())]
            out_bytes += t.n_bytes
            counts.append(t.counts)
            if u_first is None:      # the uncompressed stream of file 1, for the host's framing: the payloads of the blocks
                got = t.host()
                n_blk = t.counts[2]
                u_first = np.concatenate([got[b * (PAYLOAD + 31) + 23:min((b + 1) * (PAYLOAD + 31), len(got) - 28) - 8] for b in range(n_blk)]).tobytes()
                del got
            t.close()
        if best is None or ms[2] < best["pass_b_ms"]:
            best = {"pass_a_ms": round(ms[0], 4), "scans_ms": round(ms[1], 4), "pass_b_ms": round(ms[2], 4), "tagged_wall_ms": round(wall * 1e3, 3),
                    "out_bytes": out_bytes, "passed": sum(c[0] for c in counts), "failed": sum(c[1] for c in counts), "blocks": sum(c[2] for c in counts)}
    # the same with verdicts that fail records (the synthetic reads have one alignment each: the filter fails none of them)
    rng = np.random.default_rng(a.seed)
    some_fail = [(rng.random(len(v)) >= a.fail_frac).astype(np.uint8) for v in verdicts]
    with_fails = None
    for _ in range(max(1, a.repeat)):
        ms, failed = [0.0, 0.0, 0.0], 0
        for f, (tb, to, n_bytes, n_rec) in enumerate(files):
            t = pp.BamTagged(ctx, (tb.data_ptr(), n_bytes), 0, (to.data_ptr(), n_rec), some_fail[f], pp.MEM_DEVICE)
            ms = [x + y for x, y in zip(ms, t.stage_ms().values())]
            failed += t.counts[1]
            t.close()
        if with_fails is None or ms[2] < with_fails["pass_b_ms"]:
            with_fails = {"fail_frac": a.fail_frac, "failed": failed, "pass_a_ms": round(ms[0], 4), "scans_ms": round(ms[1], 4), "pass_b_ms": round(ms[2], 4)}
    ctx.set_profiling(0)
    # ---- the yardstick: a device-to-device copy of the same arrays
    copy_ms = None
    dsts = [torch.empty_like(tb) for tb, _, _, _ in files]
    for _ in range(max(2, a.repeat + 1)):      # (the first round warms up)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for d, (tb, _, _, _) in zip(dsts, files):
            d.copy_(tb)
        e1.record()
        torch.cuda.synchronize()
        took = e0.elapsed_time(e1)
        copy_ms = took if copy_ms is None else min(copy_ms, took)
    del dsts
    bam_bytes = sum(f[2] for f in files)
    out = {"input": f"{a.mbp:g} Mbp x {a.coverage}, {n} records in two files as uncompressed BAM (seed {a.seed})", "records": int(n), "filter_low_high": [a.low, a.high], "bam_bytes": bam_bytes, **best,
           "copy_ms": round(copy_ms, 4), "pass_b_over_copy": round(best["pass_b_ms"] / copy_ms, 2),
           "pass_b_gbps": round((bam_bytes + best["out_bytes"]) / 1e9 / (best["pass_b_ms"] / 1e3), 1), "copy_gbps": round(2 * bam_bytes / 1e9 / (copy_ms / 1e3), 1),
           "random_verdicts": dict(with_fails, pass_b_over_copy=round(with_fails["pass_b_ms"] / copy_ms, 2))}
    # ---- the host's framing of the same stream (file 1 measured, scaled to both by their bytes)
    took, _ = host_frame(u_first)
    out["host_zlib0_ms"] = round(took * 1e3 * (best["out_bytes"] / (len(u_first) + 31 * ((len(u_first) + PAYLOAD - 1) // PAYLOAD) + 28)), 1)
    out["host_zlib0_note"] = "file 1 framed on 16 threads, scaled to both files by their bytes"
    del u_first

    def emit(final):
        line = json.dumps(out)
        if final:
            print(line)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
    emit(False)      # (the device's figures are on disk before the text lap starts)
    if not a.no_text:
        if synthjob.samgen_lib() is None:
            out["filter_write_ms"] = "skipped: tools/_build/libsamgen.so is missing"
        else:
            with tempfile.TemporaryDirectory(prefix="pp_bam_tag_", dir=os.environ.get("TMPDIR", "/tmp")) as tmp:
                _, sams = synthjob.write_sam_pair(job, tmp, qual=True)
                loaded = pp.FilterLoaded(sams[0], sams[1])
                assert [c[0] for c in loaded.counts] == [len(v) for v in verdicts], "the text has the aligned records of the BAM"
                t0 = time.perf_counter()
                for f in range(2):
                    loaded.write(f, verdicts[f], os.path.join(tmp, f"filtered_{f + 1}.sam"))
                out["filter_write_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                out["sam_text_bytes"] = sum(os.path.getsize(s) for s in sams)
                loaded.close()
    emit(True)
    ctx.close()


if __name__ == "__main__":
    main()
