#!/usr/bin/env python3
"""What pp_batch_regroup costs on a configs[1]-shaped input: the records of tools/synthjob.py's SAM pair (make_job(pairs=True)), each
file's records coordinate-sorted on the host -- stable by (contig, ref_start), the unaligned ones last -- and encoded to uncompressed
BAM bytes (tools/bam_timing.py's encoder), decoded by pp_bam_records with their QNAMEs interned by pp_names: the raw batches of the
polish driver under --regroup, resident in HBM.  Prints one JSON line, every time the sum over the two files:
  intern_ms / sort_ms / gather_ms   HIP-event time of pp_batch_regroup's stages on the sorted records: the ids' first records | the
                     radix sort of the indices | counts, the gather of the nine arrays and the verdict map
  moved              records that change place;  groups: distinct read ids
  gate_ms            pp_batch_gate's kernels on the regrouped view, the same run: the link behind, the first yardstick
  copy_ms            a device-to-device copy of nine arrays of the per-record arrays' sizes (46 bytes a record, read and written
                     once): the second
  identity_ms        pp_batch_regroup on the name-grouped pair (nothing moves: no gather, the view is the input), by stage
  scattered_ms       the sorted records once more with read_id >> 1 for an id: neighbouring reads become one read of two records that lie
                     wherever the coordinate sort put them, so that nearly every record moves (scattered_moved) -- the sort and the
                     gather at full size, whatever the input's own reads look like.  (configs[1] has no repeats: a read has one
                     record per file, and its sorted files regroup to themselves.)
Every figure is the median of --repeat timed rounds behind one warm-up round; *_spread_ms = max - min over the rounds of the regroup's
total.  --out FILE writes the line to FILE as well.  Measurement only: no threshold is attached to any of it."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import polypolish_amd as pp  # noqa: E402
import bam_timing  # noqa: E402
import synthjob  # noqa: E402

PER_RECORD = ("flag", "read", "contig", "ref_start", "nm", "seq_off", "seq_len", "cig_off", "n_cig")
NINE = (("flag", 2), ("read_id", 8), ("contig", 4), ("ref_start", 4), ("nm", 4), ("seq_off", 8), ("seq_len", 4), ("cig_off", 8), ("n_cig", 4))


def coordinate_sorted(S, lo, hi):
    """the job's records [lo, hi) as a job of their own, stable by (contig, ref_start), unaligned records last"""
    col = lambda k: S[k][lo:hi].cpu().numpy().astype(np.int64)  # noqa: E731
    flag, contig, pos = col("flag"), col("contig"), col("ref_start")
    unal = (flag & 4) != 0
    key = np.where(unal, np.int64(1) << 62, contig * (np.int64(1) << 32) + pos)
    order = torch.from_numpy(np.argsort(key, kind="stable") + lo).to(S["flag"].device)
    out = dict(S)
    for k in PER_RECORD:
        out[k] = S[k][order]
    return out, int(hi - lo)


def decode(ctx, table, S, lo, hi, dev):
    """records [lo, hi) -> (BamRecords with read_id filled in, what it borrows)"""
    b, off = bam_timing.encode_bam(S, lo, hi)
    tb, to = torch.from_numpy(b).to(dev), torch.from_numpy(off.view(np.int64)).to(dev)
    torch.cuda.synchronize()
    rec = pp.BamRecords(ctx, (tb.data_ptr(), len(b)), (to.data_ptr(), len(off)), None, pp.MEM_DEVICE)
    table.ids(**rec.names(), mem=pp.MEM_DEVICE, out=rec.read_id_ptr)
    return rec, (tb, to)


def copy_ms(n_rec):
    """HIP-event time of copying nine arrays of the per-record arrays' sizes device to device"""
    src = [torch.zeros(n_rec * size, dtype=torch.uint8, device="cuda:0") for _, size in NINE]
    dst = [torch.empty_like(x) for x in src]
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for x, y in zip(src, dst):
        y.copy_(x)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mbp", type=float, default=5.0, help="assembly size (configs[1]: 5)")
    ap.add_argument("--coverage", type=int, default=200)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--out", help="also write the JSON line to this file")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    job = synthjob.make_job(dev, contig_lens=(int(a.mbp * 1e6),), coverage=a.coverage, seed=a.seed, pairs=True, unaligned_frac=1e-3)
    torch.cuda.synchronize()
    S = job["sam"]
    n, half = S["n"], S["half"]
    ctx = pp.Context(0)
    ctx.set_profiling(1)
    table = pp.Names(ctx)
    sorted_recs, grouped_recs, keep = [], [], []
    for lo, hi in ((0, half), (half, n)):
        rec, k = decode(ctx, table, S, lo, hi, dev)
        grouped_recs.append(rec)
        keep.append(k)
        S2, m = coordinate_sorted(S, lo, hi)
        rec, k = decode(ctx, table, S2, 0, m, dev)
        sorted_recs.append(rec)
        keep.append(k)
        print(f"[regroup_timing] records [{lo}, {hi}) decoded, name-grouped and coordinate-sorted", file=sys.stderr, flush=True)

    # the sorted files' read ids, halved (torch has no uint64: the ids are small, int64 holds them)
    halved = [torch.from_numpy((ctx.download(rec.raw()["read_id"], rec.n_rec, np.uint64) >> np.uint64(1)).view(np.int64)).to(dev) for rec in sorted_recs]
    torch.cuda.synchronize()
    rounds, scattered = [], []
    moved = groups = 0
    for r in range(max(1, a.repeat) + 1):  # (round 0 warms every shape up)
        row = {"intern": 0.0, "sort": 0.0, "gather": 0.0, "gate": 0.0, "copy": 0.0, "id_intern": 0.0, "id_sort": 0.0, "id_gather": 0.0}
        moved = groups = 0
        for rec, same in zip(sorted_recs, grouped_recs):
            g = pp.regroup_records(ctx, rec.raw(), mem=pp.MEM_DEVICE)
            for k, v in g.stage_ms().items():
                row[k] += v
            ng, nm = g.counts()
            groups, moved = groups + ng, moved + nm
            gated = pp.gate_records(ctx, g.raw(), passed=g.carry_pass(rec.zp), mem=pp.MEM_DEVICE)
            row["gate"] += gated.kernel_ms()
            gated.close()
            g.close()
            row["copy"] += copy_ms(rec.n_rec)
            g = pp.regroup_records(ctx, same.raw(), mem=pp.MEM_DEVICE)
            assert g.counts()[1] == 0, "the name-grouped records regroup to themselves"
            for k, v in g.stage_ms().items():
                row["id_" + k] += v
            g.close()
            raw = dict(rec.raw(), read_id=halved[len(scattered) % 2].data_ptr())
            g = pp.regroup_records(ctx, raw, mem=pp.MEM_DEVICE)
            for k, v in g.stage_ms().items():
                row["sc_" + k] = row.get("sc_" + k, 0.0) + v
            scattered.append(g.counts()[1])
            g.close()
        if r:
            rounds.append(row)
    med = lambda k: round(statistics.median(x[k] for x in rounds), 4)  # noqa: E731
    total = [x["intern"] + x["sort"] + x["gather"] for x in rounds]
    out = {"input": f"{a.mbp:g} Mbp x {a.coverage}, {n} records in two files as uncompressed BAM, coordinate-sorted (seed {a.seed})",
           "records": int(n), "moved": int(moved), "groups": int(groups), "rounds": len(rounds),
           "intern_ms": med("intern"), "sort_ms": med("sort"), "gather_ms": med("gather"),
           "regroup_ms": round(statistics.median(total), 4), "regroup_spread_ms": round(max(total) - min(total), 4),
           "gate_ms": med("gate"), "copy_ms": med("copy"), "copy_bytes": 2 * 46 * int(n),
           "identity_ms": {"intern": med("id_intern"), "sort": med("id_sort"), "gather": med("id_gather")},
           "scattered_ms": {"intern": med("sc_intern"), "sort": med("sc_sort"), "gather": med("sc_gather")},
           "scattered_moved": int(scattered[-1] + scattered[-2])}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    for o in sorted_recs + grouped_recs + [table]:
        o.close()
    ctx.close()


if __name__ == "__main__":
    main()
