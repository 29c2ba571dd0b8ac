#!/usr/bin/env python3
"""What pp_names costs on the QNAMEs of a configs[1]-shaped SAM pair.

The names are those tools/samgen.c writes for tools/synthjob.py's job (make_job(pairs=True): "r<read>" for EVERY record, unaligned
ones too), made with numpy -- no SAM text.  One table takes file 1's names, then file 2's.  Prints one JSON line:
  device   HIP-event ms of the two calls on names resident in HBM (best of --repeat), their bytes, the distinct names behind each, the
           bytes per second of each call (name bytes + offsets + lengths + ids over the event time) and the time by stage
  host     wall ms of the same two calls from host memory, upload and download included
  rec_intern_ms   the rec_intern span of pp_filter_records on raw batches whose read_id are these ids
  dict     one host core: a Python dict over the same names (bytes objects), building the list of names not included
--out FILE writes the line to FILE as well.  Measurement only: no threshold is attached to any of it."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import polypolish_amd as pp  # noqa: E402
import synthjob  # noqa: E402


def qnames(read):
    """"r<read>" for every record -> (bytes, off, len)"""
    r = np.asarray(read).astype(np.int64)
    nd = np.ones(len(r), np.int64)
    for k in range(1, 19):
        nd += r >= 10 ** k
    ln = nd + 1
    off = np.cumsum(ln) - ln
    b = np.empty(int(ln.sum()), np.uint8)
    b[off] = ord("r")
    for d in range(int(nd.max())):
        sel = nd > d
        b[(off + ln - 1 - d)[sel]] = 48 + (r[sel] // 10 ** d) % 10
    return b, off.astype(np.uint64), ln.astype(np.uint32)


def stage_ms(table):
    ms = table._stage_ms("pp_names_stage_ms_", ("lookup", "rehash", "insert_rank", "entries_bytes", "ids"))
    return {k: round(v, 4) for k, v in ms.items()}


def on_device(call, dev):
    b, off, ln = call
    t = [torch.from_numpy(b).to(dev), torch.from_numpy(off.view(np.int64)).to(dev), torch.from_numpy(ln.view(np.int32)).to(dev),
         torch.empty(len(off), dtype=torch.int64, device=dev)]
    torch.cuda.synchronize()
    return t


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mbp", type=float, default=5.0, help="assembly size (configs[1]: 5)")
    ap.add_argument("--coverage", type=int, default=200)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", help="also write the JSON line to this file")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    job = synthjob.make_job(dev, contig_lens=(int(a.mbp * 1e6),), coverage=a.coverage, seed=a.seed, pairs=True, unaligned_frac=1e-3)
    torch.cuda.synchronize()
    S = job["sam"]
    n, half = S["n"], S["half"]
    read = S["read"].cpu().numpy()
    calls = [qnames(read[:half]), qnames(read[half:])]
    L = pp.lib()
    ctx = pp.Context(0)
    ctx.set_profiling(1)

    # ---- names resident in HBM ----
    tensors = [on_device(c, dev) for c in calls]
    best, ids = None, None
    for _ in range(max(1, a.repeat)):
        table, ms, distinct, got, stages = pp.Names(ctx), [], [], [], []
        for c, t in zip(calls, tensors):
            got.append(table.ids((t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr()), mem=pp.MEM_DEVICE, n=len(c[1]), n_bytes=len(c[0]),
                                 out=t[3].data_ptr()))
            ms.append(table.kernel_ms())
            stages.append(stage_ms(table))
            distinct.append(table.count)
        table.close()
        if best is None or sum(ms) < sum(best["ms"]):
            best, ids = {"ms": ms, "distinct": distinct, "stages": stages}, got
    moved = [len(c[0]) + 20 * len(c[1]) for c in calls]         # name bytes + off (8) + len (4) + id64 (8)
    device = {"file1_ms": round(best["ms"][0], 4), "file2_ms": round(best["ms"][1], 4), "names": [len(c[1]) for c in calls],
              "name_bytes": [len(c[0]) for c in calls], "distinct_after": best["distinct"],
              "gbps": [round(m / 1e9 / (t / 1e3), 1) for m, t in zip(moved, best["ms"])], "file1_stages_ms": best["stages"][0],
              "file2_stages_ms": best["stages"][1]}

    # ---- from host memory ----
    host_ms = []
    for _ in range(max(1, a.repeat)):
        table, w = pp.Names(ctx), []
        for c, want in zip(calls, ids):
            t0 = time.perf_counter()
            got = table.ids(c)
            w.append(1e3 * (time.perf_counter() - t0))
            assert np.array_equal(got, want)
        table.close()
        if not host_ms or sum(w) < sum(host_ms):
            host_ms = w
    host = {"file1_wall_ms": round(host_ms[0], 3), "file2_wall_ms": round(host_ms[1], 3)}

    # ---- pp_filter_records on the ids ----
    raws, keep = [], []
    for f, (lo, hi) in enumerate(((0, half), (half, n))):
        t = {"flag": S["flag"][lo:hi].to(torch.int16).contiguous(), "read_id": tensors[f][3], "contig": S["contig"][lo:hi].to(torch.int32).contiguous(),
             "ref_start": S["ref_start"][lo:hi].to(torch.int32).contiguous(), "cig_off": S["cig_off"][lo:hi].to(torch.int64).contiguous(),
             "n_cig": S["n_cig"][lo:hi].to(torch.int32).contiguous(), "cigar": S["cigar"].to(torch.int32).contiguous()}
        keep.append(t)
        p = {k: v.data_ptr() for k, v in t.items()}
        p.update(n_rec=hi - lo, seq_bytes=0, n_cig_total=t["cigar"].numel())
        raws.append(p)
    torch.cuda.synchronize()
    rec_intern = None
    try:
        spans = []
        for _ in range(max(1, a.repeat)):
            pp.filter_records(ctx, raws[0], raws[1], mem=pp.MEM_DEVICE)
            kt = pp.KernelTimes()
            L.pp_filter_kernel_times(ctx._h, C.byref(kt))
            spans.append(kt.as_dict()["ms"]["rec_intern"])
        rec_intern = round(min(spans), 4)
    except pp.PolypolishError as e:
        rec_intern = {"error": str(e)[:200]}

    # ---- one host core: a dict over the same names ----
    dict_ms, state = [], {}
    for c, want in zip(calls, ids):
        raw, off, ln = c[0].tobytes(), c[1].tolist(), c[2].tolist()
        names = [raw[o:o + k] for o, k in zip(off, ln)]
        t0 = time.perf_counter()
        got = [state.setdefault(x, len(state)) for x in names]
        dict_ms.append(1e3 * (time.perf_counter() - t0))
        assert np.array_equal(np.array(got, np.uint64), want)
    out = {"input": f"{a.mbp:g} Mbp x {a.coverage}, {n} records in two files (seed {a.seed})", "device": device, "host": host,
           "rec_intern_ms": rec_intern, "dict": {"file1_ms": round(dict_ms[0], 1), "file2_ms": round(dict_ms[1], 1)}}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
