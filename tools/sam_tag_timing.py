#!/usr/bin/env python3
"""What pp_sam_tagged costs on configs[1]'s SAM text: the two files tools/synthjob.py writes for make_job(pairs=True) (every record, QUAL
included; the recipe of tools/sam_records_timing.py), each resident in HBM in an allocation of exactly its length, decoded, named and
filtered on the device (SamRecords -> Names -> filter_records), then tagged with the filter's verdicts with mem = MEM_DEVICE.  Prints
one JSON line and writes it to profiles/sam_tag_timing.json (--out); every figure is the sum over the two files:
  stages_ms        HIP-event time by stage: newline_index (k_st_nl_count, k_tscan, k_st_nl_write) | pass_a (k_st_lines) | scans
                   (k_colscan x 2 + k_st_off x 2) | pass_b (k_st_copy); the pass with the best pass_b of --repeat
  tagged_wall_ms   host clock around pp_sam_tagged: its allocations, the upload of the verdicts and its four read-backs included
  copy_ms          HIP-event time of a plain device-to-device copy of the same texts, the same visit: the same bytes read once and
                   written once -- the memory-rate yardstick;  pass_b_over_copy = pass_b / copy_ms
  random_verdicts  the stages once more with --fail-frac of the aligned records failing at random: the job's reads have one alignment
                   each, so the filter itself fails none of them and the spliced tags would go unmeasured
  out_bytes        the two outputs;  pass_b_gbps = (text_bytes + out_bytes) over pass B's time
  write_ms         pp_sam_out_write of the two outputs (the read-back in slices and the file) to a directory under --tmp, a tmpfs path by default
  host_write_text_ms   pp_filter_write_text on the same texts and verdicts in host memory, to the same directory
Measurement only: no threshold is attached to any of it."""
import argparse
import ctypes as C
import json
import os
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

STAGES = ("newline_index", "pass_a", "scans", "pass_b")


def tagged_best(ctx, texts, verdicts, repeat):
    """the pass with the least pass_b of `repeat`: stages, wall time, counts, bytes"""
    best = None
    for _ in range(max(1, repeat)):
        ms, wall, out_bytes, counts = dict.fromkeys(STAGES, 0.0), 0.0, 0, []
        for t, v in zip(texts, verdicts):
            t0 = time.perf_counter()
            o = pp.SamOut.tagged(ctx, (t.data_ptr(), t.numel()), v, mem=pp.MEM_DEVICE)
            wall += time.perf_counter() - t0
            for k, x in o.stage_ms().items():
                ms[k] += x
            out_bytes += o.n_bytes
            counts.append(o.counts())
            o.close()
        if best is None or ms["pass_b"] < best["stages_ms"]["pass_b"]:
            best = {"stages_ms": {k: round(x, 4) for k, x in ms.items()}, "kernels_ms": round(sum(ms.values()), 4), "tagged_wall_ms": round(wall * 1e3, 3),
                    "out_bytes": out_bytes, "passed": sum(c[0] for c in counts), "failed": sum(c[1] for c in counts), "lines": sum(c[2] for c in counts)}
    return best


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mbp", type=float, default=5.0, help="assembly size (configs[1]: 5)")
    ap.add_argument("--coverage", type=int, default=200)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--fail-frac", type=float, default=0.02, help="share of failing records in the second measurement, with random verdicts")
    ap.add_argument("--tmp", default="/dev/shm" if os.path.isdir("/dev/shm") else None, help="where the files go (default: tmpfs)")
    ap.add_argument("--no-host", action="store_true", help="leave out pp_sam_out_write and pp_filter_write_text")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sam_tag_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sam_tag_timing: no GPU (nothing is measured without one)")
    if synthjob.samgen_lib() is None:
        sys.exit("sam_tag_timing: tools/_build/libsamgen.so is missing (make)")
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

    with tempfile.TemporaryDirectory(prefix="pp_sam_tag_", dir=os.environ.get("TMPDIR", "/tmp")) as tmp, \
            tempfile.TemporaryDirectory(prefix="pp_sam_tag_", dir=a.tmp) as fast:      # the inputs | the outputs
        _, sams = synthjob.write_sam_pair(job, tmp, qual=True)
        host = [np.fromfile(p, np.uint8) for p in sams]
        texts = [torch.from_numpy(h).to(dev) for h in host]
        torch.cuda.synchronize()
        print(f"[sam_tag_timing] texts: {[len(h) for h in host]} bytes", file=sys.stderr, flush=True)
        ctx = pp.Context(0)
        # ---- the verdicts: decode, name, filter
        table, recs = pp.Names(ctx), []
        for t in texts:
            rec = pp.SamRecords(ctx, (t.data_ptr(), t.numel()), pp.MEM_DEVICE)
            table.ids(**rec.names(), mem=pp.MEM_DEVICE, out=rec.read_id_ptr)
            recs.append(rec)
        verdicts = pp.filter_records(ctx, recs[0].raw(), recs[1].raw(), mem=pp.MEM_DEVICE)["pass"]
        for o in recs + [table]:
            o.close()
        print(f"[sam_tag_timing] verdicts: {[int((v == 0).sum()) for v in verdicts]} of {[len(v) for v in verdicts]} fail", file=sys.stderr, flush=True)
        # ---- the tagging
        ctx.set_profiling(1)
        tagged_best(ctx, texts, verdicts, 1)        # (warms up: code objects, the allocator)
        best = tagged_best(ctx, texts, verdicts, a.repeat)
        rng = np.random.default_rng(a.seed)
        some_fail = [(rng.random(len(v)) >= a.fail_frac).astype(np.uint8) for v in verdicts]
        with_fails = tagged_best(ctx, texts, some_fail, a.repeat)
        ctx.set_profiling(0)
        # ---- the yardstick: a device-to-device copy of the same texts
        copy_ms = None
        dsts = [torch.empty_like(t) for t in texts]
        for _ in range(max(2, a.repeat + 1)):       # (the first round warms up)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for d, t in zip(dsts, texts):
                d.copy_(t)
            e1.record()
            torch.cuda.synchronize()
            took = e0.elapsed_time(e1)
            copy_ms = took if copy_ms is None else min(copy_ms, took)
        del dsts
        text_bytes = sum(len(h) for h in host)

        def against_copy(b):
            return dict(b, pass_b_over_copy=round(b["stages_ms"]["pass_b"] / copy_ms, 2),
                        pass_b_gbps=round((text_bytes + b["out_bytes"]) / 1e9 / (b["stages_ms"]["pass_b"] / 1e3), 1))
        out.update(text_bytes=text_bytes, **against_copy(best), copy_ms=round(copy_ms, 4), copy_gbps=round(2 * text_bytes / 1e9 / (copy_ms / 1e3), 1),
                   random_verdicts=dict(against_copy(with_fails), fail_frac=a.fail_frac))
        emit(False)         # (the device's figures are on disk before the host laps start)
        if not a.no_host:
            # ---- the read-back: the two outputs (2 % failing) to files
            outs = [pp.SamOut.tagged(ctx, (t.data_ptr(), t.numel()), v, mem=pp.MEM_DEVICE) for t, v in zip(texts, some_fail)]
            t0 = time.perf_counter()
            for f, o in enumerate(outs):
                o.write(os.path.join(fast, f"device_{f + 1}.sam"))
            out["write_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            for o in outs:
                o.close()
            # ---- the host routine on the same texts and verdicts
            err = C.create_string_buffer(600)
            t0 = time.perf_counter()
            for f, (h, v) in enumerate(zip(host, some_fail)):
                rc = pp.lib().pp_filter_write_text(h.ctypes.data, len(h), v.ctypes.data, len(v), os.path.join(fast, f"host_{f + 1}.sam").encode(), None, None, err, 600)
                assert rc == 0, err.value
            out["host_write_text_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            out["files_equal"] = all(os.path.getsize(os.path.join(fast, f"device_{f}.sam")) == os.path.getsize(os.path.join(fast, f"host_{f}.sam")) and
                                     open(os.path.join(fast, f"device_{f}.sam"), "rb").read(1 << 24) == open(os.path.join(fast, f"host_{f}.sam"), "rb").read(1 << 24)
                                     for f in (1, 2))
            out["tmp"] = a.tmp or tempfile.gettempdir()
        ctx.close()
    emit(True)


if __name__ == "__main__":
    main()
