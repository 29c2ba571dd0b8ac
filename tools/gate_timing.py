#!/usr/bin/env python3
"""What pp_batch_gate costs on a configs[1]-shaped input, next to the device tokenizer on the same records as SAM text.

The raw records are those of tools/synthjob.py's SAM pair (make_job(pairs=True): every record, the ones the gates reject and the
unaligned ones too, secondary records with SEQ "*"), one pp_raw_batch per file, in device memory.  Prints one JSON line:
  gate_ms        HIP-event time of the gate's kernels, summed over the two files (best of --repeat)
  seq_copy_gbps  bytes k_gate_seq reads and writes (SEQ in, rooms out, CIGAR runs both ways) over its own HIP-event time
  prepare_ms     pp_batch_prepare's kernels on the two gated batches
  tokenizer_stages_ms   the tokenizer's own stage timers (bin/polypolish polish, PP_TIMING=1) on the SAM text of the same job
--out FILE writes the line to FILE as well.  Measurement only: no threshold is attached to any of it."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import polypolish_amd as pp  # noqa: E402
import synthjob  # noqa: E402


def raw_of(job, lo, hi):
    """the records [lo, hi) of the job's SAM pair as the addresses of a pp_raw_batch (device memory) -> (ptrs, tensors to keep)"""
    S = job["sam"]
    keep = {"flag": S["flag"][lo:hi].to(torch.int16).contiguous(), "read_id": S["read"][lo:hi].to(torch.int64).contiguous(),
            "contig": S["contig"][lo:hi].to(torch.int32).contiguous(), "ref_start": S["ref_start"][lo:hi].to(torch.int32).contiguous(),
            "nm": S["nm"][lo:hi].to(torch.int32).contiguous(), "seq_off": S["seq_off"][lo:hi].to(torch.int64).contiguous(),
            "seq_len": S["seq_len"][lo:hi].to(torch.int32).contiguous(), "cig_off": S["cig_off"][lo:hi].to(torch.int64).contiguous(),
            "n_cig": S["n_cig"][lo:hi].to(torch.int32).contiguous(), "seq": S["seq"].contiguous(), "cigar": S["cigar"].to(torch.int32).contiguous()}
    ptrs = {k: v.data_ptr() for k, v in keep.items()}
    ptrs.update(n_rec=hi - lo, seq_bytes=keep["seq"].numel(), n_cig_total=keep["cigar"].numel())
    return ptrs, keep


def tokenizer_stages(job, tmp):
    exe = os.path.join(ROOT, "bin", "polypolish")
    if not os.path.exists(exe) or synthjob.samgen_lib() is None:
        return {"skipped": "bin/polypolish or tools/_build/libsamgen.so is missing"}
    fa, sams = synthjob.write_sam_pair(job, tmp, qual=True)
    r = subprocess.run([exe, "polish", fa] + sams, env=dict(os.environ, PP_DEVICE_INGEST="1", PP_TIMING="1"), capture_output=True)
    if r.returncode:
        return {"error": r.stderr.decode(errors="replace")[-300:]}
    tot = {}
    for l in r.stderr.decode(errors="replace").splitlines():
        m = re.match(r"\[timing\]\s+tokenizer:\s+(.*?)\s+([0-9.]+) s\b", l)
        if m:
            tot[m.group(1)] = round(tot.get(m.group(1), 0.0) + 1e3 * float(m.group(2)), 3)
    return tot


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mbp", type=float, default=5.0, help="assembly size (configs[1]: 5)")
    ap.add_argument("--coverage", type=int, default=200)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--no-text", action="store_true", help="leave the SAM text and the tokenizer's stages out")
    ap.add_argument("--out", help="also write the JSON line to this file")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    job = synthjob.make_job(dev, contig_lens=(int(a.mbp * 1e6),), coverage=a.coverage, seed=a.seed, pairs=True, unaligned_frac=1e-3)
    torch.cuda.synchronize()
    n, half = job["sam"]["n"], job["sam"]["half"]
    ctx = pp.Context(0)
    ctx.set_profiling(1)
    best = None
    for _ in range(max(1, a.repeat)):
        tot, copy_ms, copy_bytes, prep_ms, used = 0.0, 0.0, 0, 0.0, 0
        for lo, hi in ((0, half), (half, n)):
            ptrs, keep = raw_of(job, lo, hi)
            g = pp.gate_records(ctx, ptrs, mem=pp.MEM_DEVICE)
            tot += g.kernel_ms()
            copy_ms += g._stage_ms("pp_gated_stage_ms_", ("gates", "placement", "copy"))["copy"]
            h_len = ctx.download(g._ptrs["seq_len"], g.n_aln, np.uint32)
            copy_bytes += int(h_len.sum(dtype=np.int64)) + g.seq_bytes + 8 * g.n_cig_total
            p = pp.prepare_batch(ctx, job["contig_off"], g.n_aln, g.ptrs(), g.seq_bytes, g.n_cig_total, pp.MEM_DEVICE)
            prep_ms += p.kernel_ms()
            used += g.n_aln
            p.close()
            g.close()
            del keep
        if best is None or tot < best["gate_ms"]:
            best = {"gate_ms": round(tot, 4), "seq_copy_ms": round(copy_ms, 4),
                    "seq_copy_gbps": round(copy_bytes / 1e9 / (copy_ms / 1e3), 1) if copy_ms else None, "prepare_ms": round(prep_ms, 4),
                    "records": int(n), "good": used}
    out = {"input": f"{a.mbp:g} Mbp x {a.coverage}, {n} raw records in two files (seed {a.seed})", **best}
    if not a.no_text:
        with tempfile.TemporaryDirectory(prefix="pp_gate_", dir=os.environ.get("TMPDIR", "/tmp")) as tmp:
            out["tokenizer_stages_ms"] = tokenizer_stages(job, tmp)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
