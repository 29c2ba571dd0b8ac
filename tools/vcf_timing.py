#!/usr/bin/env python3
"""What pp_polish_vcf costs on bench.py's configs[1] job (5 Mbp / 200x, resident in HBM), stage by stage, next to what else reads or
writes as many bytes.  One warm-up pass, then --repeat passes; every figure is the median of the passes with their minimum and maximum.
Writes one JSON line to profiles/vcf_timing.json (--out) and prints it.
  own_edits / every_tenth     the job as it is, and the same reads over an assembly whose every tenth base was changed (the reads outvote
                              it: every tenth position is an edit): records, text_bytes, stage_ms (HIP-event spans on the context's stream:
                              mark | runs | records | text -- a span holds the host's work between its launches too: the read-backs,
                              the allocations and the uploads of `records` and `text`), kernel_ms (their sum), call_ms (wall time
                              of the whole call)
  d2d_copy_ms                 HIP-event time of a device-to-device copy of G bytes
  debug_tsv_ms                wall time of pp_polish_debug_tsv over the whole assembly into device memory (the job polished with the
                              --debug records kept), and its bytes
  host_loop_ms                wall time of what a host would do instead: the emit codes and the multi-byte winners downloaded
                              (pp_polish_debug_extra) and compared with the assembly, the runs cut with numpy
  polish_e2e_s                `polypolish polish` on the job's SAM pair with and without --vcf, the runs alternating: wall seconds
Measurement only: no threshold is attached to any of it."""
import argparse
import ctypes as C
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import polypolish_amd as pp  # noqa: E402


class DebugExtra(C.Structure):  # pp_debug_extra (include/polypolish_hip.h)
    _fields_ = [("emit", C.POINTER(C.c_uint8)), ("n_multi", C.c_uint64), ("multi_pos", C.c_void_p), ("multi_len", C.c_void_p),
                ("multi_off", C.c_void_p), ("n_keys", C.c_uint64), ("key_pos", C.c_void_p), ("key_len", C.c_void_p),
                ("key_count", C.c_void_p), ("key_off", C.c_void_p)]


def spread(values):
    return {"median": round(statistics.median(values), 4), "min": round(min(values), 4), "max": round(max(values), 4)}


def wall_ms(f):
    t = time.perf_counter()
    f()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mbp", type=float, default=5.0, help="assembly size (configs[1]: 5)")
    ap.add_argument("--coverage", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--runs", type=int, default=3, help="end-to-end runs per variant (0: leave the end-to-end leg out)")
    ap.add_argument("--tmp", default="/dev/shm" if os.path.isdir("/dev/shm") else None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vcf_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("vcf_timing: no GPU (nothing is measured without one)")
    import synthjob
    dev = torch.device("cuda:0")
    G0 = int(a.mbp * 1e6)
    # bench.py's configs[1] job, seed included (config 1, rank 0), as tools/prepare_timing.py makes it
    job = synthjob.with_wo(synthjob.with_seq4(synthjob.make_job(dev, contig_lens=[G0], coverage=a.coverage, read_len=150, seed=42 + 1 + 1,
                                                                indel_read_frac=synthjob.SURVEY_INDEL_READ_FRAC, recipe="survey")))
    torch.cuda.synchronize()
    G = int(job["contig_off"][-1])
    ptrs = {k: v.data_ptr() for k, v in job["recs"].items()}
    ptrs.update(seq4=job["seq4"].data_ptr(), wo=job["wo"].data_ptr(), wo_runs=job["wo_runs"])
    tenth = job["bases"].clone()
    idx = torch.arange(0, G, 10, device=dev)
    code = ((tenth[idx] >> 1) & 3).long()  # A C T G -> 0 1 2 3
    tenth[idx] = torch.tensor(list(b"CTGA"), dtype=torch.uint8, device=dev)[code]
    torch.cuda.synchronize()
    L = pp.lib()
    ctx = pp.Context(0)
    ctx.trust_mirrors(True)
    names = [b"chr1"]
    out = {"tool": "tools/vcf_timing.py", "workload": f"configs[1]: {G / 1e6:g} Mbp / {a.coverage}x, {job['n_aln']} records resident in HBM",
           "repeat": a.repeat}

    def polish(bases, debug=0):
        L.pp_polish_set_debug(ctx._h, debug)
        ctx.prepared_job(job["contig_off"], bases.data_ptr(), pp.MEM_DEVICE, job["n_aln"], ptrs, job["recs"]["seq"].numel(),
                         job["recs"]["cigar"].numel(), pp.MEM_DEVICE, 5, 0.5, 0.2)()
        L.pp_polish_set_debug(ctx._h, 0)

    ctx.set_profiling(1)
    for name, bases in (("own_edits", job["bases"]), ("every_tenth", tenth)):
        polish(bases)
        stages, call = {k: [] for k in ("mark", "runs", "records", "text")}, []
        for i in range(a.repeat + 1):  # (the first pass warms up)
            box = []
            ms = wall_ms(lambda: box.append(pp.Vcf(ctx, names)))
            v = box[0]
            if i:
                call.append(ms)
                for k, x in v.stage_ms().items():
                    stages[k].append(x)
            rec, nb = v.n_records, v.n_bytes
            v.close()
        kernel = [sum(x) for x in zip(*stages.values())]
        out[name] = {"records": rec, "text_bytes": nb, "stage_ms": {k: spread(x) for k, x in stages.items()}, "kernel_ms": spread(kernel),
                     "call_ms": spread(call)}
    ctx.set_profiling(0)
    # ---- a device-to-device copy of G bytes ----
    src = torch.empty(G, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    d2d = []
    for i in range(a.repeat + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        if i:
            d2d.append(e0.elapsed_time(e1))
    del src, dst
    out["d2d_copy_ms"] = spread(d2d)
    out["own_edits"]["kernel_over_d2d"] = round(out["own_edits"]["kernel_ms"]["median"] / out["d2d_copy_ms"]["median"], 2)
    out["every_tenth"]["kernel_over_d2d"] = round(out["every_tenth"]["kernel_ms"]["median"] / out["d2d_copy_ms"]["median"], 2)
    # ---- pp_polish_debug_tsv over the whole assembly, into device memory ----
    polish(job["bases"], debug=1)
    cap = 96 * G
    room = torch.empty(cap, dtype=torch.uint8, device=dev)
    arr = (C.c_char_p * 1)(*names)
    n, nxt = C.c_uint64(), C.c_uint64()
    tsv = []
    for i in range(a.repeat + 1):
        def whole():
            assert L.pp_polish_debug_tsv(ctx._h, C.cast(arr, C.c_void_p), 0, G, room.data_ptr(), pp.MEM_DEVICE, cap, C.byref(n), C.byref(nxt)) == 0
            assert nxt.value == G
        ms = wall_ms(whole)
        if i:
            tsv.append(ms)
    out["debug_tsv_ms"] = spread(tsv)
    out["debug_tsv_bytes"] = int(n.value)
    del room
    # ---- the host loop over a downloaded debug record ----
    h_bases = job["bases"].cpu().numpy()
    L.pp_polish_set_debug(ctx._h, 1)  # (pp_polish_debug_extra asks for the flag as well as for the job's records)
    loop = []
    for i in range(a.repeat + 1):
        def host_loop():
            ex = DebugExtra()
            assert L.pp_polish_debug_extra(ctx._h, C.byref(ex)) == 0
            emit = np.ctypeslib.as_array(ex.emit, shape=(G,))
            edited = emit != h_bases
            d = np.diff(np.concatenate([[0], edited.view(np.int8), [0]]))
            box.clear()
            box.append((int((d == 1).sum()), int(ex.n_multi)))
            L.pp_debug_extra_free(C.byref(ex))
        box = []
        ms = wall_ms(host_loop)
        if i:
            loop.append(ms)
    L.pp_polish_set_debug(ctx._h, 0)
    out["host_loop_ms"] = spread(loop)
    out["host_loop_runs"] = box[0][0]
    ctx.close()
    del job, tenth
    torch.cuda.empty_cache()
    # ---- `polish` end to end with and without --vcf, the runs alternating ----
    if a.runs > 0:
        import text_chain_timing as tct
        tmp = tempfile.mkdtemp(prefix="vcf_timing_", dir=a.tmp)
        try:
            pairs = synthjob.make_job(dev, contig_lens=(G0,), coverage=a.coverage, seed=42, pairs=True, unaligned_frac=1e-3)
            torch.cuda.synchronize()
            fasta, sams = synthjob.write_sam_pair(pairs, tmp, qual=True)
            del pairs
            torch.cuda.empty_cache()  # (the child processes are the only users of the device from here on)
            vcf = os.path.join(tmp, "edits.vcf")
            variants = {"plain": [], "vcf": ["--vcf", vcf], "vcf_bgzf": ["--vcf", vcf + ".gz", "--vcf_bgzf"]}
            res = {v: [] for v in variants}
            for v, flags in variants.items():  # warm-up
                tct.timed(["polish", *flags, fasta, *sams], os.path.join(tmp, f"{v}.stdout"))
            for _ in range(a.runs):
                for v, flags in variants.items():
                    res[v].append(round(tct.timed(["polish", *flags, fasta, *sams], os.path.join(tmp, f"{v}.stdout"))[0], 3))
            out["polish_e2e_s"] = {v: {"wall_s": x, "median_s": statistics.median(x)} for v, x in res.items()}
            out["polish_e2e_s"]["same_fasta"] = tct.sha(os.path.join(tmp, "vcf.stdout")) == tct.sha(os.path.join(tmp, "plain.stdout"))
            out["polish_e2e_s"]["vcf_file_bytes"] = {"text": os.path.getsize(vcf), "bgzf": os.path.getsize(vcf + ".gz")}
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
