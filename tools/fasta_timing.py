#!/usr/bin/env python3
"""What loading the assembly costs, on the host and through the device link: the 250 Mbp single contig of BASELINE.json configs[4]
(--mbp) in six forms -- wrapped at 60 columns, wrapped at 80 columns and on one line per contig, each plain and BGZF.  One warm-up
pass, then --repeat passes; every figure is the median of the passes with their minimum and maximum.  Writes one JSON line to
profiles/fasta_timing.json (--out) and prints it.  Per form:
  file_bytes, text_bytes
  load_host_ms      wall time of pp_assembly_load (page cache warm)
  load_device_ms    wall time of pp_assembly_load_device: mapping, the staging copy or pp_bgzf_inflate, pp_fasta_records, the headers
  stages_ms         HIP-event time of pp_fasta_records' kernels on the text resident in HBM (mem = MEM_DEVICE), stage by stage: sums
                    (k_fasta<false> + k_fasta_scan) | place (k_fasta<true>) | headers; kernels_ms their sum; text_gbps = text bytes
                    over kernels_ms
  d2d_copy_ms       HIP-event time of a device-to-device copy of the same text bytes
With --e2e: `polypolish polish` end to end on that assembly with tools/synthjob.py's SAM pair (--e2e-coverage), with and without
PP_DEVICE_FASTA=1 (wall time of the child process).  Measurement only: no threshold is attached to any of it."""
import argparse
import ctypes as C
import json
import os
import statistics
import struct
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import polypolish_amd as pp  # noqa: E402

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def spread(values):
    return {"median": round(statistics.median(values), 4), "min": round(min(values), 4), "max": round(max(values), 4)}


def bgzf(data, level=1, piece=65280):
    """the bytes as a BGZF file, as bgzip cuts it: a block every 65,280 bytes, the EOF block behind them"""
    out = []
    for lo in range(0, len(data), piece):
        raw = bytes(data[lo:lo + piece])
        z = zlib.compressobj(level, zlib.DEFLATED, -15)
        body = z.compress(raw) + z.flush()
        out.append(b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(body) + 25) + body +
                   struct.pack("<II", zlib.crc32(raw), len(raw)))
    return b"".join(out) + EOF_BLOCK


def wrapped(bases, width):
    """>chr1 + the bases at `width` columns (0: one line), LF ends, a final newline"""
    head = b">chr1 synthetic\n"
    if not width:
        return head + bases.tobytes() + b"\n"
    n = len(bases)
    full = n // width
    body = np.empty((full, width + 1), np.uint8)
    body[:, :width] = bases[:full * width].reshape(full, width)
    body[:, width] = 10
    tail = bases[full * width:].tobytes()
    return head + body.tobytes() + (tail + b"\n" if tail else b"")


def wall_ms(f):
    t = time.perf_counter()
    f()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mbp", type=float, default=250.0, help="assembly size (configs[4]: 250)")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--e2e", action="store_true", help="also run `polypolish polish` end to end with and without PP_DEVICE_FASTA=1")
    ap.add_argument("--e2e-coverage", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fasta_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fasta_timing: no GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    n = int(a.mbp * 1e6)
    bases = np.frombuffer(b"ACGT", np.uint8)[np.random.RandomState(a.seed).randint(0, 4, n, dtype=np.uint8)]
    L = pp.lib()
    ctx = pp.Context(0)
    ctx.set_profiling(1)
    out = {"input": f"{a.mbp:g} Mbp, one contig (seed {a.seed})", "repeat": a.repeat, "forms": {}}
    with tempfile.TemporaryDirectory(prefix="pp_fasta_", dir=os.environ.get("TMPDIR", "/tmp")) as tmp:
        for name, width in (("wrap60", 60), ("wrap80", 80), ("one_line", 0)):
            text = wrapped(bases, width)
            t_dev = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).to(dev)
            t_dst = torch.empty_like(t_dev)
            torch.cuda.synchronize()
            stages, d2d = [], []
            for i in range(a.repeat + 1):  # (the first pass warms up: code objects, the allocator)
                rec = pp.FastaRecords(ctx, (t_dev.data_ptr(), len(text)), pp.MEM_DEVICE)
                ms = rec.stage_ms()
                assert rec.n_bases == n and rec.n_contigs == 1
                rec.close()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                t_dst.copy_(t_dev)
                e1.record()
                torch.cuda.synchronize()
                if i:
                    stages.append(ms)
                    d2d.append(e0.elapsed_time(e1))
            del t_dev, t_dst
            kernels = [r["sums"] + r["place"] + r["headers"] for r in stages]
            shared = {"text_bytes": len(text), "stages_ms": {k: spread([r[k] for r in stages]) for k in ("sums", "place", "headers")},
                      "kernels_ms": spread(kernels), "text_gbps": spread([len(text) / 1e9 / (k / 1e3) for k in kernels]), "d2d_copy_ms": spread(d2d)}
            for form, data in ((name, text), (name + "_bgzf", None)):
                data = bgzf(text) if data is None else data
                path = os.path.join(tmp, form + (".fasta.gz" if form.endswith("bgzf") else ".fasta"))
                with open(path, "wb") as f:
                    f.write(data)
                host, device = [], []
                for i in range(a.repeat + 1):
                    for device_link, into in ((False, host), (True, device)):
                        h, err = C.c_void_p(), C.create_string_buffer(1024)
                        call = (lambda: L.pp_assembly_load_device(ctx._h, path.encode(), C.byref(h), err, 1024)) if device_link else \
                               (lambda: L.pp_assembly_load(path.encode(), C.byref(h), err, 1024))
                        rcs = []
                        ms = wall_ms(lambda: rcs.append(call()))
                        assert rcs == [0], err.value
                        assert L.pp_assembly_offsets(h)[1] == n and bool(L.pp_assembly_bases_device(h)) == device_link
                        L.pp_assembly_free(h)
                        if i:
                            into.append(ms)
                out["forms"][form] = dict(shared, file_bytes=len(data), load_host_ms=spread(host), load_device_ms=spread(device))
                os.unlink(path)
                del data
            if a.e2e and name == "wrap60":
                out["polish_e2e"] = polish_e2e(a, bases, text, tmp, dev)
            del text
    ctx.close()
    if not a.e2e:
        out["polish_e2e"] = {"not_measured": "run with --e2e"}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


def polish_e2e(a, bases, text, tmp, dev):
    """wall time of `polypolish polish` as a child process on the wrapped assembly and synthjob's SAM pair, the switch off and on"""
    try:
        import synthjob
        if synthjob.samgen_lib() is None:
            return {"not_measured": "tools/_build/libsamgen.so is missing (make)"}
        job = synthjob.make_job(dev, contig_lens=(len(bases),), coverage=a.e2e_coverage, seed=a.seed, pairs=True)
        torch.cuda.synchronize()
        fa, sams = synthjob.write_sam_pair(job, tmp, qual=False)
        del job
        torch.cuda.empty_cache()
        exe = os.path.join(ROOT, "bin", "polypolish")
        base = {k: v for k, v in os.environ.items() if k != "PP_DEVICE_FASTA"}
        res = {"assembly": "the job's own FASTA as synthjob writes it", "coverage": a.e2e_coverage}
        for tag, env in (("host_ms", base), ("device_ms", dict(base, PP_DEVICE_FASTA="1"))):
            runs, outs = [], []
            for i in range(a.repeat + 1):
                t = time.perf_counter()
                r = subprocess.run([exe, "polish", fa] + sams, env=env, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=600)
                ms = (time.perf_counter() - t) * 1e3
                if r.returncode:
                    return {"not_measured": f"polypolish polish ended with {r.returncode}"}
                outs.append(zlib.crc32(r.stdout))
                if i:
                    runs.append(ms)
            res[tag] = spread(runs)
            res[tag + "_crc32"] = outs[-1]
        res["same_bytes"] = res["host_ms_crc32"] == res["device_ms_crc32"]
        return res
    except Exception as e:  # (measurement infrastructure: report, do not lose the loader's figures)
        return {"not_measured": f"{type(e).__name__}: {e}"[:300]}


if __name__ == "__main__":
    main()
