#!/usr/bin/env python3
"""What the polished assembly costs on its way out, through the device link and on the host: the 250 Mbp single contig of
BASELINE.json configs[4] (--mbp) resident in HBM, as FASTA text at width 0, 60 and 80.  One warm-up pass, then --repeat passes;
every figure is the median of the passes with their minimum and maximum (the host zlib figures: one pass each).  Writes one JSON
line to profiles/fasta_text_timing.json (--out) and prints it.  Per width:
  text_bytes
  text_ms           HIP-event time of pp_fasta_text's kernel (mem = MEM_DEVICE); text_gbps = text bytes over it
  d2d_copy_ms       HIP-event time of a device-to-device copy of the same text bytes
  deflate_ms        HIP-event time of pp_bgzf_deflate's kernels on the text; file_bytes = the compressed file
  read_back_ms      wall time of the download of the text, and of the compressed file, into touched host memory
  device_route_ms   text_ms + read_back_ms.text -- and text_ms + deflate_ms + read_back_ms.file for the bgzipped file
  host_loop_ms      wall time of what write_fasta_and_log does: the header and the polished bytes, fetched off the device, into the
                    prepared host buffer (width 0, the only form it knows)
  host_zlib_ms      wall time of zlib level 6 over the same text cut every 65,280 bytes, on 1 and on 16 threads
Measurement only: no threshold is attached to any of it."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import polypolish_amd as pp  # noqa: E402

PIECE = 65280
HEADER = b"chr1 synthetic polypolish"


def spread(values):
    return {"median": round(statistics.median(values), 4), "min": round(min(values), 4), "max": round(max(values), 4)}


def wall_ms(f):
    t = time.perf_counter()
    f()
    return (time.perf_counter() - t) * 1e3


def deflate_piece(raw):
    z = zlib.compressobj(6, zlib.DEFLATED, -15)
    return len(z.compress(raw) + z.flush()) + 26


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mbp", type=float, default=250.0, help="assembly size (configs[4]: 250)")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--no-host-zlib", action="store_true", help="leave the host zlib passes out (they take seconds per width)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fasta_text_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fasta_text_timing: no GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    n = int(a.mbp * 1e6)
    bases = np.frombuffer(b"ACGT", np.uint8)[np.random.RandomState(a.seed).randint(0, 4, n, dtype=np.uint8)]
    d_bases = torch.from_numpy(bases.copy()).to(dev)
    torch.cuda.synchronize()
    L = pp.lib()
    ctx = pp.Context(0)
    ctx.set_profiling(1)
    off = np.array([0, n], np.uint64)
    out = {"input": f"{a.mbp:g} Mbp, one contig (seed {a.seed})", "repeat": a.repeat, "widths": {}}
    # ---- the host loop of write_fasta_and_log: header, bytes off the device, newline, into a buffer touched beforehand ----
    buf = np.zeros(len(HEADER) + n + 3, np.uint8)
    loop = []
    for i in range(a.repeat + 1):
        def host_loop():
            buf[0] = 62
            buf[1:1 + len(HEADER)] = np.frombuffer(HEADER, np.uint8)
            buf[1 + len(HEADER)] = 10
            assert L.pp_ctx_download(ctx._h, buf.ctypes.data + 2 + len(HEADER), d_bases.data_ptr(), n) == 0
            buf[2 + len(HEADER) + n] = 10
        ms = wall_ms(host_loop)
        if i:
            loop.append(ms)
    out["host_loop_ms"] = spread(loop)
    for width in (0, 60, 80):
        text_ms, d2d, deflate_ms, back_text, back_file = [], [], [], [], []
        text_bytes = file_bytes = 0
        host_text = host_file = None  # (allocated and touched on the warm-up pass: no page fault inside a measured copy)
        for i in range(a.repeat + 1):  # (the first pass warms up: code objects, the allocator)
            t = pp.FastaText(ctx, (d_bases.data_ptr(), n), off, [HEADER], width, pp.MEM_DEVICE)
            text_bytes = t.n_bytes
            z = t.deflate()
            file_bytes = z.n_bytes
            src = torch.empty(text_bytes, dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(src)
            e1.record()
            torch.cuda.synchronize()
            del src, dst
            if host_text is None:
                host_text, host_file = np.ones(text_bytes, np.uint8), np.ones(file_bytes, np.uint8)
            assert len(host_text) == text_bytes and len(host_file) == file_bytes  # (the same bytes every pass)
            bt = wall_ms(lambda: L.pp_ctx_download(ctx._h, host_text.ctypes.data, t.bytes_ptr, text_bytes))
            bf = wall_ms(lambda: L.pp_ctx_download(ctx._h, host_file.ctypes.data, z.bytes_ptr, file_bytes))
            if i:
                text_ms.append(t.kernel_ms())
                deflate_ms.append(z.kernel_ms())
                d2d.append(e0.elapsed_time(e1))
                back_text.append(bt)
                back_file.append(bf)
            z.close()
            t.close()
        assert bytes(host_text[:2 + len(HEADER)]) == b">" + HEADER + b"\n" and host_text[-1] == 10
        row = {"text_bytes": text_bytes, "file_bytes": file_bytes, "text_ms": spread(text_ms),
               "text_gbps": spread([text_bytes / 1e9 / (k / 1e3) for k in text_ms]), "d2d_copy_ms": spread(d2d),
               "deflate_ms": spread(deflate_ms), "read_back_ms": {"text": spread(back_text), "file": spread(back_file)},
               "device_route_ms": {"text": spread([x + y for x, y in zip(text_ms, back_text)]),
                                   "bgzf": spread([x + y + w for x, y, w in zip(text_ms, deflate_ms, back_file)])}}
        if a.no_host_zlib:
            row["host_zlib_ms"] = {"not_measured": "--no-host-zlib"}
        else:
            view = memoryview(host_text)
            pieces = [view[lo:lo + PIECE] for lo in range(0, text_bytes, PIECE)]
            sizes = {}
            for threads in (1, 16):
                with ThreadPoolExecutor(threads) as pool:
                    ms = wall_ms(lambda: sizes.__setitem__(threads, sum(pool.map(deflate_piece, pieces, chunksize=16))))
                row.setdefault("host_zlib_ms", {})[f"threads_{threads}"] = round(ms, 1)
            row["host_zlib_file_bytes"] = sizes[1]
        out["widths"][str(width)] = row
        del host_text, host_file
    ctx.close()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
