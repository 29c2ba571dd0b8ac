"""What the --debug TSV tests share (test_debug_tsv_gpu.py, test_long_winner_outputs_gpu.py, long_sites.py): the TSV's header line, a
line-wise difference for assertion messages, one raw call of pp_polish_debug_tsv, and a hand-built FASTA / SAM pair."""
import ctypes as C
import os

import numpy as np

HEADER = b"name\tpos\tbase\tdepth\tinvalid\tvalid\tpileup\tstatus\tnew_base\n"


def _diff(got, want):
    gl, wl = got.split(b"\n"), want.split(b"\n")
    return len(gl), len(wl), [(a, b) for a, b in zip(gl, wl) if a != b][:4]


def _raw(pp, ctx, names, lo, hi, cap, mem=0, out=None):
    arr = (C.c_char_p * len(names))(*[n.encode() for n in names])
    buf = np.full(max(cap, 1), 0xEE, dtype=np.uint8) if out is None else None
    n, nxt = C.c_uint64(), C.c_uint64()
    rc = pp.lib().pp_polish_debug_tsv(ctx._h, C.cast(arr, C.c_void_p), lo, hi, buf.ctypes.data if out is None else out, mem, cap,
                                      C.byref(n), C.byref(nxt))
    return rc, buf, n.value, nxt.value


def _write_job(tmp, contigs, alns, name="hand"):
    """contigs: [(name, bytes)]; alns: [(qname, contig, pos0, cigar, seq)] -- consecutive records of one qname are one
    read group (share 1/k)."""
    fa, sam = os.path.join(tmp, f"{name}.fasta"), os.path.join(tmp, f"{name}.sam")
    with open(fa, "w") as f:
        for n, s in contigs:
            f.write(f">{n}\n{s}\n")
    with open(sam, "w") as f:
        for n, s in contigs:
            f.write(f"@SQ\tSN:{n}\tLN:{len(s)}\n")
        for q, c, p, cig, seq in alns:
            f.write(f"{q}\t0\t{c}\t{p + 1}\t60\t{cig}\t*\t0\t0\t{seq}\t*\tNM:i:0\n")
    return fa, sam
