"""The definition of the bytes pp_depth_bedgraph / pp_polish_depth (pp_k_depth.h, pp_depth_host.h) write, in plain Python.
tests/test_depth_model_cpu.py pins this file on the CPU (hand-written bytes for both forms, the ties, the oracle's --debug TSV against
its per-position depths); the GPU tests hold the library against it byte for byte, fed from the oracle, never from the device alone.

  tenths(x)  for a depth x (a double, 0 <= x < 2^32): the integer 10 x rounded from x's exact binary value, ties to even -- what Rust's
             format!("{:.1}") and the --debug TSV print, without the point.  Taken from Python's '%.1f' % x, which is correctly rounded
  text       no header or track line.  Per record, in assembly order:  name \\t start \\t end \\t value \\n  -- start and end 0-based,
             half-open and local to the contig.  Names are written verbatim
  bin == 0   (runs, the -bga form) a record is a maximal run of consecutive positions of ONE contig (runs never join across a contig
             boundary) that share one tenths value: two doubles that print alike are one run, zero-depth runs are written like any
             other.  value = tenths // 10 '.' tenths % 10
  bin == W   (bins, 1 <= W <= 2^24) per contig of length L one record per bin [kW, min((k+1)W, L)), k = 0 .. ceil(L/W) - 1; equal
             neighbours are not merged.  value = the mean of the bin's depths AS THE TSV PRINTS THEM, to two decimals, in integers:
             S = the sum of the bin's tenths, n = its length, q, r = divmod(10 S, n), q + 1 when 2r > n or 2r == n and q is odd;
             written q // 100 '.' and the two digits of q % 100.  Order-free and exact
  summary    zero_positions: the positions whose tenths are 0; max_tenths; sum_tenths over all positions (not per bin)"""
import math

import numpy as np

BIN_MAX = 1 << 24
DEPTH_LIMIT = float(1 << 32)


def _b(x):
    return x.encode() if isinstance(x, str) else bytes(x)


def tenths(x):
    x = float(x)
    assert not math.isnan(x) and math.copysign(1.0, x) > 0 and x < DEPTH_LIMIT, x
    s = "%.1f" % x
    return int(s[:-2]) * 10 + int(s[-1])


def tenths_of(depth):
    """tenths of every position, as Python ints in a numpy object-free int64 array (tenths stay below 2^36)"""
    d = np.ascontiguousarray(depth, np.float64).reshape(-1)
    u, inv = np.unique(d.view(np.uint64), return_inverse=True)  # (by their bits: -0.0 is not 0.0; each distinct double is formatted once)
    return np.array([tenths(v) for v in u.view(np.float64).tolist()], np.int64)[inv.reshape(-1)] if len(d) else np.zeros(0, np.int64)


def _offsets(contig_off, n):
    off = [int(x) for x in contig_off]
    assert off[0] == 0 and off[-1] == n and all(a <= b for a, b in zip(off[:-1], off[1:]))
    return off


def run_records(depth, contig_off):
    """[(contig index, start, end, tenths)] -- start and end local to the contig"""
    t = tenths_of(depth)
    off = _offsets(contig_off, len(t))
    out = []
    for c in range(len(off) - 1):
        lo, hi = off[c], off[c + 1]
        if hi == lo:
            continue
        s = t[lo:hi]
        cuts = np.concatenate([[0], np.nonzero(s[1:] != s[:-1])[0] + 1, [hi - lo]])  # every change of the printed depth begins a run
        out += [(c, int(a), int(b), int(s[a])) for a, b in zip(cuts[:-1], cuts[1:])]
    return out


def mean_hundredths(S, n):
    q, r = divmod(10 * int(S), int(n))
    return q + (1 if 2 * r > n or (2 * r == n and q % 2 == 1) else 0)


def bin_records(depth, contig_off, W):
    """[(contig index, start, end, hundredths)]"""
    assert 1 <= W <= BIN_MAX
    t = tenths_of(depth)
    off = _offsets(contig_off, len(t))
    out = []
    for c in range(len(off) - 1):
        lo, hi = off[c], off[c + 1]
        for a in range(0, hi - lo, W):
            b = min(a + W, hi - lo)
            out.append((c, a, b, mean_hundredths(sum(t[lo + a:lo + b].tolist()), b - a)))
    return out


def bedgraph(depth, contig_off, names, bin=0):  # noqa: A002 (the C argument's name)
    if bin == 0:
        return b"".join(b"%s\t%d\t%d\t%d.%d\n" % (_b(names[c]), a, b, v // 10, v % 10) for c, a, b, v in run_records(depth, contig_off))
    return b"".join(b"%s\t%d\t%d\t%d.%02d\n" % (_b(names[c]), a, b, q // 100, q % 100) for c, a, b, q in bin_records(depth, contig_off, bin))


def summary(depth):
    t = tenths_of(depth).tolist()
    return {"zero_positions": sum(1 for v in t if v == 0), "max_tenths": max(t, default=0), "sum_tenths": sum(t)}


def parse(text):
    """[(name, start, end, value text)] of a text this model writes"""
    out = []
    for ln in bytes(text).split(b"\n")[:-1]:
        name, a, b, v = ln.rsplit(b"\t", 3)
        out.append((name, int(a), int(b), v))
    return out


def expand(text, contig_off, names):
    """a runs-form text back to one value text per position"""
    off = _offsets(contig_off, int(contig_off[-1]))
    idx = {_b(n): c for c, n in enumerate(names)}
    out = [None] * off[-1]
    for name, a, b, v in parse(text):
        lo = off[idx[name]]
        for p in range(lo + a, lo + b):
            assert out[p] is None
            out[p] = v
    return out


def depth_column_of_debug_tsv(tsv):
    """column 4 (depth) of a --debug TSV, line by line behind its header line, as the bytes it prints"""
    lines = bytes(tsv).split(b"\n")
    assert lines[0].startswith(b"name\tpos\tbase\tdepth\t") and lines[-1] == b""
    return [ln.split(b"\t", 4)[3] for ln in lines[1:-1]]
