"""The plain model of the BGZF compressor (pp_bgzf_deflate, pp_bam_out_deflate): THE DEFINITION of the bytes the device makes.  One
BGZF block around ONE DEFLATE block (BFINAL = 1) per piece of at most 65,280 bytes; every rule is a function of the piece's bytes
alone, so lanes, waves and atomics may run in any order and the result is the same.

  candidates   positions in strips of S; a table T of 2^HB entries, empty at the piece's start.  Every position i of a strip with
               i + 4 <= n reads T[h(i)] as the strips in front left it; after the strip has read, T[h(i)] = max(T[h(i)], i).  A
               candidate is never in i's own strip and never in another piece.
  match        L(i) = the common prefix of data[cand:] and data[i:], capped at min(258, n - i) (source and target may overlap); it
               counts when L(i) >= 4 and i - cand <= 32,768
  parse        greedy from 0: a counted match is (L, dist) and skips L positions, anything else is a literal
  lengths      used symbols sorted by (count, symbol); two-queue Huffman merge, a tie takes the leaf; depths beyond the limit (15; 7
               for the code-length code) are folded into it, then `over` times (over = the Kraft sum's excess in units of 2^-limit)
               one leaf of the longest length below the limit moves down a level and takes a code from the limit as its sibling:
               each step takes exactly one unit off; the lengths per level are handed out again in sorted order, the longest first
  header       HLIT, HDIST trimmed to the last used symbol (no distance: HDIST = 1, one zero length; one distance: one 1-bit code);
               the lengths of both codes as ONE sequence; greedy: zeros in runs of 11 .. 138 are 18, of 3 .. 10 are 17; a length
               equal to the one in front, 3 .. 6 times, is 16; anything else is itself; HCLEN trimmed in the code-length order
  choice       the exact bit costs of stored, fixed and dynamic; the smallest wins, a tie goes to the earlier: at most n + 31 bytes
  frame        pp_bgzf_host.h's 18-byte header with the real BSIZE, the stream, CRC32, ISIZE; blocks dense, the EOF block last
"""
import bisect
import random
import struct

import bgzf_model as M

S, HB = 256, 13
PIECE = 0xff00
MIN_MATCH, MAX_MATCH, MAX_DIST = 4, 258, 32768
STORED, FIXED, DYNAMIC = 0, 1, 2


def _hash(data, i):
    return ((struct.unpack_from("<I", data, i)[0] * 2654435761) & 0xFFFFFFFF) >> (32 - HB)


def tokens(data):
    """the greedy parse: a literal is an int, a match (length, distance)"""
    n, table, out, free = len(data), {}, [], 0
    for s0 in range(0, n, S):
        s1 = min(s0 + S, n)
        cands = {i: table.get(_hash(data, i)) for i in range(s0, s1) if i + 4 <= n}     # every position reads first ...
        for i in cands:                                                                  # ... then the strip is put in
            h = _hash(data, i)
            table[h] = max(table.get(h, -1), i)
        while free < s1:                     # (L(i) is worked out only where the parse arrives: the others are never asked for)
            cand, l = cands.get(free), 0
            if cand is not None and free - cand <= MAX_DIST:
                cap = min(MAX_MATCH, n - free)
                while l < cap and data[cand + l] == data[free + l]:
                    l += 1
            if l >= MIN_MATCH:
                out.append((l, free - cand))
                free += l
            else:
                out.append(data[free])
                free += 1
    return out


_LEN_SYM = [0] * 3 + [max(i for i in range(29) if M.LEN_BASE[i] <= n and (i == 28 or n < 258)) for n in range(3, 259)]


def len_sym(length):
    return _LEN_SYM[length]


def dist_sym(dist):
    return bisect.bisect_right(M.DIST_BASE, dist) - 1


def histograms(toks):
    lit, dist = [0] * 286, [0] * 30
    for t in toks:
        if isinstance(t, int):
            lit[t] += 1
        else:
            lit[257 + len_sym(t[0])] += 1
            dist[dist_sym(t[1])] += 1
    lit[256] = 1
    return lit, dist


def code_lengths(count, limit):
    """-> the length of every symbol of count[] (0: unused)"""
    lens = [0] * len(count)
    order = sorted((s for s in range(len(count)) if count[s]), key=lambda s: (count[s], s))
    m = len(order)
    if m == 0:
        return lens
    if m == 1:
        lens[order[0]] = 1
        return lens
    w, parent = [count[s] for s in order] + [0] * (m - 1), [0] * (2 * m - 1)
    a, b = 0, m
    for k in range(m, 2 * m - 1):
        for _ in range(2):
            if a < m and (b >= k or w[a] <= w[b]):
                idx, a = a, a + 1
            else:
                idx, b = b, b + 1
            w[k] += w[idx]
            parent[idx] = k
    depth = [0] * (2 * m - 1)
    for k in range(2 * m - 3, -1, -1):
        depth[k] = depth[parent[k]] + 1
    bl = [0] * (limit + 1)
    for j in range(m):
        bl[min(depth[j], limit)] += 1
    over = sum(bl[l] << (limit - l) for l in range(1, limit + 1)) - (1 << limit)
    for _ in range(over):
        bits = limit - 1
        while bl[bits] == 0:
            bits -= 1
        bl[bits] -= 1
        bl[bits + 1] += 2
        bl[limit] -= 1
    j = 0
    for l in range(limit, 0, -1):
        for _ in range(bl[l]):
            lens[order[j]] = l
            j += 1
    return lens


def header_runs(seq):
    """the greedy run-length coding of the lengths -> [(symbol, extra bits' value)]"""
    out, p = [], 0
    while p < len(seq):
        v, r = seq[p], 1
        cap = 6 if v else 138
        while r < cap and p + r < len(seq) and seq[p + r] == v:
            r += 1
        if v == 0 and r >= 11:
            out.append((18, r - 11))
        elif v == 0 and r >= 3:
            out.append((17, r - 3))
        elif v != 0 and r >= 3 and p > 0 and seq[p - 1] == v:
            out.append((16, r - 3))
        else:
            out.append((v, 0))
            r = 1
        p += r
    return out


CL_XBITS = {16: 2, 17: 3, 18: 7}


def deflate_piece(data):
    """-> (the raw DEFLATE stream of one piece, the form chosen)"""
    n = len(data)
    assert n <= PIECE
    toks = tokens(data)
    lit, dist = histograms(toks)
    lit_len, dist_len = code_lengths(lit, 15), code_lengths(dist, 15)
    hlit = max([257] + [s + 1 for s in range(286) if lit_len[s]])
    hdist = max([1] + [s + 1 for s in range(30) if dist_len[s]])
    runs = header_runs(lit_len[:hlit] + dist_len[:hdist])
    cl_hist = [0] * 19
    for s, _ in runs:
        cl_hist[s] += 1
    cl_len = code_lengths(cl_hist, 7)
    hclen = max([4] + [i + 1 for i in range(19) if cl_len[M.CL_ORDER[i]]])
    extra = sum(lit[257 + c] * M.LEN_EXTRA[c] for c in range(29)) + sum(dist[c] * M.DIST_EXTRA[c] for c in range(30))
    fixed = 3 + sum(lit[s] * M.FIXED_LIT[s] for s in range(286)) + 5 * sum(dist) + extra
    dyn = (3 + 14 + 3 * hclen + sum(cl_len[s] + CL_XBITS.get(s, 0) for s, _ in runs) + sum(lit[s] * lit_len[s] for s in range(286))
           + sum(dist[s] * dist_len[s] for s in range(30)) + extra)
    stored = 8 * (5 + n)
    w = M.Writer()
    if stored <= fixed and stored <= dyn:
        w.stored(data, last=True)
        assert w.nbits == stored
        return w.bytes(), STORED
    if fixed <= dyn:
        form, cost, lit_codes, dist_codes = FIXED, fixed, M.FIXED_LIT_CODES, M.FIXED_DIST_CODES
        w.bits(1, 1).bits(1, 2)
    else:
        form, cost, lit_codes, dist_codes = DYNAMIC, dyn, M._canonical(lit_len), M._canonical(dist_len)
        cl_codes = M._canonical(cl_len)
        w.bits(1, 1).bits(2, 2).bits(hlit - 257, 5).bits(hdist - 1, 5).bits(hclen - 4, 4)
        for i in range(hclen):
            w.bits(cl_len[M.CL_ORDER[i]], 3)
        for s, x in runs:
            w.code(cl_codes[s]).bits(x, CL_XBITS.get(s, 0))
    for t in toks:
        if isinstance(t, int):
            w.code(lit_codes[t])
        else:
            ls, ds = len_sym(t[0]), dist_sym(t[1])
            w.code(lit_codes[257 + ls]).bits(t[0] - M.LEN_BASE[ls], M.LEN_EXTRA[ls])
            w.code(dist_codes[ds]).bits(t[1] - M.DIST_BASE[ds], M.DIST_EXTRA[ds])
    w.code(lit_codes[256])
    assert w.nbits == cost, (w.nbits, cost)
    return w.bytes(), form


def block(data):
    """one piece as a BGZF block -> (bytes, form)"""
    raw, form = deflate_piece(data)
    return M.wrap(raw, data), form


def deflate_file(data):
    """-> (the file, blk_off with the EOF block's offset last, [stored, fixed, dynamic] counts)"""
    data = bytes(data)
    out, off, counts = bytearray(), [], [0, 0, 0]
    for at in range(0, len(data), PIECE):
        b, form = block(data[at:at + PIECE])
        off.append(len(out))
        out += b
        counts[form] += 1
    off.append(len(out))
    return bytes(out + M.EOF_BLOCK), off, counts


# ---- the inputs of the tests: what each one was built to reach is asserted in tests/test_bgzf_deflate_model_cpu.py ---------------------
TEXT_40 = b"Sphinx of black quartz, judge my vow 123"


def far_repeat(dist):
    """eight letters twice, `dist` bytes apart, zeros around them: the only candidate of the second group is the first"""
    d = bytearray(300 + dist + 300)
    d[300:308] = d[300 + dist:308 + dist] = b"ABCDEFGH"
    return bytes(d)


def no_repeats(values):
    """every value followed by the two bytes (128 ..) of its index: no 4-byte group occurs twice, so there is no match at all"""
    out = bytearray()
    for k, v in enumerate(values):
        out += bytes((v, 128 + (k >> 7), 128 + (k & 127)))
    return bytes(out)


def fibonacci_counts():
    """18 byte values with the counts 1, 2, 3, 5, ... 4181 in a shuffled order, without matches; the end-of-block symbol is the ladder's
    first 1 (a second value with the count 1 would split it into two chains of half the depth): a tree 17 levels deep"""
    vals, a, b = [], 1, 2
    for k in range(18):
        vals += [k] * a
        a, b = b, a + b
    random.Random(4).shuffle(vals)
    return no_repeats(vals)


def all_values_equally():
    """every byte value 64 times in 64 different orders (x -> x * odd + k): no 4-byte group twice"""
    return bytes((x * (2 * k + 1) + k) & 255 for k in range(64) for x in range(256))


def skewed(n_sym=30, ratio=1.62, total=6000, seed=1):
    r = random.Random(seed)
    w = [ratio ** k for k in range(n_sym)]
    out = []
    for k in range(n_sym):
        out += [k] * max(1, int(total * w[n_sym - 1 - k] / sum(w)))
    r.shuffle(out)
    return bytes(out)
