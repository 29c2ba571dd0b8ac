"""A plain model of the device walk over the BAM block_size chain (include/polypolish_hip.h: pp_bam_walk_device; polypolish_amd/csrc/
pp_bam_walk.hip).  Test infrastructure: it does not call the library.  It restates the SCHEME, not only the result: the chunk tables
band by band, the entry zones, the pass-through, the slow path, the groups and the chain over them -- so that a test can say which
path an input takes before any GPU is involved (tests/test_bam_walk_model_cpu.py pins it to bam_model.walk; tests/test_bam_walk_gpu.py
holds the library's path counts against it).

A record takes 4 + block_size >= 36 bytes, so the record behind one at offset o starts at o + 36 or later.  With chunks of C bytes, a
zone of the first Z offsets of every chunk and groups of G chunks:
  tables   per chunk and offset o, from the top band of 32 offsets down: last[o] = the last offset inside the chunk on the chain from
           o (its step leaves the chunk, reaches the end of the bytes, or is refused), cnt[o] = the good records on the way.  The 32
           offsets of a band only look at bands above.  The first Z entries are kept.
  a chunk  entered at e: at or behind its end -> passed through; inside the zone -> (last, cnt) and one step at last; behind the
           zone (the record in front is longer than Z) -> the slow path, record by record.  The chunk that holds the start is always
           walked record by record and counts as none of the three.
  a group  the composition of its chunks for an entry into the zone of its first chunk, as long as every chunk is passed or entered
           through its zone and no step is refused; otherwise, and in the start's group, the chain goes chunk by chunk.
walk() returns (n_rec, end, kind, offsets, stats): kind OK / CUT / SMALL / PAST / START, offsets None where the chain breaks, stats =
[chunks on the chain, entered through a zone, on the slow path, passed through]."""
import numpy as np

OK, CUT, SMALL, PAST, START = 0, 1, 2, 3, 4
SERIAL = None


def step(b, n, o):
    """one record at o <= n: (kind, the offset behind it or o)"""
    left = n - o
    if left < 4:
        return CUT, o
    bs = int(b[o]) | int(b[o + 1]) << 8 | int(b[o + 2]) << 16 | int(b[o + 3]) << 24
    if bs < 32:
        return SMALL, o
    if bs > left - 4:
        return PAST, o
    return OK, o + 4 + bs


def zone_tables(b, C, Z):
    """-> (last, cnt): int64 arrays [number of chunks, Z], chunk-relative; every chunk at once, the bands one after the other"""
    n = len(b)
    nch = (n + C - 1) // C
    pad = np.zeros(nch * C + 4, np.int64)
    pad[:n] = np.frombuffer(bytes(b), np.uint8)
    o_all = np.arange(nch * C, dtype=np.int64)
    bs = pad[:-4] | pad[1:-3] << 8 | pad[2:-2] << 16 | pad[3:-1] << 24
    left = n - o_all
    good = (left >= 4) & (bs >= 32) & (bs <= left - 4)           # (an offset at or behind n: left <= 0, never good)
    nxt = o_all + 4 + bs
    hi = np.minimum((np.arange(nch, dtype=np.int64) + 1) * C, n)[:, None]
    lo = (np.arange(nch, dtype=np.int64) * C)[:, None]
    last, cnt = np.zeros((nch, C), np.int64), np.zeros((nch, C), np.int64)
    rows = np.arange(nch)[:, None]
    assert C % 32 == 0
    for band in range(C // 32 - 1, -1, -1):
        rel = band * 32 + np.arange(32, dtype=np.int64)[None, :]
        o = lo + rel
        g, t = good[o], nxt[o]
        stays = g & (t < hi)
        trel = np.where(stays, t - lo, 0)
        assert not stays.any() or int(trel[stays].min()) >= (band + 1) * 32, "a record shorter than 36 bytes"
        last[:, band * 32:band * 32 + 32] = np.where(stays, last[rows, trel], rel)
        cnt[:, band * 32:band * 32 + 32] = np.where(stays, cnt[rows, trel] + 1, g.astype(np.int64))
    return last[:, :Z].copy(), cnt[:, :Z].copy()


class Walk:
    def __init__(self, b, start, C, Z, G):
        self.b, self.n, self.start, self.C, self.Z, self.G = bytes(b), len(b), int(start), C, Z, G
        self.nch = (self.n + C - 1) // C
        self.c0 = self.start // C
        self.last, self.cnt = zone_tables(self.b, C, Z)

    def hi(self, c):
        return min((c + 1) * self.C, self.n)

    def walk_chunk(self, c, e):
        k = 0
        while e < self.hi(c):
            kind, t = step(self.b, self.n, e)
            if kind != OK:
                return e, k, kind
            k, e = k + 1, t
        return e, k, OK

    def zone_step(self, c, e):
        la, k = c * self.C + int(self.last[c, e - c * self.C]), int(self.cnt[c, e - c * self.C])
        kind, t = step(self.b, self.n, la)
        return (t if kind == OK else la), k, kind

    def chunk_step(self, c, e):
        """entry e into chunk c -> (entry of the next chunk or the break's offset, records, kind, via)"""
        assert e >= c * self.C
        if c == self.c0:
            return self.walk_chunk(c, e) + ("direct",)
        if e >= self.hi(c):
            return e, 0, OK, "pass"
        if e - c * self.C < self.Z:
            return self.zone_step(c, e) + ("zone",)
        return self.walk_chunk(c, e) + ("slow",)

    def group_entry(self, g, z):
        """the table entry of group g for entry z of its first chunk: (entry of the next group, records, chunks passed) or SERIAL"""
        cb, ce = g * self.G, min((g + 1) * self.G, self.nch)
        e, cnt, passed = cb * self.C + z, 0, 0
        if e >= self.n:
            return SERIAL
        for c in range(cb, ce):
            if e >= self.hi(c):
                passed += 1
                continue
            if e - c * self.C >= self.Z:
                return SERIAL
            e, k, kind = self.zone_step(c, e)
            if kind != OK:
                return SERIAL
            cnt += k
        return e, cnt, passed

    def run(self):
        if self.start > self.n:
            return 0, self.start, START, None, [0, 0, 0, 0]
        st = {"chain": 0, "zone": 0, "slow": 0, "pass": 0, "direct": 0}
        stats = lambda: [st["chain"], st["zone"], st["slow"], st["pass"]]     # noqa: E731
        if self.start == self.n:
            return 0, self.start, OK, [], stats()
        e, total, g0, n_groups = self.start, 0, self.c0 // self.G, (self.nch + self.G - 1) // self.G
        gentry = {}
        for g in range(g0, n_groups):
            cb, ce = (self.c0 if g == g0 else g * self.G), min((g + 1) * self.G, self.nch)
            gentry[g] = e
            if g != g0:
                if e >= min(ce * self.C, self.n):
                    st["chain"] += ce - cb
                    st["pass"] += ce - cb
                    continue
                z = e - cb * self.C
                t = self.group_entry(g, z) if z < self.Z else SERIAL
                if t is not SERIAL:
                    e, total = t[0], total + t[1]
                    st["chain"] += ce - cb
                    st["zone"] += ce - cb - t[2]
                    st["pass"] += t[2]
                    continue
            for c in range(cb, ce):
                e, k, kind, via = self.chunk_step(c, e)
                st["chain"] += 1
                st[via] += 1
                total += k
                if kind != OK:
                    return total, e, kind, None, stats()
        # every chunk's entry from its group's entry, then the offsets chunk by chunk
        end, off = e, []
        for g in range(g0, n_groups):
            e = gentry[g]
            for c in range(self.c0 if g == g0 else g * self.G, min((g + 1) * self.G, self.nch)):
                at, k = e, self.chunk_step(c, e)[1]
                for _ in range(k):
                    off.append(at)
                    at = step(self.b, self.n, at)[1]
                e = self.chunk_step(c, e)[0]
        assert len(off) == total and e == end
        return total, end, OK, off, stats()


def walk(b, start=0, C=16384, Z=1024, G=64):
    return Walk(b, start, C, Z, G).run()


# ---- hand-built inputs: the seams of the device walk (shared by the CPU pin of the paths they take and the GPU test) ----------------------
CHAIN, ZONE, SLOW, PASS = 0, 1, 2, 3        # indices into stats


def rec(length, fill=0xA5):
    """a record of `length` >= 36 bytes in all: its block_size word and filler"""
    assert length >= 36
    return int(length - 4).to_bytes(4, "little") + bytes([fill]) * (length - 4)


def fill_to(out, target, rng, lens=(36, 37, 41, 64, 100, 150, 333)):
    """records appended to the bytearray `out` until it is exactly `target` bytes long; -> the offsets of the records added"""
    off = []
    assert target == len(out) or target - len(out) >= 36
    while len(out) < target:
        rem = target - len(out)
        ln = min(rem, int(rng.choice(lens)))
        if 0 < rem - ln < 36:
            ln = rem if rem < 72 else rem - 36
        off.append(len(out))
        out += rec(ln, int(rng.integers(0, 256)))
    return off


def junk(n, rng):
    return bytes(rng.integers(0, 256, n, dtype=np.uint8))


def cases(C, Z, G, seed=7):
    """[(name, bytes, start, check)]: check(stats) says whether the input took the path it was built for (None: nothing to say).
    Every chain here holds; breaks() plants the defects."""
    rng = np.random.default_rng(seed)
    out = []

    def add(name, b, start=0, check=None):
        out.append((name, bytes(b), start, check))

    for k in (0, 1, 2, 3):                                  # a block_size word that starts k bytes in front of a boundary
        b = bytearray()
        fill_to(b, C - k, rng)
        fill_to(b, 2 * C + 500, rng)
        add(f"word {k} in front of a boundary", b)
    for d in (0, 1, 2, 3, 4):                               # the bytes end d behind a boundary
        b = bytearray()
        if d == 0:
            fill_to(b, 2 * C, rng)
        else:
            fill_to(b, 2 * C - 50, rng)
            b += rec(50 + d)
        add(f"n_bytes {d} behind a boundary", b)
        if d == 1:
            add("from == n_bytes", b, len(b))
    add("n_bytes 0", b"")
    add("n_bytes 36", rec(36))
    for lead in (C - 1, C, C + 1, C + Z + 100, 2 * C + 77):  # from on, around a boundary; behind the zone of its chunk; behind junk
        b = bytearray(junk(lead, rng))
        fill_to(b, lead + 2 * C + 200, rng)
        add(f"from {lead - C} behind a boundary", b, lead)
    b = bytearray()
    fill_to(b, 3 * 36 * (C // 36) + 36 * 7, rng, lens=(36,))
    add("36-byte records", b, 0, lambda st: st[SLOW] == 0 and st[PASS] == 0)
    b = bytearray()
    fill_to(b, 3 * C + 123, rng, lens=tuple(range(36, 101)))
    add("records of 36..100 bytes", b, 0, lambda st: st[SLOW] == 0)
    b = bytearray()                                          # longer than the zone, shorter than a chunk
    fill_to(b, C - 100, rng)
    b += rec(Z + 500)
    fill_to(b, 3 * C + 10, rng)
    add("a record longer than the zone", b, 0, lambda st: st[SLOW] > 0)
    b = bytearray()                                          # more than two whole chunks
    fill_to(b, C + C // 2, rng)
    b += rec(3 * C)
    fill_to(b, len(b) + C + 300, rng)
    add("a record over two whole chunks", b, 0, lambda st: st[PASS] >= 2)
    b = bytearray(junk((G - 1) * C + 10, rng))               # ... a whole group
    fill_to(b, G * C - 100, rng)
    b += rec(G * C + 200)
    fill_to(b, len(b) + 2 * C + 300, rng)
    add("a record over a whole group", b, (G - 1) * C + 10, lambda st: st[PASS] >= G and st[ZONE] > 0)
    # ---- the chain from group to group: the start's group goes chunk by chunk, the later ones through their tables
    lead = (G - 2) * C + 5
    b = bytearray(junk(lead, rng))
    fill_to(b, G * C, rng)                                   # a record starts at the first byte of group 1
    fill_to(b, 2 * G * C + 3 * C, rng)
    add("group seam at a group's first byte", b, lead, lambda st: st[SLOW] == 0 and st[PASS] == 0 and st[ZONE] == st[CHAIN] - 1)
    b = bytearray(junk(lead, rng))
    fill_to(b, (G + 3) * C - 50, rng)
    b += rec(50 + C + 300)                                   # skips a chunk in the middle of group 1: its table counts the pass
    fill_to(b, 2 * G * C - 50, rng)
    b += rec(50 + C + 300)                                   # skips the first chunk of group 2
    fill_to(b, 2 * G * C + 4 * C, rng)
    add("group seam through a pass-through", b, lead, lambda st: st[PASS] == 2 and st[SLOW] == 0)
    b = bytearray(junk(lead, rng))
    fill_to(b, (G + 5) * C - 100, rng)
    b += rec(Z + 500)                                        # a slow chunk in the middle of group 1: its table says chunk by chunk
    fill_to(b, 2 * G * C - 100, rng)
    b += rec(Z + 500)                                        # group 2 is entered behind the zone of its first chunk
    fill_to(b, 2 * G * C + 4 * C, rng)
    add("group seam through a slow chunk", b, lead, lambda st: st[SLOW] == 2 and st[PASS] == 0)
    # ---- hostile filler: bytes off the chain that read as block_size words
    for w, what in ((0, "0"), (31, "31"), (32, "32"), (0xFFFFFFFF, "0xFFFFFFFF"), (None, "exactly to n_bytes")):
        b = bytearray()
        offs = fill_to(b, 2 * C + 700, rng, lens=(200, 333, 1000))
        n = len(b)
        for o in offs:
            ln = int.from_bytes(b[o:o + 4], "little")
            for p in range(o + 4 + (o % 3), o + 4 + ln - 4, 7):
                b[p:p + 4] = (n - p - 4 if w is None else w).to_bytes(4, "little")
        add(f"off-chain words {what}", b, 0, lambda st: st[SLOW] == 0)
    return out


def breaks(C, Z, G, seed=9):
    """[(name, bytes, start, kind, check)]: the three kinds of break planted in the first chunk, over a boundary, in a zone, behind a
    zone (the slow path finds it), in the last chunk, in the second group"""
    rng = np.random.default_rng(seed)
    small = bytearray()
    offs = fill_to(small, C - 2, rng)
    first = offs[len(offs) // 2]
    offs += fill_to(small, 2 * C - 100, rng)
    small += rec(Z + 500)
    slow = len(small)
    offs.append(slow - Z - 500)
    offs += fill_to(small, 4 * C + 50, rng)
    lead = (G - 1) * C + 7
    big = bytearray(junk(lead, rng))
    big_offs = fill_to(big, (G + 3) * C + 11, rng)
    places = (("first chunk", small, 0, first, None), ("over a boundary", small, 0, C - 2, None),
              ("in a zone", small, 0, min(o for o in offs if o >= C), None),
              ("behind a zone", small, 0, min(o for o in offs if o > slow), lambda st: st[SLOW] > 0),
              ("last chunk", small, 0, offs[-1], None),
              ("second group", big, lead, min(o for o in big_offs if o >= (G + 1) * C + Z), lambda st: st[ZONE] >= 2 and st[SLOW] == 0))
    out = []
    for where, base, start, o, check in places:
        for kind in (CUT, SMALL, PAST):
            b = bytearray(base)
            if kind == CUT:
                del b[o + 3:]
            elif kind == SMALL:
                b[o:o + 4] = (31).to_bytes(4, "little")
            else:
                b[o:o + 4] = (len(b) - o - 3).to_bytes(4, "little")
            out.append((f"{('', 'cut', 'small', 'past')[kind]} {where}", bytes(b), start, kind, check, o))
    return out
