"""The plain model of the BGZF front end (pp_bgzf_walk, pp_bgzf_inflate): a pure-Python inflate of one raw-DEFLATE stream that
also REPORTS what the stream exercised, a bit writer for hand-built streams, the BGZF block wrapper / unwrapper / walk, and the
inputs and defect streams that tests/test_bgzf_model_cpu.py pins against zlib and tests/test_bgzf_inflate_gpu.py runs on the
device.  Which malformed code sets are refused is zlib's decision (inftrees.c): an over-subscribed set always, an incomplete one
unless it is a literal/length or distance code whose longest code has one bit (or, for distances, no code at all)."""
import random
import struct
import zlib

LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
MAX_ISIZE = 65536
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


class Defect(Exception):
    """what the model refuses; .kind names it"""

    def __init__(self, kind):
        super().__init__(kind)
        self.kind = kind


# ---- inflate -----------------------------------------------------------------------------------------------------------------------
class _Bits:
    def __init__(self, raw):
        self.raw, self.pos = raw, 0          # pos in bits

    def take(self, n):
        v = 0
        for i in range(n):
            at = self.pos + i
            if at >= 8 * len(self.raw):
                raise Defect("past")
            v |= ((self.raw[at >> 3] >> (at & 7)) & 1) << i
        self.pos += n
        return v


def _code(lens, kind):
    """canonical code of the lengths -> (count per length, symbols by length then symbol); zlib's verdict on the set"""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    left = 1
    for l in range(1, 16):
        left = 2 * left - count[l]
        if left < 0:
            raise Defect("codes:over-subscribed")
    longest = max([l for l in range(16) if count[l]], default=0)
    if left > 0 and (kind == "cl" or longest > 1 or (kind == "lit" and longest == 0)):
        raise Defect("codes:incomplete")
    return count, [s for l in range(1, 16) for s in range(len(lens)) if lens[s] == l]


def _symbol(bits, code):
    count, symbols = code
    c = first = index = 0
    for l in range(1, 16):
        c |= bits.take(1)
        if c - count[l] < first:
            return symbols[index + c - first], l
        index += count[l]
        first = (first + count[l]) << 1
        c <<= 1
    raise Defect("symbol:no such code")


def inflate(raw, limit=MAX_ISIZE):
    """one raw-DEFLATE stream -> (bytes, report); Defect on anything zlib refuses too.  `limit`: Defect("long") beyond it."""
    rep = {"types": [], "blocks": 0, "max_dist": 0, "max_len": 0, "overlaps": 0, "max_lit_code": 0, "max_dist_code": 0,
           "repeats": set(), "stored": [], "no_dist_code": False, "end_bit": 0}
    bits, out = _Bits(raw), bytearray()
    last = 0
    while not last:
        last, kind = bits.take(1), bits.take(2)
        rep["types"].append(kind)
        rep["blocks"] += 1
        if kind == 3:
            raise Defect("btype")
        if kind == 0:
            bits.pos = (bits.pos + 7) & ~7
            n, inv = bits.take(16), bits.take(16)
            if n ^ inv != 0xFFFF:
                raise Defect("stored")
            at = bits.pos >> 3
            if at + n > len(raw):
                raise Defect("past")
            out += raw[at:at + n]
            bits.pos += 8 * n
            rep["stored"].append(n)
            if len(out) > limit:
                raise Defect("long")
            continue
        if kind == 1:
            lit_lens, dist_lens = FIXED_LIT, FIXED_DIST
        else:
            hlit, hdist, hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
            if hlit > 286 or hdist > 30:
                raise Defect("codes:too many")
            cl = [0] * 19
            for i in range(hclen):
                cl[CL_ORDER[i]] = bits.take(3)
            cl_code = _code(cl, "cl")
            lens = []
            while len(lens) < hlit + hdist:
                s, _ = _symbol(bits, cl_code)
                if s < 16:
                    lens.append(s)
                    continue
                rep["repeats"].add(s)
                if s == 16:
                    if not lens:
                        raise Defect("codes:repeat without a length")
                    val, n = lens[-1], 3 + bits.take(2)
                else:
                    val, n = 0, (3 + bits.take(3) if s == 17 else 11 + bits.take(7))
                if len(lens) + n > hlit + hdist:
                    raise Defect("codes:overrun")
                lens += [val] * n
            if lens[256] == 0:
                raise Defect("codes:no end-of-block")
            lit_lens, dist_lens = lens[:hlit], lens[hlit:]
            rep["no_dist_code"] |= not any(dist_lens)
        lit, dist = _code(lit_lens, "lit"), _code(dist_lens, "dist")
        while True:
            s, l = _symbol(bits, lit)
            rep["max_lit_code"] = max(rep["max_lit_code"], l)
            if s < 256:
                out.append(s)
            elif s == 256:
                break
            else:
                if s > 285:
                    raise Defect("symbol:length 286")
                n = LEN_BASE[s - 257] + bits.take(LEN_EXTRA[s - 257])
                d, l = _symbol(bits, dist)
                rep["max_dist_code"] = max(rep["max_dist_code"], l)
                if d > 29:
                    raise Defect("symbol:distance 30")
                d = DIST_BASE[d] + bits.take(DIST_EXTRA[d])
                if d > len(out):
                    raise Defect("distance")
                rep["max_dist"], rep["max_len"] = max(rep["max_dist"], d), max(rep["max_len"], n)
                rep["overlaps"] += d < n
                for _ in range(n):
                    out.append(out[-d])
            if len(out) > limit:
                raise Defect("long")
    rep["end_bit"] = bits.pos
    return bytes(out), rep


# ---- the writer of hand-built streams ------------------------------------------------------------------------------------------------
def _canonical(lens):
    code, codes = 0, {}
    for l in range(1, 16):
        for s, sl in enumerate(lens):
            if sl == l:
                codes[s] = (code, l)
                code += 1
        code <<= 1
    return codes


FIXED_LIT_CODES, FIXED_DIST_CODES = _canonical(FIXED_LIT), _canonical(FIXED_DIST)


class Writer:
    def __init__(self):
        self.out, self.nbits = bytearray(), 0

    def bits(self, v, n):                      # low bit first
        for i in range(n):
            if self.nbits % 8 == 0:
                self.out.append(0)
            self.out[-1] |= ((v >> i) & 1) << (self.nbits % 8)
            self.nbits += 1
        return self

    def code(self, c):                         # a Huffman code: high bit first
        v, n = c
        for i in range(n - 1, -1, -1):
            self.bits((v >> i) & 1, 1)
        return self

    def stored(self, data, last=False, nlen=None):
        self.bits(int(last), 1).bits(0, 2)
        self.nbits = (self.nbits + 7) & ~7
        self.out += struct.pack("<HH", len(data), (~len(data) & 0xFFFF) if nlen is None else nlen) + bytes(data)
        self.nbits += 8 * (4 + len(data))
        return self

    def fixed(self, items, last=False, end=True):
        """items: a literal (int < 256), a (length, distance) pair, or ("lit", symbol) / ("dist", length, symbol): a raw symbol"""
        self.bits(int(last), 1).bits(1, 2)
        for it in items:
            if isinstance(it, int):
                self.code(FIXED_LIT_CODES[it])
            elif it[0] == "lit":
                self.code(FIXED_LIT_CODES[it[1]])
            else:
                n, d = (it[1], None) if it[0] == "dist" else it
                ls = max(i for i in range(29) if LEN_BASE[i] <= n and (i == 28 or n < 258))
                self.code(FIXED_LIT_CODES[257 + ls]).bits(n - LEN_BASE[ls], LEN_EXTRA[ls])
                if d is None:
                    self.code(FIXED_DIST_CODES[it[2]])
                else:
                    ds = max(i for i in range(30) if DIST_BASE[i] <= d)
                    self.code(FIXED_DIST_CODES[ds]).bits(d - DIST_BASE[ds], DIST_EXTRA[ds])
        if end:
            self.code(FIXED_LIT_CODES[256])
        return self

    def dynamic_header(self, hlit, hdist, cl_lens, last=True):
        """the head of a dynamic block: HLIT HDIST HCLEN = 19 and all 19 lengths of the code lengths' code (by symbol)"""
        self.bits(int(last), 1).bits(2, 2).bits(hlit - 257, 5).bits(hdist - 1, 5).bits(15, 4)
        for s in CL_ORDER:
            self.bits(cl_lens.get(s, 0), 3)
        return _canonical([cl_lens.get(s, 0) for s in range(19)])

    def bytes(self):
        return bytes(self.out)


# ---- BGZF -------------------------------------------------------------------------------------------------------------------------
def wrap(raw, data, extra_front=b"", isize=None, crc=None):
    """one BGZF block around a raw-DEFLATE stream that inflates to `data`; extra_front: subfields in front of BC"""
    xlen = len(extra_front) + 6
    total = 12 + xlen + len(raw) + 8
    assert total <= 65536, total
    head = struct.pack("<4BI2BH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, xlen) + extra_front + b"BC" + struct.pack("<HH", 2, total - 1)
    return head + raw + struct.pack("<II", zlib.crc32(data) if crc is None else crc, len(data) if isize is None else isize)


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return c.compress(data) + c.flush()


def block(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, **kw):
    return wrap(deflate(data, level, strategy), data, **kw)


def unwrap(b, at=0):
    """the block at `at` -> (total, payload offset in b, payload length, crc, isize); Defect("header:...") as pp_bgzf_walk refuses"""
    left = len(b) - at
    if at > len(b) or left < 12:
        raise Defect("header:range")
    if b[at:at + 3] != b"\x1f\x8b\x08" or not b[at + 3] & 4:
        raise Defect("header:magic")
    xlen = struct.unpack_from("<H", b, at + 10)[0]
    if xlen > left - 12:
        raise Defect("header:extra")
    p, bsize = 0, None
    while xlen - p >= 4:
        slen = struct.unpack_from("<H", b, at + 12 + p + 2)[0]
        if slen > xlen - p - 4:
            raise Defect("header:extra")
        if bsize is None and b[at + 12 + p:at + 14 + p] == b"BC" and slen == 2:
            bsize = struct.unpack_from("<H", b, at + 16 + p)[0]
        p += 4 + slen
    if p != xlen:
        raise Defect("header:extra")
    if bsize is None:
        raise Defect("header:no BC")
    total = bsize + 1
    if total < 12 + xlen + 8:
        raise Defect("header:bsize")
    if total > left:
        raise Defect("header:past")
    crc, isize = struct.unpack_from("<II", b, at + total - 8)
    if isize > MAX_ISIZE:
        raise Defect("header:isize")
    return total, at + 12 + xlen, total - 12 - xlen - 8, crc, isize


def walk(b, start=0):
    """-> (blk_off, out_off, end, ok): the BSIZE chain as pp_bgzf_walk follows it; ok False: block len(blk_off) at `end` is refused"""
    off, out, at = [], [0], start
    while at < len(b):
        try:
            total, _, _, _, isize = unwrap(b, at)
        except Defect:
            return off, out, at, False
        off.append(at)
        out.append(out[-1] + isize)
        at += total
    return off, out, at, True


def inflate_block(b, at=0):
    """the model of the device's work on one block: header, stream, length, CRC -> bytes; Defect otherwise"""
    total, pay, n, crc, isize = unwrap(b, at)
    data, _ = inflate(b[pay:pay + n], limit=isize)
    if len(data) != isize:
        raise Defect("short")
    if zlib.crc32(data) != crc:
        raise Defect("crc")
    return data


# ---- the inputs of the tests ----------------------------------------------------------------------------------------------------------
FULL = 65280      # 0xff00: what htslib puts into a block


def bam_like(n=FULL, seed=1, whole=False):
    """bytes with the statistics of BAM records: a fixed part with small fields, a name that counts up, packed SEQ, QUAL, an NM tag"""
    r, out, i = random.Random(seed), bytearray(), 0
    template = bytes(r.choice(b"\x11\x12\x14\x18\x21\x22\x24\x28\x41\x42\x44\x48\x81\x82\x84\x88") for _ in range(20000))
    while len(out) < n:
        l_seq = r.choice((150, 150, 150, 151, 100, 75))
        at = r.randrange(len(template) - 80)
        seq = bytearray(template[at:at + (l_seq + 1) // 2])
        for _ in range(r.choice((0, 0, 1, 2))):
            seq[r.randrange(len(seq))] = r.choice(b"\x11\x12\x14\x18\xff")
        name = b"read_%d/%d\0" % (i // 2, 1 + i % 2)
        qual = bytes(min(41, max(2, int(r.gauss(36, 5)))) for _ in range(l_seq))
        core = struct.pack("<iiBBHHHIiii", r.randrange(3), at * 2, len(name), r.choice((60, 60, 60, 0, 23)), 4680 + r.randrange(40), 1,
                           r.choice((99, 147, 83, 163, 0, 16)), l_seq, r.randrange(3), at * 2 + r.randrange(500), r.randrange(-600, 600))
        rec = core + name + struct.pack("<I", l_seq << 4) + bytes(seq) + qual + b"NMC" + bytes([r.choice((0, 0, 0, 1, 2))])
        if whole and len(out) + 4 + len(rec) > n:      # whole records only: a little short of n
            break
        out += struct.pack("<I", len(rec)) + rec
        i += 1
    return bytes(out[:n])


def acgt(n=FULL, seed=10):      # (this seed: the stream uses the repeat symbols 16, 17 and 18)
    r = random.Random(seed)
    return bytes(r.choice(b"ACGT") for _ in range(n))


def noise(n, seed=3):
    return random.Random(seed).getrandbits(8 * n).to_bytes(n, "little") if n else b""


def table_inputs():
    """the rows of the issue's table: name -> (data, raw stream)"""
    bam, text, rnd = bam_like(), acgt(), noise(60000)
    return {
        "stored": (bam, deflate(bam, 0)),
        "fixed": (bam, deflate(bam, 6, zlib.Z_FIXED)),
        "dynamic_bam": (bam, deflate(bam, 6)),
        "dynamic_acgt": (text, deflate(text, 6)),
        "zeros": (bytes(FULL), deflate(bytes(FULL), 6)),
        "huffman_only": (bam, deflate(bam, 6, zlib.Z_HUFFMAN_ONLY)),
        "two_stored": (rnd, deflate(rnd, 6)),
        "empty": (b"", deflate(b"", 6)),
        "one_byte": (b"x", deflate(b"x", 6)),
    }


def seam_streams():
    """hand-built streams: name -> (data, raw stream)"""
    r = random.Random(7)
    out = {}

    def add(name, w):
        raw = w.bytes()
        out[name] = (inflate(raw)[0], raw)

    half = noise(32768, 5)
    add("match_258_at_32768_first_in_a_fixed_block", Writer().stored(half).fixed([(258, 32768), 65, (3, 1)], last=True))
    items = list(b"abcdefghijklmnopqrstuvwxyz" * 3)
    for d in (1, 2, 3, 4, 63, 64, 65):
        items += [(3, d), r.randrange(256), (258, d), r.randrange(256)]
    add("matches_3_and_258_at_small_distances", Writer().fixed(items, last=True))
    add("stored_len_0_and_1", Writer().stored(b"").stored(b"q").stored(b"", last=True))
    add("stored_largest", Writer().stored(noise(65536 - 26 - 5, 6), last=True))    # header 18 + footer 8, the block's 5 bytes
    for k in range(8):                                                              # the fixed block ends at bit (10 + 9 k) % 8
        add(f"stored_after_huffman_phase_{(10 + 9 * k) % 8}", Writer().fixed([200 + i for i in range(k)]).stored(b"tail-%d" % k, last=True))
    add("five_blocks_mixed", Writer().stored(b"one ").fixed(list(b"two "), last=False).stored(b"three ")
        .fixed([ord("f"), (5, 1), (4, 10)]).stored(b" five", last=True))
    w = Writer().fixed([150 + i for i in range(6)], last=True)                      # 3 + 6 * 9 + 7 = 64 bits
    assert w.nbits == 64
    add("last_code_ends_on_the_last_bit", w)
    add("isize_65536", Writer().stored(noise(30000, 8)).fixed([7, (258, 1)] * 3 + [9], last=False).stored(noise(65536 - 30000 - 3 * 259 - 1, 9), last=True))
    return out


def defect_blocks():
    """name -> (block, kind the model names, how zlib meets it: "raw" = zlib.decompress(payload, -15) raises, "gzip" = (block, 31)
    raises, None = a BGZF matter zlib does not see).  Every stream is made from valid ones by the writer above."""
    good = b"The kernel's duty is to return an error. " * 4
    out = {}

    def add(name, raw, kind, how="raw", **kw):
        out[name] = (wrap(raw, kw.pop("data", good), **kw), kind, how)

    add("block_type_3", Writer().fixed(list(good)).bits(1, 1).bits(3, 2).bytes(), "btype")
    add("len_not_nlen", Writer().stored(good, last=True, nlen=len(good)).bytes(), "stored")
    add("distance_beyond_the_output", Writer().fixed([65, 66, (3, 3)], last=True).bytes(), "distance")
    valid = deflate(good, 6)
    add("longer_than_isize", valid, "long", "gzip", isize=len(good) - 1)
    add("shorter_than_isize", valid, "short", "gzip", isize=len(good) + 1)
    add("stream_past_the_payload", deflate(bam_like(4000), 6)[:-9], "past", data=bam_like(4000))
    w = Writer()
    w.dynamic_header(257, 1, {s: 1 for s in range(19)})
    add("oversubscribed_code_lengths", w.bits(0, 64).bytes(), "codes:over-subscribed")
    w = Writer()
    cl = w.dynamic_header(257, 1, {0: 1, 16: 1})
    add("repeat_16_without_a_length", w.code(cl[16]).bits(0, 2).bits(0, 64).bytes(), "codes:repeat without a length")
    w = Writer()
    cl = w.dynamic_header(257, 1, {0: 1, 18: 1})
    add("code_lengths_overrun", w.code(cl[18]).bits(127, 7).code(cl[18]).bits(127, 7).bits(0, 64).bytes(), "codes:overrun")
    add("length_symbol_286", Writer().fixed([65, ("lit", 286)], last=True).bits(0, 32).bytes(), "symbol:length 286")
    add("distance_symbol_30", Writer().fixed([65, ("dist", 3, 30)], last=True).bits(0, 32).bytes(), "symbol:distance 30")
    flipped = bytearray(Writer().stored(good, last=True).bytes())
    flipped[20] ^= 0x40
    add("flipped_payload_byte", bytes(flipped), "crc", "gzip")
    add("wrong_footer_crc", valid, "crc", "gzip", crc=zlib.crc32(good) ^ 1)
    blk = bytearray(block(good))
    blk[1] = 0x8c
    out["bad_magic"] = (bytes(blk), "header:magic", "gzip")
    blk = bytearray(block(good))
    struct.pack_into("<H", blk, 16, len(blk) + 40)
    out["bsize_past_the_end"] = (bytes(blk), "header:past", None)
    return out


def many_blocks(n=2000, seed=13):
    """n blocks of 300 .. 65280 bytes of mixed content and settings -> (file bytes, [data])"""
    r = random.Random(seed)
    bam, text = bam_like(FULL, 21), acgt(FULL, 22)
    sizes = [300, FULL] + [r.choice((300, 301, 1000, 4093, 20000, FULL)) if r.random() < .9 else r.randrange(300, FULL + 1) for _ in range(n - 2)]
    blocks, datas = [], []
    for i, size in enumerate(sizes):
        src = r.choice((bam, text, bam))
        at = r.randrange(len(src) - size + 1)
        data = src[at:at + size] if r.random() < .95 else noise(size, i)
        level, strategy = r.choice(((6, zlib.Z_DEFAULT_STRATEGY), (1, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_DEFAULT_STRATEGY), (0, zlib.Z_DEFAULT_STRATEGY),
                                    (6, zlib.Z_FIXED), (6, zlib.Z_HUFFMAN_ONLY), (6, zlib.Z_DEFAULT_STRATEGY)))
        blocks.append(block(data, level, strategy))
        datas.append(data)
    return b"".join(blocks), datas
