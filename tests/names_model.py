"""A plain model of pp_names (include/polypolish_hip.h): a dict in first-appearance order over calls -- the id of a name is the number
of distinct names in front of its first occurrence.  Test infrastructure: tests/test_names_model_cpu.py pins it to what the library's
host loader already does (pp_filter_load's read numbers), tests/test_names_gpu.py runs the device table (pp_names.hip) against it on
the cases built here.  It does not call the library.

A call is a triple (bytes, off, len) of numpy arrays (uint8, uint64, uint32), as pp_names_ids takes it."""
import numpy as np


def ids(state, names):
    """state: a dict that lives as long as the table (start with {}); names: a list of bytes -> their ids"""
    return [state.setdefault(bytes(n), len(state)) for n in names]


def sam_column(text, column=0, aligned_only=True):
    """QNAME (column 0) or RNAME (column 2) of the records of a SAM text (bytes) in file order, as bytes"""
    out = []
    for ln in text.split(b"\n"):
        if not ln or ln[:1] == b"@":
            continue
        cols = ln.split(b"\t")
        if not (aligned_only and int(cols[1]) & 4):
            out.append(cols[column])
    return out


def empty_qname_rule(read_id, qnames, flag):
    """The reference's quirk on top of interned ids (alignment.rs:255; gate_model.raw_from_text has the same rule): an ALIGNED
    record joins the aligned record in front when that one's QNAME is equal -- or EMPTY.  In a table the empty name has an id
    of its own, so a caller who wants the quirk copies the predecessor's id; a new group whose id the group in front borrowed that
    way gets a fresh one (>= 2^40).  -> read_id, changed only where an empty QNAME is involved."""
    out, fresh = np.array(read_id, np.uint64), 1 << 40
    prev = None
    for r in np.flatnonzero((np.asarray(flag) & 4) == 0).tolist():
        if prev is not None and (qnames[prev] in ("", b"") or qnames[prev] == qnames[r]):
            out[r] = out[prev]
        elif prev is not None and out[r] == out[prev]:
            out[r], fresh = fresh, fresh + 1
        prev = r
    return out


def names_of(call):
    b, off, ln = call
    raw = b.tobytes()
    return [raw[int(o):int(o) + int(n)] for o, n in zip(off.tolist(), ln.tolist())]


def pack(names, lead=0, tail=b""):
    """the names back to back behind `lead` filler bytes, `tail` behind the last: nothing else follows"""
    names = [bytes(n) for n in names]
    ln = np.array([len(n) for n in names], np.uint32)
    off = (lead + np.cumsum(ln, dtype=np.int64) - ln).astype(np.uint64)
    return np.frombuffer(b"\xA5" * lead + b"".join(names) + tail, np.uint8).copy(), off, ln


class Builder:
    """a byte array in which every name is planted at a chosen `off & 7`, with chosen bytes behind it"""

    def __init__(self):
        self.buf, self.off, self.len = bytearray(), [], []

    def place(self, name, align, tail=b""):
        while len(self.buf) & 7 != align:
            self.buf.append(0xA5)
        self.off.append(len(self.buf))
        self.len.append(len(name))
        self.buf += name + tail
        return len(self.off) - 1

    def call(self):
        return np.frombuffer(bytes(self.buf), np.uint8).copy(), np.array(self.off, np.uint64), np.array(self.len, np.uint32)


SEAM_LENS = tuple(range(18)) + (31, 32, 33)      # around one, two and four 8-byte loads
PAIR_BYTES = (0, 7, 8, 15)                       # first and last byte of the first and of the second load


def seam_case(seed=7):
    """-> (call, quads, pairs).  quads: for every off & 7 and every length of SEAM_LENS the indices (copy, copy, last byte changed,
    one byte shorter) -- the two copies at different alignments and followed by DIFFERENT bytes, the changed and the shorter string
    None at length 0.  pairs: indices of two 16-byte names that differ in one byte of PAIR_BYTES only."""
    rng = np.random.default_rng(seed)
    B, quads, pairs = Builder(), [], []
    for a in range(8):
        for n in SEAM_LENS:
            name = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
            i1 = B.place(name, a, b"\x01\x02\x03\x04\x05\x06\x07\x08\x09")
            i2 = B.place(name, (a + 3) & 7, b"\xFE\xFD\xFC\xFB\xFA\xF9\xF8\xF7\xF6")
            i3 = i4 = None
            if n:
                i3 = B.place(name[:-1] + bytes([name[-1] ^ 0x5A]), a, b"\x01\x02\x03")
                i4 = B.place(name[:-1], (a + 5) & 7, bytes([name[-1] ^ 0xFF]) + b"\x00" * 8)     # (not the byte the longer name has there)
            quads.append((i1, i2, i3, i4))
    for a in (0, 3):
        for k in PAIR_BYTES:
            name = rng.integers(0, 256, 16, dtype=np.uint8).tobytes()
            other = name[:k] + bytes([name[k] ^ 0x01]) + name[k + 1:]
            pairs.append((B.place(name, a, b"zz"), B.place(other, (a + 1) & 7, b"yy")))
    return B.call(), quads, pairs


def shifted(call, by):
    """the same names, every offset `by` bytes further on"""
    b, off, ln = call
    return np.concatenate([np.full(by, 0x5A, np.uint8), b]), off + np.uint64(by), ln


LONG = 10000


def raw_bytes_case(seed=8):
    rng = np.random.default_rng(seed)
    long_name = rng.integers(0, 256, LONG, dtype=np.uint8).tobytes()
    names = [b"\x00", b"", b"\x00\x00", b"\xff", b"a\x00b", b"a\x00c", b"\xff\xfe\x80", b"a\x00b", long_name, b"\x00",
             long_name[:-1] + bytes([long_name[-1] ^ 0x80]), b"", long_name, b"\xff\xfe\x80\x00", b"\xff"]
    return pack(names, lead=3)


def array_end_cases():
    """calls whose last name ends exactly where the array ends, n_bytes no multiple of 8: the last name shorter than one load, longer
    than one load, and the whole array shorter than one load"""
    a = pack([b"first_name", b"second", b"xyz"], lead=2)          # 21 bytes: "xyz" has no eight bytes left
    b = pack([b"first_name", b"thirteen_byte"], lead=4)           # 27 bytes: one load, then five bytes one by one
    c = pack([b"ab", b"abc"], lead=0)                             # 5 bytes
    d = pack([b"first_name", b"thirteen_byt?", b"xyz", b"abc", b"x"], lead=1)    # 31 bytes: the last name is the array's last byte
    for call in (a, b, c, d):
        assert len(call[0]) % 8 and int(call[1][-1]) + int(call[2][-1]) == len(call[0])
    return [a, b, c, d]


def order_case(seed=9, n=5000, distinct=1200):
    """n names of `distinct` different ones, shuffled (every one of them occurs); lengths 3..40"""
    rng = np.random.default_rng(seed)
    pool = [(b"read_%d:" % i) + b"x" * int(rng.integers(0, 33)) for i in range(distinct)]
    pick = np.concatenate([np.arange(distinct), rng.integers(0, distinct, n - distinct)])
    rng.shuffle(pick)
    return [pool[i] for i in pick.tolist()]


def contention_case(copies=4096):
    return [b"one", b"two", b"three"] + [b"the_one_name_everybody_has"] * copies


def growth_calls(seed=10, calls=4, per_call=5000):
    rng = np.random.default_rng(seed)
    out = []
    for c in range(calls):
        out.append([b"g%d_%d_" % (c, i) + rng.integers(97, 123, int(rng.integers(0, 20)), dtype=np.uint8).tobytes() for i in range(per_call)])
    return out


LOOKUP_SWEEP = 2048 * 256       # names k_nm_lookup takes in one sweep of its workgroups (NM_LOOKUP_BLOCKS x 256, pp_names.hip)


def numbered_case(n, distinct, seed=11):
    """n names "r<k>" with k drawn from `distinct` numbers, made with numpy (a case too large for lists of bytes)
    -> (call, ids by first appearance)"""
    rng = np.random.default_rng(seed)
    r = rng.integers(0, distinct, n).astype(np.int64) * 7919
    nd = np.ones(n, np.int64)
    for k in range(1, 12):
        nd += r >= 10 ** k
    ln = nd + 1
    off = np.cumsum(ln) - ln + 3
    b = np.full(int(ln.sum()) + 3, 0xA5, np.uint8)
    b[off] = ord("r")
    for d in range(int(nd.max())):
        sel = nd > d
        b[(off + ln - 1 - d)[sel]] = 48 + (r[sel] // 10 ** d) % 10
    _, first, inverse = np.unique(r, return_index=True, return_inverse=True)
    rank = np.empty(len(first), np.uint64)
    rank[np.argsort(first)] = np.arange(len(first), dtype=np.uint64)
    return (b, off.astype(np.uint64), ln.astype(np.uint32)), rank[inverse]
