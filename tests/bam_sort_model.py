"""A plain model of pp_bam_sort and pp_bam_tagged_head (include/polypolish_hip.h): the coordinate order of BAM records, the header
that says SO:coordinate, and the sorted stream.  Test infrastructure: it does not call the library.  tests/test_bam_sort_model_cpu.py
pins it to hand-written headers and to bam_model's encoder; tests/test_bam_sort_gpu.py runs the device link (pp_bam_sort.hip) against it.

key(record) is 64 bits: the high word ref_id, or 0xFFFFFFFF for ref_id == -1; the low word (uint32)(pos + 1) << 1 | reverse strand, in
32 bits.  perm is the STABLE order of the indices by that key: reference id, position, strand, input order.  This is the project's
reading of `samtools sort`'s coordinate order; it has not been compared with samtools.

bai() is the definition of the sorted file's .bai -- one chunk per maximal run of records with one (reference, bin), the linear index
filled from the right, the pseudo-bin 37450, n_no_coor; no merging of bins or chunks: a valid BAI, not `samtools index`'s bytes --
and query() / read_chunks() a plain reader of it.  tests/test_bam_index_gpu.py runs pp_bam_index against it; the CPU test holds the
definition to a hand-computed index and to what a brute-force scan finds."""
import struct

import numpy as np

import bam_model as bm
import bam_tag_model as tm
import regroup_model as rm

ARG, LIMIT = 4, 5
POS, REF = "pos", "ref"             # what pp_bam_sort refuses a record for, behind bam_tag_model's CUT / SMALL / PAST
HD_LINE = b"@HD\tVN:1.6\tSO:coordinate\n"


class SortError(Exception):
    def __init__(self, code, kind, bad_record=None):
        super().__init__(f"[{code}] {kind} at record {bad_record}")
        self.code, self.kind, self.bad_record = code, kind, bad_record


def fields(b, o):
    """(ref_id, pos, flag) of the record at offset o"""
    ref_id, pos = struct.unpack_from("<ii", b, o + 4)
    return ref_id, pos, b[o + 18] | b[o + 19] << 8


def key_of(ref_id, pos, flag):
    return ((ref_id if ref_id >= 0 else 0xFFFFFFFF) << 32) | ((((pos + 1) & 0xFFFFFFFF) << 1) & 0xFFFFFFFF) | ((flag >> 4) & 1)


def head_sorted(head):
    """the BAM header `head` (magic ... reference table, nothing behind it) with the first line of its text made to say SO:coordinate;
    raises SortError(ARG, "header") for what is no header or ends elsewhere than at len(head)"""
    head = bytes(head)
    try:
        h = bm.header(head)
    except bm.BamError:
        raise SortError(ARG, "header")
    if h["records_at"] != len(head):
        raise SortError(ARG, "header")
    l_text = bm._le32(head, 4)
    text = head[8:8 + l_text]
    body = text.rstrip(b"\0")
    pad = text[len(body):]
    nl = body.find(b"\n")
    eol = len(body) if nl < 0 else nl
    if eol and body[eol - 1:eol] == b"\r":
        eol -= 1
    line, rest = body[:eol], body[eol:]
    if line == b"@HD" or line.startswith(b"@HD\t"):
        cols = line.split(b"\t")
        at = next((i for i, c in enumerate(cols) if i and c.startswith(b"SO:")), None)
        if at is None:
            cols.append(b"SO:coordinate")
        else:
            cols[at] = b"SO:coordinate"
        body = b"\t".join(cols) + rest
    else:
        body = HD_LINE + body
    new = body + pad
    if len(new) > 0x7FFFFFFF:
        raise SortError(LIMIT, "l_text")
    return head[:4] + struct.pack("<I", len(new)) + new + head[8 + l_text:]


def keys(b, records_at, rec_off):
    """the records' keys (np.uint64) and flags; raises SortError for the header, then for the first defective record in index order"""
    b = bytes(b)
    if records_at > len(b):
        raise SortError(ARG, "records_at")
    try:
        n_ref = len(bm.header(b[:records_at])["names"])
        if bm.header(b[:records_at])["records_at"] != records_at:
            raise SortError(ARG, "header")
    except bm.BamError:
        raise SortError(ARG, "header")
    out, flags = [], []
    for r, o in enumerate(int(x) for x in rec_off):
        kind = tm.defect(b, o)
        if kind:
            raise SortError(ARG, kind, r)
        ref_id, pos, flag = fields(b, o)
        if pos < -1:
            raise SortError(ARG, POS, r)
        if ref_id < -1 or ref_id >= n_ref:
            raise SortError(ARG, REF, r)
        out.append(key_of(ref_id, pos, flag))
        flags.append(flag)
    return np.array(out, np.uint64), np.array(flags, np.uint16)


def perm_of(key):
    return np.argsort(np.asarray(key, np.uint64), kind="stable").astype(np.uint32)


def sort(b, records_at, rec_off):
    """-> {"perm", "rec_off": rec_off[perm], "head", "counts": (records that changed place, records with ref_id == -1), "flag"}"""
    k, flag = keys(b, records_at, rec_off)
    p = perm_of(k)
    off = np.asarray(rec_off, np.uint64)
    return {"perm": p, "rec_off": off[p] if len(p) else off[:0], "head": head_sorted(bytes(b)[:records_at]),
            "counts": (int((p != np.arange(len(p), dtype=np.uint32)).sum()), int((k >> np.uint64(32) == np.uint64(0xFFFFFFFF)).sum())), "flag": flag}


def carry_pass(flag, p, passed):
    """one byte per ALIGNED input record -> the same verdicts in the numbering of the sorted records (regroup_model's rule)"""
    return rm.carry_pass(flag, p, passed)


def tagged_head(b, records_at, rec_off, passed, head):
    """pp_bam_tagged_head's stream: bam_tag_model.tagged with `head` in the place of b[:records_at]"""
    u = tm.tagged(b, records_at, rec_off, passed)
    return bytes(head) + u[records_at:]


def sorted_stream(b, records_at, rec_off, passed):
    """the uncompressed sorted file: pp_bam_sort, pp_bam_sorted_pass, pp_bam_tagged_head"""
    s = sort(b, records_at, rec_off)
    v = None if passed is None else carry_pass(s["flag"], s["perm"], passed)
    return tagged_head(b, records_at, s["rec_off"], v, s["head"])


# ---- the index ------------------------------------------------------------------------------------------------------------------------
PAYLOAD = tm.PAYLOAD
PSEUDO_BIN = 37450
MAX_END = 1 << 29
ORDER, PLACED, END = "order", "placed", "end"   # what pp_bam_index refuses a record for, behind CUT / SMALL / PAST


def reg2bin(beg, end):
    """the SAM specification's section 5.3: the smallest bin that holds [beg, end)"""
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def reg2bins(beg, end):
    """... every bin that may hold a record overlapping [beg, end)"""
    end -= 1
    out = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out.extend(range(first + (beg >> shift), first + (end >> shift) + 1))
    return out


def voffset(u, blk_off):
    """stream offset u -> virtual offset: the block that holds u (a multiple of 65,280: the block that STARTS there), the offset in it"""
    return (int(blk_off[u // PAYLOAD]) << 16) | (u % PAYLOAD)


def ref_end(b, o):
    """(pos, end, flag, ref_id) of the record at o: end = pos + the lengths of its M D N = X runs, pos + 1 where that is 0 or flag & 4"""
    ref_id, pos, flag = fields(b, o)
    l_name, n_cig = b[o + 12], b[o + 16] | b[o + 17] << 8
    span = 0
    for i in range(n_cig):
        w = bm._le32(b, o + 36 + l_name + 4 * i)
        if (w & 15) in (0, 2, 3, 7, 8):
            span += w >> 4
    return pos, pos + (span if span and not flag & 4 else 1), flag, ref_id


def index_tables(b, n_head, rec_off, passed, n_ref, blk_off):
    """what the index is made of: per reference {"bins": {bin: [(beg, end)]}, "linear": [ioffset], "span": (beg, end), "mapped",
    "unmapped"}, and n_no_coor.  Raises SortError for the first record, in index order, that cannot be indexed."""
    b = bytes(b)
    offs = [int(o) for o in rec_off]
    for r, o in enumerate(offs):
        kind = tm.defect(b, o)
        if kind:
            raise SortError(ARG, kind, r)
    for r, o in enumerate(offs):                          # (a CIGAR that leaves its record is a defect like the walk's)
        if 32 + b[o + 12] + 4 * (b[o + 16] | b[o + 17] << 8) > bm._le32(b, o):
            raise SortError(ARG, "cigar", r)
    aligned = [not (b[o + 18] & 4) for o in offs]
    if sum(aligned) != (0 if passed is None else len(passed)):
        raise SortError(ARG, "n_pass")
    for x in blk_off:
        if int(x) >= 1 << 48:
            raise SortError(LIMIT, "blk_off")
    refs = [{"bins": {}, "linear": {}, "span": None, "mapped": 0, "unmapped": 0} for _ in range(n_ref)]
    u, a, n_no_coor, last, prev_key = n_head, 0, 0, {}, None
    for r, (o, al) in enumerate(zip(offs, aligned)):
        fail = bool(al and not passed[a])
        a += 1 if al else 0
        u_end = u + 4 + bm._le32(b, o) + 8 * fail
        pos, end, flag, ref_id = ref_end(b, o)
        if ref_id < -1 or ref_id >= n_ref:
            raise SortError(ARG, REF, r)
        if ref_id >= 0 and pos < 0:
            raise SortError(ARG, PLACED, r)
        key = (ref_id & 0xFFFFFFFF, pos & 0xFFFFFFFF if ref_id < 0 else pos)
        if ref_id < 0:
            key = (key[0], 0)                              # unplaced records are in order whatever their pos
        if prev_key is not None and key < prev_key:
            raise SortError(ARG, ORDER, r)
        prev_key = key
        if ref_id >= 0 and end > MAX_END:
            raise SortError(LIMIT, END, r)
        vb, ve = voffset(u, blk_off), voffset(u_end, blk_off)
        u = u_end
        if ref_id < 0:
            n_no_coor += 1
            continue
        R = refs[ref_id]
        bin_ = reg2bin(pos, end)
        if last.get("at") == (ref_id, bin_):               # the run goes on: its chunk ends where this record ends
            R["bins"][bin_][-1] = (R["bins"][bin_][-1][0], ve)
        else:
            R["bins"].setdefault(bin_, []).append((vb, ve))
        last["at"] = (ref_id, bin_)
        for w in range(pos >> 14, ((end - 1) >> 14) + 1):
            R["linear"][w] = min(R["linear"].get(w, vb), vb)
        R["span"] = (R["span"][0] if R["span"] else vb, ve)
        R["unmapped" if flag & 4 else "mapped"] += 1
    for R in refs:
        n_intv = max(R["linear"]) + 1 if R["linear"] else 0
        lin, nxt = [0] * n_intv, 0
        for w in range(n_intv - 1, -1, -1):
            nxt = R["linear"].get(w, nxt)
            lin[w] = nxt
        R["linear"] = lin
    return refs, n_no_coor


def bai_bytes(refs, n_no_coor):
    out = [b"BAI\1", struct.pack("<i", len(refs))]
    for R in refs:
        out.append(struct.pack("<i", len(R["bins"]) + (1 if R["span"] else 0)))
        for bin_ in sorted(R["bins"]):
            out.append(struct.pack("<Ii", bin_, len(R["bins"][bin_])))
            out.extend(struct.pack("<QQ", *c) for c in R["bins"][bin_])
        if R["span"]:
            out.append(struct.pack("<IiQQQQ", PSEUDO_BIN, 2, R["span"][0], R["span"][1], R["mapped"], R["unmapped"]))
        out.append(struct.pack("<i", len(R["linear"])))
        out.extend(struct.pack("<Q", v) for v in R["linear"])
    out.append(struct.pack("<Q", n_no_coor))
    return b"".join(out)


def bai(b, n_head, rec_off, passed, n_ref, blk_off):
    """the .bai of the file pp_bam_tagged_head makes of the same arguments, whose blocks start at blk_off (n_blocks + 1 entries)"""
    return bai_bytes(*index_tables(b, n_head, rec_off, passed, n_ref, blk_off))


def level0_blk_off(u_len):
    """the blocks of pp_bam_tagged's level-0 file of u_len stream bytes: b * 65,311, the EOF block's last"""
    return [k * tm.BLOCK for k in range((u_len + PAYLOAD - 1) // PAYLOAD + 1)]


def parse_bai(data):
    """-> ([{"bins": {bin: [(beg, end)]}, "linear": [ioffset]}], n_no_coor or None); the pseudo-bin is a bin like the others"""
    assert data[:4] == b"BAI\1"
    n_ref, at = struct.unpack_from("<i", data, 4)[0], 8
    refs = []
    for _ in range(n_ref):
        n_bin, at = struct.unpack_from("<i", data, at)[0], at + 4
        bins = {}
        for _ in range(n_bin):
            bin_, n_chunk = struct.unpack_from("<Ii", data, at)
            at += 8
            assert bin_ not in bins
            bins[bin_] = [struct.unpack_from("<QQ", data, at + 16 * i) for i in range(n_chunk)]
            at += 16 * n_chunk
        n_intv, at = struct.unpack_from("<i", data, at)[0], at + 4
        refs.append({"bins": bins, "linear": list(struct.unpack_from("<%dQ" % n_intv, data, at))})
        at += 8 * n_intv
    n_no_coor = struct.unpack_from("<Q", data, at)[0] if at + 8 <= len(data) else None
    assert at + (8 if n_no_coor is not None else 0) == len(data)
    return refs, n_no_coor


def query(data, tid, beg, end):
    """a plain BAI reader: the chunks [(beg, end)] of virtual offsets that may hold a record of reference tid overlapping [beg, end),
    in file order -- the bins of reg2bins, without the chunks that end at or in front of the linear index's lower bound"""
    refs, _ = parse_bai(data)
    R = refs[tid]
    w = beg >> 14
    if w >= len(R["linear"]):
        return []
    low = R["linear"][w]
    out = [c for bin_ in reg2bins(beg, end) for c in R["bins"].get(bin_, []) if c[1] > low]
    return sorted(out)


_OPENED = {}


def _open(f):
    """a BGZF BAM file inflated block by block: {"base": {block offset: stream offset}, "len": {block offset: its bytes}, "u", "bounds"}
    (the last file is kept: a test asks about one file many times)"""
    import bgzf_model as zm
    if _OPENED.get("f") != f:
        blocks, _, end, ok = zm.walk(f)
        assert ok and end == len(f)
        base, size, u = {}, {}, bytearray()
        for co in blocks:
            piece = zm.inflate_block(f, co)                # header, stream, CRC32, ISIZE: zlib starts at this block
            base[co], size[co] = len(u), len(piece)
            u += piece
        starts, _, ok = bm.walk(u, bm.header(u)["records_at"])
        assert ok
        _OPENED.clear()
        _OPENED.update(f=f, base=base, size=size, u=bytes(u), bounds=set(starts) | {len(u)})
    return _OPENED


def read_chunks(f, chunks):
    """the records of a BGZF BAM file inside the chunks of virtual offsets: [stream offset of a record].  Every block is inflated
    on its own (bgzf_model.inflate_block), so a chunk is read with zlib started at its block; a chunk that starts or ends anywhere
    but in a block of the file and between two records raises AssertionError"""
    F = _open(bytes(f))
    base, size, u, bounds = F["base"], F["size"], F["u"], F["bounds"]
    out = []
    for vb, ve in chunks:
        assert vb >> 16 in base and ve >> 16 in base, "a chunk starts or ends in no block of the file"
        assert (vb & 0xFFFF) <= size[vb >> 16] and (ve & 0xFFFF) <= size[ve >> 16]
        at, stop = base[vb >> 16] + (vb & 0xFFFF), base[ve >> 16] + (ve & 0xFFFF)
        assert at in bounds and stop in bounds and at < stop, "a chunk starts or ends inside a record"
        while at < stop:
            out.append(at)
            at += 4 + bm._le32(u, at)
        assert at == stop
    return out


# ---- generated inputs, shared by the CPU pin and the GPU test -------------------------------------------------------------------------
REFS = [("ctg_a", 5000), ("ctg_b", 70000), ("ctg_c", 1 << 29)]
HEADER = bm.header_bytes(REFS, "@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:ctg_a\tLN:5000\n")


def rec(ref_id, pos, flag=0, qname=b"r", n=4):
    """a small record at (ref_id, pos): n bases, one M run"""
    return bm.record(qname, flag, ref_id, pos, [(n << 4)], "ACGT"[:n] if n <= 4 else "A" * n, bm.aux("NM", "C", 0))


def stream(recs, header=HEADER, lead=0, pad=None):
    """(bytes, records_at, rec_off) of the header and the records behind it (lead, pad: bam_model.lay_out's junk bytes)"""
    body, off = bm.lay_out(recs, lead, pad)
    return header + body, len(header), off + np.uint64(len(header))


def random_records(n, seed, n_ref=3, max_pos=3000, unplaced=0.1):
    """n records over n_ref references: positions with many ties, both strands, some unaligned-but-placed, some unplaced"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        flag = int(rng.integers(0, 2)) << 4
        if rng.random() < unplaced:
            out.append(rec(-1, -1, flag | 4, b"u%d" % i))
            continue
        if rng.random() < 0.05:
            flag |= 4
        out.append(rec(int(rng.integers(0, n_ref)), int(rng.integers(0, max_pos)), flag, b"q%d" % i, n=int(rng.integers(1, 5))))
    return out
