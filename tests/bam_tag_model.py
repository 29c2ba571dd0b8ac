"""A plain model of the BAM write side (include/polypolish_hip.h: pp_bam_tagged).  Test infrastructure: it does not call the library.
tagged() is the uncompressed stream U' -- the header, then every record again, an aligned record whose verdict is 0 with block_size + 8
and ZP:Z:fail appended --, frame() the file: U' cut every 65,280 bytes, each piece one BGZF block around one stored DEFLATE block built
by hand from struct and zlib.crc32 (NOT bgzf_model.block(d, 0): zlib at level 0 splits a 65,279- or 65,280-byte input into two stored
blocks), then the EOF block.  tests/test_bam_tag_model_cpu.py pins both; the GPU tests compare the device's bytes with frame(tagged())."""
import struct
import zlib

import numpy as np

import bam_model as bm
import bgzf_model as zm

PAYLOAD = 65280                      # 0xff00: htslib's payload size
BLOCK = PAYLOAD + 31                 # block b of a file starts at b * BLOCK
TAG = b"ZPZfail\0"                   # 5A 50 5A 66 61 69 6C 00
ARG, LIMIT = 4, 5
CUT, SMALL, PAST = "cut", "small", "past"      # what is wrong with a record, in the order it is looked for (pp_bam_host.h: W_*)


class TagError(Exception):
    def __init__(self, code, kind, bad_record=None):
        super().__init__(f"[{code}] {kind} at record {bad_record}")
        self.code, self.kind, self.bad_record = code, kind, bad_record


def _le32(b, at):
    return b[at] | b[at + 1] << 8 | b[at + 2] << 16 | b[at + 3] << 24


def defect(b, o):
    """what pp_bam_tagged refuses the record at offset o for, or None"""
    n = len(b)
    if o > n or n - o < 4:
        return CUT
    bs = _le32(b, o)
    if bs < 32:
        return SMALL
    if bs > n - o - 4:
        return PAST
    return None


def tagged(b, records_at, rec_off, passed):
    """-> U'.  Raises TagError(ARG, kind, r) for the first defective record in index order; only without one TagError(ARG, "n_pass")
    where `passed` has another length than the number of aligned records."""
    b = bytes(b)
    if records_at > len(b):
        raise TagError(ARG, "records_at")
    offs = [int(o) for o in rec_off]
    for r, o in enumerate(offs):
        kind = defect(b, o)
        if kind:
            raise TagError(ARG, kind, r)
    aligned = [not (b[o + 18] | b[o + 19] << 8) & 4 for o in offs]
    if sum(aligned) != (0 if passed is None else len(passed)):
        raise TagError(ARG, "n_pass")
    out, a = [b[:records_at]], 0
    for o, al in zip(offs, aligned):
        bs = _le32(b, o)
        fail = False
        if al:
            fail = not passed[a]
            a += 1
        out.append(struct.pack("<I", bs + 8) + b[o + 4:o + 4 + bs] + TAG if fail else b[o:o + 4 + bs])
    return b"".join(out)


def stored_block(piece):
    """one BGZF block around one stored DEFLATE block: len(piece) + 31 bytes"""
    n = len(piece)
    assert n <= PAYLOAD
    return (bytes.fromhex("1f8b08040000000000ff060042430200") + struct.pack("<H", n + 30) + b"\x01" + struct.pack("<HH", n, n ^ 0xFFFF) + piece +
            struct.pack("<II", zlib.crc32(piece), n))


def frame(u):
    """U' -> the file"""
    return b"".join(stored_block(u[at:at + PAYLOAD]) for at in range(0, len(u), PAYLOAD)) + zm.EOF_BLOCK


def blk_off(n_blocks, n_bytes=None):
    """the offsets of a framed file's blocks: what Bgzf(..., mem=MEM_DEVICE) takes; with the file's size the EOF block's as well"""
    off = np.arange(n_blocks, dtype=np.uint64) * np.uint64(BLOCK)
    return off if n_bytes is None else np.concatenate([off, np.array([n_bytes - 28], np.uint64)])


def unframe(f):
    """the file -> U', every block through the BGZF model (walk, inflate, length, CRC)"""
    off, _, end, ok = zm.walk(f)
    assert ok and end == len(f)
    return b"".join(zm.inflate_block(f, at) for at in off)


def own_verdicts(sam_in, sam_out):
    """the filter's own verdict per aligned record, from a SAM text and what `polypolish filter` made of it (bytes): 0 where the output
    line is the input line plus the tag.  (filter_model.failed_lines looks for the tag alone: a line that came with it reads as failed.)"""
    keep = lambda t: [ln for ln in t.split(b"\n") if ln and not ln.startswith(b"@") and not int(ln.split(b"\t")[1]) & 4]      # noqa: E731
    a, b = keep(sam_in), keep(sam_out)
    assert len(a) == len(b) and all(y in (x, x + b"\tZP:Z:fail") for x, y in zip(a, b))
    return np.array([x == y for x, y in zip(a, b)], np.uint8)


# ---- generated inputs, shared by the CPU pin and the GPU test -------------------------------------------------------------------------
HEADER = bm.header_bytes([("ctg_a", 5000), ("ctg_b", 70000)], "@HD\tVN:1.6\n")


def rec(total, flag=0, qname=b"r", tags=b""):
    """one record of exactly `total` bytes (block_size word included, >= 64): NM, then an aux Z field that fills it"""
    base = bm.record(qname, flag, 0, 7, [(4 << 4)], "ACGT", bm.aux("NM", "C", 1) + tags)
    fill = total - len(base) - 4      # XZ Z ... NUL
    assert fill >= 0, (total, len(base))
    return bm.record(qname, flag, 0, 7, [(4 << 4)], "ACGT", bm.aux("NM", "C", 1) + tags + bm.aux("XZ", "Z", "x" * fill))


def records_to(u_len, fail_last=False):
    """([record], [verdict]) that bring U' behind HEADER to exactly u_len bytes: aligned records of 3,000 bytes, the last one as long as
    it takes; fail_last: the last record fails (its 8 bytes are part of u_len)"""
    left = u_len - len(HEADER) - (8 if fail_last else 0)
    recs = []
    while left >= 3000 + 64:
        recs.append(rec(3000, qname=b"q%d" % len(recs)))
        left -= 3000
    recs.append(rec(left, qname=b"last"))
    return recs, [1] * (len(recs) - 1) + [0 if fail_last else 1]


def stream(recs, verdicts, lead=0, pad=None):
    """(bytes, records_at, rec_off, passed) of HEADER and the records behind it (lead, pad: bam_model.lay_out's junk bytes)"""
    body, off = bm.lay_out(recs, lead, pad)
    return HEADER + body, len(HEADER), off + np.uint64(len(HEADER)), np.array(verdicts, np.uint8)


def stream_of(u_len, fail_last=False):
    """(bytes, records_at, rec_off, passed) whose U' has exactly u_len bytes: 0 and 1 without records, else records_to(u_len)"""
    if u_len < 2:
        return b"B" * u_len, u_len, np.zeros(0, np.uint64), np.zeros(0, np.uint8)
    return stream(*records_to(u_len, fail_last))
