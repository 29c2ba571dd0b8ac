"""A plain model of pp_bam_sam (include/polypolish_hip.h): uncompressed BAM -> SAM text.  Test infrastructure: it does not call the
library.  It is the DEFINITION of the bytes: tests/test_bam_sam_model_cpu.py pins it to hand-written lines, to C's "%g" and to
sam_bam_model (decode(encode(T)) == T for every canonical text T), tests/test_bam_sam_gpu.py runs the device (pp_bam_sam.hip) against it
byte for byte.  The output was never compared with `samtools view`.

decode(bam, records_at, rec_off, passed=None) -> the text, or raises Refused(code, record).

The header (header_text): the l_text bytes of header text without their trailing NULs, a "\\n" appended where the text is not empty and
does not end in one; where no line's first column is exactly "@SQ" and n_ref > 0, one line "@SQ\\tSN:<name>\\tLN:<l_ref>" per
reference in order.  The text is cut at "\\n" only and copied as it is, whatever its bytes.  bam[0, records_at) must be a BAM header
that ends exactly at records_at, else Refused(ARG, None); a synthesised @SQ line whose name is empty, "*", "=" or holds a byte outside
0x21..0x7E, or whose l_ref lies outside 1 .. 2^31-1, would be a line pp_sam_header refuses: Refused(LIMIT, None).

One record is one line, QNAME FLAG RNAME POS MAPQ CIGAR RNEXT PNEXT TLEN SEQ QUAL and the aux fields joined by tabs, ended by "\\n";
a 0 in `passed` (one byte per record with flag & 4 == 0, in index order) puts "\\tZP:Z:fail" in front of the "\\n".

Refusals: the first refused record in index order wins; inside one record every ARG defect goes in front of every LIMIT (both kinds
carry nothing but their code and the record).  The ARG defects are pp_bam_tagged's three (the offset, block_size < 32, a record past
the bytes) and pp_bam_records' (block_size below its parts, the name, a CIGAR op above 8, refID or next_refID outside [-1, n_ref),
an aux field that is cut, of unknown type, a Z / H without NUL, a B of unknown sub-type or too long), and pos or next_pos below -1.
LIMIT is a valid record that has no SAM line (see _limits).  Another number of verdicts than aligned records is Refused(ARG, None),
reported only where no record is refused.

Decided here, beyond the issue's list:
  * a name in the reference table that a record USES (refID or next_refID >= 0) and that is empty, "*", "=" or holds a byte outside
    0x21..0x7E is LIMIT at that record: the line would not read back as it was written;
  * a CIGAR word of length 0 prints as "0M": well-formed text, pp_sam_bam's own limit; the same holds for the bin (an end above 2^29)
    and a float beyond 10^+-22: every line written here is a line pp_sam_bam PARSES, its capacity limits stay its own;
  * bin and mapq are not checked; the unused nibble behind an odd l_seq is not looked at; QUAL whose first byte is 0xFF is "*"
    whatever follows; NM is not looked at."""
import struct

import numpy as np

import bam_model

ARG, LIMIT = 4, 5
NIBBLE = bam_model.NIBBLE
OPS = bam_model.OPS
TAG = b"\tZP:Z:fail"
HEX = b"0123456789abcdefABCDEF"


class Refused(Exception):
    def __init__(self, code, record=None, what=""):
        super().__init__(f"[{code}] record {record}: {what}")
        self.code, self.record, self.what = code, record, what


def fmt_g(bits):
    """C's printf("%g") of the float32 with these bits, widened to double"""
    return ("%g" % struct.unpack("<f", struct.pack("<I", bits & 0xFFFFFFFF))[0]).encode()


def _name_ok(name):
    return len(name) > 0 and name not in (b"*", b"=") and all(0x21 <= c <= 0x7E for c in name)


def header_text(bam, records_at):
    """-> (the header's text, names)"""
    bam = bytes(bam)
    if records_at > len(bam):
        raise Refused(ARG, None, "records_at")
    try:
        h = bam_model.header(bam[:records_at])
    except bam_model.BamError:
        raise Refused(ARG, None, "header") from None
    if h["records_at"] != records_at:
        raise Refused(ARG, None, "records_at")
    l_text = struct.unpack_from("<I", bam, 4)[0]
    t = bam[8:8 + l_text].rstrip(b"\0")
    if t and not t.endswith(b"\n"):
        t += b"\n"
    if h["names"] and not any(ln.split(b"\t")[0] == b"@SQ" for ln in t.split(b"\n")):
        for name, ln in zip(h["names"], h["ref_len"].tolist()):
            if not _name_ok(name) or not 1 <= ln <= 2**31 - 1:
                raise Refused(LIMIT, None, "@SQ")
            t += b"@SQ\tSN:" + name + b"\tLN:" + str(ln).encode() + b"\n"
    return t, h["names"]


def _structure(b, o, n_ref):
    """the ARG defects of the record at offset o, in the order they are looked for: a word, or None"""
    n = len(b)
    if o > n or n - o < 4:
        return "cut"
    bs = struct.unpack_from("<I", b, o)[0]
    if bs < 32:
        return "small"
    if bs > n - o - 4:
        return "past"
    kind, _, _ = bam_model._one(b, o, list(range(n_ref)) + [0], n_ref)
    if kind:
        return kind
    ref_id, pos = struct.unpack_from("<ii", b, o + 4)
    next_ref, next_pos = struct.unpack_from("<ii", b, o + 24)
    if next_ref < -1 or next_ref >= n_ref:
        return "next_ref_id"
    if pos < -1 or next_pos < -1:
        return "pos"
    return None


def _fields(b, o):
    """the record at o, free of ARG defects -> its parts"""
    c = o + 4
    bs = struct.unpack_from("<I", b, o)[0]
    ref_id, pos, lrn, mapq, _bin, nc, flag, ls, next_ref, next_pos, tlen = struct.unpack_from("<iiBBHHHIiii", b, c)
    at = c + 32
    name = b[at:at + lrn - 1]
    at += lrn
    words = struct.unpack_from(f"<{nc}I", b, at)
    at += 4 * nc
    seq = bytes(ord(NIBBLE[(b[at + i // 2] >> (0 if i & 1 else 4)) & 15]) for i in range(ls))
    at += (ls + 1) // 2
    qual = b[at:at + ls]
    at += ls
    aux, e = [], c + bs
    while at < e:
        tag, ty = b[at:at + 2], chr(b[at + 2])
        at += 3
        if ty in "ZH":
            z = b.index(b"\0", at)
            aux.append((tag, ty, b[at:z]))
            at = z + 1
        elif ty == "B":
            sub, cnt = chr(b[at]), struct.unpack_from("<I", b, at + 1)[0]
            size = bam_model.B_SIZE[sub]
            aux.append((tag, ty, (sub, b[at + 5:at + 5 + cnt * size])))
            at += 5 + cnt * size
        else:
            size = bam_model.FIXED[ty]
            aux.append((tag, ty, b[at:at + size]))
            at += size
    return dict(ref_id=ref_id, pos=pos, mapq=mapq, flag=flag, next_ref=next_ref, next_pos=next_pos, tlen=tlen, name=name, words=words,
                seq=seq, qual=qual, aux=aux)


def _is_float(v4):
    return (struct.unpack("<I", v4)[0] & 0x7F800000) != 0x7F800000


def _limits(f, names):
    """what keeps a valid record from having a SAM line: a word, or None"""
    name = f["name"]
    if len(name) == 0 or name[:1] == b"@" or any(not 0x21 <= c <= 0x7E for c in name):
        return "QNAME"
    for i in (f["ref_id"], f["next_ref"]):
        if i >= 0 and not _name_ok(names[i]):
            return "reference name"
    if len(f["qual"]) and f["qual"][0] != 0xFF and any(q > 93 for q in f["qual"]):
        return "QUAL"
    for tag, ty, v in f["aux"]:
        if not (chr(tag[0]).isascii() and chr(tag[0]).isalpha() and chr(tag[1]).isascii() and chr(tag[1]).isalnum()):
            return "tag"
        if ty == "A" and not 0x21 <= v[0] <= 0x7E:
            return "A"
        if ty == "Z" and any(not 0x20 <= c <= 0x7E for c in v):
            return "Z"
        if ty == "H" and (len(v) & 1 or any(c not in HEX for c in v)):
            return "H"
        if ty == "f" and not _is_float(v):
            return "f"
        if ty == "B" and v[0] == "f" and any(not _is_float(v[1][i:i + 4]) for i in range(0, len(v[1]), 4)):
            return "B:f"
    return None


def _aux_text(tag, ty, v):
    head = tag + b":"
    if ty == "A":
        return head + b"A:" + v
    if ty in bam_model.INT_FMT:
        return head + b"i:" + str(struct.unpack(bam_model.INT_FMT[ty], v)[0]).encode()
    if ty == "f":
        return head + b"f:" + fmt_g(struct.unpack("<I", v)[0])
    if ty in "ZH":
        return head + ty.encode() + b":" + v
    sub, raw = v
    size = bam_model.B_SIZE[sub]
    out = head + b"B:" + sub.encode()
    for i in range(0, len(raw), size):
        e = raw[i:i + size]
        out += b"," + (fmt_g(struct.unpack("<I", e)[0]) if sub == "f" else str(struct.unpack(bam_model.INT_FMT[sub], e)[0]).encode())
    return out


def line(f, names, fail=False):
    """the parts of one record -> its line, "\\n" included"""
    rname = b"*" if f["ref_id"] < 0 else names[f["ref_id"]]
    rnext = b"*" if f["next_ref"] < 0 else (b"=" if f["next_ref"] == f["ref_id"] else names[f["next_ref"]])
    cigar = b"".join(str(w >> 4).encode() + OPS[w & 15].encode() for w in f["words"]) or b"*"
    qual = b"*" if not f["qual"] or f["qual"][0] == 0xFF else bytes(q + 33 for q in f["qual"])
    cols = [f["name"], str(f["flag"]).encode(), rname, str(f["pos"] + 1).encode(), str(f["mapq"]).encode(), cigar, rnext,
            str(f["next_pos"] + 1).encode(), str(f["tlen"]).encode(), f["seq"] or b"*", qual]
    cols += [_aux_text(*a) for a in f["aux"]]
    return b"\t".join(cols) + (TAG if fail else b"") + b"\n"


def decode(bam, records_at, rec_off, passed=None):
    bam = bytes(bam)
    rec_off = [int(o) for o in rec_off]
    if len(rec_off) >= 2**32 - 1 or len(bam) >= 1 << 40:
        raise Refused(LIMIT, None, "size")
    text, names = header_text(bam, records_at)
    parts = []
    for r, o in enumerate(rec_off):
        what = _structure(bam, o, len(names))
        if what:
            raise Refused(ARG, r, what)
        f = _fields(bam, o)
        what = _limits(f, names)
        if what:
            raise Refused(LIMIT, r, what)
        parts.append(f)
    n_aligned = sum(1 for f in parts if not f["flag"] & 4)
    verdicts = None if passed is None else [int(v) for v in passed]
    if verdicts is not None and len(verdicts) != n_aligned:
        raise Refused(ARG, None, f"{len(verdicts)} verdicts for {n_aligned} aligned records")
    out, rank = [text], 0
    for f in parts:
        fail = False
        if not f["flag"] & 4:
            fail = verdicts is not None and verdicts[rank] == 0
            rank += 1
        out.append(line(f, names, fail))
    total = sum(len(x) for x in out)
    if total >= 1 << 40:
        raise Refused(LIMIT, None, "output")
    return b"".join(out)


def refusal(bam, records_at, rec_off, passed=None):
    """(code, record) of a refused input, None of an accepted one"""
    try:
        decode(bam, records_at, rec_off, passed)
    except Refused as r:
        return r.code, r.record
    return None


def canonical(text):
    """a text sam_bam_model accepts -> the canonical text of the same records: decode(encode(text))"""
    import sam_bam_model as sb
    enc = sb.encode(text)
    return decode(enc["bytes"], enc["records_at"], enc["rec_off"])


# ---- generated inputs shared by the CPU pin and the GPU tests ---------------------------------------------------------------------------
def exponent_floats():
    """every exponent with the mantissas 0, 1, 0x400000, 0x7FFFFF, inf and nan left out: 1,020 bit patterns"""
    return [e << 23 | m for e in range(255) for m in (0, 1, 0x400000, 0x7FFFFF)]


def bam_of(records, refs=(("c1", 1000), ("c2", 2000)), text="@HD\tVN:1.6\n", lead=b""):
    """header + records back to back -> (bytes, records_at, rec_off)"""
    head = bam_model.header_bytes(list(refs), text)
    body, off = bam_model.lay_out(records)
    return head + lead + body, len(head), (off + np.uint64(len(head) + len(lead))).astype(np.uint64)
