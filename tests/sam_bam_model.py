"""A plain model of pp_sam_header and pp_sam_bam (include/polypolish_hip.h): SAM text -> uncompressed BAM.  Test infrastructure: it
does not call the library.  Written from the header's contract; tests/test_sam_bam_model_cpu.py pins it to hand-written bytes and to
bam_model's encoder and decoder, tests/test_sam_bam_gpu.py runs the device (pp_sam_bam.hip) against it byte for byte.

encode(text) -> {"bytes", "records_at", "rec_off"} or raises Refused(code, line): the first refused line in file order, whatever its
kind; inside one line the checks run in the order of encode_line below (the columns left to right, the bin, the aux fields left to
right, then RNAME and RNEXT against the header)."""
import struct

import numpy as np

import bam_model

QUIT, ARG, LIMIT, NOT_ASCII = 1, 4, 5, 6
NIBBLE = bam_model.NIBBLE
OPS = bam_model.OPS
B_RANGE = {"c": (-128, 127), "C": (0, 255), "s": (-32768, 32767), "S": (0, 65535), "i": (-2**31, 2**31 - 1), "I": (0, 2**32 - 1)}


class Refused(Exception):
    def __init__(self, code, line=None, what=""):
        super().__init__(f"[{code}] line {line}: {what}")
        self.code, self.line, self.what = code, line, what


def lines_of(text):
    """[(start, content end)] of every line: cut at '\\n', one trailing '\\r' is not content; no line behind a final newline"""
    out, at, n = [], 0, len(text)
    while at < n:
        e = text.find(b"\n", at)
        e = n if e < 0 else e
        ce = e - 1 if e > at and text[e - 1] == 13 else e
        out.append((at, ce))
        at = e + 1
    return out


# ---- the header ---------------------------------------------------------------------------------------------------------------------
def _digits(b):
    return len(b) > 0 and all(48 <= c <= 57 for c in b)


def header(text):
    """pp_sam_header: {"header_end", "n_lines" (header lines), "name_off", "name_len", "ref_len", "names"}; Refused(QUIT, line)"""
    text = bytes(text)
    all_lines = lines_of(text)
    off, ln, rl, names, end, n_hdr = [], [], [], [], len(text), len(all_lines)
    for k, (s, e) in enumerate(all_lines):
        if e == s or text[s] != 64:
            end, n_hdr = s, k
            break
        cols, at = [], s
        for part in text[s:e].split(b"\t"):
            cols.append((at, part))
            at += len(part) + 1
        if cols[0][1] != b"@SQ":
            continue
        sn = next(((a + 3, p[3:]) for a, p in cols[1:] if p[:3] == b"SN:"), None)
        if sn is None or not sn[1]:
            raise Refused(QUIT, k, "SN")
        lnf = next((p[3:] for _, p in cols[1:] if p[:3] == b"LN:"), None)
        if lnf is None or not _digits(lnf) or not 1 <= int(lnf) <= 2**31 - 1:
            raise Refused(QUIT, k, "LN")
        if sn[1] in names:
            raise Refused(QUIT, k, "duplicate")
        names.append(sn[1])
        off.append(sn[0])
        ln.append(len(sn[1]))
        rl.append(int(lnf))
    return {"header_end": end, "n_lines": n_hdr, "name_off": np.array(off, np.uint64), "name_len": np.array(ln, np.uint32),
            "ref_len": np.array(rl, np.uint32), "names": names}


def bam_header(text, h):
    """the BAM header of a text whose header() is h"""
    t = b"".join(text[s:e] + b"\n" for s, e in lines_of(text[:h["header_end"]]))
    return bam_model.header_bytes(list(zip(h["names"], (int(x) for x in h["ref_len"]))), t.decode("latin-1"))


# ---- numbers ------------------------------------------------------------------------------------------------------------------------
def reg2bin(pos, end):
    end -= 1
    for shift, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if pos >> shift == end >> shift:
            return base + (pos >> shift)
    return 0


def _unsigned(b, hi, what):
    """[+]digits in 0 .. hi"""
    d = b[1:] if b[:1] == b"+" else b
    if not _digits(d):
        raise Refused(QUIT, None, what)
    if int(d) > hi:
        raise Refused(LIMIT, None, what)
    return int(d)


def _signed(b):
    """[+-]digits -> int, or None"""
    d = b[1:] if b[:1] in (b"+", b"-") else b
    return int(b) if _digits(d) else None


def float_bits(b):
    """the header's float rule: [+-]digits[.digits][(e|E)[+-]digits] -> the four bytes, or None where the rule refuses"""
    at, n = 0, len(b)
    neg = b[:1] == b"-"
    if b[:1] in (b"+", b"-"):
        at = 1
    s = at
    while at < n and 48 <= b[at] <= 57:
        at += 1
    if at == s:
        return None
    digits, frac = b[s:at], 0
    if at < n and b[at] == 46:
        s = at = at + 1
        while at < n and 48 <= b[at] <= 57:
            at += 1
        if at == s:
            return None
        digits += b[s:at]
        frac = at - s
    exp = 0
    if at < n and b[at] in (69, 101):
        at += 1
        esign = -1 if b[at:at + 1] == b"-" else 1
        if b[at:at + 1] in (b"+", b"-"):
            at += 1
        s = at
        while at < n and 48 <= b[at] <= 57:
            at += 1
        if at == s:
            return None
        exp = esign * int(b[s:at])
    if at != n:
        return None
    w = int(digits)
    if w == 0:
        return struct.pack("<f", -0.0 if neg else 0.0)
    e10 = exp - frac
    if len(str(w)) > 15 or abs(e10) > 22:
        return None
    v = float(w) * float(10 ** e10) if e10 >= 0 else float(w) / float(10 ** -e10)
    return struct.pack("<f", -v if neg else v)


# ---- one line -----------------------------------------------------------------------------------------------------------------------
def _cigar(b):
    """-> (words, reference length)"""
    if b == b"*":
        return [], 0
    words, ref, at, n = [], 0, 0, len(b)
    while at < n:
        s = at
        while at < n and 48 <= b[at] <= 57:
            at += 1
        op = OPS.find(chr(b[at])) if at < n else -1
        if at == s or op < 0:
            raise Refused(QUIT, None, "CIGAR")
        ln = int(b[s:at])
        if ln == 0 or ln >= 1 << 28:
            raise Refused(LIMIT, None, "CIGAR")
        words.append(ln << 4 | op)
        if op in (0, 2, 3, 7, 8):
            ref += ln
        at += 1
    if len(words) > 65535:
        raise Refused(LIMIT, None, "CIGAR")
    return words, ref


def _aux(f):
    tag = f[:2].decode("latin-1")
    if len(f) < 5 or f[2] != 58 or f[4] != 58:
        raise Refused(QUIT, None, f"aux {tag}")
    ty, val = chr(f[3]), f[5:]
    if ty == "A":
        if len(val) != 1:
            raise Refused(QUIT, None, f"aux {tag}")
        return bam_model.aux(tag, "A", val)
    if ty == "i":
        v = _signed(val)
        if v is None:
            raise Refused(QUIT, None, f"aux {tag}")
        if not -2**31 <= v <= 2**32 - 1:
            raise Refused(LIMIT, None, f"aux {tag}")
        return bam_model.aux(tag, bam_model.smallest_int_type(v), v)
    if ty == "Z":
        return bam_model.aux(tag, "Z", val)
    if ty == "H":
        if len(val) & 1 or any(chr(c) not in "0123456789abcdefABCDEF" for c in val):
            raise Refused(QUIT, None, f"aux {tag}")
        return bam_model.aux(tag, "H", val)
    if ty == "f":
        bits = float_bits(val)
        if bits is None:
            raise Refused(LIMIT, None, f"aux {tag}")
        return tag.encode("latin-1") + b"f" + bits
    if ty == "B":
        sub = chr(val[0]) if val else ""
        if sub == "" or sub not in "cCsSiIf" or (len(val) > 1 and val[1] != 44):
            raise Refused(QUIT, None, f"aux {tag}")
        elems = val[2:].split(b",") if len(val) > 1 else []
        out = b""
        for e in elems:
            if not e:
                raise Refused(QUIT, None, f"aux {tag}")
            if sub == "f":
                bits = float_bits(e)
                if bits is None:
                    raise Refused(LIMIT, None, f"aux {tag}")
                out += bits
            else:
                v = _signed(e)
                if v is None or not B_RANGE[sub][0] <= v <= B_RANGE[sub][1]:
                    raise Refused(QUIT, None, f"aux {tag}")
                out += struct.pack(bam_model.INT_FMT[sub], v)
        return tag.encode("latin-1") + b"B" + sub.encode() + struct.pack("<I", len(elems)) + out
    raise Refused(QUIT, None, f"aux {tag}")


def encode_line(line, ref_index):
    """one record line (bytes, no line end) -> the record's bytes; Refused(code, None, what)"""
    p = line.split(b"\t")
    if len(p) < 11:
        raise Refused(QUIT, None, "columns")
    if not 1 <= len(p[0]) <= 254:
        raise Refused(LIMIT, None, "QNAME")
    flag = _unsigned(p[1], 0xFFFF, "FLAG")
    pos = _unsigned(p[3], 2**31, "POS") - 1
    mapq = _unsigned(p[4], 255, "MAPQ")
    words, ref = _cigar(p[5])
    next_pos = _unsigned(p[7], 2**31, "PNEXT") - 1
    tlen = _signed(p[8])
    if tlen is None:
        raise Refused(QUIT, None, "TLEN")
    if not -2**31 <= tlen <= 2**31 - 1:
        raise Refused(LIMIT, None, "TLEN")
    seq = b"" if p[9] == b"*" else p[9]
    if any(NIBBLE.find(chr(c).upper()) < 0 for c in seq):
        raise Refused(LIMIT, None, "SEQ")
    qual = None
    if p[10] != b"*":
        if len(seq) == 0 or len(p[10]) != len(seq) or any(c < 33 for c in p[10]):
            raise Refused(QUIT, None, "QUAL")
        qual = bytes(c - 33 for c in p[10])
    end = pos + ref if not flag & 4 and ref > 0 else pos + 1
    if end > 1 << 29:
        raise Refused(LIMIT, None, "bin")
    tags = b"".join(_aux(f) for f in p[11:])
    ids = []
    for col, what in ((p[2], "RNAME"), (p[6], "RNEXT")):
        if col == b"*":
            ids.append(-1)
        elif col == b"=" and what == "RNEXT":
            ids.append(ids[0])
        elif col in ref_index:
            ids.append(ref_index[col])
        else:
            raise Refused(QUIT, None, what)
    rec = bytearray(bam_model.record(p[0], flag, ids[0], pos, words, seq.decode("latin-1"), tags, qual=qual, mapq=mapq, next_ref=ids[1],
                                     next_pos=next_pos, tlen=tlen))
    rec[14:16] = struct.pack("<H", reg2bin(pos, end))
    return bytes(rec)


def encode(text):
    """pp_sam_bam: -> {"bytes": uncompressed BAM, "records_at", "rec_off": np.uint64, "lines": the 0-based line of every record}"""
    text = bytes(text)
    if any(c >= 0x80 for c in text):
        raise Refused(NOT_ASCII, None, "byte")
    if len(text) >= 1 << 40:
        raise Refused(LIMIT, None, "bytes")
    h = header(text)
    out = bytearray(bam_header(text, h))
    ref_index = {n: i for i, n in enumerate(h["names"])}
    records_at, off, lines, seen = len(out), [], [], False
    for li, (s, e) in enumerate(lines_of(text)):
        if e == s or li < h["n_lines"]:
            continue
        if text[s] == 64:
            if seen:
                raise Refused(QUIT, li, "@ behind a record")
            continue
        seen = True
        try:
            rec = encode_line(text[s:e], ref_index)
        except Refused as r:
            raise Refused(r.code, li, r.what) from None
        off.append(len(out))
        lines.append(li)
        out += rec
    return {"bytes": bytes(out), "records_at": records_at, "rec_off": np.array(off, np.uint64), "lines": np.array(lines, np.uint32)}


def refusal(text):
    """(code, line) of a refused text, None of an accepted one"""
    try:
        encode(text)
    except Refused as r:
        return r.code, r.line
    return None


def with_fitting_qual(text):
    """synth.rich_dataset writes a QUAL of the read's nominal length on every line, also where an indel made SEQ longer or shorter:
    such a line is no valid SAM and pp_sam_bam refuses it (QUIT).  -> the text with those QUAL columns cut or repeated to SEQ's
    length, nothing else touched: the lines, their order, every column the filter and the polish read stay what they are."""
    out = []
    for ln in bytes(text).split(b"\n"):
        p = ln.split(b"\t")
        if ln and ln[:1] != b"@" and len(p) >= 11 and p[10] != b"*" and p[9] != b"*" and len(p[10]) != len(p[9]) and p[10]:
            p[10] = (p[10] * (len(p[9]) // len(p[10]) + 1))[:len(p[9])]
            ln = b"\t".join(p)
        out.append(ln)
    return b"\n".join(out)
