"""A plain model of the BAM front end (include/polypolish_hip.h: pp_bam_header, pp_bam_walk, pp_bam_records).  Test infrastructure: it
does not call the library.  tests/test_bam_model_cpu.py pins decode(encode(text)) to gate_model.raw_from_text(text) -- the model of
Alignment::new per SAM line -- and the two host helpers to header() / walk(); tests/test_bam_records_gpu.py runs the device decode
(pp_bam.hip) against decode() byte for byte.

encode() writes uncompressed BAM: a header (magic, text, references) and alignment records block_size | refID pos l_read_name mapq
bin n_cigar_op flag l_seq next_refID next_pos tlen | read_name NUL | CIGAR words len << 4 | op | SEQ nibbles, high first | QUAL | typed
aux fields.  It RAISES NotBam where a line has no equivalent record -- a SEQ character outside =ACMGRSVTWYHKDBN, a value beyond a
field, a zero-length CIGAR run (the text's expansion drops it, a BAM word keeps it) -- and never papers over one.
decode() restates the header's contract byte by byte, the defect kinds and their order included."""
import struct

import numpy as np

NIBBLE = "=ACMGRSVTWYHKDBN"
OPS = "MIDNSHP=X"
SEQ_ALIGN = 32
QUIT, ARG, PANIC = 1, 4, 101
NO_CONTIG = 0xFFFFFFFF
# defect kinds of a record, in the order they are looked for (pp_bam.hip: BA_*), then what Alignment::new refuses (BE_*)
RANGE, BLOCK, NAME, CIGAR_OP, REF_ID, AUX = "range", "block_size", "name", "cigar_op", "ref_id", "aux"
PANIC_NM, MISSING_NM = "negative_nm", "missing_nm"
FIXED = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
B_SIZE = {"c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
INT_FMT = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}


class NotBam(Exception):
    """the line has no equivalent BAM record"""


class BamError(Exception):
    def __init__(self, code, kind, bad_record=None):
        super().__init__(f"[{code}] {kind} at record {bad_record}")
        self.code, self.kind, self.bad_record = code, kind, bad_record


# ---- writing -------------------------------------------------------------------------------------------------------------------------
def smallest_int_type(v):
    for t, (lo, hi) in (("C", (0, 255)), ("c", (-128, 127)), ("S", (0, 65535)), ("s", (-32768, 32767)), ("I", (0, 2**32 - 1)),
                        ("i", (-2**31, 2**31 - 1))):
        if lo <= v <= hi:
            return t
    raise NotBam(f"integer {v} beyond 32 bits")


def aux(tag, ty, value=None):
    """one aux field: tag (2 characters), type, value -- an int for c C s S i I, a float for f, a character for A, a str / bytes for
    Z and H (the NUL is added), (sub-type, [values]) for B"""
    head = tag.encode("latin-1") + ty.encode("latin-1")
    if ty in INT_FMT:
        return head + struct.pack(INT_FMT[ty], value)
    if ty == "f":
        return head + struct.pack("<f", value)
    if ty == "A":
        return head + (value.encode("latin-1") if isinstance(value, str) else bytes(value))
    if ty in "ZH":
        return head + (value.encode("latin-1") if isinstance(value, str) else bytes(value)) + b"\0"
    if ty == "B":
        sub, vals = value
        fmt = "<f" if sub == "f" else INT_FMT[sub]
        return head + sub.encode() + struct.pack("<I", len(vals)) + b"".join(struct.pack(fmt, v) for v in vals)
    raise NotBam(f"aux type {ty!r}")


def pack_seq(seq):
    """SEQ characters (either case) -> nibbles, high nibble first; raises NotBam on a character outside the table"""
    up = seq.upper()
    codes = []
    for c in up:
        k = NIBBLE.find(c)
        if k < 0 or len(c) != 1:
            raise NotBam(f"SEQ character {c!r} has no nibble")
        codes.append(k)
    if len(codes) & 1:
        codes.append(0)
    return bytes((codes[i] << 4) | codes[i + 1] for i in range(0, len(codes), 2))


def record(qname, flag, ref_id, pos, runs, seq, aux_bytes=b"", qual=None, mapq=60, next_ref=-1, next_pos=-1, tlen=0, seq_pad_nibble=0,
           **override):
    """one alignment record.  qname: bytes without the NUL; runs: packed CIGAR words; seq: characters of the table.  override: any of
    block_size, l_read_name, n_cigar_op, l_seq, name (the bytes written for the name, NUL included) -- to write DEFECTIVE records;
    seq_pad_nibble: the unused low nibble behind an odd l_seq (a decoder must not let it through)."""
    name = override.get("name", bytes(qname) + b"\0")
    nib = bytearray(pack_seq(seq))
    if len(seq) & 1:
        nib[-1] |= seq_pad_nibble & 15
    q = bytes([0xFF]) * len(seq) if qual is None else bytes(qual)
    body = struct.pack("<iiBBHHHIiii", ref_id, pos, override.get("l_read_name", len(name)), mapq, 4680, override.get("n_cigar_op", len(runs)),
                       flag, override.get("l_seq", len(seq)), next_ref, next_pos, tlen)
    body += name + b"".join(struct.pack("<I", w) for w in runs) + bytes(nib) + q + aux_bytes
    return struct.pack("<I", override.get("block_size", len(body))) + body


def header_bytes(refs, text=""):
    """refs: [(name, length)] -> magic, l_text, text, n_ref, then l_name name NUL l_ref"""
    t = text.encode("latin-1")
    out = b"BAM\1" + struct.pack("<i", len(t)) + t + struct.pack("<i", len(refs))
    for name, ln in refs:
        nm = (name.encode("latin-1") if isinstance(name, str) else bytes(name)) + b"\0"
        out += struct.pack("<i", len(nm)) + nm + struct.pack("<i", ln)
    return out


def _cigar_words(cigar):
    if cigar == "*":
        return []
    words, num = [], ""
    for ch in cigar:
        if ch.isdigit() and ch.isascii():
            num += ch
            continue
        if ch not in OPS or num == "":
            raise NotBam(f"CIGAR {cigar!r}")
        n = int(num)
        if n == 0 or n >= 1 << 28:
            raise NotBam(f"CIGAR run length {n} (zero expands to nothing in the text, 2^28 and above has no word)")
        words.append((n << 4) | OPS.index(ch))
        num = ""
    if num:
        raise NotBam(f"CIGAR {cigar!r}")
    if len(words) > 0xFFFF:
        raise NotBam("more than 65535 CIGAR runs")
    return words


def _aux_from_text(field, nm_type):
    parts = field.split(":", 2)
    if len(parts) != 3 or len(parts[0]) != 2 or len(parts[1]) != 1:
        raise NotBam(f"aux field {field!r}")
    tag, ty, val = parts
    try:
        if ty == "i":
            if not (val.lstrip("+-").isdigit() and val.isascii()):
                raise NotBam(f"aux field {field!r}")
            v = int(val)
            if tag == "NM" and val[0] == "+":
                raise NotBam("NM with a sign the text parses and a BAM writer drops")
            return aux(tag, nm_type if (tag == "NM" and nm_type) else smallest_int_type(v), v)
        if ty == "A":
            if len(val) != 1:
                raise NotBam(f"aux field {field!r}")
            return aux(tag, "A", val)
        if ty == "f":
            return aux(tag, "f", float(val))
        if ty in "ZH":
            return aux(tag, ty, val)
        if ty == "B":
            sub, *vals = val.split(",")
            return aux(tag, "B", (sub, [float(v) if sub == "f" else int(v) for v in vals]))
    except (ValueError, struct.error, KeyError):
        raise NotBam(f"aux field {field!r}")
    raise NotBam(f"aux type {ty!r} of {field!r}")


def _int_field(s, lo, hi, what):
    if not (s.isascii() and s.lstrip("+").isdigit()) or not lo <= int(s) <= hi:
        raise NotBam(f"{what} {s!r}")
    return int(s)


def encode_line(line, ref_index, nm_type=None, extra_front=b"", extra_back=b""):
    """one SAM alignment line -> one record (NM in the smallest integer type unless nm_type forces one)"""
    p = line.split("\t")
    if len(p) < 11:
        raise NotBam("too few columns")
    qname = p[0].encode("latin-1")
    if len(qname) > 254 or b"\0" in qname:
        raise NotBam("QNAME beyond l_read_name")
    flag = _int_field(p[1], 0, 0xFFFF, "FLAG")
    if p[2] != "*" and p[2] not in ref_index:
        raise NotBam(f"RNAME {p[2]!r} is not in the header")
    ref_id = -1 if p[2] == "*" else ref_index[p[2]]
    pos = _int_field(p[3], 0, 2**31, "POS") - 1
    mapq = _int_field(p[4], 0, 255, "MAPQ")
    runs = _cigar_words(p[5])
    next_ref = -1 if p[6] == "*" else (ref_id if p[6] == "=" else ref_index.get(p[6], -1))
    next_pos = _int_field(p[7], 0, 2**31, "PNEXT") - 1
    try:
        tlen = int(p[8])
    except ValueError:
        raise NotBam(f"TLEN {p[8]!r}")
    seq = "" if p[9] == "*" else p[9]
    qual = None if p[10] == "*" or len(p[10]) != len(seq) else bytes(ord(c) - 33 for c in p[10])
    tags = extra_front + b"".join(_aux_from_text(f, nm_type) for f in p[11:]) + extra_back
    return record(qname, flag, ref_id, pos, runs, seq, tags, qual=qual, mapq=mapq, next_ref=next_ref, next_pos=next_pos, tlen=tlen)


def lay_out(records, lead=0, pad=None):
    """records back to back behind `lead` junk bytes, pad(i) junk bytes behind record i (None: none) -> (bytes, rec_off)"""
    out, off = bytearray(b"\xA5" * lead), []
    for i, r in enumerate(records):
        off.append(len(out))
        out += r
        if pad is not None:
            out += b"\x5A" * int(pad(i))
    return bytes(out), np.array(off, np.uint64)


def encode(text, ref_names, ref_lens=None, nm_type=None, extra_front=None, extra_back=None, lead=0, pad=None):
    """SAM text -> {"header": bytes, "records": bytes, "rec_off": offsets into records}.  ref_names: the header's references in the
    header's order.  Hooks: nm_type forces NM's type; extra_front(i) / extra_back(i): aux bytes in front of / behind record i's own;
    lead / pad(i): junk bytes in front of the first record / behind record i (such a stream has no block_size chain)."""
    if isinstance(text, bytes):
        text = text.decode("ascii")
    ref_index = {n: i for i, n in enumerate(ref_names)}
    lens = ref_lens or [0] * len(ref_names)
    lines = [ln[:-1] if ln.endswith("\r") else ln for ln in text.split("\n")]
    recs = []
    for ln in lines:
        if not ln or ln[0] == "@":
            continue
        i = len(recs)
        recs.append(encode_line(ln, ref_index, nm_type, extra_front(i) if extra_front else b"", extra_back(i) if extra_back else b""))
    body, off = lay_out(recs, lead, pad)
    return {"header": header_bytes(list(zip(ref_names, lens)), "@HD\tVN:1.6\n"), "records": body, "rec_off": off}


# ---- reading: the host helpers -----------------------------------------------------------------------------------------------------------
def _le32(b, at):
    return b[at] | b[at + 1] << 8 | b[at + 2] << 16 | b[at + 3] << 24


def header(b):
    """-> {"names": [bytes], "name_off", "name_len", "ref_len", "records_at"}, or raises BamError(ARG, "header")"""
    n = len(b)
    if n < 12 or b[:4] != b"BAM\1":
        raise BamError(ARG, "header")
    l_text, at = _le32(b, 4), 8
    if l_text > 0x7FFFFFFF or l_text > n - at or n - at - l_text < 4:
        raise BamError(ARG, "header")
    at += l_text
    n_ref = _le32(b, at)
    at += 4
    if n_ref > 0x7FFFFFFF:
        raise BamError(ARG, "header")
    names, off, ln, rl = [], [], [], []
    for _ in range(n_ref):
        if n - at < 4:
            raise BamError(ARG, "header")
        l_name = _le32(b, at)
        at += 4
        if l_name == 0 or l_name > 0x7FFFFFFF or l_name > n - at or n - at - l_name < 4 or b[at + l_name - 1] != 0:
            raise BamError(ARG, "header")
        names.append(bytes(b[at:at + l_name - 1]))
        off.append(at)
        ln.append(l_name - 1)
        rl.append(_le32(b, at + l_name))
        at += l_name + 4
    return {"names": names, "name_off": np.array(off, np.uint64), "name_len": np.array(ln, np.uint32), "ref_len": np.array(rl, np.uint32),
            "records_at": at}


def walk(b, start=0):
    """-> (rec_off list, end, ok): the block_size chain from `start`; ok is False where the chain breaks (end = the break's offset)"""
    n, at, off = len(b), start, []
    if start > n:
        return off, start, False
    while at < n:
        if n - at < 4:
            return off, at, False
        bs = _le32(b, at)
        if bs < 32 or bs > n - at - 4:
            return off, at, False
        off.append(at)
        at += 4 + bs
    return off, at, True


# ---- reading: the records ------------------------------------------------------------------------------------------------------------------
def _one(b, o, ref_map, n_ref):
    """record at offset o -> (defect kind or None, refused kind or None, fields)"""
    n = len(b)
    if o > n or n - o < 4:
        return RANGE, None, None
    bs = _le32(b, o)
    if bs > n - o - 4:
        return RANGE, None, None
    if bs < 32:
        return BLOCK, None, None
    c = o + 4
    ref_id, pos = struct.unpack_from("<ii", b, c)
    lrn, _mapq, _bin, nc, flag, ls = struct.unpack_from("<BBHHHI", b, c + 8)
    need = 32 + lrn + 4 * nc + (ls + 1) // 2 + ls
    if bs < need:
        return BLOCK, None, None
    if lrn == 0 or b[c + 32 + lrn - 1] != 0:
        return NAME, None, None
    cig = c + 32 + lrn
    words = [_le32(b, cig + 4 * j) for j in range(nc)]
    if any((w & 15) > 8 for w in words):
        return CIGAR_OP, None, None
    if ref_id < -1 or (ref_map is not None and ref_id >= n_ref):
        return REF_ID, None, None
    p, e = c + need, c + bs
    nm, negative, zp_fail = 0xFFFFFFFF, False, False
    while p < e:
        if e - p < 3:
            return AUX, None, None
        tag, ty = bytes(b[p:p + 2]), chr(b[p + 2])
        p += 3
        if ty in "ZH":
            z = p
            while p < e and b[p] != 0:
                p += 1
            if p == e:
                return AUX, None, None
            if ty == "Z" and tag.lower() == b"zp" and bytes(b[z:p]).lower() == b"fail":
                zp_fail = True
            p += 1
            continue
        if ty == "B":
            if e - p < 5:
                return AUX, None, None
            size, cnt = B_SIZE.get(chr(b[p])), _le32(b, p + 1)
            p += 5
            if size is None or cnt * size > e - p:
                return AUX, None, None
            p += cnt * size
            continue
        size = FIXED.get(ty)
        if size is None or e - p < size:
            return AUX, None, None
        if tag == b"NM" and ty in INT_FMT:
            v = struct.unpack_from(INT_FMT[ty], b, p)[0]
            if v < 0:
                negative = True
            nm = v & 0xFFFFFFFF
        p += size
    refused = PANIC_NM if negative else (MISSING_NM if not (flag & 4) and nm == 0xFFFFFFFF else None)
    if ref_id < 0:
        contig = NO_CONTIG if ref_map is None else int(ref_map[n_ref])
    else:
        contig = ref_id if ref_map is None else int(ref_map[ref_id])
    seq_at = cig + 4 * nc
    seq = bytes(ord(NIBBLE[(b[seq_at + i // 2] >> (0 if i & 1 else 4)) & 15]) for i in range(ls))
    return None, refused, {"flag": flag, "contig": contig, "ref_start": max(pos, 0), "nm": nm, "seq": seq, "runs": words, "name_off": c + 32,
                           "name_len": lrn - 1, "zp_fail": zp_fail}


def decode(b, rec_off, ref_map=None):
    """the contract of pp_bam_records over the bytes b: -> the arrays of pp_raw_batch (read_id zero), "name_off", "name_len" and "zp"
    (one byte per ALIGNED record, 0 = ZP:Z:fail).  Raises BamError(ARG, kind, r) for the first defective record in index order; only
    without one BamError(QUIT, "missing_nm", r) / BamError(PANIC, "negative_nm", r) for the first record Alignment::new refuses."""
    b = bytes(b)
    n_ref = None if ref_map is None else len(ref_map) - 1
    got = [_one(b, int(o), ref_map, n_ref) for o in rec_off]
    for r, (defect, _, _) in enumerate(got):
        if defect:
            raise BamError(ARG, defect, r)
    for r, (_, refused, _) in enumerate(got):
        if refused:
            raise BamError(PANIC if refused == PANIC_NM else QUIT, refused, r)
    f = [g[2] for g in got]
    seq_len = np.array([len(x["seq"]) for x in f], np.uint32)
    room = (seq_len.astype(np.int64) + SEQ_ALIGN - 1) & ~(SEQ_ALIGN - 1)
    seq_off = (np.cumsum(room) - room).astype(np.uint64)
    seq = np.zeros(int(room.sum()), np.uint8)
    for x, at in zip(f, seq_off.tolist()):
        seq[at:at + len(x["seq"])] = np.frombuffer(x["seq"], np.uint8)
    n_cig = np.array([len(x["runs"]) for x in f], np.uint32)
    flag = np.array([x["flag"] for x in f], np.uint16)
    return {"flag": flag, "read_id": np.zeros(len(f), np.uint64), "contig": np.array([x["contig"] for x in f], np.uint32),
            "ref_start": np.array([x["ref_start"] for x in f], np.uint32), "nm": np.array([x["nm"] for x in f], np.uint32),
            "seq_off": seq_off, "seq_len": seq_len, "cig_off": (np.cumsum(n_cig, dtype=np.int64) - n_cig).astype(np.uint64), "n_cig": n_cig,
            "seq": seq, "cigar": np.array([w for x in f for w in x["runs"]], np.uint32),
            "name_off": np.array([x["name_off"] for x in f], np.uint64), "name_len": np.array([x["name_len"] for x in f], np.uint32),
            "zp": np.array([0 if x["zp_fail"] else 1 for x in f if not x["flag"] & 4], np.uint8)}


KEYS = ("flag", "read_id", "contig", "ref_start", "nm", "seq_off", "seq_len", "cig_off", "n_cig", "seq", "cigar", "name_off", "name_len")


def same(got, want, keys=KEYS):
    """the arrays byte for byte"""
    for k in keys:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (k, a[:8], b[:8])


# ---- generated inputs: the seams of the device decode (shared by the CPU pin of their shape and the GPU test) ---------------------------
SEAM_LENS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257)
BAM_BLOCK = 1024    # records per workgroup of the scanning kernel (pp_bam.hip)


def seam_records(seed=3):
    """every l_seq of SEAM_LENS x l_read_name 2..9, one to three CIGAR words, all 16 nibble codes, the unused nibble behind an odd
    l_seq set: -> [record bytes]"""
    rng = np.random.default_rng(seed)
    recs = []
    for li, ls in enumerate(SEAM_LENS):
        for lrn in range(2, 10):
            qname = bytes(rng.integers(33, 127, lrn - 1).astype(np.uint8))
            seq = "".join(NIBBLE[(5 * i + li + lrn) % 16] for i in range(ls))
            k = (li + lrn) % 3
            runs = [(max(ls, 1) << 4) | 0] if k == 0 else ([(2 << 4) | 4, (max(ls, 3) - 2) << 4 | 7] if k == 1 else
                                                            [(1 << 4) | 0, (3 << 4) | 2, (max(ls, 2) - 1) << 4 | 8])
            flag = (16 if lrn & 1 else 0) | (256 if ls == 0 else 0)
            recs.append(record(qname, flag, int(rng.integers(0, 3)), int(rng.integers(0, 5000)), runs, seq,
                               aux("AS", "C", 90) * (li & 1) + aux("NM", "C", (li * lrn) % 20), seq_pad_nibble=0xF))
    return recs


def _good(nm_aux, flag=0, seq="ACGTN=MR", qname=b"q"):
    return record(qname, flag, 0, 10, [(len(seq) << 4)], seq, nm_aux)


def aux_records():
    """[(what, record bytes, nm, pass byte or None for an unaligned record)]: the aux walk's cases, every one a GOOD record"""
    out = []
    for ty, v in (("c", 7), ("C", 200), ("s", 300), ("S", 40000), ("i", 70000), ("I", 4000000000)):
        out.append((f"NM:{ty}", _good(aux("NM", ty, v)), v, 1))
    out.append(("NM twice", _good(aux("NM", "C", 3) + aux("XS", "i", -5) + aux("NM", "S", 999)), 999, 1))
    out.append(("NM behind a long Z", _good(aux("MD", "Z", "A" * 700) + aux("NM", "C", 4)), 4, 1))
    out.append(("NM behind an H", _good(aux("XH", "H", "1AE301") + aux("NM", "C", 5)), 5, 1))
    for sub in "cCsSiIf":
        for cnt in (0, 1, 300):
            out.append((f"NM behind B:{sub} x {cnt}", _good(aux("XB", "B", (sub, [1] * cnt)) + aux("NM", "C", 6)), 6, 1))
    out.append(("NM:Z ignored", _good(aux("NM", "Z", "12") + aux("NM", "C", 8) + aux("NM", "Z", "13")), 8, 1))
    out.append(("NM:f ignored", _good(aux("NM", "C", 9) + aux("NM", "f", 2.0)), 9, 1))
    out.append(("NM:A ignored", _good(aux("NM", "C", 10) + aux("NM", "A", "7")), 10, 1))
    out.append(("unaligned without NM", _good(aux("AS", "C", 1), flag=4), 0xFFFFFFFF, None))
    out.append(("unaligned, no aux at all", _good(b"", flag=4), 0xFFFFFFFF, None))
    for what, field, ok in (("ZP:Z:fail", aux("ZP", "Z", "fail"), 0), ("zp:Z:FAIL", aux("zp", "Z", "FAIL"), 0), ("ZP:Z:failed", aux("ZP", "Z", "failed"), 1),
                            ("ZP:Z:fai", aux("ZP", "Z", "fai"), 1), ("ZP:A:f", aux("ZP", "A", "f"), 1)):
        out.append((what, _good(aux("NM", "C", 1) + field), 1, ok))
    out.append(("ZP:Z:fail in front of NM", _good(aux("ZP", "Z", "fail") + aux("NM", "C", 2)), 2, 0))
    return out


def defect_records():
    """[(kind, record bytes)]: every ARG defect of the contract as ONE record that is otherwise good (a range defect is an offset, not
    a record: the test makes those itself).  A record keeps its true length where block_size lies, so that neighbours stay in place."""
    ok_aux = aux("NM", "C", 1)
    base = dict(qname=b"name", flag=0, ref_id=1, pos=5, runs=[(8 << 4)], seq="ACGTACGT")
    cut = lambda extra: record(aux_bytes=ok_aux + extra, **base)      # noqa: E731
    out = [(BLOCK, record(aux_bytes=ok_aux, block_size=31, **base)),
           (BLOCK, record(aux_bytes=b"", block_size=32 + 5 + 4 + 4 + 8 - 1, **base)),
           (BLOCK, record(aux_bytes=ok_aux, l_seq=0x80000000, **base)),
           (NAME, record(aux_bytes=ok_aux, name=b"name!", **base)),
           (NAME, record(aux_bytes=ok_aux + b"\0", name=b"", **base)),
           (CIGAR_OP, record(aux_bytes=ok_aux, **dict(base, runs=[(4 << 4), (4 << 4) | 9]))),
           (REF_ID, record(aux_bytes=ok_aux, **dict(base, ref_id=-2))),
           (REF_ID, record(aux_bytes=ok_aux, **dict(base, ref_id=3))),      # n_ref = 3 in the test: with a ref_map only
           (AUX, cut(b"XY")), (AUX, cut(b"XYi\1\2\3")), (AUX, cut(b"XYS\1")), (AUX, cut(b"XYq\1\2\3\4")), (AUX, cut(b"XYZabc")), (AUX, cut(b"XYH")),
           (AUX, cut(b"XYBc\5\0\0\0\1\2\3\4")), (AUX, cut(b"XYBI\xff\xff\xff\xff" + b"\0" * 8)), (AUX, cut(b"XYBz\0\0\0\0")), (AUX, cut(b"XYB\1\0"))]
    return out


def mixed_records(n=5000, seed=11):
    """n records of every kind the decode meets: unaligned ones, l_seq 0, one to four CIGAR words, NM in several types, extra aux
    fields, ZP:Z:fail now and then, refID -1 and pos -1"""
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(n):
        kind = i % 11
        ls = 0 if kind == 3 else int(rng.integers(1, 260))
        seq = "".join(NIBBLE[j] for j in rng.integers(0, 16, ls))
        runs = [int(rng.integers(1, 1 << 20)) << 4 | int(rng.integers(0, 9)) for _ in range(int(rng.integers(1, 5)))]
        unal = kind == 5
        tags = b"" if unal and i % 2 else aux("AS", "i", -70000) * (i % 3 == 0) + aux("NM", "CSI"[i % 3], int(rng.integers(0, 200)))
        if kind == 7:
            tags += aux("ZP", "Z", "fail")
        if kind == 9:
            tags = aux("MD", "Z", "12A3^CC9") + tags + aux("XB", "B", ("s", [3, -3, 9]))
        recs.append(record(bytes(rng.integers(48, 123, int(rng.integers(1, 30))).astype(np.uint8)), (4 if unal else 0) | (16 if i & 1 else 0),
                           -1 if unal else int(rng.integers(0, 3)), -1 if unal or kind == 2 else int(rng.integers(0, 100000)),
                           [] if unal else runs, seq, tags))
    return recs
