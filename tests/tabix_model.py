"""A plain model of pp_tabix_index (include/polypolish_hip.h): the .tbi of a bgzipped, position-sorted, tab-separated text.  Test
infrastructure: it does not call the library.  tests/test_tabix_model_cpu.py pins it to bytes written out by hand and to what a plain
scan of the text finds; tests/test_tabix_index_gpu.py runs the device link (pp_tabix.hip) against it, byte for byte.

No `tabix` binary and no pysam are at hand here, so the check of the index is this file's own reader: parse_tbi() / query() are a
plain reader of the tabix specification's layout (the bins of reg2bins, cut by the linear index), lines_at() reads the chunks out of a
real BGZF file with zlib started at each chunk's block -- as it was for the .bai (tests/bam_sort_model.py).  The index is a valid .tbi,
not `tabix`'s bytes: one chunk per maximal run of lines with one (name, bin), nothing merged.

  lines      the text cut at every "\\n"; last bytes without one are a line; a line that starts with "#" is a meta line
  BED        name, beg, end = columns 1, 2, 3 (column 3 ends at a tab or the line's end); numbers are 1 to 10 decimal digits
  VCF        name, POS = columns 1, 2; beg = POS - 1, end = beg + len(column 4), which a tab must close; INFO/END is not read
  both       end == beg counts as [beg, beg + 1); a name's lines are consecutive and their beg does not decrease
  a run      consecutive lines of the text with one (name, bin): a meta line between two data lines ends it"""
import struct

from bam_sort_model import PAYLOAD, PSEUDO_BIN, MAX_END, level0_blk_off, reg2bin, reg2bins, voffset  # noqa: F401 (the tests take them from here)

ARG, LIMIT = 4, 5
VCF, BED = 0, 1
HEAD = {VCF: (2, 1, 2, 0), BED: (0x10000, 1, 2, 3)}      # format, col_seq, col_beg, col_end
LANE_BYTES = 64                                          # PP_TBX_LANE_BYTES: the columns a lane closes lie in the line's first 64 bytes
EMPTY, NAME, COLUMN, NUMBER, POS0, REF, ENDBEG, END, ORDER, BACK, BLK, PRESET, N_BLK = (
    "empty", "name", "column", "number", "pos0", "ref", "endbeg", "end", "order", "back", "blk_off", "preset", "n_blk")


class TabixError(Exception):
    def __init__(self, code, kind, bad_line=None):
        super().__init__(f"[{code}] {kind} at line {bad_line}")
        self.code, self.kind, self.bad_line = code, kind, bad_line


def cut(text):
    """[(start, end behind the newline, the line without it)] of every line"""
    text, out, at = bytes(text), [], 0
    while at < len(text):
        nl = text.find(b"\n", at)
        stop = len(text) if nl < 0 else nl
        out.append((at, len(text) if nl < 0 else nl + 1, text[at:stop]))
        at = stop + 1
    return out


def _number(s):
    if not 1 <= len(s) <= 10 or not all(48 <= c <= 57 for c in s):
        return None
    return int(s)


def row(line, preset):
    """(name, beg, end) of a data line, or the kind it is refused for"""
    if not line:
        return EMPTY
    cols = line.split(b"\t")
    if len(cols) > 1 and not cols[0]:
        return NAME
    if preset == VCF:
        if len(cols) < 5:                                  # column 4 must be closed by a tab
            return COLUMN
        pos = _number(cols[1])
        if pos is None:
            return NUMBER
        if pos == 0:
            return POS0
        if not cols[3]:
            return REF
        beg, end = pos - 1, pos - 1 + len(cols[3])
    else:
        if len(cols) < 3:
            return COLUMN
        beg, end = _number(cols[1]), _number(cols[2])
        if beg is None or end is None:
            return NUMBER
        if end < beg:
            return ENDBEG
        if end == beg:
            end = beg + 1
    if end > MAX_END:
        return END
    return cols[0], beg, end


def rows(text, preset):
    """[(line number, start, end offset, name, beg, end)] of the data lines; raises TabixError for the first line, in line order, that
    cannot be indexed"""
    out, seen, prev = [], set(), None
    for l, (start, stop, line) in enumerate(cut(text)):
        if line[:1] == b"#":
            continue
        r = row(line, preset)
        if isinstance(r, str):
            raise TabixError(LIMIT if r == END else ARG, r, l)
        name, beg, end = r
        if prev is not None and prev[0] == name:
            if beg < prev[1]:
                raise TabixError(ARG, ORDER, l)
        else:
            if name in seen:
                raise TabixError(ARG, BACK, l)
            seen.add(name)
        prev = (name, beg)
        out.append((l, start, stop, name, beg, end))
    return out


def index_tables(text, preset, blk_off):
    """what the index is made of: [{"name", "bins": {bin: [(beg, end)]}, "linear": [ioff], "span": (beg, end), "lines"}] in the order
    of the names' first lines"""
    text = bytes(text)
    if preset not in HEAD:
        raise TabixError(ARG, PRESET)
    if len(blk_off) - 1 != (len(text) + PAYLOAD - 1) // PAYLOAD:
        raise TabixError(ARG, N_BLK)
    if any(int(x) >= 1 << 48 for x in blk_off):
        raise TabixError(LIMIT, BLK)
    refs, last = [], None                                   # last: (line number, name, bin) of the data line in front
    for l, start, stop, name, beg, end in rows(text, preset):
        vb, ve = voffset(start, blk_off), voffset(stop, blk_off)
        if not refs or refs[-1]["name"] != name:
            refs.append({"name": name, "bins": {}, "linear": {}, "span": None, "lines": 0})
        R, b = refs[-1], reg2bin(beg, end)
        if last == (l - 1, name, b):                       # the run goes on: its chunk ends where this line ends
            R["bins"][b][-1] = (R["bins"][b][-1][0], ve)
        else:
            R["bins"].setdefault(b, []).append((vb, ve))
        last = (l, name, b)
        for w in range(beg >> 14, ((end - 1) >> 14) + 1):
            R["linear"][w] = min(R["linear"].get(w, vb), vb)
        R["span"] = (R["span"][0] if R["span"] else vb, ve)
        R["lines"] += 1
    for R in refs:
        n_intv = max(R["linear"]) + 1
        lin, nxt = [0] * n_intv, 0
        for w in range(n_intv - 1, -1, -1):
            nxt = R["linear"].get(w, nxt)
            lin[w] = nxt
        R["linear"] = lin
    return refs


def tbi_bytes(refs, preset):
    names = b"".join(R["name"] + b"\0" for R in refs)
    out = [b"TBI\1", struct.pack("<8i", len(refs), *HEAD[preset], 35, 0, len(names)), names]
    for R in refs:
        out.append(struct.pack("<i", len(R["bins"]) + 1))
        for b in sorted(R["bins"]):
            out.append(struct.pack("<Ii", b, len(R["bins"][b])))
            out.extend(struct.pack("<QQ", *c) for c in R["bins"][b])
        out.append(struct.pack("<IiQQQQ", PSEUDO_BIN, 2, R["span"][0], R["span"][1], R["lines"], 0))
        out.append(struct.pack("<i", len(R["linear"])))
        out.extend(struct.pack("<Q", v) for v in R["linear"])
    out.append(struct.pack("<Q", 0))
    return b"".join(out)


def tbi_raw(text, preset, blk_off):
    """the uncompressed bytes of the .tbi of the file whose blocks start at blk_off (n_blocks + 1 entries) and hold `text`"""
    return tbi_bytes(index_tables(text, preset, blk_off), preset)


def parse_tbi(raw):
    """-> {"format", "col_seq", "col_beg", "col_end", "meta", "skip", "names": [bytes], "refs": [{"bins", "linear"}], "n_no_coor"};
    the pseudo-bin is a bin like the others"""
    assert raw[:4] == b"TBI\1"
    n_ref, fmt, col_seq, col_beg, col_end, meta, skip, l_nm = struct.unpack_from("<8i", raw, 4)
    blob, at = raw[36:36 + l_nm], 36 + l_nm
    assert len(blob) == l_nm and (not l_nm or blob[-1:] == b"\0")
    names = blob.split(b"\0")[:-1] if l_nm else []
    assert len(names) == n_ref
    refs = []
    for _ in range(n_ref):
        n_bin, at = struct.unpack_from("<i", raw, at)[0], at + 4
        bins = {}
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", raw, at)
            at += 8
            assert b not in bins
            bins[b] = [struct.unpack_from("<QQ", raw, at + 16 * i) for i in range(n_chunk)]
            at += 16 * n_chunk
        n_intv, at = struct.unpack_from("<i", raw, at)[0], at + 4
        refs.append({"bins": bins, "linear": list(struct.unpack_from("<%dQ" % n_intv, raw, at))})
        at += 8 * n_intv
    n_no_coor = struct.unpack_from("<Q", raw, at)[0]
    assert at + 8 == len(raw)
    return {"format": fmt, "col_seq": col_seq, "col_beg": col_beg, "col_end": col_end, "meta": meta, "skip": skip, "names": names,
            "refs": refs, "n_no_coor": n_no_coor}


_PARSED = {}


def query(raw, name, beg, end):
    """a plain tabix reader: the chunks [(beg, end)] of virtual offsets that may hold a line of `name` overlapping [beg, end), in file
    order -- the bins of reg2bins, without the chunks that end at or in front of the linear index's lower bound.  A name the index
    does not list has none."""
    if _PARSED.get("raw") != raw:
        _PARSED.clear()
        _PARSED.update(raw=raw, t=parse_tbi(raw))
    t = _PARSED["t"]
    if name not in t["names"] or end <= beg:
        return []
    R = t["refs"][t["names"].index(name)]
    w = beg >> 14
    if w >= len(R["linear"]):
        return []
    low = R["linear"][w]
    return sorted(c for b in reg2bins(beg, min(end, MAX_END)) for c in R["bins"].get(b, []) if c[1] > low)


_OPENED = {}


def _open(f):
    import bgzf_model as zm
    if _OPENED.get("f") != f:
        blocks, _, end, ok = zm.walk(f)
        assert ok and end == len(f)
        base, size, u = {}, {}, bytearray()
        for co in blocks:
            piece = zm.inflate_block(f, co)                # header, stream, CRC32, ISIZE: zlib starts at this block
            base[co], size[co] = len(u), len(piece)
            u += piece
        starts = {s for s, _, _ in cut(u)}
        _OPENED.clear()
        _OPENED.update(f=f, base=base, size=size, u=bytes(u), bounds=starts | {len(u)})
    return _OPENED


def lines_at(file_bytes, chunks):
    """the lines (without their newline) of a BGZF text file inside the chunks of virtual offsets, meta lines included.  Every block
    is inflated on its own, so a chunk is read with zlib started at its block; a chunk that starts or ends anywhere but in a block of
    the file and at a line's start raises AssertionError"""
    F = _open(bytes(file_bytes))
    base, size, u, bounds = F["base"], F["size"], F["u"], F["bounds"]
    out = []
    for vb, ve in chunks:
        assert vb >> 16 in base and ve >> 16 in base, "a chunk starts or ends in no block of the file"
        assert (vb & 0xFFFF) <= size[vb >> 16] and (ve & 0xFFFF) <= size[ve >> 16]
        at, stop = base[vb >> 16] + (vb & 0xFFFF), base[ve >> 16] + (ve & 0xFFFF)
        assert at in bounds and stop in bounds and at < stop, "a chunk starts or ends inside a line"
        out.extend(line for _, _, line in cut(u[at:stop]))
    return out


def fetch(file_bytes, raw, preset, name, beg, end):
    """what `tabix file name:beg+1-end` prints: the data lines inside the index's chunks that overlap [beg, end)"""
    out = []
    for line in lines_at(file_bytes, query(raw, name, beg, end)):
        if line[:1] == b"#":
            continue
        n, b, e = row(line, preset)
        if n == name and b < end and e > beg:
            out.append(line)
    return out


def scan(text, preset, name, beg, end, rs=None):
    """the same lines by a plain scan of the text (rs: its rows(), where the caller asks about one text many times)"""
    text = bytes(text)
    return [text[s:t].rstrip(b"\n") for _, s, t, n, b, e in (rows(text, preset) if rs is None else rs) if n == name and b < end and e > beg]


# ---- generated inputs, shared by the CPU pin and the GPU test -------------------------------------------------------------------------
def bed_line(name, beg, end, rest=None):
    return b"\t".join([name, b"%d" % beg, b"%d" % end] + ([rest] if rest is not None else []))


def vcf_line(name, pos, ref=b"A", alt=b"C", id_=b"."):
    return b"\t".join([name, b"%d" % pos, id_, ref, alt, b".", b".", b"."])


def join(lines, last_newline=True):
    return b"\n".join(lines) + (b"\n" if lines and last_newline else b"")


def random_text(preset, seed, n_lines=300, n_names=4, max_pos=200_000, meta=0.03):
    """a sorted text of n_lines data lines over n_names names: ties, spans of 1 to 40,000 bases, some meta lines between"""
    import numpy as np
    rng = np.random.default_rng(seed)
    lines = [b"##header %d" % seed, b"#CHROM\tPOS"] if seed & 1 else []
    per = rng.multinomial(n_lines, np.ones(n_names) / n_names)
    for k in range(n_names):
        name = b"ctg%d_%s" % (k, b"x" * int(rng.integers(0, 12)))
        begs = np.sort(rng.integers(0, max_pos, per[k]))
        for b in begs:
            span = int(rng.choice([0, 1, 1, 2, 10, 300, 20_000, 40_000]))
            if preset == VCF:
                lines.append(vcf_line(name, int(b) + 1, b"ACGT"[int(rng.integers(0, 4)):][:1] * max(1, min(span, 500))))
            else:
                lines.append(bed_line(name, int(b), int(b) + span, b"%d" % int(rng.integers(0, 99)) if rng.random() < 0.5 else None))
            if rng.random() < meta:
                lines.append(b"#track %d" % len(lines))
    return join(lines, last_newline=bool(seed & 2) or not lines)


def random_regions(text, preset, seed, n=200):
    """n regions (name, beg, end): around the lines' own ends, anywhere, behind everything, and on a name the text does not have"""
    import numpy as np
    rng = np.random.default_rng(seed)
    rs = rows(text, preset)
    out = []
    for i in range(n):
        if rs and i % 4 != 3:
            _, _, _, name, b, e = rs[int(rng.integers(0, len(rs)))]
            at = (b, e, b - 1, e + 1, (b + e) // 2)[int(rng.integers(0, 5))] + int(rng.integers(-2, 3))
            beg = max(0, at)
            out.append((name, beg, beg + int(rng.choice([1, 1, 2, 50, 16384, 100_000]))))
        elif i % 8 == 3:
            out.append((b"absent", 0, 1 << 20))
        else:
            name = rs[int(rng.integers(0, len(rs)))][3] if rs else b"ctg0_"
            beg = int(rng.integers(0, 1 << 22))
            out.append((name, beg, beg + int(rng.integers(1, 70_000))))
    return out
