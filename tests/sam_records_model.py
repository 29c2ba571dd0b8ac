"""A plain model of pp_sam_records (include/polypolish_hip.h): "SAM text -> the raw records of its lines", and the generated texts its
tests run on.  Test infrastructure: tests/test_sam_records_model_cpu.py pins it to gate_model.raw_from_text and to bam_model on the
same texts, tests/test_sam_records_gpu.py runs the device decode (pp_sam.hip) against it.  It does not call the library.

decode() is Alignment::new per line through ingest_model._parse (oracle/pyref.py), the runs of ingest_model.packed_runs, and the byte
offsets of the columns in the text: the SEQ bytes are not copied, seq_off points into the text."""
import numpy as np

import ingest_model as im
from ingest_model import PANIC, QUIT

LIMIT, NOT_ASCII = 5, 6
NO_NM = 0xFFFFFFFF
SAM_BLOCK = 1024            # lines per workgroup of the placing kernel (pp_sam.hip)
MAX_RUN = im.MAX_RUN
FIELDS = (("flag", np.uint16), ("read_id", np.uint64), ("contig", np.uint32), ("ref_start", np.uint32), ("nm", np.uint32),
          ("seq_off", np.uint64), ("seq_len", np.uint32), ("cig_off", np.uint64), ("n_cig", np.uint32), ("cigar", np.uint32),
          ("name_off", np.uint64), ("name_len", np.uint32), ("rname_off", np.uint64), ("rname_len", np.uint32), ("line", np.uint32))


class SamError(Exception):
    """code: QUIT / PANIC / LIMIT / NOT_ASCII; bad_line: the 0-based index of the refused line among all lines (None for NOT_ASCII,
    which refuses the text as a whole)"""

    def __init__(self, code, bad_line, kind=""):
        super().__init__(f"[{code}] {kind} at line {bad_line}")
        self.code, self.bad_line, self.kind = code, bad_line, kind


def decode(text):
    """-> {the arrays of FIELDS, "zp": one byte per ALIGNED record (0 = the line carries ZP:Z:fail), "seq": the text itself}, or raises
    SamError for the first refused line in file order.  read_id and contig are zeros: the caller's to fill."""
    text = bytes(text)
    if any(b >= 0x80 for b in text):        # as pp_dev_ingest_sam: the whole text, wherever the byte is
        raise SamError(NOT_ASCII, None, "not_ascii")
    lines = im._lines(text)
    starts = im.line_spans(text)[0]
    assert len(lines) == len(starts)
    rows, zp, cigar = [], [], []
    for li, line in enumerate(lines):
        if not line or line[0] == "@":
            continue
        try:
            a = im._parse(line, "text", li + 1)
        except im.ModelError as e:
            raise SamError(e.code, li, e.kind)
        parts = line.split("\t")
        at = [sum(len(p) for p in parts[:k]) + k for k in range(11)]    # the columns' offsets in the line
        # a line the reference takes but a raw batch cannot hold
        if a.flags > 0xFFFF:
            raise SamError(LIMIT, li, "flag_above_u16")
        if a.ref_start > 0xFFFFFFFE:
            raise SamError(LIMIT, li, "pos_above_u32")
        if a.is_aligned() and parts[9] == "":
            raise SamError(LIMIT, li, "empty_seq")
        runs = im.packed_runs(a.cigar)
        s = int(starts[li])
        rows.append((a.flags, 0, 0, a.ref_start, a.mismatches, s + at[9], 0 if parts[9] == "*" else len(parts[9]), len(cigar), len(runs),
                     None, s, len(parts[0]), s + at[2], len(parts[2]), li))
        cigar += runs
        if a.is_aligned():
            zp.append(1 if a.pass_qc else 0)
    out = {k: np.array([r[i] for r in rows], dt) for i, (k, dt) in enumerate(FIELDS) if k != "cigar"}
    out["cigar"] = np.array(cigar, np.uint32)
    out["zp"] = np.array(zp, np.uint8)
    out["seq"] = np.frombuffer(text, np.uint8)
    return out


def seq_bytes(dec):
    """the SEQ bytes of every record, gathered through seq_off and seq_len (b"" for "*")"""
    s = dec["seq"].tobytes()
    return [s[int(o):int(o) + int(n)] for o, n in zip(dec["seq_off"], dec["seq_len"])]


def column(dec, which):
    """the QNAMEs (which = "name") or RNAMEs ("rname") gathered through their ranges"""
    s = dec["seq"].tobytes()
    return [s[int(o):int(o) + int(n)] for o, n in zip(dec[which + "_off"], dec[which + "_len"])]


def same(got, want, keys=None):
    """the arrays byte for byte (all of FIELDS and the text by default)"""
    for k in keys or [k for k, _ in FIELDS] + ["seq"]:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (k, a[:8], b[:8])


# ---- generated inputs: the seams of pp_sam.hip ------------------------------------------------------------------------------------
RECORD_COUNTS = (1, 63, 64, 65, SAM_BLOCK - 1, SAM_BLOCK, SAM_BLOCK + 1, 2 * SAM_BLOCK + 1)
ALL_OPS = "1M1I1D1N1S1H1P1=1X"
LONG_RUNS = (MAX_RUN, MAX_RUN + 1, 3 * MAX_RUN + 1)


def unaligned(g, **kw):
    return g.line(flag=4, cigar="*", nm=None, rname="*", **kw)


def count_text(n_rec, plain=False, seed=300):
    """n_rec records, aligned and unaligned in turn, the aligned ones with 1..5 CIGAR runs and now and then ZP:Z:fail; unless
    `plain`, header lines and empty lines in between (a record's line is then not its index), the first line a header"""
    g, T = im.Gen(seed + n_rec), im.Text()
    if not plain:
        T.add("@HD\tVN:1.6")
    for r in range(n_rec):
        if not plain and r % 3 == 1:
            T.add("@CO\tbetween " + "x" * (r % 7))
        if not plain and r % 5 == 2:
            T.add("")
        if r % 2:
            T.add(unaligned(g))
        else:
            k = r // 2 % 5 + 1
            T.add(g.line(n=24, cigar="2M1I" * (k // 2) + ("3M" if k % 2 else ""), nm=r % 4, tags=("ZP:Z:fail",) if r % 7 == 0 else ()))
    return T.bytes()


def cigar_text(seed=310):
    """(text, the expected n_cig of every record)"""
    g, T = im.Gen(seed), im.Text()
    cig = ["30M", "*", "0S30M", "15M0I15M", "30M0S", "0M"] + [f"{n}M" for n in LONG_RUNS] + [ALL_OPS, "30M", "1M1I" * 20, "30M"]
    for c in cig:
        T.add(g.line(n=30, cigar=c, qual="*"))
    return T.bytes(), [1, 0, 1, 2, 1, 0, 1, 2, 4, 9, 1, 40, 1]


def tag_text(seed=320):
    """(text, the expected nm of every record, the expected pass byte of every aligned record)"""
    g, T = im.Gen(seed), im.Text()
    nm, zp = [], []

    def add(line, want_nm, want_zp):
        T.add(line)
        nm.append(want_nm)
        if want_zp is not None:
            zp.append(want_zp)
    add(unaligned(g), NO_NM, None)                                      # eleven columns, no tag fields
    add(unaligned(g) + "\t", NO_NM, None)                               # ... and one empty field behind a trailing tab
    add(g.line(nm=4) + "\t", 4, 1)
    add(g.line(nm="+7"), 7, 1)
    add(g.line(tags=("NM:i:99",), nm=3), 3, 1)                          # the last NM:i: wins
    add(g.line(tags=("NM:Z:9",), nm=1), 1, 1)
    add(unaligned(g, tags=("NM:Z:9",)), NO_NM, None)
    add(g.line(tags=("nm:i:5",), nm=2), 2, 1)
    add(unaligned(g, tags=("nm:i:5", "Nm:i:6")), NO_NM, None)
    add(unaligned(g, tags=("NM:i:8",)), 8, None)                        # an unaligned line may carry one
    for z in ("ZP:Z:fail", "zp:z:FAIL", "Zp:Z:FaIl"):
        add(g.line(tags=(z,), nm=0), 0, 0)                              # in front of NM
        add(g.line(nm=0) + "\t" + z, 0, 0)                              # ... and behind it
    add(g.line(tags=("ZP:Z:failx",), nm=0), 0, 1)                       # ten bytes
    add(g.line(nm=0) + "\tZP:Z:fai", 0, 1)                              # eight
    add(g.line(tags=("ZP:Z:fail ",), nm=0), 0, 1)
    add(unaligned(g, tags=("ZP:Z:fail",)), NO_NM, None)                 # no pass byte for an unaligned line
    return T.bytes(), nm, zp


HOSTILE = b"\tNM:i:7\tZP:Z:fail\n"


def array_end_cases(seed=330):
    """[(name, whole, n)]: `whole` = a text of n bytes followed by hostile bytes that continue its last line with NM:i:7 and ZP:Z:fail
    and then add a whole line.  The prefix ends with a line's last byte, inside a line (in front of its NM tag: the prefix alone is
    refused, the bytes behind it would give the line one), right behind a "\\r" and right behind a "\\n"."""
    out = []
    for name, eol, cut in (("line_end", "\n", "eol"), ("inside_a_line", "\n", "inside"), ("behind_cr", "\r\n", "cr"), ("behind_lf", "\n", None)):
        g, T = im.Gen(seed, (3000,)), im.Text(eol)
        for i in range(70):
            T.add(g.line(nm=i % 3, length=150))         # (the pad tag XX:Z:aaa... sits in front of NM)
        text = T.bytes()
        if cut == "eol":
            text = text[:-1]
        elif cut == "cr":
            text = text[:-1]
            assert text.endswith(b"\r")
        elif cut == "inside":
            text = text[:text.rindex(b"\tNM:i:")]       # the last line ends inside its pad tag, without NM: refused -- what follows
        extra = g.line(name="beyond_the_end", nm=0).encode() + b"\n"
        out.append((name, text + HOSTILE + extra, len(text)))
    return out


def error_texts(seed=340):
    """{kind: (text, code, bad_line)}: every kind of ingest_model._parse, each on line 7 of 12, behind a header and an empty line"""
    bad = {"too_few_columns": (QUIT, lambda g: "x\t0\tctg0\t1\t60\t24M"), "missing_NM_tag": (QUIT, lambda g: g.line(nm=None)),
           "invalid_cigar": (QUIT, lambda g: g.line(cigar="24Q")), "flag": (PANIC, lambda g: g.line(flag="0x10")),
           "pos": (PANIC, lambda g: g.line().replace("\tctg0\t", "\tctg0\t-", 1)), "nm": (PANIC, lambda g: g.line(nm="7x")),
           "cigar_overflow": (PANIC, lambda g: g.line(cigar="4294967296M"))}
    out = {}
    for kind, (code, make) in bad.items():
        g, T = im.Gen(seed), im.Text()
        T.add("@HD\tVN:1.6")
        T.add("")
        for _ in range(5):
            T.add(g.line())
        T.add(make(g))
        for _ in range(4):
            T.add(g.line())
        out[kind] = (T.bytes(), code, 7)
    return out


def limit_texts(seed=350):
    """{kind: (text, bad_line)}: lines the reference takes and a raw batch cannot hold; and their neighbours it can"""
    out = {}
    lines = {"flag_above_u16": lambda g: g.line(flag=65536), "pos_above_u32": lambda g: g.line(pos=(1 << 32) - 1),
             "empty_seq": lambda g: g.line(seq="", qual="*", cigar="24M")}
    for kind, make in lines.items():
        g, T = im.Gen(seed), im.Text()
        for _ in range(3):
            T.add(g.line())
        T.add(make(g))
        T.add(g.line())
        out[kind] = (T.bytes(), 3)
    g, T = im.Gen(seed), im.Text()
    T.add(g.line(flag=65535 & ~4))
    T.add(g.line(pos=(1 << 32) - 2))                    # POS 2^32-1
    T.add(unaligned(g, seq="", qual="*"))               # an empty SEQ on an unaligned line is nobody's read
    T.add(g.line(seq="*", cigar="24M"))
    out["fits"] = (T.bytes(), None)
    return out


def two_bad_lines(seed=360):
    """[(text, code, bad_line)]: two refused lines of different kinds in either order, and a LIMIT line in front of a QUIT line"""
    out = []
    for first, second, code in (("pos", "missing", PANIC), ("missing", "pos", QUIT), ("limit", "missing", LIMIT), ("missing", "limit", QUIT)):
        g, T = im.Gen(seed), im.Text()
        make = {"pos": lambda: g.line().replace("\tctg0\t", "\tctg0\t-", 1), "missing": lambda: g.line(nm=None), "limit": lambda: g.line(flag=70000)}
        for _ in range(3):
            T.add(g.line())
        T.add(make[first]())
        for _ in range(100):        # (the second one in another wave of the scan)
            T.add(g.line())
        T.add(make[second]())
        out.append((T.bytes(), code, 3))
    return out
