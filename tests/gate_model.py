"""A plain model of pp_batch_gate (include/polypolish_hip.h): "the raw alignment records of one SAM file -> the good records".
Test infrastructure: tests/test_gate_model_cpu.py pins it to ingest_model.model() -- the model of the text ingests -- on every
named case of that table, tests/test_batch_gate_gpu.py runs the device gate (pp_gate.hip) against it.  It does not call the
library.

raw_from_text is Alignment::new (oracle/pyref.py) per line, laid out as a FOREIGN batch: SEQ bytes as the line has them (any
case) packed back to back at odd offsets, the array ending exactly at the last read's last byte.  gate() restates
process_one_read (alignment.rs:275-322) over those arrays."""
import numpy as np

from oracle import pyref

import ingest_model
from ingest_model import ARG, PANIC, QUIT, SEQ_ALIGN

NO_CONTIG = 0xFFFFFFFF      # RNAME that is not in the assembly: an index out of range, which travels on to the polish
RAW_FIELDS = (("flag", np.uint16), ("read_id", np.uint64), ("contig", np.uint32), ("ref_start", np.uint32), ("nm", np.uint32),
              ("seq_off", np.uint64), ("seq_len", np.uint32), ("cig_off", np.uint64), ("n_cig", np.uint32), ("seq", np.uint8),
              ("cigar", np.uint32))
REC_KEYS = ("contig", "ref_start", "k", "seq_off", "seq_len", "cig_off", "n_cig", "seq", "cigar")
COMP = {a: b for a, b in zip("ATGCRYSWKMBVDHN.-?", "TACGYRSWMKVBHDN.-?")}    # misc.rs:170-182


class NotRaw(Exception):
    """the text has a line Alignment::new refuses, or a value a pp_raw_batch cannot hold: its records are nobody's raw batch"""


class GateError(Exception):
    def __init__(self, code, kind, bad_record=None):
        super().__init__(f"[{code}] {kind} at record {bad_record}")
        self.code, self.kind, self.bad_record = code, kind, bad_record


def raw_from_text(contigs, text):
    """(raw, zp): the arrays of pp_raw_batch for one SAM text, and one byte per ALIGNED record, 0 where its line carries
    ZP:Z:fail.  Unaligned lines are kept (FLAG & 4).  QNAMEs are interned to ids so that "equal ids" is the reference's grouping:
    an aligned record joins the one in front when that one's QNAME is equal -- or empty (alignment.rs:255), which a caller who
    interns names has to know; such a record takes the id of the record in front."""
    index = {name: i for i, (name, _) in enumerate(contigs)}
    ids, rows, zp = {}, [], []
    prev_name, prev_id, fresh = None, None, 1 << 40
    for ln, line in enumerate(ingest_model._lines(text), 1):
        if not line or line[0] == "@":
            continue
        try:
            a = ingest_model._parse(line, "file", ln)
        except ingest_model.ModelError as e:
            raise NotRaw(e.kind)
        if a.flags > 0xFFFF or a.ref_start > 0xFFFFFFFE:
            raise NotRaw("value beyond the raw batch's fields")
        runs = ingest_model.packed_runs(a.cigar)
        seq = line.split("\t")[9]
        rid = ids.setdefault(a.read_name, len(ids))
        if a.is_aligned():
            if prev_name is not None and (prev_name == "" or prev_name == a.read_name):
                rid = prev_id
            elif rid == prev_id:    # a new group whose name's id the group in front borrowed through an empty QNAME
                rid, fresh = fresh, fresh + 1
            prev_name, prev_id = a.read_name, rid
            zp.append(1 if a.pass_qc else 0)
        rows.append((a.flags, rid, index.get(a.ref_name, NO_CONTIG), a.ref_start, a.mismatches, b"" if seq == "*" else seq.encode("ascii"), runs))
    return pack_raw(rows), np.array(zp, np.uint8)


def pack_raw(rows, lead=3):
    """rows of (flag, read_id, contig, ref_start, nm, seq bytes, runs) -> the arrays; `lead` bytes in front of the first read make
    the offsets odd, nothing follows the last read"""
    seq_len = np.array([len(r[5]) for r in rows], np.uint32)
    n_cig = np.array([len(r[6]) for r in rows], np.uint32)
    have = bool(seq_len.sum())
    seq = np.frombuffer((b"x" * lead if have else b"") + b"".join(r[5] for r in rows), np.uint8).copy()
    return {"flag": np.array([r[0] for r in rows], np.uint16), "read_id": np.array([r[1] for r in rows], np.uint64),
            "contig": np.array([r[2] for r in rows], np.uint32), "ref_start": np.array([r[3] for r in rows], np.uint32),
            "nm": np.array([r[4] for r in rows], np.uint32),
            "seq_off": ((lead if have else 0) + np.cumsum(seq_len, dtype=np.int64) - seq_len).astype(np.uint64), "seq_len": seq_len,
            "cig_off": (np.cumsum(n_cig, dtype=np.int64) - n_cig).astype(np.uint64), "n_cig": n_cig, "seq": seq,
            "cigar": np.array([x for r in rows for x in r[6]], np.uint32)}


def upper(b):
    return bytes(c - 32 if 97 <= c <= 122 else c for c in b)


def revcomp_upper(b):
    return "".join(COMP.get(chr(c), "N") for c in reversed(upper(b))).encode("ascii")


def groups(raw):
    """[[raw indices]]: maximal runs of adjacent ALIGNED records with equal read_id"""
    out, last = [], None
    for r in np.flatnonzero((raw["flag"] & 4) == 0).tolist():
        rid = int(raw["read_id"][r])
        if out and rid == last:
            out[-1].append(r)
        else:
            out.append([r])
        last = rid
    return out


def gate(raw, max_errors=10, careful=False, passed=None):
    """-> {"recs": the arrays of pp_aln_batch (SEQ rooms in record order), "orig", "counts": (alignments, used, reads)}, or raises
    GateError(code, kind, bad_record) for the first failing group in file order (ARG "verdict_count" behind every defect)."""
    seq_all, cig_all = raw["seq"].tobytes(), raw["cigar"]
    n_seq, n_cig_total = len(seq_all), len(cig_all)
    grp = groups(raw)
    rank = {r: a for a, r in enumerate(r for g in grp for r in g)}
    out = []
    for g in grp:
        if careful and len(g) > 1:
            continue
        for r in g:     # the contract: checked before anything is read through a range
            so, sl, co, nc = int(raw["seq_off"][r]), int(raw["seq_len"][r]), int(raw["cig_off"][r]), int(raw["n_cig"][r])
            if sl and so + sl > n_seq:
                raise GateError(ARG, "seq_range", r)
            if nc and co + nc > n_cig_total:
                raise GateError(ARG, "cig_range", r)
    for g in grp:
        if careful and len(g) > 1:
            continue
        src = next((r for r in g if raw["seq_len"][r] > 0), None)
        if src is None:
            raise GateError(QUIT, "no_sequence", g[0])
        good = []
        for r in g:
            co, nc = int(raw["cig_off"][r]), int(raw["n_cig"][r])
            if nc == 0:
                raise GateError(PANIC, "empty_cigar", g[0])
            ok = passed is None or rank[r] >= len(passed) or bool(passed[rank[r]])
            if (int(cig_all[co]) & 15) in (0, 7) and (int(cig_all[co + nc - 1]) & 15) in (0, 7) and int(raw["nm"][r]) <= max_errors and ok:
                good.append(r)
        for r in good:
            so, sl = int(raw["seq_off"][r]), int(raw["seq_len"][r])
            if sl:
                seq = upper(seq_all[so:so + sl])
            else:
                s = seq_all[int(raw["seq_off"][src]):int(raw["seq_off"][src]) + int(raw["seq_len"][src])]
                seq = upper(s) if (int(raw["flag"][r]) ^ int(raw["flag"][src])) & 16 == 0 else revcomp_upper(s)
            co, nc = int(raw["cig_off"][r]), int(raw["n_cig"][r])
            out.append((r, len(good), seq, cig_all[co:co + nc]))
    if passed is not None and len(passed) != len(rank):
        raise GateError(ARG, "verdict_count")
    seq_len = np.array([len(o[2]) for o in out], np.uint32)
    room = (seq_len.astype(np.int64) + SEQ_ALIGN - 1) & ~(SEQ_ALIGN - 1)
    seq_off = (np.cumsum(room) - room).astype(np.uint64)
    seq = np.zeros(int(room.sum()), np.uint8)
    for o, at in zip(out, seq_off.tolist()):
        seq[at:at + len(o[2])] = np.frombuffer(o[2], np.uint8)
    n_cig = np.array([len(o[3]) for o in out], np.uint32)
    orig = np.array([o[0] for o in out], np.uint32)
    recs = {"contig": raw["contig"][orig], "ref_start": raw["ref_start"][orig], "k": np.array([o[1] for o in out], np.uint32),
            "seq_off": seq_off, "seq_len": seq_len, "cig_off": (np.cumsum(n_cig, dtype=np.int64) - n_cig).astype(np.uint64),
            "n_cig": n_cig, "seq": seq,
            "cigar": np.concatenate([o[3] for o in out]).astype(np.uint32) if out else np.zeros(0, np.uint32)}
    return {"recs": recs, "orig": orig, "counts": (len(rank), len(out), len(grp))}


def same(got, want):
    """the nine arrays byte for byte"""
    for k in REC_KEYS:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (k, a[:8], b[:8])


def passed_for(c, f, zp):
    """the caller's verdicts for file f of ingest_model case c: the case's own, as many as they are, AND "the line carries no
    ZP:Z:fail" (None when there is nothing to say)"""
    if c.verdicts is None:
        return zp if not zp.all() else None
    v = np.asarray(c.verdicts[f], np.uint8).copy()
    n = min(len(v), len(zp))
    v[:n] &= zp[:n]
    return v


def expect_from_model(c, f, zp):
    """What the gate owes on file f of ingest_model case c, taken from ingest_model.model() of that file alone:
    ("ok", model result) | ("error", code, kind) | ("contig", None): the model quits over an RNAME that is not in the assembly,
    which the gate cannot know -- the index travels on and the polish reports it | ("empty", None): no aligned records, which is
    the caller's sentence.  verdicts = the case's AND zp are the caller's `passed`."""
    v = None if c.verdicts is None else [c.verdicts[f]]
    try:
        return ("ok", ingest_model.model(c.contigs, [c.texts[f]], None, c.max_errors, c.careful, v))
    except ingest_model.ModelError as e:
        if e.kind == "not_in_assembly":
            return ("contig", None)
        if e.kind == "empty_group":
            return ("empty", None)
        return ("error", e.code, e.kind)


# ---- generated inputs: the seams of the gate's kernels ---------------------------------------------------------------------------
GATE_BLOCK = 1024           # records per workgroup of the scanning kernels (pp_gate.hip)
START_RANKS = (63, 64, 65, 255, 256, 257, GATE_BLOCK)    # aligned ranks at which a group has to start
ACGT = np.frombuffer(b"ACGT", np.uint8)
SRC33 = b"acgtRYSWKMBVDHNryswkmbvdhn.-?xZ@[`{"[:33]


def _row(rng, rid, n=24, flag=0, nm=0, seq=None, runs=None, contig=0, lower=False):
    if seq is None:
        seq = ACGT[rng.integers(0, 4, n)].tobytes()
        if lower:
            seq = seq.lower()
    if runs is None:
        runs = [(max(len(seq), 1) << 4)]
    return (flag, rid, contig, int(rng.integers(0, 5000)), nm, seq, runs)


def seam_rows(seed=5):
    """~9,000 records: groups that start at every rank of START_RANKS, unaligned records first, last and between equal ids, good
    and rejected records by every gate, "*" fills on both strands, every read length of the list, a 33-byte source filled into
    three records.  -> (rows, passed)"""
    rng = np.random.default_rng(seed)
    rows, n_al, rid = [], 0, 100

    def add(row):
        nonlocal n_al
        rows.append(row)
        n_al += 0 if row[0] & 4 else 1

    add(_row(rng, 1, flag=4, runs=[]))                      # unaligned first
    add(_row(rng, 2, flag=4, seq=b"", runs=[]))
    while n_al < GATE_BLOCK + 40:
        rid += 1
        if n_al + 1 in START_RANKS:                         # a single record, so that the next group starts on the rank
            add(_row(rng, rid))
            continue
        if n_al in START_RANKS:                             # a group of three across the rank's edge, an unaligned record inside
            add(_row(rng, rid, lower=True))
            add(_row(rng, 7, flag=4, runs=[]))
            add(_row(rng, rid, flag=256 | 16, seq=b"", runs=[24 << 4]))
            add(_row(rng, rid, flag=256, seq=b"", runs=[24 << 4], nm=11))
            continue
        add(_row(rng, rid, n=int(rng.integers(1, 200))))
    for sl in (1, 15, 16, 17, 31, 32, 33, 160):
        for lower in (False, True):
            rid += 1
            add(_row(rng, rid, n=sl, lower=lower))
    rid += 1                                                # a source of 33 bytes filled into three records, both strands
    add(_row(rng, rid, seq=b"", runs=[33 << 4], flag=256))
    add(_row(rng, rid, seq=SRC33, runs=[(30 << 4) | 7, (1 << 4) | 1, (2 << 4)], flag=16, nm=3))
    add(_row(rng, rid, seq=b"", runs=[33 << 4], flag=256 | 16))
    add(_row(rng, rid, seq=b"", runs=[33 << 4], flag=2048))
    for i in range(8000):                                   # the bulk: groups of 1-3, every gate rejecting now and then
        rid += 1
        size = (1, 1, 1, 2, 3)[i % 5]
        for j in range(size):
            how = (i + j) % 7
            runs = [(4 << 4) | 4, (20 << 4)] if how == 3 else ([(20 << 4), (4 << 4) | 5] if how == 5 else [(24 << 4)])
            star = j > 0 and (i % 3 == 0)
            add(_row(rng, rid, seq=b"" if star else None, runs=runs, flag=(256 if j else 0) | (16 if (i + j) % 4 == 0 else 0),
                     nm=11 if how == 1 else (10 if how == 2 else 0), lower=i % 11 == 0))
        if i % 97 == 0:
            add(_row(rng, 9, flag=4, runs=[]))
    add(_row(rng, 3, flag=4, runs=[]))                      # unaligned last
    passed = (rng.random(n_al) < 0.8).astype(np.uint8)
    return rows, passed


def big_group_rows(seed=6):
    """77 single reads, then ONE group of 3,000 records (several workgroups) whose only sequence is on its record 2,500, strands
    mixed, every third record failing a gate; then 50 single reads"""
    rng = np.random.default_rng(seed)
    rows = [_row(rng, 10 + i) for i in range(77)]
    src = ACGT[rng.integers(0, 4, 131)].tobytes().lower()
    for i in range(3000):
        rows.append(_row(rng, 5, seq=src if i == 2500 else b"", runs=[131 << 4], flag=(256 if i else 0) | (16 if i % 5 in (1, 3) else 0),
                         nm=11 if i % 3 == 0 else 2))
    rows += [_row(rng, 1000 + i) for i in range(50)]
    return rows
