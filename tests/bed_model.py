"""The definition of the bytes pp_status_bed / pp_polish_bed and pp_polish_masked (pp_k_bed.h, pp_bed_host.h) write, in plain Python.
tests/test_bed_model_cpu.py pins this file on the CPU (hand-written bytes for every word; the oracle's --debug TSV against its
per-position records); the GPU tests hold the library against it byte for byte, fed from the oracle, never from the device.

  status    one of six per assembly position, PP_ST_* in the order of src/pileup.rs:156-163: WORDS
  text      no header line.  Per record, in assembly order:  name \\t start \\t end \\t word \\n  -- start and end 0-based, half-open and
            local to the contig
  record    a maximal run of consecutive positions of ONE contig (runs never join across a contig boundary) that share one status
            whose bit 1 << status is set in the mask.  Names are written verbatim
  masked    position p emits emit_len[p] bytes of the polished output, one position behind the other; every byte 'A'..'Z' emitted by a
            position with a selected status becomes lower case, every other byte stays"""
import numpy as np

WORDS = (b"kept", b"changed", b"low_depth", b"none", b"multiple", b"too_close")
KEPT, CHANGED, LOW_DEPTH, NONE, MULTIPLE, TOO_CLOSE = range(6)
ALL = (1 << 6) - 1
UNDECIDED = (1 << LOW_DEPTH) | (1 << NONE) | (1 << MULTIPLE) | (1 << TOO_CLOSE)  # PP_BED_UNDECIDED


def _b(x):
    return x.encode() if isinstance(x, str) else bytes(x)


def _u8(x):
    return np.frombuffer(x, np.uint8) if isinstance(x, (bytes, bytearray)) else np.asarray(x, np.uint8)


def records(status, contig_off, mask):
    """[(contig index, start, end, status)] -- start and end local to the contig"""
    st = _u8(status)
    off = [int(x) for x in contig_off]
    assert off[0] == 0 and len(st) == off[-1] and 0 < mask <= ALL and (len(st) == 0 or int(st.max()) < 6)
    out = []
    for c in range(len(off) - 1):
        lo, hi = off[c], off[c + 1]
        if hi == lo:
            continue
        s = st[lo:hi]
        cuts = np.concatenate([[0], np.nonzero(s[1:] != s[:-1])[0] + 1, [hi - lo]])  # every change of status begins a run
        for a, b in zip(cuts[:-1], cuts[1:]):
            if (mask >> int(s[a])) & 1:
                out.append((c, int(a), int(b), int(s[a])))
    return out


def bed(status, contig_off, names, mask=UNDECIDED):
    return b"".join(b"%s\t%d\t%d\t%s\n" % (_b(names[c]), a, b, WORDS[s]) for c, a, b, s in records(status, contig_off, mask))


def counts(status, contig_off, mask=UNDECIDED):
    """positions per status inside the records"""
    n = [0] * 6
    for _, a, b, s in records(status, contig_off, mask):
        n[s] += b - a
    return tuple(n)


def masked(polished, emit_len, status, mask=UNDECIDED):
    pol = np.frombuffer(bytes(polished), np.uint8).copy()
    ln = np.asarray(emit_len, np.int64)
    st = _u8(status)
    assert len(ln) == len(st) and int(ln.sum()) == len(pol) and 0 < mask <= ALL
    sel = np.repeat(((mask >> st.astype(np.int64)) & 1).astype(bool), ln)  # per output byte: its position is selected
    up = (pol >= ord("A")) & (pol <= ord("Z"))
    pol[sel & up] |= 0x20
    return pol.tobytes()


def parse_status_list(text):
    """the mask of a --bed_status list: comma-separated words, each one of the six; ValueError for an empty list, an empty item or an
    unknown word"""
    text = _b(text)
    if not text:
        raise ValueError("an empty status list")
    mask = 0
    for w in text.split(b","):
        if w not in WORDS:
            raise ValueError("%r is not a status" % w)
        mask |= 1 << WORDS.index(w)
    return mask


def status_of_debug_tsv(tsv):
    """the status column (the last but one) of a --debug TSV, line by line behind its header line, as PP_ST_* bytes"""
    lines = bytes(tsv).split(b"\n")
    assert lines[0].startswith(b"name\tpos\t") and lines[-1] == b""
    return np.array([WORDS.index(ln.rsplit(b"\t", 2)[1]) for ln in lines[1:-1]], np.uint8)


def parse(text):
    """[(name, start, end, word)] of a text this model writes"""
    out = []
    for ln in bytes(text).split(b"\n")[:-1]:
        name, a, b, w = ln.rsplit(b"\t", 3)
        out.append((name, int(a), int(b), w))
    return out
