"""A plain model of the SAM-text write side (include/polypolish_hip.h: pp_sam_tagged).  Test infrastructure: it does not call the library.
tagged() is the output text: every line again, cut at "\\n" with one trailing "\\r" dropped, every line ended by "\\n", and "\\tZP:Z:fail"
behind the content of the aligned records whose verdict is 0.  tests/test_sam_tag_model_cpu.py pins it to pp_filter_write_text and to
the oracle's `filter`; tests/test_sam_tagged_gpu.py runs the device (pp_sam_out.hip) against it.

Also here: the vocabulary of lines both test files build their texts from."""
import re

import numpy as np

TAG = b"\tZP:Z:fail"
U32 = re.compile(rb"\+?[0-9]+")


class TagError(Exception):
    """PP_ERR_ARG: another number of verdicts than aligned records"""

    def __init__(self, n_pass, n_aligned):
        super().__init__(f"{n_pass} verdicts for {n_aligned} aligned records")
        self.n_pass, self.n_aligned = n_pass, n_aligned


def aligned(line):
    """is this line's content (no "\\n", no dropped "\\r") an aligned record?  Not empty, no "@" in front, a tab, and a second column that
    is a u32 (str::parse: digits behind at most one "+", at most 4294967295) with bit 2 clear.  Nothing else is looked at."""
    if not line or line[:1] == b"@" or b"\t" not in line:
        return False
    flag = line.split(b"\t")[1]
    return bool(U32.fullmatch(flag)) and int(flag) <= 0xFFFFFFFF and not int(flag) & 4


def contents(text):
    """the lines' contents: cut at "\\n" (a last line needs none), one trailing "\\r" dropped"""
    lines = bytes(text).split(b"\n")
    if lines[-1] == b"":
        lines.pop()                      # (behind the last "\n", or an empty text: no line)
    return [ln[:-1] if ln.endswith(b"\r") else ln for ln in lines]


def tagged(text, pass_):
    """-> (the output bytes, aligned records that passed, that failed, lines).  Raises TagError where pass_ (None: no verdicts) has
    another length than the number of aligned records."""
    lines = contents(text)
    verdicts = [] if pass_ is None else [int(v) for v in pass_]
    n_aligned = sum(1 for ln in lines if aligned(ln))
    if len(verdicts) != n_aligned:
        raise TagError(len(verdicts), n_aligned)
    out, rank, n_fail = [], 0, 0
    for ln in lines:
        fail = False
        if aligned(ln):
            fail, rank = verdicts[rank] == 0, rank + 1
        n_fail += fail
        out.append(ln + (TAG if fail else b"") + b"\n")
    return b"".join(out), n_aligned - n_fail, n_fail, len(lines)


def n_aligned(text):
    return sum(1 for ln in contents(text) if aligned(ln))


# ---- the vocabulary: line contents, and whether each is an aligned record -----------------------------------------------------------
def record(name=b"r1", flag=b"0", rest=b"ctg\t1\t60\t4M\t*\t0\t0\tACGT\tIIII\tNM:i:0"):
    return name + b"\t" + flag + b"\t" + rest


VOCABULARY = [
    (record(), True),
    (record(flag=b"16"), True),
    (record(flag=b"+16"), True),                              # parse::<u32> takes one "+"
    (record(flag=b"4294967291"), True),                       # bit 2 clear, below 2^32
    (record(flag=b"4294967295"), False),                      # the largest u32: bit 2 set
    (record(flag=b"4294967296"), False),                      # no u32
    (record(flag=b"00000000000000000000000000000000000016"), True),
    (record(flag=b"4"), False),
    (record(flag=b"+4"), False),
    (record(flag=b"77"), False),                              # 64 + 8 + 4 + 1
    (record(flag=b"0x10"), False),
    (record(flag=b"-0"), False),
    (record(flag=b"++1"), False),
    (record(flag=b"+"), False),
    (record(flag=b""), False),
    (record(flag=b" 0"), False),
    (record(flag=b"0 "), False),
    (b"name_only\t0", True),                                  # two columns are enough: the flag column runs to the line's end
    (b"name_only\t", False),
    (b"\t0", True),                                           # an empty QNAME
    (b"\t", False),
    (b"no tab at all 0", False),
    (b"", False),
    (b"@HD\tVN:1.6", False),
    (b"@SQ\t0\tSN:ctg", False),                               # "@" in front: never a record, whatever follows
    (b"@", False),
    (record() + TAG, True),                                   # already tagged: a failing one gets a second tag
    (record(flag=b"4") + TAG, False),
    (record(name=b"r\xc3\xa9ad\xff\x80") + b"\tco:Z:\xfe", True),     # bytes >= 0x80 are bytes
    (b"\xff\xfe\t4\t\x80", False),
    (b"\r", False),                                           # contents that END in "\r": the text has "\r\r\n" there
    (record() + b"\r", True),
    (b"x\t0\r", False),                                       # the flag column is "0\r"
    (record(rest=b"ctg\t1\t60\t4M"), True),                   # six columns: pp_sam_records would refuse the line, this copy does not
    (record(rest=b"*\t0\t0\t*\t*\t0\t0\t" + b"ACGT" * 200 + b"\t" + b"I" * 800), True),
]


def mixed_text(n_lines, seed, eol_mix=True):
    """(text, n_aligned): n_lines lines whose contents are drawn from the vocabulary (plain records most often), "\\n" and "\\r\\n" endings
    mixed, the last line without a newline"""
    rng = np.random.default_rng(seed)
    out, n = [], 0
    for i in range(n_lines):
        k = int(rng.integers(0, 3 * len(VOCABULARY)))
        line, al = VOCABULARY[k] if k < len(VOCABULARY) else (record(name=b"read_%d" % i, flag=b"%d" % (16 * int(rng.integers(0, 2)))), True)
        assert aligned(line) == al, line
        n += al
        cr = line.endswith(b"\r") or (eol_mix and rng.integers(0, 4) == 0)     # (a content that ends in "\r" needs one more to keep it)
        out.append(line + (b"\r" if cr else b"") + (b"" if i + 1 == n_lines else b"\n"))
    return b"".join(out), n
