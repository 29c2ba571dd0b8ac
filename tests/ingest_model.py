"""A plain model of "SAM text -> pp_aln_batch" (include/polypolish_hip.h) and a generator of SAM texts built to the byte.
Test infrastructure: tests/test_ingest_model_cpu.py pins the model to the host ingest and to the oracle on every named case of
CASES, tests/test_tokenizer_seam_gpu.py runs the device tokenizer (pp_tokenize.hip, pp_devtext.h) against it on the same
cases.  It does not call the library.

The model leans on oracle/pyref.py for Alignment::new (src/alignment.rs:49-98) and the reverse complement; new here are the
grouping with its event order (alignment.rs:225-272), process_one_read as a producer of records (alignment.rs:275-322), the
arrays of pp_aln_batch in file order, and the error outcome.  The layout of the seq array is tests/layout_check.py's business.

Also here: a restatement of how the tokenizer stages a wave's lines through LDS (tok_stage_for, the `staged` predicate of
stage_wave_lines) and of its window split's block count, so that a case can state -- and the CPU pin can check -- which
staging instance it takes, which lines are parsed out of LDS and which straight from memory, and how many blocks the window
split runs with."""
import numpy as np

from oracle import pyref

QUIT, ARG, PANIC = 1, 4, 101
OPS = "MIDNSHP=X"
TOK_STAGE = {"S": 16 * 1024 - 64, "M": 26 * 1024 - 64, "L": 40 * 1024 - 64}   # pp_devtext.h
NL_BLOCK = 65536            # bytes per workgroup of the newline kernels, 64 per thread
WIN_LDS_MAX = 8192          # windows the LDS multisplit holds; beyond: the global-atomic kernels
WINDOW = 2048
SEQ_ALIGN = 32
MAX_RUN = 0x0FFFFFFF        # a packed run holds 28 bits of length


# ---- the tokenizer's staging and block counts, restated ---------------------------------------------------------------------

def line_spans(text):
    """(starts, ends) of the lines as the newline index gives them: end = the position of the line's "\\n", or the size of the
    text for a last line without one."""
    a = np.frombuffer(text, np.uint8)
    ends = np.flatnonzero(a == 10).astype(np.int64)
    if len(a) and a[-1] != 10:
        ends = np.append(ends, len(a))
    starts = np.concatenate([[0], ends[:-1] + 1]).astype(np.int64) if len(ends) else np.zeros(0, np.int64)
    return starts, ends


def tok_stage_for(text_bytes, n_lines):
    need = (text_bytes // n_lines + 1) * 64 * 115 // 100 if n_lines else 0
    return "S" if need <= TOK_STAGE["S"] else ("M" if need <= TOK_STAGE["M"] else "L")


def staging(text):
    """(instance, staged): the staging instance the file takes and, per line, whether it is parsed out of LDS: a wave is 64
    consecutive lines, its stretch starts at a0 = (start of its first line) & ~15, and a line is staged when
    end - a0 + 8 <= TOK_STAGE + 16."""
    # Nothing on the GPU can observe `staged`: that a case straddles the boundary rests on this restatement alone.  It follows
    # pp_devtext.h -- tok_stage_for (:121-124), and in stage_wave_lines l0 / s0 / a0 (:130-133) and the predicate (:154) -- and,
    # for split_blocks below, per_block / nb in ingest_text of pp_tokenize.hip.  Whoever changes those changes these.
    starts, ends = line_spans(text)
    n = len(ends)
    inst = tok_stage_for(len(text), n)
    if n == 0:
        return inst, np.zeros(0, bool)
    a0 = starts[(np.arange(n) // 64) * 64] & ~15
    return inst, ends - a0 + 8 <= TOK_STAGE[inst] + 16


def split_blocks(n_aln):
    """workgroups of the LDS window split (k_tok_win_hist): 16384 records each, more when there would be over 1024 of them"""
    per_block = max(16384, ((n_aln + 1023) // 1024 + 1023) & ~1023)
    return (n_aln + per_block - 1) // per_block


def n_windows(contigs):
    return max(1, (sum(len(s) for _, s in contigs) + WINDOW - 1) // WINDOW)


# ---- the model ------------------------------------------------------------------------------------------------------------------

class ModelError(Exception):
    """code: QUIT / PANIC / ARG; kind: which check; msg: the reference's message for a quit, None for a panic (its text is the
    Rust runtime's)."""

    def __init__(self, code, kind, msg=None):
        super().__init__(f"[{code}] {kind}: {msg}")
        self.code, self.kind, self.msg = code, kind, msg


def packed_runs(cigar):
    """get_expanded_cigar (alignment.rs:325-346) kept as runs of length << 4 | op: a zero-length run expands to nothing, a run
    above 28 bits is cut into pieces"""
    runs = []
    if cigar == "*":
        return runs
    for m in pyref.CIGAR_TOKEN.finditer(cigar):
        tok = m.group(0)
        num, op = int(tok[:-1]), OPS.index(tok[-1])
        while num > 0:
            piece = min(num, MAX_RUN)
            runs.append((piece << 4) | op)
            num -= piece
    return runs


def _lines(text):
    out = text.split(b"\n")
    if out and out[-1] == b"":
        out.pop()
    return [(b[:-1] if b.endswith(b"\r") else b).decode("ascii") for b in out]


def _parse(line, path, ln):
    """Alignment::new of one line; a panic of the reference is a ModelError(PANIC) named after the column"""
    try:
        a = pyref.Alignment.new(line)
    except pyref.Panic:
        parts = line.split("\t")
        for kind, bits, s in (("flag", 32, parts[1]), ("pos", 64, parts[3])):
            try:
                pyref._parse_uint(s, bits)
            except pyref.Panic:
                raise ModelError(PANIC, kind)
        if any(p.startswith("NM:i:") and not _is_uint(p[5:], 32) for p in parts[11:]):
            raise ModelError(PANIC, "nm")
        raise ModelError(PANIC, "cigar_overflow")
    except pyref.Quit as e:
        raise ModelError(QUIT, "invalid_cigar", str(e))
    if isinstance(a, str):
        raise ModelError(QUIT, a.replace(" ", "_"), f'{a} in "{path}" (line {ln})')
    return a


def _is_uint(s, bits):
    try:
        pyref._parse_uint(s, bits)
        return True
    except pyref.Panic:
        return False


def model(contigs, texts, paths=None, max_errors=10, careful=False, verdicts=None):
    """contigs: [(name, sequence)]; texts: the SAM files as bytes; verdicts: per file None or the filter's verdict byte of every
    aligned record (0 = as if "ZP:Z:fail" were on its line).  Returns {"recs": the arrays of pp_aln_batch with the SEQ bytes in
    file order, "counts": [(alignments, used, reads)] per file, "name_lens": the QNAME lengths of the aligned records}, or
    raises ModelError for the first event of the reference's streaming order: a line that fails to parse, or a read group
    that fails when it is flushed -- which is when the first record of the next group HAS BEEN parsed, or at the end of
    the file."""
    index = {name: i for i, (name, _) in enumerate(contigs)}
    out, counts, name_lens = [], [], set()

    def flush(group):  # process_one_read, alignment.rs:275-322
        if not group:
            raise ModelError(PANIC, "empty_group")
        if careful and len(group) > 1:
            return
        src = next((a for a, _, _ in group if a.read_seq != "*"), None)
        if src is None:
            raise ModelError(QUIT, "no_sequence", f"no alignments for read {group[0][0].read_name} contain sequence")
        good = []
        for a, runs, passed in group:
            if not runs:
                raise ModelError(PANIC, "empty_cigar")
            if (runs[0] & 15) in (0, 7) and (runs[-1] & 15) in (0, 7) and a.mismatches <= max_errors and a.pass_qc and passed:
                good.append((a, runs))
        for a, runs in good:
            if a.ref_name not in index:
                raise ModelError(QUIT, "not_in_assembly", f"query name {a.ref_name} in SAM but not in assembly")
            if a.ref_start > 0xFFFFFFFE:   # (the batch holds 32-bit starts; the reference would index past the contig)
                raise ModelError(PANIC, "start_past_u32")
        for a, runs in good:
            seq = a.read_seq
            if seq == "*":
                seq = src.read_seq if a.forward() == src.forward() else pyref.reverse_complement(src.read_seq)
            out.append((index[a.ref_name], a.ref_start, len(good), seq.encode("ascii"), runs))

    for f, text in enumerate(texts):
        path = paths[f] if paths else f"file{f}"
        v = None if verdicts is None else verdicts[f]
        n_before, n_aligned, n_groups = len(out), 0, 0
        current, group = "", []
        for ln, line in enumerate(_lines(text), 1):
            if not line or line[0] == "@":
                continue
            a = _parse(line, path, ln)
            if not a.is_aligned():
                continue
            passed = True if v is None or n_aligned >= len(v) else bool(v[n_aligned])
            n_aligned += 1
            name_lens.add(len(a.read_name))
            item = (a, packed_runs(a.cigar), passed)
            if current == "" or current == a.read_name:
                group.append(item)
            else:
                flush(group)
                n_groups += 1
                group = [item]
            current = a.read_name
        if group:
            flush(group)
            n_groups += 1
        # verdicts that are there must be one per aligned record -- none at all for a file with records included; said once the
        # text has been found free of defects (the verdicts that are there were applied, a record beyond them passes)
        if v is not None and len(v) != n_aligned:
            raise ModelError(ARG, "verdict_count")
        if not group:
            flush(group)    # process_one_read on the empty group after the loop (alignment.rs:268)
        counts.append((n_aligned, len(out) - n_before, n_groups))

    n = len(out)
    seq_len = np.array([len(o[3]) for o in out], np.uint32)
    room = (seq_len.astype(np.int64) + SEQ_ALIGN - 1) & ~(SEQ_ALIGN - 1)
    seq_off = (np.cumsum(room) - room).astype(np.uint64)
    n_cig = np.array([len(o[4]) for o in out], np.uint32)
    seq = np.zeros(int(room.sum()), np.uint8)
    for o, at in zip(out, seq_off.tolist()):
        seq[at:at + len(o[3])] = np.frombuffer(o[3], np.uint8)
    recs = {"contig": np.array([o[0] for o in out], np.uint32), "ref_start": np.array([o[1] for o in out], np.uint32),
            "k": np.array([o[2] for o in out], np.uint32), "seq_off": seq_off, "seq_len": seq_len,
            "cig_off": (np.cumsum(n_cig, dtype=np.int64) - n_cig).astype(np.uint64), "n_cig": n_cig, "seq": seq,
            "cigar": np.array([r for o in out for r in o[4]], np.uint32)}
    assert len(recs["contig"]) == n
    return {"recs": recs, "counts": counts, "name_lens": name_lens}


def write_case(c, d):
    """the case's assembly and SAM files under directory d (a pathlib.Path): (fasta path, [sam paths])"""
    fa = d / "assembly.fasta"
    fa.write_bytes(fasta_text(c.contigs))
    sams = []
    for i, t in enumerate(c.texts):
        p = d / f"reads{i}.sam"
        p.write_bytes(t)
        sams.append(str(p))
    return str(fa), sams


def seqs(fasta_bytes):
    """the sequence lines of a FASTA, joined: what a polish of records gives back"""
    return "".join(l for l in fasta_bytes.decode().split("\n") if l and not l.startswith(">")).encode()


def fasta_text(contigs, width=70):
    out = []
    for name, s in contigs:
        out.append(f">{name}\n")
        out.extend(s[i:i + width] + "\n" for i in range(0, len(s), width))
    return "".join(out).encode("ascii")


# ---- the generator ----------------------------------------------------------------------------------------------------------

class Gen:
    """Seeded source of an assembly and of SAM lines on it.  mate = True gives the same lines on the other strand (FLAG ^ 16): the
    second file of a pair for the filter; a line built with length= keeps its length, so the two texts have the same shape."""

    def __init__(self, seed, contig_lens=(6000,), mate=False):
        self.rng = np.random.default_rng(seed)
        acgt = np.frombuffer(b"ACGT", np.uint8)
        self.contigs = [(f"ctg{i}", acgt[self.rng.integers(0, 4, n)].tobytes().decode()) for i, n in enumerate(contig_lens)]
        self.mate, self.serial = mate, 0

    def line(self, name=None, contig=0, pos=None, n=24, flag=0, cigar=None, seq=None, qual=None, nm=0, tags=(), length=None,
             rname=None):
        """one alignment line without its line end.  pos: 0-based start (random by default); seq: the contig's bases there by
        default; qual: "I"s by default, "*" for none; nm: None for no NM tag; length: the exact length of the line, made up by
        a pad tag XX:Z:aaa... that sits BEFORE the NM tag (a parser that loses the end of the line loses the NM tag)."""
        cname, cseq = self.contigs[contig]
        if pos is None:
            pos = int(self.rng.integers(0, max(1, len(cseq) - n)))
        if seq is None:
            at = pos if 0 <= pos < len(cseq) else 0
            seq = cseq[at:at + n]
        if cigar is None:
            cigar = f"{len(seq)}M"
        if name is None:
            name = f"r{self.serial}"
            self.serial += 1
        if self.mate and isinstance(flag, int):
            flag ^= 16
        if qual is None:
            qual = "*" if seq == "*" else "I" * len(seq)
        cols = [name, str(flag), rname or cname, str(pos + 1), "60", cigar, "*", "0", "0", seq, qual]
        tail = list(tags) + ([f"NM:i:{nm}"] if nm is not None else [])
        if length is None:
            return "\t".join(cols + tail)
        need = length - len("\t".join(cols + tail))
        assert need >= 6, ("no room for the pad tag", length, need)
        s = "\t".join(cols + ["XX:Z:" + "a" * (need - 6)] + tail)
        assert len(s) == length
        return s


class Text:
    """a SAM text under construction that knows its size and line count"""

    def __init__(self, eol="\n"):
        self.parts, self.size, self.n, self.eol = [], 0, 0, eol

    def add(self, line):
        self.parts.append(line + self.eol)
        self.size += len(line) + len(self.eol)
        self.n += 1

    def raw(self, s):   # bytes as they are (runs of empty lines, a header without line end)
        self.parts.append(s)
        self.size += len(s)
        self.n += s.count("\n")

    def bytes(self, final=True):
        t = "".join(self.parts)
        if not final:
            assert t.endswith(self.eol)
            t = t[:-len(self.eol)]
        return t.encode("ascii")


class Case:
    def __init__(self, family, contigs, texts, shape=None, max_errors=10, careful=False, verdicts=None, error=None,
                 filter_pair=False, about_mirrors=False, valid_job=True):
        self.family, self.contigs, self.texts = family, contigs, texts
        self.shape = shape or {}          # what the case declares about itself: checked by the CPU pin
        self.max_errors, self.careful, self.verdicts = max_errors, careful, verdicts
        self.error = error                # (code, kind) the case is meant to end with, or None
        self.filter_pair = filter_pair    # the filter's front end takes the text and its mate
        self.about_mirrors = about_mirrors  # also run with PP_SEQ4=0 / PP_WO=0
        self.valid_job = valid_job and error is None   # the oracle polishes it: its bytes are the model's records polished

    def model(self, paths=None):
        return model(self.contigs, self.texts, paths, self.max_errors, self.careful, self.verdicts)


SHORT = 110                                  # a short alignment line of the staging cases
FILLER = {"S": 110, "M": 300, "L": 600}      # line lengths that pull a file's average into an instance (64 of them fit its stage)


def _critical_wave(g, T, inst, k, delta, mod16, tail=True):
    """At a multiple of 64 lines: one wave of short lines and a header that leaves the next wave's start at mod16 modulo 16,
    then the wave under test: its k-th line (from 1) ends with end - a0 + 8 == TOK_STAGE + delta, so with delta = 16 it is the
    last staged line and with 17 the first unstaged one; 64 - k short lines follow (tail)."""
    assert T.n % 64 == 0 and delta in (16, 17)
    eol = len(T.eol)
    for _ in range(63):
        T.add(g.line(length=SHORT))
    T.add("@CO\t" + "x" * (4 + (mod16 - (T.size + 8 + eol)) % 16))
    assert T.size % 16 == mod16
    s0 = T.size
    end_k = (s0 & ~15) + TOK_STAGE[inst] + delta - 8
    body = end_k - s0 - (k - 1) * eol - (eol - 1)    # the lengths of the k lines together
    base, extra = divmod(body, k)
    for i in range(k):
        T.add(g.line(length=base + (1 if i < extra else 0)))
    assert T.size - 1 == end_k
    for _ in range(64 - k if tail else 0):
        T.add(g.line(length=SHORT))
    return (64 - k if tail else 0) + (1 if delta == 17 else 0)   # unstaged lines of the wave


def _steered(seed, inst, fill, eol="\n", final=True, mate=False, contig_lens=(6000,)):
    """The text of fill(g, T) behind as many waves of filler lines as it takes for the file's average line length to pick
    `inst`; returns (g, text, what fill returned)."""
    for n_fill in range(0, 400):
        g, T = Gen(seed, contig_lens, mate), Text(eol)
        for _ in range(64 * n_fill):
            T.add(g.line(length=FILLER[inst]))
        ret = fill(g, T)
        text = T.bytes(final)
        if tok_stage_for(len(text), len(line_spans(text)[1])) == inst:
            return g, text, ret
    raise AssertionError(("no number of filler waves picks", inst))


def _stage_case(seed, inst, specs, eol="\n", final=True, tail=True):
    def build(mate=False):
        def fill(g, T):
            return sum(_critical_wave(g, T, inst, k, d, m, tail=tail or i + 1 < len(specs)) for i, (k, d, m) in enumerate(specs))
        g, text, unstaged = _steered(seed, inst, fill, eol, final, mate)
        return Case("stage_" + inst, g.contigs, [text], {"stage": [inst], "unstaged": [unstaged]}, filter_pair=True)
    return build


def _stage_long_line(seed, inst):
    def build(mate=False):
        def fill(g, T):
            for _ in range(64 + 20):
                T.add(g.line(length=SHORT))
            T.add(g.line(length=TOK_STAGE[inst] + 100))
            for _ in range(43 + 64):
                T.add(g.line(length=SHORT))
        g, text, _ = _steered(seed, inst, fill, mate=mate)
        return Case("stage_" + inst, g.contigs, [text], {"stage": [inst], "unstaged": [44]}, filter_pair=True)
    return build


def _stage_last_waves(seed, inst):
    def build(mate=False):
        g, texts = Gen(seed, mate=mate), []
        for last, final in ((1, False), (63, True), (64, True)):
            T = Text()
            for _ in range(128 + last):
                T.add(g.line(length=FILLER[inst] + (5 if inst != "S" else 0)))
            texts.append(T.bytes(final))
        return Case("stage_" + inst, g.contigs, texts, {"stage": [inst] * 3, "unstaged": [0, 0, 0]}, filter_pair=True)
    return build


def _only_line(mate=False):
    g = Gen(41, mate=mate)
    line = g.line(length=TOK_STAGE["L"] + 4000)
    return Case("stage_L", g.contigs, [(line + "\n").encode(), line.encode()], {"stage": ["L", "L"], "unstaged": [1, 1]}, filter_pair=True)


def _no_final_newline(seed, inst):
    def build(mate=False):
        texts, contigs = [], None
        for delta in (16, 17):
            g, text, unstaged = _steered(seed, inst, lambda g, T: _critical_wave(g, T, inst, 10, delta, 5, tail=False), final=False,
                                         mate=mate)
            assert unstaged == delta - 16
            texts.append(text)
            contigs = g.contigs
        return Case("stage_" + inst, contigs, texts, {"stage": [inst, inst], "unstaged": [0, 1]}, filter_pair=True)
    return build


def _skewed_short_average(mate=False):
    g, T = Gen(51, mate=mate), Text()
    for _ in range(30_000):
        T.add("@CO")
    for _ in range(256):
        T.add(g.line(length=600))
    return Case("skewed_average", g.contigs, [T.bytes()], {"stage": ["S"], "unstaged_min": [100]}, filter_pair=True)


def _skewed_long_average(mate=False):
    g, T = Gen(52, mate=mate), Text()
    for i in range(200):
        T.add(g.line(length=60_000 if i in (3, 130) else SHORT))
    # (the lines behind a 60,000-byte line in its wave lie beyond any stage)
    return Case("skewed_average", g.contigs, [T.bytes()], {"stage": ["L"], "unstaged": [(64 - 3) + (192 - 130)]}, filter_pair=True)


def _block_edge_size(k, d, final):
    def build(mate=False):
        g, T = Gen(60 + 3 * k + d, mate=mate), Text()
        size = NL_BLOCK * k + d
        eol = 1 if final else 0
        while size - eol - T.size > 700:
            T.add(g.line(length=200))
        T.add(g.line(length=size - eol - T.size))      # ... and the last line ends in its NM tag
        text = T.bytes(final)
        assert len(text) == size and text.rstrip(b"\n").endswith(b"NM:i:0")
        return Case("block_edges", g.contigs, [text], {"size": [size]}, filter_pair=True)
    return build


def _block_edge_newlines(mate=False):
    """newlines on bytes 63 and 64 (the edge of a thread's 64 bytes), 65,535 and 65,536 (of a workgroup's), and a run of twelve
    empty lines across byte 131,072"""
    g, T = Gen(70, mate=mate), Text()
    T.add("@CO\t" + "y" * 59)
    T.add("")
    assert T.size == 65
    for edge, empties in ((NL_BLOCK, 1), (2 * NL_BLOCK, 12)):
        while edge - 1 - T.size > 700:
            T.add(g.line(length=200))
        first = edge - (empties // 2 if empties > 1 else 0)     # where the first of the newlines goes
        T.add(g.line(length=first - 1 - T.size))
        assert T.size == first
        T.raw("\n" * empties)
    for _ in range(10):
        T.add(g.line(length=200))
    text = T.bytes()
    assert text[63:65] == b"\n\n" and text[NL_BLOCK - 1:NL_BLOCK + 1] == b"\n\n" and text[2 * NL_BLOCK - 7:2 * NL_BLOCK + 6] == b"\n" * 13
    return Case("block_edges", g.contigs, [text], {}, filter_pair=True)


def _block_edge_newlines_no_empty_lines(mate=False):
    """newlines on byte 63 (the last of a thread's 64 bytes), 65,535 (the last of a workgroup's) and 131,072 (the first of the
    next one's), no empty line anywhere: a text the filter takes as well"""
    g, T = Gen(71, mate=mate), Text()
    T.add("@CO\t" + "y" * 59)
    for nl_at in (NL_BLOCK - 1, 2 * NL_BLOCK):
        while nl_at - T.size > 700:
            T.add(g.line(length=200))
        T.add(g.line(length=nl_at - T.size))
        assert T.size == nl_at + 1
    for _ in range(10):
        T.add(g.line(length=200))
    text = T.bytes()
    assert text[63] == 10 and text[NL_BLOCK - 1] == 10 and text[2 * NL_BLOCK] == 10 and b"\n\n" not in text
    return Case("block_edges", g.contigs, [text], {}, filter_pair=True)


def _names(mate=False):
    """QNAMEs of 1..18 bytes: neighbours that differ in one byte only (every position: each is a read of its own), equal names
    (a group of two), equal prefixes of different lengths, an empty QNAME in the middle of a group (it pulls the next record
    in, alignment.rs:255), and one read of 3,000 alignments behind 77 others, so that its group crosses the 256-thread edges
    of k_tok_group_start wherever they are."""
    g, T = Gen(80, (3000,), mate), Text()
    alpha = "ABCDEFGHIJKLMNOPQR"
    for n in range(1, 19):
        base = alpha[:n]
        for p in range(n):
            T.add(g.line(name=base))
            T.add(g.line(name=base[:p] + "z" + base[p + 1:]))      # differs in byte p only
        T.add(g.line(name=base))
        T.add(g.line(name=base, flag=256))                         # equal: one read, k = 2
        T.add(g.line(name=base + "x"))                             # the same bytes and one more
        T.add(g.line(name=base[:-1]))                              # ... and one fewer (n = 1: the empty QNAME joins, and pulls
        T.add(g.line(name="q" * n))                                #     the next record in)
    T.add(g.line(name="abcdefghi"))
    T.add(g.line(name=""))
    T.add(g.line(name="abcdefghi", flag=256))
    for i in range(77):
        T.add(g.line(name=f"pre{i}"))
    for i in range(3000):
        T.add(g.line(name="big_group_of_3000", flag=0 if i == 0 else 256))
    T.add(g.line(name="big_group_of_300"))
    return Case("names", g.contigs, [T.bytes()], {"name_lens": set(range(0, 20)), "max_k": 3000})


READ_LENS = (1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 255, 256, 257, 3000)
IUPAC_SRC = "acgtRYSWKMBVDHNryswkmbvdhn.-?xZ@[`{ACGT"     # lower case, IUPAC, bytes the complement turns into N


def _seq_bytes(careful):
    def build(mate=False):
        g, T = Gen(90, (9000, 700), mate), Text()
        for n in READ_LENS:
            for flag in (0, 16):
                T.add(g.line(n=n, flag=flag))
                s = g.contigs[0][1][100:100 + n]
                T.add(g.line(pos=100, seq=s.lower(), flag=flag))                       # lower case in every byte lane
                mixed = "".join(c.lower() if (i * 7 + n) % 3 == 0 else c for i, c in enumerate(s))
                T.add(g.line(pos=100, seq=mixed, flag=flag))
                odd = "".join("`{@[az"[(i + n) % 6] if i % 5 == 2 else c for i, c in enumerate(s))   # the neighbours of a..z stay
                T.add(g.line(pos=100, seq=odd, flag=flag, nm=2))
        # "*" records: the group's sequence from its 1st, 2nd and last line, on the same and on the other strand
        src = (IUPAC_SRC * 4)[:131]
        for where in ("first", "second", "last"):
            for src_flag in (0, 16):
                name = f"star_{where}_{src_flag}"
                stars = [g.line(name=name, pos=40 + 7 * i, seq="*", cigar="131M", flag=256 | (16 if i % 2 else 0)) for i in range(4)]
                s = g.line(name=name, pos=300, seq=src, flag=src_flag, nm=9)
                at = {"first": 0, "second": 1, "last": 4}[where]
                for ln in stars[:at] + [s] + stars[at:]:
                    T.add(ln)
        T.add(g.line(name="star_short", pos=5, seq="a", flag=16))
        T.add(g.line(name="star_short", pos=9, seq="*", cigar="1M", flag=256))
        return Case("seq_bytes", g.contigs, [T.bytes()], {"read_lens": set(READ_LENS) | (set() if careful else {131})}, careful=careful, about_mirrors=True)
    return build


def _win_one_window(mate=False):
    g, T = Gen(100, (1500,), mate), Text()
    for _ in range(300):
        T.add(g.line(n=40))
    return Case("windows", g.contigs, [T.bytes()], {"n_win": 1, "nb": [1]}, about_mirrors=True)


def _win_edge(n_win):
    """an assembly of exactly n_win windows, the last one partial, two contigs; a few thousand sparse reads, and reads placed in
    windows 0, 8,191, 8,192 (where there is one) and the last, partial one -- the very last possible start included"""
    def build(mate=False):
        total = (n_win - 1) * WINDOW + 500
        g, T = Gen(110 + n_win % 7, (5 * WINDOW + 100, total - 5 * WINDOW - 100), mate), Text()
        c1 = 5 * WINDOW + 100

        def at(gpos, n=30):    # a read that starts at position gpos of the assembly
            c = 0 if gpos < c1 else 1
            T.add(g.line(contig=c, pos=gpos - (c1 if c else 0), n=n, qual="*"))
        for i in range(2500):
            at(int(g.rng.integers(0, total - 30)))
            if i % 250 == 0:
                for w in (0, 8191, 8192, n_win - 1):
                    if w < n_win:
                        at(w * WINDOW)
                        at(min(w * WINDOW + WINDOW - 1, total - 1), n=1)
        return Case("windows", g.contigs, [T.bytes()], {"n_win": n_win, "nb": [1]}, about_mirrors=True)
    return build


def _win_two_blocks(mate=False):
    g, T = Gen(120, (40_000,), mate), Text()
    for _ in range(20_000):
        T.add(g.line(n=8, qual="*"))
    return Case("windows", g.contigs, [T.bytes()], {"nb": [2], "n_win": 20})


def _win_all_in_one(mate=False):
    g, T = Gen(121, (30_000,), mate), Text()
    for _ in range(17_000):
        T.add(g.line(n=8, qual="*", pos=3 * WINDOW + int(g.rng.integers(0, WINDOW))))
    return Case("windows", g.contigs, [T.bytes()], {"nb": [2], "n_win": 15})


def _win_alternating(mate=False):
    """good and not-good records in turn (too many mismatches, ZP:Z:fail, a clipped end), some of them in groups"""
    g, T = Gen(122, (50_000,), mate), Text()
    for i in range(6000):
        bad = i % 2 == 1
        how = (i // 2) % 3
        T.add(g.line(name=f"r{i // 3}", n=12, qual="*", flag=0 if i % 3 == 0 else 256, nm=11 if bad and how == 0 else 0,
                     tags=("ZP:Z:fail",) if bad and how == 1 else (), cigar="2S10M" if bad and how == 2 else None))
    return Case("windows", g.contigs, [T.bytes()], {"nb": [1], "n_win": 25}, about_mirrors=True)


def many_blocks(n, mate=False):
    """n aligned records of 8 bases without QUAL: above 64 x 16,384 of them the column scan of the window split (k_tok_win_cols)
    takes a second step.  Every 9th read has a second alignment, every 13th record too many mismatches."""
    g = Gen(130, (60_000,), mate)
    ctg = g.contigs[0][1]
    pos = g.rng.integers(0, len(ctg) - 8, n).tolist()
    lines = []
    for i, p in enumerate(pos):
        lines.append(f"m{i - 1 if i % 9 == 8 else i}\t{256 if i % 9 == 8 else 0}\tctg0\t{p + 1}\t60\t8M\t*\t0\t0\t{ctg[p:p + 8]}\t*\tNM:i:{11 if i % 13 == 0 else 0}\n")
    text = "".join(lines).encode()
    return Case("many_blocks", g.contigs, [text], {"nb": [split_blocks(n)], "n_win": 30})


def _file_of(g, inst, n_lines, good=True):
    T = Text()
    for _ in range(n_lines):
        T.add(g.line(length=FILLER[inst] + 8, nm=0 if good else 11))
    return T.bytes()


def _several(order, verdict_seed=None, count_off=0, none_for_last=False):
    """a batch of files that take the staging instances of `order` in turn; "0" is a file whose aligned records are all beyond
    max_errors (none good: it adds no run to the mirror's run table)"""
    def build(mate=False):
        g = Gen(140 + len(order), (8000, 3000), mate)
        texts = [_file_of(g, c if c != "0" else "S", 150 + 37 * i, good=c != "0") for i, c in enumerate(order)]
        shape = {"stage": [c if c != "0" else "S" for c in order]}
        verdicts = None
        if verdict_seed is not None:
            rng = np.random.default_rng(verdict_seed)
            verdicts = [(rng.random(150 + 37 * i) < 0.6).astype(np.uint8) for i in range(len(order))]
            last = len(verdicts[-1]) + count_off          # a wrong count for the last file: too few, too many, none at all
            verdicts[-1] = np.resize(verdicts[-1], 0 if none_for_last else last)
        wrong = count_off or none_for_last
        return Case("several_files", g.contigs, texts, shape, verdicts=verdicts, error=(ARG, "verdict_count") if wrong else None,
                    about_mirrors=True)
    return build


def _filtered_events(kind):
    """verdicts and defects in one file: a defect of the text comes first, a wrong verdict count is said behind it; the verdicts
    that are there count -- one of them takes the only good record of a read on an unknown contig out, and the read no longer
    fails; verdicts for a file without aligned records are a wrong count, said before the empty group is"""
    def build(mate=False):
        g, T = Gen(170, (5000,), mate), Text()
        if kind == "empty":
            T.add("@HD\tVN:1.6")
            T.add(g.line(flag=4, nm=None))
            return Case("several_files", g.contigs, [T.bytes()], {}, verdicts=[np.ones(3, np.uint8)], error=(ARG, "verdict_count"))
        for _ in range(50):
            T.add(g.line())
        if kind != "line":
            T.add(g.line(rname="elsewhere"))              # aligned record 50: a read that fails when it is flushed, if good
        for _ in range(50):
            T.add(g.line())
        if kind == "line":
            T.add("x\t0\tctg0\t1\t60\t24M")
            T.add(g.line())
        if kind == "spared":
            v = np.ones(101, np.uint8)
            v[50] = 0
            return Case("several_files", g.contigs, [T.bytes()], {}, verdicts=[v])
        v = np.ones(40, np.uint8)                         # too few, and none for record 50: it stays good
        return Case("several_files", g.contigs, [T.bytes()], {}, verdicts=[v],
                    error=(QUIT, "not_in_assembly" if kind == "group" else "too_few_columns"))
    return build


def _details(mate=False):
    """oddities of single lines: header and empty lines anywhere, an unaligned line with a bad CIGAR-free body, zero-length runs,
    a run beyond 28 bits, "+" in numbers, NM twice, ZP:Z:fail in any case, a trailing tab, POS 0, QUAL "*" """
    g, T = Gen(150, (5000, 400), mate), Text()
    T.add("@HD\tVN:1.6")
    T.add("")
    T.add(g.line(n=30))
    T.add(g.line(n=30, cigar="0S30M0I", nm=1))
    T.add("@CO\tin the middle")
    T.add(g.line(name="un", flag=4, cigar="*", nm=None, rname="*"))
    T.add(g.line(n=30, cigar="10=1X19=", nm=1, contig=1))
    T.add(g.line(n=30, flag="+16", tags=("NM:i:99",), nm=3))       # the last NM tag counts
    T.add(g.line(n=30, tags=("zp:Z:FaIl",)))
    T.add(g.line(n=30, tags=("ZP:Z:failed", "AS:i:7")) + "\t")
    T.add("")
    T.add(g.line(n=30, pos=-1))                                     # POS 0: start 0
    T.add(g.line(n=30, cigar="5S20M5H", nm=0))
    T.add(g.line(n=30, cigar="30M", nm=10))
    T.add(g.line(n=30, cigar="30M", nm=11))
    return Case("details", g.contigs, [T.bytes(final=False)], {})


def _long_run(mate=False):
    """a run beyond 28 bits is cut in two (0x0FFFFFFF and 2); the record is in the batch, the job it makes is not a valid one"""
    g, T = Gen(151, (5000,), mate), Text()
    T.add(g.line(n=30))
    T.add(g.line(n=12, cigar="268435457M", qual="*"))
    T.add(g.line(n=30))
    return Case("details", g.contigs, [T.bytes()], {}, valid_job=False)


def _error(kind):
    """files that end in an error: the first event in the reference's streaming order decides"""
    def build(mate=False):
        g, T = Gen(160, (5000,), mate), Text()
        for _ in range(200):
            T.add(g.line())
        bad_group = [g.line(name="nos", seq="*", cigar="24M"), g.line(name="nos", seq="*", cigar="24M", flag=256)]
        few = "x\t0\tctg0\t1\t60\t24M"
        code = QUIT
        if kind == "too_few_columns":
            T.add(few)
        elif kind == "missing_NM_tag":
            T.add(g.line(nm=None))
        elif kind == "invalid_cigar":
            T.add(g.line(cigar="24Q"))
        elif kind == "no_sequence":                      # flushed by the next read's first line: before the parse error behind it
            for ln in bad_group + [g.line(), few]:
                T.add(ln)
        elif kind == "too_few_columns_before_flush":     # the line that would flush the failing group does not parse: it wins
            for ln in bad_group + [few]:
                T.add(ln)
        elif kind == "no_sequence_at_eof":
            for ln in bad_group:
                T.add(ln)
        elif kind == "not_in_assembly":
            T.add(g.line(rname="elsewhere"))
        elif kind == "not_in_assembly_not_good":         # ... which nobody looks at when the record is not good: no error
            T.add(g.line(rname="elsewhere", nm=11))
            code = None
        elif kind in ("flag", "pos", "nm", "cigar_overflow", "empty_cigar", "start_past_u32"):
            code = PANIC
            T.add({"flag": g.line(flag="0x10"), "pos": g.line().replace("\tctg0\t", "\tctg0\t-", 1),
                   "nm": g.line(nm="7x"), "cigar_overflow": g.line(cigar="4294967296M"), "empty_cigar": g.line(cigar="0M"),
                   "start_past_u32": g.line(pos=5_000_000_000)}[kind])
        elif kind == "empty_group":
            code = PANIC
            T = Text()
            T.add("@HD\tVN:1.6")
            T.add(g.line(flag=4, nm=None))
            return Case("errors", g.contigs, [T.bytes()], {}, error=(PANIC, kind))
        for _ in range(100):
            T.add(g.line())
        k = "too_few_columns" if kind == "too_few_columns_before_flush" else kind.replace("_at_eof", "")
        return Case("errors", g.contigs, [T.bytes()], {}, error=(code, k) if code else None)
    return build


def _table():
    t = {}
    for i, inst in enumerate("SML"):
        t[f"stage_{inst}_fits_exactly"] = _stage_case(200 + i, inst, [(64, 16, 9)])
        t[f"stage_{inst}_first_unstaged"] = _stage_case(210 + i, inst, [(k, d, (5 * j + 3) % 16) for j, (k, d) in enumerate(
            (k, d) for k in (1, 32, 63, 64) for d in (16, 17))])
        t[f"stage_{inst}_offsets"] = _stage_case(220 + i, inst, [(32, 17 if r % 2 else 16, r) for r in range(16)])
        t[f"stage_{inst}_long_line"] = _stage_long_line(230 + i, inst)
        t[f"stage_{inst}_last_waves"] = _stage_last_waves(240 + i, inst)
        t[f"stage_{inst}_crlf"] = _stage_case(250 + i, inst, [(32, 16, 2), (32, 17, 11), (64, 16, 0), (1, 17, 15)], eol="\r\n")
        t[f"stage_{inst}_no_final_newline"] = _no_final_newline(260 + i, inst)
    t["stage_L_only_line"] = _only_line
    t["skewed_short_average_long_lines"] = _skewed_short_average
    t["skewed_long_average_short_lines"] = _skewed_long_average
    for k in (1, 2):
        for d in (-1, 0, 1):
            t[f"block_edge_size_{k}x65536{d:+d}"] = _block_edge_size(k, d, final=False)
    t["block_edge_newline_is_the_last_byte"] = _block_edge_size(1, 0, final=True)
    t["block_edge_newlines"] = _block_edge_newlines
    t["block_edge_newlines_no_empty_lines"] = _block_edge_newlines_no_empty_lines
    t["names"] = _names
    t["seq_bytes"] = _seq_bytes(False)
    t["seq_bytes_careful"] = _seq_bytes(True)
    t["win_one_window"] = _win_one_window
    t["win_8192"] = _win_edge(8192)
    t["win_8193"] = _win_edge(8193)
    t["win_two_blocks"] = _win_two_blocks
    t["win_all_in_one_window"] = _win_all_in_one
    t["win_good_and_not_good_alternating"] = _win_alternating
    t["many_blocks_tenth"] = lambda mate=False: many_blocks(MANY_BLOCKS_N // 10, mate)
    for order in ("SL", "LS", "MSL", "LMSM", "0S", "S0L", "M0"):
        t[f"files_{order}"] = _several(order)
    t["files_SLM_filtered"] = _several("SLM", verdict_seed=7)
    t["files_LS_filtered_one_verdict_short"] = _several("LS", verdict_seed=8, count_off=-1)
    t["files_SL_filtered_one_verdict_too_many"] = _several("SL", verdict_seed=9, count_off=1)
    t["files_MS_filtered_no_verdicts_for_a_file_with_records"] = _several("MS", verdict_seed=10, none_for_last=True)
    t["files_S_filtered_no_verdicts"] = _several("S", verdict_seed=11, none_for_last=True)
    t["filtered_wrong_count_behind_a_failing_group"] = _filtered_events("group")
    t["filtered_wrong_count_behind_a_failing_line"] = _filtered_events("line")
    t["filtered_verdict_spares_a_failing_group"] = _filtered_events("spared")
    t["filtered_nothing_aligned_and_verdicts"] = _filtered_events("empty")
    t["details"] = _details
    t["details_run_beyond_28_bits"] = _long_run
    for kind in ("too_few_columns", "missing_NM_tag", "invalid_cigar", "no_sequence", "too_few_columns_before_flush",
                 "no_sequence_at_eof", "not_in_assembly", "not_in_assembly_not_good", "flag", "pos", "nm", "cigar_overflow",
                 "empty_cigar", "start_past_u32", "empty_group"):
        t[f"error_{kind}"] = _error(kind)
    return t


MANY_BLOCKS_N = 64 * 16384 + 5000       # the GPU case; the CPU pin runs a tenth of it against the model
CASES = _table()
FAMILIES = ("stage_S", "stage_M", "stage_L", "skewed_average", "block_edges", "names", "seq_bytes", "windows", "many_blocks",
            "several_files", "details", "errors")
# one case per family that also runs end to end (the command with either ingest, the device batch through the polish)
END_TO_END = ("stage_S_first_unstaged", "stage_M_crlf", "stage_L_offsets", "skewed_short_average_long_lines",
              "block_edge_size_1x65536+0", "names", "seq_bytes", "win_8193", "many_blocks_tenth", "files_S0L")
_built = {}


def case(name, mate=False):
    """the named case (built once: the generator is seeded)"""
    if (name, mate) not in _built:
        _built[name, mate] = CASES[name](mate) if mate else CASES[name]()
    return _built[name, mate]
