"""Hand-built polish jobs for the VCF tests: a `spec` names, per global assembly position, the string the reads carry there (the
reference's per-position key: b"T" a substitution, b"-" a deletion, b"GT" an insertion behind the base, b"-T" a deletion with an
insertion behind it), and reads() tiles the contigs with reads that ALL carry it, so that with min_depth 1 every covered position's
vote is fixed by construction.  The homopolymer trim takes the last bases of every read: the tiles overlap by half a read, so only
a stretch's last few positions stay uncovered -- no wanted edit may lie there.  Every read comes in three copies: at a depth of 3
and more the invalid threshold is at least 1, so a base that no read carries is not "too close".  A position whose ASSEMBLY byte is
'-' emits nothing without any read (polish.rs:188): that is how a run reaches a contig's last position, covers a whole contig or a
contig of one base.  No read is laid over such a byte.

new_bases() turns the ORACLE's result on the same records (polish_records(positions=True)) into the per-position strings
vcf_model.vcf_from_positions takes."""
import numpy as np

OP_M, OP_I, OP_D = 0, 1, 2


def assembly(lens, seed, dash=()):
    """random ACGT contigs without a homopolymer longer than 3; dash: global positions whose byte is '-'"""
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    b = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(off[-1]))].copy()
    for i in range(3, len(b)):
        if b[i] == b[i - 1] == b[i - 2] == b[i - 3]:
            b[i] = b"ACGT"[(b"ACGT".index(int(b[i])) + 1 + i % 3) % 4]
    for p in dash:
        b[p] = ord("-")
    return off, b


def other(base, k=1):
    """a base that differs from `base`"""
    return bytes([b"ACGT"[(b"ACGT".index(base) + k) % 4]])


def reads(contig_off, bases, spec, read_len=100, copies=3, cover=None):
    """the records (numpy SoA, pp_aln_batch's field names) of reads that tile every stretch without a '-' assembly byte; cover: the
    global ranges [(lo, hi)] to tile instead of everything (sparse reads over a long contig), each inside one contig"""
    bases = np.asarray(bases, np.uint8)
    step = read_len // 2
    out = {k: [] for k in ("contig", "ref_start", "seq_len", "n_cig", "seq_off", "cig_off")}
    seq, cig = bytearray(), []

    def key(p):
        return spec.get(p, bytes(bases[p:p + 1]))

    def plain(p):  # a read may begin and end here: one M
        k = key(p)
        return len(k) == 1 and k != b"-"

    def tile(c, lo, p, hi):
        while p < hi:  # stretches between '-' bytes
            if bases[p] == ord("-"):
                p += 1
                continue
            q = p
            while q < hi and bases[q] != ord("-"):
                q += 1
            for s in range(p, q, step):
                a, b = s, min(s + read_len, q)
                while a < b and key(a)[0:1] == b"-":  # (a read begins with an M)
                    a += 1
                while b > a and not plain(b - 1):
                    b -= 1
                if b - a < 4:
                    continue
                ops, s_bytes = [], bytearray()
                for x in range(a, b):
                    k = key(x)
                    for op, n in ((OP_D, 1) if k[0:1] == b"-" else (OP_M, 1), (OP_I, len(k) - 1)):
                        if n == 0:
                            continue
                        if ops and ops[-1][0] == op:
                            ops[-1][1] += n
                        else:
                            ops.append([op, n])
                    s_bytes += k.replace(b"-", b"")
                for _ in range(copies):
                    out["contig"].append(c)
                    out["ref_start"].append(a - lo)
                    out["seq_len"].append(len(s_bytes))
                    out["n_cig"].append(len(ops))
                    out["seq_off"].append(len(seq))
                    out["cig_off"].append(len(cig))
                    seq.extend(s_bytes)
                    cig.extend((n << 4) | op for op, n in ops)
            p = q

    for c in range(len(contig_off) - 1):
        lo, hi = int(contig_off[c]), int(contig_off[c + 1])
        for p, end in ([(lo, hi)] if cover is None else [(a, b) for a, b in cover if lo <= a and b <= hi]):
            tile(c, lo, p, end)
    n = len(out["contig"])
    recs = {k: np.array(out[k], np.uint64 if k.endswith("_off") else np.uint32) for k in out}
    recs["k"] = np.ones(n, np.uint32)
    recs["seq"] = np.frombuffer(bytes(seq), np.uint8).copy() if seq else np.zeros(0, np.uint8)
    recs["cigar"] = np.array(cig, np.uint32)
    return recs


def new_bases(res):
    """per position the bytes the oracle emits there: its polished string cut by its per-position emit lengths"""
    cum = np.concatenate([[0], np.cumsum(res["positions"]["emit_len"].astype(np.int64))])
    pol = res["polished"]
    return [pol[int(cum[i]):int(cum[i + 1])] for i in range(len(cum) - 1)]


def expected_edits(bases, spec):
    """{position: emitted bytes} the spec and the '-' assembly bytes ask for (where they differ from the assembly byte)"""
    bases = np.asarray(bases, np.uint8)
    want = {int(p): b"" for p in np.nonzero(bases == ord("-"))[0]}
    for p, k in spec.items():
        e = k.replace(b"-", b"")
        if e != bytes(bases[p:p + 1]):
            want[p] = e
    return want


def check_oracle_made(bases, spec, nb):
    """the job is what it was built to be: the oracle edits exactly the wanted positions, to the wanted bytes"""
    bases = np.asarray(bases, np.uint8)
    got = {p: e for p, e in enumerate(nb) if e != bytes(bases[p:p + 1])}
    want = expected_edits(bases, spec)
    assert got == want, (sorted(set(got) ^ set(want))[:10], [(p, got[p], want[p]) for p in got if p in want and got[p] != want[p]][:10])
