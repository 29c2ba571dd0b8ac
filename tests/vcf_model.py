"""The definition of the bytes pp_polish_vcf (pp_k_vcf.h, pp_vcf_host.h) writes, in plain Python: the polish's edits as VCF 4.2 text.
tests/test_vcf_model_cpu.py pins this file on the CPU (hand-written bytes; apply() of the model's text on the oracle's --debug TSV gives
the oracle's FASTA); the GPU tests hold the library against it byte for byte, fed from the oracle, never from the device.

  header    "##fileformat=VCFv4.2\\n", "##source=" + version + "\\n", per contig in assembly order "##contig=<ID=name,length=L>\\n", then
            "#CHROM\\tPOS\\tID\\tREF\\tALT\\tQUAL\\tFILTER\\tINFO\\n"
  edited    position p emits e(p): its bytes in the polished output (the vote's winner without its '-', so it may be empty).  p is
            edited iff e(p) is not exactly the one byte bases[p]
  records   each maximal run [a, b) of edited positions inside ONE contig (runs never join across a contig boundary) gives one line
            name \\t POS \\t . \\t REF \\t ALT \\t . \\t . \\t . \\n  with R = bases[a..b), A = e(a) ... e(b-1), positions local and 0-based:
                A not empty                       POS a+1   REF R                 ALT A
                A empty, a > 0                    POS a     REF bases[a-1] + R    ALT bases[a-1]      (the anchor is unedited: the run is maximal)
                A empty, a == 0, b < L            POS 1     REF R + bases[b]      ALT bases[b]
                A empty, the run is the contig    POS 1     REF R                 ALT <DEL>
            in assembly order.  Bytes are written as they are: nothing is re-cased, trimmed or normalised."""

COLUMNS = b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"


def header(names, contig_off, version):
    out = [b"##fileformat=VCFv4.2\n", b"##source=" + _b(version) + b"\n"]
    for c, name in enumerate(names):
        out.append(b"##contig=<ID=%s,length=%d>\n" % (_b(name), int(contig_off[c + 1]) - int(contig_off[c])))
    out.append(COLUMNS)
    return b"".join(out)


def _b(x):
    return x.encode() if isinstance(x, str) else bytes(x)


def records(names, contig_off, bases, new_base_per_position):
    """[(contig index, POS, REF, ALT)] -- new_base_per_position[p]: the winner's bytes at global position p ('-' allowed, dropped here)"""
    bases = bytes(bases)
    e = [_b(x).replace(b"-", b"") for x in new_base_per_position]
    assert len(e) == len(bases) == int(contig_off[-1]) - int(contig_off[0]) and int(contig_off[0]) == 0
    out = []
    for c in range(len(names)):
        lo, hi = int(contig_off[c]), int(contig_off[c + 1])
        p = lo
        while p < hi:
            if e[p] == bases[p:p + 1]:
                p += 1
                continue
            a = p
            while p < hi and e[p] != bases[p:p + 1]:
                p += 1
            b = p
            R, A = bases[a:b], b"".join(e[a:b])
            if A:
                out.append((c, a - lo + 1, R, A))
            elif a > lo:
                out.append((c, a - lo, bases[a - 1:a] + R, bases[a - 1:a]))
            elif b < hi:
                out.append((c, 1, R + bases[b:b + 1], bases[b:b + 1]))
            else:
                out.append((c, 1, R, b"<DEL>"))
    return out


def vcf_from_positions(names, contig_off, bases, new_base_per_position, version):
    lines = [header(names, contig_off, version)]
    for c, pos, ref, alt in records(names, contig_off, bases, new_base_per_position):
        lines.append(b"%s\t%d\t.\t%s\t%s\t.\t.\t.\n" % (_b(names[c]), pos, ref, alt))
    return b"".join(lines)


def new_bases_of_debug_tsv(tsv):
    """the new_base column (the last one) of a --debug TSV, line by line behind its header line"""
    lines = bytes(tsv).split(b"\n")
    assert lines[0].startswith(b"name\tpos\t") and lines[-1] == b""
    return [ln.rsplit(b"\t", 1)[1] for ln in lines[1:-1]]


def from_debug_tsv(names, contig_off, bases, tsv, version):
    """the VCF of a polish whose --debug TSV (the ORACLE's) is `tsv`: new_base is the winner, '-' and all"""
    return vcf_from_positions(names, contig_off, bases, new_bases_of_debug_tsv(tsv), version)


def parse(vcf):
    """(header lines, [(name, POS, REF, ALT)]) of a text this model writes"""
    head, recs = [], []
    for ln in bytes(vcf).split(b"\n")[:-1]:
        if ln[:1] == b"#":
            head.append(ln)
            continue
        f = ln.split(b"\t")
        assert len(f) == 8 and f[2] == b"." and f[5:] == [b".", b".", b"."], ln
        recs.append((f[0], int(f[1]), f[3], f[4]))
    return head, recs


def apply(contigs, vcf):
    """contigs: [(name, bytes)] -> the polished contigs [(name, bytes)]: a plain consensus applier.  Every record replaces its REF
    (checked against the contig) by its ALT; <DEL> by nothing.  Records of a contig are in ascending order and do not overlap."""
    _, recs = parse(vcf)
    index = {_b(n): i for i, (n, _) in enumerate(contigs)}
    per = [[] for _ in contigs]
    for name, pos, ref, alt in recs:
        per[index[name]].append((pos - 1, ref, alt))
    out = []
    for (name, seq), rs in zip(contigs, per):
        seq = bytes(seq)
        parts, at = [], 0
        for p0, ref, alt in rs:
            assert p0 >= at and seq[p0:p0 + len(ref)] == ref, (name, p0, ref)
            parts.append(seq[at:p0])
            parts.append(b"" if alt == b"<DEL>" else alt)
            at = p0 + len(ref)
        parts.append(seq[at:])
        out.append((name, b"".join(parts)))
    return out
