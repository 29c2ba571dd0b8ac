"""The definition of the bytes pp_fasta_text (pp_fasta_out.hip) writes and of the two indexes that follow from the same tables, in
plain Python: text(), fai(), gzi().  tests/test_fasta_text_model_cpu.py pins this file on the CPU (against the golden FASTA files,
against fasta_model's parse, by random access through the .fai rows, by zlib started at the .gzi entries); the GPU tests hold the
library against it byte for byte.

  text     for each contig in order: '>', the header, "\\n", then the body.  width == 0: the contig's bytes and one "\\n" (a contig of
           no bytes gives an empty line) -- what the polish command prints.  width == W > 0: ceil(L / W) lines of W bytes, the last one
           shorter, each ended by "\\n"; L == 0 gives no body line at all.  Bytes are copied as they are.
  fai      per contig: name \\t L \\t offset \\t linebases \\t linewidth \\n.  name = the header up to its first ASCII space or tab; offset =
           the text offset of the contig's first base; linebases = min(L, W), or L when W == 0; linewidth = linebases + 1; "0 0" for
           L == 0, with offset where the first base would lie.
  gzi      for a BGZF file whose blocks hold 65,280 uncompressed bytes each (the last one fewer): little-endian uint64 -- the number of
           pairs, then per block except the first its offset in the file and the uncompressed bytes in front of it.  No pair for the
           EOF block.  blk_off is the list of the blocks' offsets with the EOF block's offset last.
Both indexes follow the published formats (samtools faidx, bgzip -i) as this project reads them."""
import struct

PIECE = 65280  # uncompressed bytes per BGZF block (pp_bgzf_deflate)


def body(seq, width):
    seq = bytes(seq)
    if width == 0:
        return seq + b"\n"
    return b"".join(seq[i:i + width] + b"\n" for i in range(0, len(seq), width))


def text(headers, seqs, width):
    assert len(headers) == len(seqs) and width >= 0
    return b"".join(b">" + bytes(h) + b"\n" + body(s, width) for h, s in zip(headers, seqs))


def name_of(header):
    h = bytes(header)
    for i, c in enumerate(h):
        if c in (0x20, 0x09):
            return h[:i]
    return h


def fai(headers, seqs, width):
    out, at = [], 0
    for h, s in zip(headers, seqs):
        n = len(s)
        at += 2 + len(h)
        lb = n if width == 0 else min(n, width)
        out.append(b"%s\t%d\t%d\t%d\t%d\n" % (name_of(h), n, at, lb, lb + 1 if n else 0))
        at += len(body(s, width))
    return b"".join(out)


def gzi(blk_off):
    """blk_off: the offsets of the file's blocks, the EOF block's last (bgzf_deflate_model.deflate_file's second result)"""
    n_blk = len(blk_off) - 1
    pairs = [(int(blk_off[b]), b * PIECE) for b in range(1, n_blk)]
    return struct.pack("<Q", len(pairs)) + b"".join(struct.pack("<QQ", a, u) for a, u in pairs)


def parse_gzi(b):
    (n,) = struct.unpack_from("<Q", b, 0)
    assert len(b) == 8 + 16 * n
    return [struct.unpack_from("<QQ", b, 8 + 16 * i) for i in range(n)]


def parse_fai(b):
    rows = []
    for line in bytes(b).split(b"\n")[:-1]:
        f = line.split(b"\t")
        rows.append((f[0], int(f[1]), int(f[2]), int(f[3]), int(f[4])))
    return rows


def parse_headers(fasta):
    """(headers, seqs) of a one-line-per-contig or wrapped FASTA text whose lines end in "\\n" -- the inverse of text() for the tests"""
    headers, seqs = [], []
    for line in bytes(fasta).split(b"\n")[:-1]:
        if line[:1] == b">":
            headers.append(line[1:])
            seqs.append(bytearray())
        else:
            seqs[-1] += line
    return headers, [bytes(s) for s in seqs]
