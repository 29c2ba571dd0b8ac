"""tests/fasta_text_model.py pinned without a GPU: text() rebuilds the golden FASTA files from their own contigs, fasta_model's parse
reads text() back at every small width, every .fai row finds every base by random access, and zlib started at every .gzi entry
yields the text from the entry's uncompressed offset on."""
import os
import struct
import zlib

import pytest

import bgzf_deflate_model as dm
import fasta_model as fm
import fasta_text_model as tm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "derived_e2e")


def seq(n, seed):
    return bytes(b"ACGT"[(i * 7 + seed * 3 + (i >> 3)) & 3] for i in range(n))


@pytest.mark.parametrize("name", ["polished_after_filter.fasta", "polished_raw_careful_d3.fasta"])
def test_width_0_rebuilds_the_golden_files(name):
    golden = open(os.path.join(GOLDEN, name), "rb").read()
    headers, seqs = tm.parse_headers(golden)
    assert headers and all(seqs)
    assert tm.text(headers, seqs, 0) == golden
    # ... and the wrapped text holds the same contigs
    assert tm.parse_headers(tm.text(headers, seqs, 60)) == (headers, seqs)


@pytest.mark.parametrize("W", range(0, 21))
def test_the_fasta_parse_reads_the_text_back(W):
    """contigs of 1 .. 2W + 1 bases come back from fasta_model.parse; a contig of 0 bases is written as the definition says (an empty
    line at width 0, no line at all otherwise), which the parse -- the assembly loader's rules -- names an empty sequence"""
    lens = list(range(1, 2 * W + 2))
    headers = [b"c%d len=%d" % (i, n) for i, n in enumerate(lens)]
    seqs = [seq(n, i) for i, n in enumerate(lens)]
    t = tm.text(headers, seqs, W)
    names, descs, off, bases = fm.parse(t)
    assert names == [tm.name_of(h) for h in headers] and descs == [b"len=%d" % n for n in lens]
    assert [bases[off[i]:off[i + 1]] for i in range(len(lens))] == seqs
    for n, s in zip(lens, seqs):  # the line lengths themselves
        lines = tm.body(s, W).split(b"\n")[:-1]
        assert b"".join(lines) == s
        assert all(len(x) == W for x in lines[:-1]) and (W == 0 or 1 <= len(lines[-1]) <= W) and len(lines) == (1 if W == 0 else -(-n // W))
    empty = tm.text([b"a", b"e", b"z"], [b"AC", b"", b"GT"], W)
    assert empty == (b">a\nAC\n>e\n\n>z\nGT\n" if W == 0 else b">a\n" + tm.body(b"AC", W) + b">e\n>z\n" + tm.body(b"GT", W))
    with pytest.raises(fm.FastaError) as e:
        fm.parse(empty)
    assert e.value.words == fm.EMPTY_SEQUENCE


@pytest.mark.parametrize("W", [0, 1, 2, 3, 7, 16, 60])
def test_every_fai_row_finds_every_base(W):
    lens = [0, 1, 2, W, W + 1, 2 * W, 2 * W + 1, 3 * W + 5, 0, 131]
    headers = [b"n%d" % i + (b"", b" a description", b"\ttabbed", b"  two")[i % 4] for i in range(len(lens))]
    seqs = [seq(n, i + 11) for i, n in enumerate(lens)]
    t = tm.text(headers, seqs, W)
    rows = tm.parse_fai(tm.fai(headers, seqs, W))
    assert len(rows) == len(lens)
    for (name, L, offset, lb, lw), h, s in zip(rows, headers, seqs):
        assert name == b"n%d" % headers.index(h) and L == len(s)
        assert t[offset - 1:offset] == b"\n" and t[offset - 2 - len(h):offset - 1] == b">" + h
        if L == 0:
            assert (lb, lw) == (0, 0)
            continue
        assert lb == (L if W == 0 else min(L, W)) and lw == lb + 1
        for p in range(L):
            assert t[offset + p // lb * lw + p % lb] == s[p], (W, name, p)


def test_gzi_entries_start_zlib_inside_the_file():
    import numpy as np
    headers = [b"first contig", b"second"]
    seqs = [np.random.RandomState(3).choice(np.frombuffer(b"ACGT", np.uint8), n).tobytes() for n in (150_000, 20_000)]
    t = tm.text(headers, seqs, 60)
    file, blk_off, _ = dm.deflate_file(t)
    n_blk = len(blk_off) - 1
    assert n_blk == -(-len(t) // tm.PIECE) == 3
    g = tm.gzi(blk_off)
    # by hand: a count of 2, no entry for the first block (0, 0), none for the EOF block
    assert g[:8] == struct.pack("<Q", 2) and len(g) == 8 + 2 * 16
    pairs = tm.parse_gzi(g)
    assert pairs == [(blk_off[1], 65280), (blk_off[2], 130560)]
    assert all(p[0] != 0 for p in pairs) and blk_off[3] not in [p[0] for p in pairs] and file[blk_off[3]:] == dm.M.EOF_BLOCK
    for at, u in pairs:
        d = zlib.decompressobj(31)
        out = d.decompress(file[at:])
        while d.eof and d.unused_data:  # the members behind it
            rest = d.unused_data
            d = zlib.decompressobj(31)
            out += d.decompress(rest)
        assert out == t[u:], (at, u)
    # a file of one block, and the empty file: a count of 0
    assert tm.gzi(dm.deflate_file(b"ACGT\n")[1]) == struct.pack("<Q", 0)
    assert tm.gzi(dm.deflate_file(b"")[1]) == struct.pack("<Q", 0)
