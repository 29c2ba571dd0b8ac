"""The plain model of the BGZF compressor (tests/bgzf_deflate_model.py: the definition of pp_bgzf_deflate's bytes) against zlib, gzip
and the inflate model's feature report (tests/bgzf_model.py): every input comes back, every block keeps the bound of n + 31 bytes, and
each input reaches what it was built to reach.  No GPU."""
import gzip
import zlib

import pytest

import bgzf_deflate_model as D
import bgzf_model as M

INPUTS = {
    "empty": b"", "one": b"x", "three": b"abc", "four": b"abcd", "five": b"abcde",
    "strip-1": M.bam_like(D.S - 1, 2), "strip": M.bam_like(D.S, 2), "strip+1": M.bam_like(D.S + 1, 2), "2strips+3": M.bam_like(2 * D.S + 3, 2),
    "zeros_514": bytes(514), "zeros_1000": bytes(1000), "zeros_full": bytes(M.FULL), "one_value": b"\xa7" * 5000,
    "all_values": D.all_values_equally(), "noise": M.noise(60000), "text_40": D.TEXT_40, "acgt": M.acgt(), "acgt_256": M.acgt(256),
    "bam_like": M.bam_like(), "fibonacci": D.fibonacci_counts(), "skewed": D.skewed(),
    "far_32768": D.far_repeat(32768), "far_32769": D.far_repeat(32769), "two_pieces": M.bam_like(M.FULL + 1, 3),
}


@pytest.fixture(scope="module")
def made():
    """name -> (stream, form, inflate's report) of the first piece, and the whole file"""
    out = {}
    for name, data in INPUTS.items():
        raw, form = D.deflate_piece(data[:D.PIECE])
        out[name] = (raw, form, M.inflate(raw)[1], D.deflate_file(data))
    return out


@pytest.mark.parametrize("name", list(INPUTS))
def test_every_input_comes_back_within_the_bound(made, name):
    data = INPUTS[name]
    raw, form, rep, (file, off, counts) = made[name]
    assert zlib.decompress(raw, -15) == data[:D.PIECE]
    assert M.inflate(raw)[0] == data[:D.PIECE] and rep["blocks"] == 1 and rep["types"] == [form]
    assert gzip.decompress(file) == data
    n_blk = (len(data) + D.PIECE - 1) // D.PIECE
    assert len(off) == n_blk + 1 and sum(counts) == n_blk and file[off[-1]:] == M.EOF_BLOCK
    blk_off, out_off, end, ok = M.walk(file)
    assert ok and blk_off == off and end == len(file)
    for b in range(n_blk):
        assert off[b + 1] - off[b] <= min(D.PIECE, len(data) - b * D.PIECE) + 31
        assert M.inflate_block(file, off[b]) == data[b * D.PIECE:(b + 1) * D.PIECE]


def test_each_input_reaches_what_it_was_built_for(made):
    form = {k: v[1] for k, v in made.items()}
    rep = {k: v[2] for k, v in made.items()}
    assert form["noise"] == D.STORED and form["text_40"] == D.FIXED and form["bam_like"] == D.DYNAMIC and form["one"] == D.FIXED
    assert made["empty"][3][0] == M.EOF_BLOCK, "no bytes: the EOF block alone"
    assert rep["skewed"]["repeats"] == {16, 17, 18}
    assert rep["zeros_1000"]["max_len"] == 258 and rep["zeros_1000"]["overlaps"] and D.tokens(bytes(1000))[256:] == [(258, 1), (258, 3), (228, 5)]
    # a distance of exactly 32,768 is taken, 32,769 is refused: the letters come as literals a second time
    assert rep["far_32768"]["max_dist"] == 32768 and (258, 32768) in D.tokens(INPUTS["far_32768"])
    assert rep["far_32769"]["max_dist"] <= D.S and D.tokens(INPUTS["far_32769"]).count(ord("A")) == 2
    # the two headers zlib's inflate and the device's accept as they are
    assert rep["acgt_256"]["no_dist_code"] and form["acgt_256"] == D.DYNAMIC and not any(isinstance(t, tuple) for t in D.tokens(INPUTS["acgt_256"]))
    assert D.tokens(bytes(514)) == [0] * 256 + [(258, 1)], "one match: one distance symbol, a code of one bit"
    assert form["zeros_514"] == D.DYNAMIC and rep["zeros_514"]["max_dist_code"] == 1 and not rep["zeros_514"]["no_dist_code"]
    # the repair: a tree deeper than the limit without it, exactly the limit with it
    lit, dist = D.histograms(D.tokens(INPUTS["fibonacci"]))
    assert not any(dist) and max(D.code_lengths(lit, 99)) == 17 and max(D.code_lengths(lit, 15)) == 15
    assert form["fibonacci"] == D.DYNAMIC and rep["fibonacci"]["max_lit_code"] == 15
    cl = _cl_hist(INPUTS["bam_like"])
    assert max(D.code_lengths(cl, 99)) > 7 and max(D.code_lengths(cl, 7)) == 7
    # all values equally: 8- and 9-bit codes, which the stored form beats by the header
    lit, _ = D.histograms(D.tokens(INPUTS["all_values"]))
    assert set(lit[:256]) == {64} and sorted(set(D.code_lengths(lit, 15)) - {0}) == [8, 9] and form["all_values"] == D.STORED


def _cl_hist(data):
    lit, dist = D.histograms(D.tokens(data))
    ll, dl = D.code_lengths(lit, 15), D.code_lengths(dist, 15)
    hlit, hdist = max([257] + [s + 1 for s in range(286) if ll[s]]), max([1] + [s + 1 for s in range(30) if dl[s]])
    h = [0] * 19
    for s, _ in D.header_runs(ll[:hlit] + dl[:hdist]):
        h[s] += 1
    return h


def test_code_lengths_are_complete_and_limited():
    import random
    r = random.Random(11)
    for trial in range(300):
        n = r.choice((2, 3, 19, 30, 286))
        limit = 7 if n == 19 else 15
        count = [r.choice((0, 0, 1, 1, 2, 3, r.randrange(1, 10 ** r.randrange(1, 6)))) for _ in range(n)]
        if trial % 3 == 0:      # Fibonacci-like: deeper than any limit
            a, b = 1, 1
            for s in range(n):
                if count[s]:
                    count[s] = a
                    a, b = b, a + b if b < 1 << 40 else b
        lens = D.code_lengths(count, limit)
        used = [l for l in lens if l]
        assert all((l > 0) == (c > 0) for l, c in zip(lens, count)) and max(lens, default=0) <= limit
        if len(used) > 1:
            assert sum(1 << (limit - l) for l in used) == 1 << limit, "complete"
            order = sorted((s for s in range(n) if count[s]), key=lambda s: (count[s], s))
            assert [lens[s] for s in order] == sorted((lens[s] for s in order), reverse=True), "a rarer symbol is never shorter"
        elif used:
            assert used == [1]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_smaller_than_huffman_only_on_bam_like_bytes(seed):
    data = M.bam_like(M.FULL, seed)
    mine = len(D.block(data)[0])
    sizes = {k: len(M.block(data, *a)) for k, a in (("huffman_only", (6, zlib.Z_HUFFMAN_ONLY)), ("level_1", (1,)), ("level_6", (6,)))}
    print(f"bam_like seed {seed}: {mine} bytes; zlib Z_HUFFMAN_ONLY {sizes['huffman_only']}, level 1 {sizes['level_1']} (ratio "
          f"{mine / sizes['level_1']:.3f}), level 6 {sizes['level_6']} (ratio {mine / sizes['level_6']:.3f})")
    assert mine < sizes["huffman_only"]
