"""pp_fasta_text (pp_fasta_out.hip) against tests/fasta_text_model.py, byte for byte, with the bases in host memory and in device memory;
its .fai and the .gzi of the compressed text against the same model.  The model is pinned on the CPU
(tests/test_fasta_text_model_cpu.py).  The shapes are built to the byte around the kernel's seams, from fasta_out_geometry(): S bytes
per store, G per workgroup; a few hundred KB at the most.  Nothing here depends on a fault.  Needs an MI355X: `-m gpu`."""
import ctypes as C
import gzip

import numpy as np
import pytest

import bgzf_deflate_model as dm
import fasta_text_model as tm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pp():
    import polypolish_amd
    return polypolish_amd


@pytest.fixture(scope="module")
def ctx(pp):
    c = pp.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def geo(pp):
    S, G = pp.fasta_out_geometry()
    assert S == 16 and G % S == 0 and G >= 4 * S
    return S, G


def bases(n, seed):
    return np.random.RandomState(seed).choice(np.frombuffer(b"ACGTNRYK", np.uint8), n).tobytes()


def header(n, tag):
    h = (b"c%d some words " % tag) + b"h" * n
    return h[:n]


def on_device(whole, skip=0):
    """a device copy of `whole` in an allocation of its length; the bases begin `skip` bytes into it"""
    import torch
    dev = torch.device("cuda:0")
    t = torch.from_numpy(np.frombuffer(bytes(whole), np.uint8).copy()).to(dev) if len(whole) else torch.zeros(1, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    assert t.data_ptr() % 16 == 0
    return t.data_ptr() + skip, t


def offsets(seqs):
    return np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)


def made(pp, ctx, headers, seqs, W, mem, front=b"", behind=b""):
    """FastaText over the contigs; front / behind: bytes that surround the bases in their memory"""
    whole = front + b"".join(seqs) + behind
    n = sum(len(s) for s in seqs)
    if mem == pp.MEM_HOST:
        return pp.FastaText(ctx, np.frombuffer(whole, np.uint8)[len(front):len(front) + n], offsets(seqs), headers, W, mem)
    ptr, keep = on_device(whole, len(front))
    t = pp.FastaText(ctx, (ptr, n), offsets(seqs), headers, W, mem)
    del keep  # (the caller's bases may go when the call has returned)
    return t


def check(pp, ctx, headers, seqs, W, mems=None, **around):
    want, want_fai = tm.text(headers, seqs, W), tm.fai(headers, seqs, W)
    for mem in mems or (pp.MEM_HOST, pp.MEM_DEVICE):
        t = made(pp, ctx, headers, seqs, W, mem, **around)
        try:
            got = t.bytes()
            assert t.n_bytes == len(want), (W, mem)
            assert got == want, (W, mem, "first difference at", next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), None))
            assert t.fai() == want_fai, (W, mem)
        finally:
            t.close()
    return want


def widths(geo):
    S, G = geo
    return [0, 1, 2, S - 1, S, S + 1, 60, 80, G - 1, G, G + 1, 2 * G + 3]


@pytest.mark.parametrize("wi", range(12))
def test_widths_contig_lengths_and_header_lengths(pp, ctx, geo, wi):
    """every width with contigs of 0, 1, kW - 1, kW, kW + 1 bases (k = 1..3) and one of 3G + 5, the headers 1, S - 2, S - 1, S, G - 1
    and G + 7 bytes long in turn"""
    S, G = geo
    W = widths(geo)[wi]
    lens = [0, 1] + [k * W + d for k in (1, 2, 3) for d in (-1, 0, 1) if k * W + d > 1] + [3 * G + 5]
    hl = [1, S - 2, S - 1, S, G - 1, G + 7]
    headers = [header(hl[i % len(hl)], i) for i in range(len(lens))]
    seqs = [bases(n, 17 * wi + i) for i, n in enumerate(lens)]
    check(pp, ctx, headers, seqs, W)


@pytest.mark.parametrize("W", [0, 1, 60])
def test_400_one_base_contigs(pp, ctx, W):
    """">a\\nA\\n" is five bytes: three whole contigs inside one store"""
    headers = [bytes([97 + i % 26]) for i in range(400)]
    seqs = [bytes([b"ACGT"[i % 4]]) for i in range(400)]
    t = check(pp, ctx, headers, seqs, W)
    assert len(t) == 2000


@pytest.mark.parametrize("W", [4, 20])
@pytest.mark.parametrize("centre", [1, 2])
def test_seam_sweep(pp, ctx, geo, W, centre):
    """a header's '>', a header's newline, a body newline and a contig's last byte at every text offset from c - S - 1 to c + S + 1, for
    c = G and 2G: the first header is padded byte by byte (it grows longer than a workgroup's stretch on the way)"""
    S, G = geo
    c = centre * G
    L0 = 2 * W + 5
    seqs = [bases(L0, 5), bases(3, 6), bases(300, 7)]
    feats = None
    seen = {k: set() for k in (">", "hdr_nl", "body_nl", "last")}
    lo, hi = c - S - 1, c + S + 1
    # the features behind the first header's newline (at text offset 1 + h): the first body newline W + 1 behind it, the contig's
    # last base and its last newline, the next contig's '>'
    spread = 2 + len(tm.body(seqs[0], W))
    for i, h in enumerate(range(lo - 1 - spread, hi)):
        headers = [b"p" * h, b"x", b"tail t"]
        want = check(pp, ctx, headers, seqs, W, mems=(pp.MEM_DEVICE if i % 2 else pp.MEM_HOST,))
        nl = 1 + h
        feats = {"hdr_nl": nl, "body_nl": nl + W + 1, "last": nl + len(tm.body(seqs[0], W)) - 1, ">": nl + len(tm.body(seqs[0], W)) + 1}
        assert want[feats[">"]:feats[">"] + 3] == b">x\n" and want[feats["body_nl"]] == 10 and want[feats["last"]] == seqs[0][-1]
        for k, at in feats.items():
            seen[k].add(at)
    for k in seen:
        assert set(range(lo, hi + 1)) <= seen[k], k


@pytest.mark.parametrize("W", [0, 60])
def test_source_alignment_and_what_surrounds_the_bases(pp, ctx, geo, W):
    """the device bases begin at every offset 0..15 of an allocation that ends exactly at the last base, 0xFF and newlines in front; and
    again with such bytes behind them inside a larger allocation: the same text"""
    S, G = geo
    seqs = [bases(G + 77, 1), bases(5, 2), bases(1000, 3)]
    headers = [b"a", b"b b", b"c"]
    want = tm.text(headers, seqs, W)
    for skip in range(16):
        front = (b"\xff\n" * 8)[:skip]
        for behind in (b"", b"\n\xff" * 40):
            got = check(pp, ctx, headers, seqs, W, mems=(pp.MEM_DEVICE,), front=front, behind=behind)
            assert got == want


def test_no_contigs_and_two_calls(pp, ctx, geo):
    S, G = geo
    for mem in (pp.MEM_HOST, pp.MEM_DEVICE):
        t = made(pp, ctx, [], [], 60, mem)
        assert (t.n_bytes, t.bytes(), t.fai()) == (0, b"", b"")
        t.close()
    seqs, headers = [bases(2 * G + 9, 4), bases(70, 5)], [b"one", b"two 2"]
    a, b = made(pp, ctx, headers, seqs, 80, pp.MEM_DEVICE), made(pp, ctx, headers, seqs, 80, pp.MEM_DEVICE)
    assert a.bytes() == b.bytes() == tm.text(headers, seqs, 80)
    a.close()
    b.close()


@pytest.mark.parametrize("W", [0, 70])
def test_the_fasta_parse_on_the_device_reads_it_back(pp, ctx, geo, W):
    """pp_fasta_records(pp_fasta_text(...)) returns the bases, names and descriptions"""
    S, G = geo
    seqs = [bases(G + 3, 8), bases(1, 9), bases(141, 10)]
    headers = [b"k1 first one", b"k2", b"k3 x"]
    t = made(pp, ctx, headers, seqs, W, pp.MEM_DEVICE)
    rec = pp.FastaRecords(ctx, t.dev(), pp.MEM_DEVICE)
    assert rec.names == [b"k1", b"k2", b"k3"] and rec.descriptions == [b"first one", b"", b"x"]
    assert rec.offsets.tolist() == offsets(seqs).tolist() and rec.host()["bases"] == b"".join(seqs)
    rec.close()
    t.close()


def test_the_contracts_refusals(pp, ctx):
    """all decided on the host, before anything is uploaded: the 2^40 case passes offsets only and a 1-byte array"""
    L = pp.lib()
    one = np.zeros(1, np.uint8)
    hdr = np.frombuffer(b"ab\ncd", np.uint8).copy()

    def call(bases_ptr, mem, off, hoff, width=0, hdr_ptr=hdr.ctypes.data, out=True):
        off = None if off is None else np.asarray(off, np.uint64)
        hoff = None if hoff is None else np.asarray(hoff, np.uint64)
        n = (len(off) if off is not None else len(hoff)) - 1
        p = C.c_void_p()
        rc = L.pp_fasta_text(ctx._h, bases_ptr, mem, n, None if off is None else off.ctypes.data, hdr_ptr,
                             None if hoff is None else hoff.ctypes.data, width, C.byref(p) if out else None)
        assert not p.value
        return rc

    b = one.ctypes.data
    assert call(b, pp.MEM_HOST, None, [0, 1]) == pp.ERR_ARG
    assert call(b, pp.MEM_HOST, [0, 1], None) == pp.ERR_ARG
    assert call(b, pp.MEM_HOST, [0, 1], [0, 1], out=False) == pp.ERR_ARG
    assert call(b, pp.MEM_PEER, [0, 1], [0, 1]) == pp.ERR_ARG
    assert call(None, pp.MEM_HOST, [0, 1], [0, 1]) == pp.ERR_ARG            # null bases with bytes to copy
    assert call(None, pp.MEM_DEVICE, [0, 1], [0, 1]) == pp.ERR_ARG
    assert call(b, pp.MEM_HOST, [1, 0], [0, 1]) == pp.ERR_ARG               # offsets that decrease
    assert call(b, pp.MEM_HOST, [0, 1, 1], [0, 2, 1]) == pp.ERR_ARG
    assert call(b, pp.MEM_HOST, [0, 1], [0, 3]) == pp.ERR_ARG               # a header that holds "\n"
    assert call(b, pp.MEM_HOST, [0, 1], [0, 1], hdr_ptr=None) == pp.ERR_ARG  # null headers with header bytes
    assert call(b, pp.MEM_HOST, [0, 1], [0, 1], width=1 << 31) == pp.ERR_LIMIT
    assert call(b, pp.MEM_HOST, [0, 1 << 40], [0, 1]) == pp.ERR_LIMIT       # 2^40 bytes of text or more: offsets only
    assert call(b, pp.MEM_HOST, [0, (1 << 40) - 4], [0, 1]) == pp.ERR_LIMIT  # '>', the header, two newlines
    assert call(b, pp.MEM_HOST, [0, 1 << 39, 1 << 40], [0, 1, 2], width=60) == pp.ERR_LIMIT
    assert "2^40" in L.pp_last_error(ctx._h).decode()
    # ... and what is allowed: null bases with nothing to copy, a header of no bytes
    t = pp.FastaText(ctx, (0, 0), [0, 0, 0], [b"", b"e"], 0, pp.MEM_DEVICE)
    assert t.bytes() == b">\n\n>e\n\n" and t.fai() == b"\t0\t2\t0\t0\ne\t0\t6\t0\t0\n"
    t.close()


def test_deflate_and_its_gzi(pp, ctx, geo):
    """FastaText.deflate(): read back through Bgzf and through Python's gzip; its .gzi equals the model's"""
    S, G = geo
    seqs, headers = [bases(150_000, 21), bases(20_011, 22)], [b"first contig", b"second"]
    want = tm.text(headers, seqs, 60)
    t = made(pp, ctx, headers, seqs, 60, pp.MEM_DEVICE)
    z = t.deflate()
    file = z.host().tobytes()
    assert gzip.decompress(file) == want
    back = pp.Bgzf(ctx, (z.bytes_ptr, z.n_bytes), (z.blk_off_ptr, z.n_blocks), mem=pp.MEM_DEVICE)
    assert back.host().tobytes() == want
    back.close()
    model_file, model_off, _ = dm.deflate_file(want)
    assert file == model_file and z.blk_off().tolist() == model_off
    g = z.gzi()
    assert g == tm.gzi(model_off) and len(tm.parse_gzi(g)) == z.n_blocks - 1 == 2
    z.close()
    # a text of one block, and the empty text: a count of 0
    for hs, ss in (([b"s"], [b"ACGT"]), ([], [])):
        small = made(pp, ctx, hs, ss, 0, pp.MEM_HOST)
        zz = small.deflate()
        assert zz.gzi() == tm.gzi([0] * (zz.n_blocks + 1)) == bytes(8)
        zz.close()
        small.close()
    t.close()
