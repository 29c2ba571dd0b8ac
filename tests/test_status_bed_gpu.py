"""pp_status_bed (pp_k_bed.h) on a caller's status bytes through the C ABI, byte for byte against tests/bed_model.py, from host memory and
from device memory: every size around a workgroup's positions, one run with its ends at every seam of a thread's and a workgroup's
positions, a record at every position, contig boundaries on and next to a workgroup boundary, start and end at their digit seams, seeded
random arrays under all 63 masks, a device array at every alignment that ends where its allocation ends, and every refusal of the
contract.  Needs an MI355X: `-m gpu`."""
import ctypes as C

import numpy as np
import pytest

import bed_model as bm

pytestmark = pytest.mark.gpu

# the kernels' tile constants (polypolish_amd/csrc/pp_k_bed.h: BED_PPT, BED_TILE, BED_LANE, BED_TEXT_WG), repeated here and checked
# against the library's own report below
P, T, LANE, TEXT_WG = 8, 2048, 16, 16384


@pytest.fixture(scope="module")
def pp():
    import polypolish_amd
    return polypolish_amd


@pytest.fixture(scope="module")
def ctx(pp):
    c = pp.Context(0)
    yield c
    c.close()


def _names(n):
    return [b"contig_%d" % (i + 1) for i in range(n)]


def _first_diff(got, want):
    i = next((k for k, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    return len(got), len(want), i, got[max(0, i - 40):i + 40], want[max(0, i - 40):i + 40]


def _on_device(status, skip=0):
    """the bytes in device memory, `skip` hostile bytes in front of them; the allocation ends where they end"""
    import torch
    whole = np.concatenate([np.full(skip, 0xFF, np.uint8), np.asarray(status, np.uint8)])
    t = torch.from_numpy(whole.copy()).to("cuda:0") if len(whole) else torch.zeros(1, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert t.data_ptr() % 16 == 0
    return t.data_ptr() + skip, t


def check(pp, ctx, status, off, names, mask, mems=None, skip=0):
    status = np.asarray(status, np.uint8)
    want = bm.bed(status, off, names, mask)
    for mem in mems or (pp.MEM_HOST, pp.MEM_DEVICE):
        keep = None
        if mem == pp.MEM_DEVICE:
            ptr, keep = _on_device(status, skip)
        b = pp.StatusBed(ctx, names, mask, status=status if mem == pp.MEM_HOST else ptr, contig_off=off, mem=mem)
        try:
            got = b.bytes()
            assert got == want, (mem, _first_diff(got, want))
            assert b.n_bytes == len(want) and b.n_records == want.count(b"\n") and b.counts == bm.counts(status, off, mask)
        finally:
            b.close()
        del keep
    return want


def test_the_tile_constants_are_the_kernels(pp):
    assert pp.bed_geometry() == (P, T, LANE, TEXT_WG)


# ---- sizes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [0, 1, T - 1, T, T + 1, 2 * T + 3])
def test_every_size_around_a_workgroups_positions(pp, ctx, G):
    """all positions one status, in one contig and in two: selected gives one record per contig, unselected an empty text"""
    for off in ([0, G], [0, G // 2, G]):
        names = _names(len(off) - 1)
        st = np.full(G, bm.NONE, np.uint8)
        want = check(pp, ctx, st, off, names, 1 << bm.NONE)
        assert want.count(b"\n") == sum(1 for a, b in zip(off[:-1], off[1:]) if b > a)
        assert check(pp, ctx, st, off, names, bm.ALL & ~(1 << bm.NONE)) == b""
    assert check(pp, ctx, np.zeros(0, np.uint8), [0], [], bm.ALL) == b""  # no contig at all


# ---- run ends --------------------------------------------------------------------------------------------------------------------------
ENDS = [0, 1, P - 1, P, P + 1, T - 1, T, T + 1, 2 * T - 1]


@pytest.mark.parametrize("a", ENDS[:-1])
def test_one_run_with_its_ends_at_every_seam(pp, ctx, a):
    for b in [e for e in ENDS if e > a]:
        st = np.full(2 * T + 9, bm.KEPT, np.uint8)
        st[a:b] = bm.TOO_CLOSE
        want = check(pp, ctx, st, [0, len(st)], [b"c"], bm.UNDECIDED, mems=(pp.MEM_DEVICE,))
        assert want == b"c\t%d\t%d\ttoo_close\n" % (a, b)
    st = np.full(2 * T - 1, bm.KEPT, np.uint8)  # ... and the run that ends with the array
    st[a:] = bm.MULTIPLE
    check(pp, ctx, st, [0, len(st)], [b"c"], bm.UNDECIDED)


# ---- record density ----------------------------------------------------------------------------------------------------------------------
def test_a_record_at_every_position(pp, ctx):
    """statuses alternating at every position over 2T + 5 positions: the densest record table the text pass meets; names of 1 byte and
    of 300 bytes (a line longer than the 256 bytes a wave's lanes store side by side)"""
    n = 2 * T + 5
    st = (np.arange(n) % 6).astype(np.uint8)
    off, names = [0, T + 1, n], [b"x", (b"a long name; with=<words> " * 12)[:300]]
    for mask in (bm.ALL, bm.UNDECIDED, 0b010101):
        want = check(pp, ctx, st, off, names, mask)
        assert want.count(b"\n") == sum((mask >> int(s)) & 1 for s in st)
    check(pp, ctx, (np.arange(n) % 2 + 2).astype(np.uint8), off, names, bm.UNDECIDED)


# ---- contig boundaries ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [T - 2, T - 1, T, T + 1, T + 2])
def test_a_contig_boundary_splits_a_run(pp, ctx, B):
    st = np.full(B + 700, bm.LOW_DEPTH, np.uint8)  # the same status on both sides
    want = check(pp, ctx, st, [0, B, B + 700], _names(2), bm.UNDECIDED)
    assert want == b"contig_1\t0\t%d\tlow_depth\ncontig_2\t0\t700\tlow_depth\n" % B
    st[B - 1], st[B] = bm.NONE, bm.NONE
    want = check(pp, ctx, st, [0, B, B + 700], _names(2), bm.UNDECIDED)
    assert b"contig_1\t%d\t%d\tnone\ncontig_2\t0\t1\tnone\n" % (B - 1, B) in want


def test_contigs_of_one_position_and_an_empty_contig(pp, ctx):
    lens = [1, 1, 5, 0, 1, T - 9, 0, 0, 1, 1, T + 3, 1]
    off = np.concatenate([[0], np.cumsum(lens)])
    names = [b"n%d" % i for i in range(len(lens))]
    for st in (np.full(off[-1], bm.MULTIPLE, np.uint8), (np.arange(off[-1]) // 3 % 6).astype(np.uint8)):
        for mask in (bm.ALL, bm.UNDECIDED):
            want = check(pp, ctx, st, off, names, mask)
            assert b"n3\t" not in want and b"n6\t" not in want and b"n7\t" not in want
    assert check(pp, ctx, np.zeros(0, np.uint8), [0, 0, 0], [b"a", b"b"], bm.ALL) == b""


# ---- digit widths ------------------------------------------------------------------------------------------------------------------------------
def test_start_and_end_at_their_digit_seams(pp, ctx):
    """a contig of 1,000,001 positions with runs that start and end at 9, 10, 99, 100, ..., 999,999 and 1,000,000 (wider numbers: the
    host check's), behind a contig that moves its global positions off the local ones"""
    n = 1_000_001
    edges = sorted({10 ** k - 1 for k in range(1, 7)} | {10 ** k for k in range(1, 7)})
    st = np.zeros(37 + n, np.uint8)
    for i, (a, b) in enumerate(zip([0] + edges, edges + [n])):
        st[37 + a:37 + b] = 2 + i % 4
    want = check(pp, ctx, st, [0, 37, 37 + n], [b"front", b"long"], bm.UNDECIDED)
    recs = [r for r in bm.parse(want) if r[0] == b"long"]
    assert [r[1] for r in recs] == [0] + edges and [r[2] for r in recs] == edges + [n]


# ---- random ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(20))
def test_random_arrays_under_all_63_masks(pp, ctx, seed):
    rng = np.random.default_rng(1000 + seed)
    G = 3 * T + int(rng.integers(-40, 40))
    runs = rng.geometric(1.0 / (1 + seed % 5 * 6), size=G)  # mean run lengths 1, 7, 13, 19, 25
    st = np.repeat(rng.integers(0, 6, len(runs)).astype(np.uint8), runs)[:G]
    cuts = np.sort(rng.integers(0, G + 1, int(rng.integers(0, 6))))
    off = np.concatenate([[0], cuts, [G]])
    names = [b"r%d" % i * (1 + i % 3) for i in range(len(off) - 1)]
    ptr, keep = _on_device(st)
    for mask in range(1, 64):
        want = bm.bed(st, off, names, mask)
        b = pp.StatusBed(ctx, names, mask, status=ptr if mask % 2 else st, contig_off=off, mem=pp.MEM_DEVICE if mask % 2 else pp.MEM_HOST)
        got, counts = b.bytes(), b.counts
        b.close()
        assert got == want, (mask, _first_diff(got, want))
        assert counts == bm.counts(st, off, mask)
    del keep


# ---- alignment -----------------------------------------------------------------------------------------------------------------------------------
def test_a_device_array_at_every_alignment(pp, ctx):
    """the first status byte 0 to 15 bytes behind a multiple of 16, hostile bytes (0xFF) in front of it, the array's last byte at every
    place in its 16: the allocation ends where the array ends"""
    rng = np.random.default_rng(7)
    for skip in range(16):
        G = T + 21 - skip
        st = np.repeat(rng.integers(0, 6, G).astype(np.uint8), 3)[:G]
        check(pp, ctx, st, [0, 11, G], _names(2), bm.ALL, mems=(pp.MEM_DEVICE,), skip=skip)
        check(pp, ctx, st[:P + 3], [0, P + 3], [b"c"], bm.UNDECIDED, mems=(pp.MEM_DEVICE,), skip=skip)


# ---- the object -----------------------------------------------------------------------------------------------------------------------------------
def test_write_deflate_and_times(pp, ctx, tmp_path):
    import gzip
    st = (np.arange(3 * T) // 5 % 6).astype(np.uint8)
    off, names = [0, T, 3 * T], _names(2)
    want = bm.bed(st, off, names)
    b = pp.StatusBed(ctx, names, status=st, contig_off=off)
    with pytest.raises(pp.PolypolishError) as e:
        b.kernel_ms()
    assert e.value.code == pp.ERR_ARG and "pp_ctx_set_profiling" in e.value.msg
    path = str(tmp_path / "a.bed")
    b.write(path)
    assert open(path, "rb").read() == want
    z = b.deflate()
    assert gzip.decompress(z.host().tobytes()) == want
    z.close()
    b.close()
    ctx.set_profiling(True)
    try:
        b = pp.StatusBed(ctx, names, status=st, contig_off=off)
        stages = b.stage_ms()
        assert set(stages) == {"runs", "records", "text"} and all(x >= 0 for x in stages.values())
        assert abs(b.kernel_ms() - sum(stages.values())) < 1e-3 and b.bytes() == want
        b.close()
    finally:
        ctx.set_profiling(False)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(pp, ctx):
    L = pp.lib()
    st = np.full(100, bm.NONE, np.uint8)
    off = np.array([0, 60, 100], np.uint64)
    names = (C.c_char_p * 2)(b"a", b"b")
    nm = C.cast(names, C.c_void_p)
    out, bad = C.c_void_p(), C.c_uint64(77)

    def call(status=st.ctypes.data, mem=pp.MEM_HOST, n=2, o=off, names_p=nm, mask=bm.UNDECIDED, out_p=C.byref(out), bad_p=C.byref(bad)):
        rc = L.pp_status_bed(ctx._h, status, mem, n, o.ctypes.data if o is not None else None, names_p, mask, out_p, bad_p)
        return rc, L.pp_last_error(ctx._h)

    for kw, words in ((dict(status=None), b"null argument"), (dict(o=None), b"null argument"), (dict(names_p=None), b"null argument"),
                      (dict(out_p=None), b"null argument"), (dict(mem=pp.MEM_PEER), b"PP_MEM_HOST or PP_MEM_DEVICE"), (dict(mem=7), b"PP_MEM_HOST or PP_MEM_DEVICE"),
                      (dict(mask=0), b"mask of 0"), (dict(mask=64), b"bit above 5"), (dict(mask=0x80000001), b"bit above 5"),
                      (dict(o=np.array([0, 60, 59], np.uint64)), b"decrease"), (dict(o=np.array([5, 60, 100], np.uint64)), b"contig_off[0]"),
                      (dict(o=np.array([0, 60, 1 << 32], np.uint64)), b"2^32"),
                      (dict(names_p=C.cast((C.c_char_p * 2)(b"a\tb", b"c"), C.c_void_p)), b"tab or a newline"),
                      (dict(names_p=C.cast((C.c_char_p * 2)(b"a", b"c\n"), C.c_void_p)), b"tab or a newline"),
                      (dict(names_p=C.cast((C.c_char_p * 2)(b"a", None), C.c_void_p)), b"name is NULL")):
        rc, msg = call(**kw)
        assert rc == pp.ERR_ARG and not out.value and words in msg and msg.startswith(b"pp_status_bed: "), (kw, msg)
    assert L.pp_status_bed(None, st.ctypes.data, pp.MEM_HOST, 2, off.ctypes.data, nm, 1, C.byref(out), None) == pp.ERR_ARG
    # a status byte above 5: the first of two, from both kinds of memory, in the first workgroup and in the second
    for first, second in ((3, 50), (T + 5, T + 6), (2 * T - 1, 2 * T)):
        big = np.full(2 * T + 40, bm.KEPT, np.uint8)
        big[first], big[second] = 6, 255
        for mem in (pp.MEM_HOST, pp.MEM_DEVICE):
            ptr, keep = _on_device(big) if mem == pp.MEM_DEVICE else (None, None)
            with pytest.raises(pp.PolypolishError) as e:
                pp.StatusBed(ctx, [b"c"], bm.ALL, status=big if mem == pp.MEM_HOST else ptr, contig_off=[0, len(big)], mem=mem)
            assert e.value.code == pp.ERR_ARG and e.value.bad_pos == first and "status byte above 5" in e.value.msg and str(first) in e.value.msg
            del keep
    rc, msg = call(bad_p=None)  # (bad_pos may be NULL) ... and the context still makes the text
    assert rc == 0 and out.value
    L.pp_bed_out_free(out)
    assert check(pp, ctx, st, off, [b"a", b"b"], bm.UNDECIDED) == b"a\t0\t60\tnone\nb\t0\t40\tnone\n"
