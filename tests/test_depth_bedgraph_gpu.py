"""pp_depth_bedgraph (pp_k_depth.h) on a caller's depths through the C ABI, byte for byte against tests/depth_model.py, from host memory
and from device memory, in the runs form and with bins: every size around a workgroup's positions, one run with its ends at every seam,
a record at every position, contig boundaries on and next to a workgroup boundary, bins around the tile and across contigs, the ties
and digit seams of the values, starts and ends at their digit seams, seeded random arrays, a device array at every alignment a double
allows that ends where its allocation ends, the summary, and every refusal of the contract.  Needs an MI355X: `-m gpu`."""
import ctypes as C

import numpy as np
import pytest

import depth_model as dm

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
    """(positions per thread P, positions per workgroup T) as the library reports them"""
    P, T, lane, text_wg = pp.depth_geometry()
    assert 1 <= P and T % P == 0 and T // P in (64, 128, 256, 512, 1024) and lane == 16 and text_wg % lane == 0
    return P, T


def _names(n):
    return [b"contig_%d" % (i + 1) for i in range(n)]


def _first_diff(got, want):
    i = next((k for k, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    return len(got), len(want), i, got[max(0, i - 40):i + 40], want[max(0, i - 40):i + 40]


def _on_device(depth, skip=0):
    """the doubles in device memory, `skip` hostile doubles (NaN) in front of them; the allocation ends where they end"""
    import torch
    whole = np.concatenate([np.full(skip, np.nan), np.asarray(depth, np.float64)])
    t = torch.from_numpy(whole.copy()).to("cuda:0") if len(whole) else torch.zeros(1, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    assert t.data_ptr() % 16 == 0
    return t.data_ptr() + 8 * skip, t


def check(pp, ctx, depth, off, names, bins=(0,), mems=None, skip=0):
    depth = np.asarray(depth, np.float64)
    summ = dm.summary(depth)
    keep = None
    wants = []
    for W in bins:
        want = dm.bedgraph(depth, off, names, W)
        wants.append(want)
        for mem in mems or (pp.MEM_HOST, pp.MEM_DEVICE):
            if mem == pp.MEM_DEVICE and keep is None:
                ptr, keep = _on_device(depth, skip)
            d = pp.DepthTrack(ctx, names, W, depth=depth if mem == pp.MEM_HOST else ptr, contig_off=off, mem=mem)
            try:
                got = d.bytes()
                assert got == want, (W, mem, _first_diff(got, want))
                assert d.n_bytes == len(want) and d.n_records == want.count(b"\n")
                assert d.summary() == (summ if len(depth) else {"zero_positions": 0, "max_tenths": 0, "sum_tenths": 0})
            finally:
                d.close()
    del keep
    return wants[0]


# ---- sizes ---------------------------------------------------------------------------------------------------------------------------
def test_every_size_around_a_workgroups_positions(pp, ctx, geo):
    P, T = geo
    for G in (1, T - 1, T, T + 1, 2 * T, 2 * T + 1, 3 * T + 5):
        for off in ([0, G], [0, G // 2, G]):
            names = _names(len(off) - 1)
            want = check(pp, ctx, np.full(G, 17.5), off, names, bins=(0, 1000))
            assert want.count(b"\n") == sum(1 for a, b in zip(off[:-1], off[1:]) if b > a), "one value over all of it: one record per contig"
    assert check(pp, ctx, np.zeros(0), [0], [], bins=(0, 5)) == b""  # no contig at all
    assert check(pp, ctx, np.zeros(0), [0, 0, 0], [b"a", b"b"], bins=(0, 5)) == b""


# ---- run ends --------------------------------------------------------------------------------------------------------------------------
def test_one_run_with_its_ends_at_every_seam(pp, ctx, geo):
    P, T = geo
    n = 3 * T + 5
    base = np.full(n, 30.0)
    ptr_cases = []
    for a in range(T - 2, T + 3):
        for b in range(2 * T - 2, 2 * T + 3):
            d = base.copy()
            d[a:b] = 60.25
            ptr_cases.append((a, b, d))
    for a, b, d in ptr_cases:
        want = check(pp, ctx, d, [0, n], [b"c"], mems=(pp.MEM_DEVICE,))
        assert want == b"c\t0\t%d\t30.0\nc\t%d\t%d\t60.2\nc\t%d\t%d\t30.0\n" % (a, a, b, b, n)
    for a in (0, 1, P - 1, P, P + 1, T - 1, T, T + 1):  # ... and inside a thread's positions, up to the array's end
        d = base[:2 * T - 1].copy()
        d[a:] = 0.0
        check(pp, ctx, d, [0, len(d)], [b"c"], mems=(pp.MEM_DEVICE,))


def test_a_record_at_every_position(pp, ctx, geo):
    """a new value at every position over 2T + 5 positions: G records, the densest record table the text pass meets; names of 1 byte and
    of 300 bytes (a line longer than the 256 bytes a wave's lanes store side by side)"""
    P, T = geo
    n = 2 * T + 5
    d = (np.arange(n) % 7) * 0.5 + (np.arange(n) % 2) * 100.0
    off, names = [0, T + 1, n], [b"x", (b"a long name; with=<words> " * 12)[:300]]
    want = check(pp, ctx, d, off, names, bins=(0, 1))
    assert want.count(b"\n") == n


# ---- contig boundaries ---------------------------------------------------------------------------------------------------------------------
def test_a_contig_boundary_splits_a_run(pp, ctx, geo):
    P, T = geo
    for B in (T - 2, T - 1, T, T + 1, T + 2):
        d = np.full(B + 700, 4.0)  # equal values on both sides
        want = check(pp, ctx, d, [0, B, B + 700], _names(2))
        assert want == b"contig_1\t0\t%d\t4.0\ncontig_2\t0\t700\t4.0\n" % B
        d[B - 1], d[B] = 9.04, 8.96  # two doubles that print alike, one on each side
        want = check(pp, ctx, d, [0, B, B + 700], _names(2))
        assert b"contig_1\t%d\t%d\t9.0\ncontig_2\t0\t1\t9.0\n" % (B - 1, B) in want


def test_contigs_of_one_position_and_an_empty_contig(pp, ctx, geo):
    P, T = geo
    lens = [1, 1, 5, 0, 1, T - 9, 0, 0, 1, 1, T + 3, 1]
    off = np.concatenate([[0], np.cumsum(lens)])
    names = [b"n%d" % i for i in range(len(lens))]
    for d in (np.full(off[-1], 2.0), (np.arange(off[-1]) // 3 % 6) * 1.5):
        want = check(pp, ctx, d, off, names, bins=(0, 1, 4, T))
        assert b"n3\t" not in want and b"n6\t" not in want and b"n7\t" not in want and want.count(b"n0\t") == 1


# ---- bins ------------------------------------------------------------------------------------------------------------------------------
def test_bins_around_the_tile_on_three_contigs(pp, ctx, geo):
    P, T = geo
    lens = [T + 37, 1, 2 * T - 5]
    off = np.concatenate([[0], np.cumsum(lens)])
    rng = np.random.default_rng(5)
    d = np.repeat(rng.integers(0, 400, len(lens) * T).astype(np.float64) / 4.0, 5)[:off[-1]]
    bins = (1, 2, 3, T - 1, T, T + 1, 2 * T + 1, 3 * T, 1 << 24)  # (3T and 2^24: greater than every contig)
    want = check(pp, ctx, d, off, _names(3), bins=(0,) + bins, mems=(pp.MEM_DEVICE,))
    check(pp, ctx, d, off, _names(3), bins=(3, T), mems=(pp.MEM_HOST,))
    assert want.count(b"\n") > 100


def test_bins_that_end_on_a_tile_boundary_and_a_contig_boundary_inside_a_bin(pp, ctx, geo):
    P, T = geo
    rng = np.random.default_rng(6)
    d = rng.integers(0, 1000, 3 * T).astype(np.float64) / 8.0
    # bins that end exactly on a tile boundary: W divides T, one contig from 0 on
    check(pp, ctx, d, [0, 3 * T], [b"c"], bins=(T // 4, T // 2, T, P, P * 64))
    # a contig boundary in the middle of what would be a bin: the bin is cut there and the next contig's bins begin at its start
    for B in (T // 2 + 3, T - 1, T, T + 1, 2 * T - 100):
        check(pp, ctx, d, [0, B, 3 * T], _names(2), bins=(T // 2, T, 1000), mems=(pp.MEM_DEVICE,))
    # one bin over many tiles: every workgroup adds to it
    want = check(pp, ctx, np.full(3 * T, 12.3), [0, 3 * T], [b"c"], bins=(3 * T, 1 << 24))
    assert want == b"c\t0\t%d\t12.30\n" % (3 * T)


# ---- values ------------------------------------------------------------------------------------------------------------------------------
def test_ties_shares_and_digit_seams_of_the_values(pp, ctx):
    ties = [0.25, 0.75, 1.25, 0.35, 9.95, 99.95, 999.95, 0.05, 0.15, 0.04, 0.06, 1.01, 1.04, 0.0, 0.0, 5e-324, 2.2250738585072014e-308]
    shares = [n / k for k in (3, 4, 7) for n in range(0, 40)]
    seams = []
    for k in range(1, 10):
        seams += [10.0 ** k - 0.1, 10.0 ** k - 0.05, 10.0 ** k - 0.04, 10.0 ** k, 10.0 ** k + 0.04]
    top = float(1 << 32)
    seams += [top - 1.0, top - 0.1, top - 0.05, np.nextafter(top, 0.0), 4294967295.95, 1234567.85, 1234567.95]
    d = np.array(ties + shares + seams + ties[::-1])
    off = [0, len(ties), len(d)]
    want = check(pp, ctx, d, off, _names(2), bins=(0, 1, 2, 5))
    assert b"\t0.2\n" in want and b"\t0.8\n" in want and b"\t1.2\n" in want and b"\t0.3\n" in want and b"\t9.9\n" in want
    assert b"\t100.0\n" in want and b"\t1000.0\n" in want and b"\t4294967296.0\n" in want and b"\t4294967295.0\n" in want
    assert b"contig_1\t11\t13\t1.0\n" in want, "1.01 and 1.04 form one run"
    # bin sums whose hundredths cross 9.99 | 10.00, by sums and by rounding
    d = np.array([10.0] * 9 + [9.9] + [10.0] * 10 + [10.0] * 6 + [9.9] * 1 + [9.9, 10.0, 10.0, 10.0, 10.0, 10.0, 10.0])
    assert check(pp, ctx, d[:20], [0, 20], [b"c"], bins=(10,)) == b"c\t0\t10\t9.99\nc\t10\t20\t10.00\n"
    assert dm.bedgraph(d[20:], [0, 14], [b"c"], 7) == b"c\t0\t7\t9.99\nc\t7\t14\t9.99\n"  # 699 / 7 = 99.857..: 998.57 -> 999
    check(pp, ctx, d[20:], [0, 14], [b"c"], bins=(7, 14))


def test_start_and_end_at_their_digit_seams(pp, ctx):
    """a contig of 1,000,001 positions with runs that start and end at 9, 10, 99, 100, ..., 999,999 and 1,000,000 (wider numbers: the
    host check's), behind a contig that moves its global positions off the local ones; bins whose ends cross the same seams"""
    n = 1_000_001
    edges = sorted({10 ** k - 1 for k in range(1, 7)} | {10 ** k for k in range(1, 7)})
    d = np.zeros(37 + n)
    for i, (a, b) in enumerate(zip([0] + edges, edges + [n])):
        d[37 + a:37 + b] = 2.5 * (1 + i % 4)
    want = check(pp, ctx, d, [0, 37, 37 + n], [b"front", b"long"], bins=(0, 99_999), mems=(pp.MEM_DEVICE,))
    recs = [r for r in dm.parse(want) if r[0] == b"long"]
    assert [r[1] for r in recs] == [0] + edges and [r[2] for r in recs] == edges + [n]


# ---- random ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(20))
def test_random_piecewise_constant_arrays(pp, ctx, geo, seed):
    P, T = geo
    rng = np.random.default_rng(2000 + seed)
    G = 5 * T + int(rng.integers(-40, 40))
    runs = rng.geometric(1.0 / (1 + seed % 5 * 30), size=G)  # mean run lengths 1, 31, 61, 91, 121
    levels = np.cumsum(rng.integers(-3, 4, len(runs))).clip(0) / rng.choice([1.0, 2.0, 3.0, 4.0, 7.0])  # random jumps of shares
    d = np.repeat(levels, runs)[:G]
    cuts = np.sort(rng.integers(0, G + 1, int(rng.integers(0, 6))))
    off = np.concatenate([[0], cuts, [G]])
    names = [b"r%d" % i * (1 + i % 3) for i in range(len(off) - 1)]
    bins = (0,) + tuple(int(w) for w in (rng.integers(1, 20), rng.integers(20, T), rng.integers(T, 3 * T)))
    check(pp, ctx, d, off, names, bins=bins, mems=(pp.MEM_DEVICE if seed % 2 else pp.MEM_HOST,))


# ---- alignment -----------------------------------------------------------------------------------------------------------------------------------
def test_a_device_array_at_every_alignment_a_double_allows(pp, ctx, geo):
    """the first double 0 to 3 doubles behind a multiple of 32 bytes (on and off a multiple of 16), hostile values (NaN) in front of it,
    the array's last double at every place: the allocation ends where the array ends"""
    P, T = geo
    rng = np.random.default_rng(7)
    for skip in range(4):
        for G in (T + 21 - skip, T + 22 - skip, P + 3, 2 * T):
            d = np.repeat(rng.integers(0, 60, G) / 4.0, 3)[:G]
            check(pp, ctx, d, [0, min(11, G), G], _names(2), bins=(0, 9), mems=(pp.MEM_DEVICE,), skip=skip)


# ---- the object -----------------------------------------------------------------------------------------------------------------------------------
def test_summary_write_deflate_and_times(pp, ctx, geo, tmp_path):
    import gzip
    P, T = geo
    d = (np.arange(3 * T) // 5 % 6) * 0.7
    off, names = [0, T, 3 * T], _names(2)
    want = dm.bedgraph(d, off, names)
    b = ctx.depth_bedgraph(d, off, names)
    assert isinstance(b, pp.DepthTrack) and b.summary() == dm.summary(d) and b.summary()["zero_positions"] == int((d == 0).sum())
    with pytest.raises(pp.PolypolishError) as e:
        b.kernel_ms()
    assert e.value.code == pp.ERR_ARG and "pp_ctx_set_profiling" in e.value.msg
    path = str(tmp_path / "a.bedgraph")
    b.write(path)
    assert open(path, "rb").read() == want
    z = b.deflate()
    assert gzip.decompress(z.host().tobytes()) == want
    z.close()
    b.close()
    ctx.set_profiling(True)
    try:
        for W in (0, 100):
            b = ctx.depth_bedgraph(d, off, names, bin=W)
            stages = b.stage_ms()
            assert set(stages) == {"values", "records", "lengths", "text"} and all(x >= 0 for x in stages.values())
            assert abs(b.kernel_ms() - sum(stages.values())) < 1e-3 and b.bytes() == dm.bedgraph(d, off, names, W)
            b.close()
    finally:
        ctx.set_profiling(False)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(pp, ctx, geo):
    P, T = geo
    L = pp.lib()
    d = np.full(100, 3.0)
    off = np.array([0, 60, 100], np.uint64)
    names = (C.c_char_p * 2)(b"a", b"b")
    nm = C.cast(names, C.c_void_p)
    out, bad = C.c_void_p(), C.c_uint64(77)
    dptr, keep = _on_device(d)

    def call(depth=d.ctypes.data, mem=pp.MEM_HOST, n=2, o=off, names_p=nm, W=0, out_p=C.byref(out), bad_p=C.byref(bad)):
        rc = L.pp_depth_bedgraph(ctx._h, depth, mem, n, o.ctypes.data if o is not None else None, names_p, W, out_p, bad_p)
        return rc, L.pp_last_error(ctx._h)

    for kw, words in ((dict(depth=None), b"null argument"), (dict(o=None), b"null argument"), (dict(names_p=None), b"null argument"),
                      (dict(out_p=None), b"null argument"), (dict(mem=pp.MEM_PEER), b"PP_MEM_HOST or PP_MEM_DEVICE"), (dict(mem=7), b"PP_MEM_HOST or PP_MEM_DEVICE"),
                      (dict(W=(1 << 24) + 1), b"more than 2^24"), (dict(W=0xFFFFFFFF), b"more than 2^24"),
                      (dict(depth=dptr + 4, mem=pp.MEM_DEVICE), b"not aligned to 8 bytes"), (dict(depth=dptr + 1, mem=pp.MEM_DEVICE), b"not aligned to 8 bytes"),
                      (dict(o=np.array([0, 60, 59], np.uint64)), b"decrease"), (dict(o=np.array([5, 60, 100], np.uint64)), b"contig_off[0]"),
                      (dict(o=np.array([0, 60, 1 << 32], np.uint64)), b"2^32"),
                      (dict(names_p=C.cast((C.c_char_p * 2)(b"a\tb", b"c"), C.c_void_p)), b"tab or a newline"),
                      (dict(names_p=C.cast((C.c_char_p * 2)(b"a", b"c\n"), C.c_void_p)), b"tab or a newline"),
                      (dict(names_p=C.cast((C.c_char_p * 2)(b"a", None), C.c_void_p)), b"name is NULL")):
        rc, msg = call(**kw)
        assert rc == pp.ERR_ARG and not out.value and words in msg and msg.startswith(b"pp_depth_bedgraph: "), (kw, msg)
    assert L.pp_depth_bedgraph(None, d.ctypes.data, pp.MEM_HOST, 2, off.ctypes.data, nm, 0, C.byref(out), None) == pp.ERR_ARG
    rc, msg = call(W=1 << 24)  # the widest bin is taken
    assert rc == 0 and out.value
    L.pp_depth_out_free(out)
    # a bad value inside the second workgroup: the first of two, from both kinds of memory, in both forms
    for value in (float("nan"), -1.0, -0.0, float(1 << 32), float("inf")):
        for first, second in ((T + 5, T + 6), (2 * T - 1, 2 * T), (T, 3)):
            big = np.full(2 * T + 40, 1.5)
            big[first], big[second] = value, -7.0
            for mem, W in ((pp.MEM_HOST, 0), (pp.MEM_DEVICE, 0), (pp.MEM_DEVICE, 10)):
                ptr, keep2 = _on_device(big) if mem == pp.MEM_DEVICE else (None, None)
                with pytest.raises(pp.PolypolishError) as e:
                    pp.DepthTrack(ctx, [b"c"], W, depth=big if mem == pp.MEM_HOST else ptr, contig_off=[0, len(big)], mem=mem)
                lo = min(first, second)
                assert e.value.code == pp.ERR_ARG and e.value.bad_pos == lo and "negative, not a number or 2^32" in e.value.msg and str(lo) in e.value.msg
                del keep2
    rc, msg = call(bad_p=None)  # (bad_pos may be NULL) ... and the context still makes the text
    assert rc == 0 and out.value
    L.pp_depth_out_free(out)
    del keep
    assert check(pp, ctx, d, off, [b"a", b"b"]) == b"a\t0\t60\t3.0\nb\t0\t40\t3.0\n"
