"""tests/depth_model.py pinned without a GPU: hand-written bytes for both forms, the ties and near-ties of the {:.1} rounding, the mean's
rounding; on the golden pair (tests/golden/derived_e2e) the tenths of the ORACLE's per-position depths are column 4 of its --debug TSV,
the runs form expanded back to positions gives that column, the bins form at W = 1 the column with a 0 appended, and the positions of
zero tenths per contig are the positions the log counts as "a depth of zero"; the binding has the new rows."""
import os
from fractions import Fraction

import numpy as np
import pytest

import depth_model as dm
import fasta_model as fm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "derived_e2e")


def test_hand_written_bytes_for_both_forms():
    #         0    1    2     3     4    5    6    7  |  8    9    10 | (empty) | 11
    depth = [0.0, 0.0, 1.01, 1.04, 2.5, 2.5, 0.0, 12.0, 12.0, 12.0, 0.5, 3.25]
    off, names = [0, 8, 11, 11, 12], [b"one", b"two two;=<>", b"empty", b"x"]
    assert dm.bedgraph(depth, off, names) == (b"one\t0\t2\t0.0\none\t2\t4\t1.0\none\t4\t6\t2.5\none\t6\t7\t0.0\none\t7\t8\t12.0\n"
                                              b"two two;=<>\t0\t2\t12.0\ntwo two;=<>\t2\t3\t0.5\nx\t0\t1\t3.2\n")
    # bins of 3: tenths 0 0 10 | 10 25 25 | 0 120 ; 120 120 5 ; 32 -- the means 3.33.., 20, 60 ; 81.66.. ; 32 tenths
    assert dm.bedgraph(depth, off, names, 3) == (b"one\t0\t3\t0.33\none\t3\t6\t2.00\none\t6\t8\t6.00\ntwo two;=<>\t0\t3\t8.17\nx\t0\t1\t3.20\n")
    assert dm.bedgraph(depth, off, names, 1 << 24) == b"one\t0\t8\t2.38\ntwo two;=<>\t0\t3\t8.17\nx\t0\t1\t3.20\n"  # 190 / 8 = 23.75 tenths
    assert dm.bedgraph([], [0], []) == b"" and dm.bedgraph([], [0, 0], [b"c"]) == b"" and dm.bedgraph([], [0, 0], [b"c"], 5) == b""
    assert dm.summary(depth) == {"zero_positions": 3, "max_tenths": 120, "sum_tenths": 10 + 10 + 25 + 25 + 360 + 5 + 32}
    assert dm.summary([]) == {"zero_positions": 0, "max_tenths": 0, "sum_tenths": 0}
    assert dm.parse(dm.bedgraph(depth, off, names))[5] == (b"two two;=<>", 0, 2, b"12.0")
    assert dm.bedgraph([7.0] * 1_000_001, [0, 1_000_001], [b"c"]) == b"c\t0\t1000001\t7.0\n"


def test_ties_and_near_ties_of_the_tenths():
    for x, want in ((0.25, 2), (0.75, 8), (1.25, 12), (0.35, 3), (9.95, 99), (99.95, 1000), (999.95, 10000), (0.05, 1), (0.15, 1), (0.0, 0),
                    (0.04, 0), (0.06, 1), (4294967295.0, 42949672950), (4294967295.95, 42949672959), (4294967295.9999995, 42949672960)):
        assert dm.tenths(x) == want, x
        # the definition itself: 10 x rounded from the exact binary value, ties to even
        exact = Fraction(x) * 10
        lo = exact.numerator // exact.denominator
        r = exact - lo
        assert want == lo + (1 if r > Fraction(1, 2) or (r == Fraction(1, 2) and lo % 2) else 0), x
    assert Fraction(0.35) * 10 != Fraction(7, 2), "0.35 is no binary tie"
    assert dm.bedgraph([1.01, 1.04], [0, 2], ["c"]) == b"c\t0\t2\t1.0\n", "two doubles that print alike are one run"
    assert dm.bedgraph([2.0, 2.0], [0, 1, 2], ["a", "b"]) == b"a\t0\t1\t2.0\nb\t0\t1\t2.0\n", "equal values across a contig boundary are two runs"
    for bad in (-1.0, -0.0, float("nan"), 4294967296.0, float("inf")):
        with pytest.raises(AssertionError):
            dm.tenths(bad)


def test_the_means_rounding():
    assert dm.mean_hundredths(7, 1) == 70 and dm.mean_hundredths(0, 1) == 0  # n = 1: the tenths with a 0 appended
    # 2r == n: 10 S / n = q + 1/2 -- S = 1, n = 4: 2.5 -> 2 (q even); S = 3, n = 4: 7.5 -> 8 (q odd)
    assert dm.mean_hundredths(1, 4) == 2 and dm.mean_hundredths(3, 4) == 8
    assert dm.mean_hundredths(1, 3) == 3 and dm.mean_hundredths(2, 3) == 7  # 3.33.., 6.66..
    assert dm.mean_hundredths(42949672960 << 24, 1 << 24) == 429496729600
    # a last short bin: 5 positions in bins of 2
    assert dm.bedgraph([1.0, 2.0, 3.0, 4.0, 0.5], [0, 5], ["c"], 2) == b"c\t0\t2\t1.50\nc\t2\t4\t3.50\nc\t4\t5\t0.50\n"
    assert dm.bedgraph([0.1, 0.2, 0.2, 0.2], [0, 4], ["c"], 4) == b"c\t0\t4\t0.18\n"  # 70 / 4 = 17.5 -> 18 (q odd)
    assert dm.bedgraph([0.1, 0.0, 0.0, 0.0], [0, 4], ["c"], 4) == b"c\t0\t4\t0.02\n"  # 10 / 4 = 2.5 -> 2 (q even)


@pytest.fixture(scope="module")
def golden(orc):
    fa = os.path.join(GOLDEN, "case.fasta")
    res = orc.polish_files(fa, [os.path.join(GOLDEN, f"case_{i}.sam") for i in (1, 2)], debug=True, positions=True)
    names, _, off, bases = fm.parse(open(fa, "rb").read())
    return names, [int(x) for x in off], res


def test_the_tenths_of_the_oracles_depths_are_the_tsvs_column(golden):
    names, off, res = golden
    col = dm.depth_column_of_debug_tsv(res["debug"])
    depth = res["positions"]["depth"]
    assert len(col) == off[-1] == len(depth) and len(col) > 1000
    t = dm.tenths_of(depth)
    assert [b"%d.%d" % (v // 10, v % 10) for v in t.tolist()] == col
    assert len(set(col)) > 10, "the golden pair has many depths: the test cannot pass on a flat track"


def test_the_runs_form_expands_to_the_column_and_bins_of_one_append_a_zero(golden):
    names, off, res = golden
    col = dm.depth_column_of_debug_tsv(res["debug"])
    depth = res["positions"]["depth"]
    text = dm.bedgraph(depth, off, names)
    assert dm.expand(text, off, names) == col
    recs = dm.parse(text)
    assert 1 < len(recs) < len(col) and all(0 <= a < b for _, a, b, _ in recs)
    assert all(x[0] != y[0] or (x[2] == y[1] and x[3] != y[3]) for x, y in zip(recs[:-1], recs[1:])), "runs are maximal and tile their contig"
    ones = dm.parse(dm.bedgraph(depth, off, names, 1))
    assert [v for _, _, _, v in ones] == [c + b"0" for c in col] and all(b == a + 1 for _, a, b, _ in ones)
    # every bin's mean lies between its smallest and its largest member
    for W in (7, 100):
        t = dm.tenths_of(depth)
        for c, a, b, q in dm.bin_records(depth, off, W):
            s = t[off[c] + a:off[c] + b]
            assert 10 * int(s.min()) <= q <= 10 * int(s.max())


def test_zero_positions_per_contig_are_the_logs_depth_of_zero_counts(golden):
    """print_polishing_info counts the positions whose depth is 0.0 (src/polish.rs:206-227); on the golden pair no position has a depth
    that is not zero and prints as 0.0, so the summary's zero_positions, contig by contig, is that count"""
    names, off, res = golden
    depth = res["positions"]["depth"]
    total = 0
    for c in range(len(names)):
        d = depth[off[c]:off[c + 1]]
        z = dm.summary(d)["zero_positions"]
        assert z == int((d == 0.0).sum())
        total += z
    assert total == dm.summary(depth)["zero_positions"]
    assert dm.summary(depth)["sum_tenths"] == int(dm.tenths_of(depth).sum()) and dm.summary(depth)["max_tenths"] == int(dm.tenths_of(depth).max())


def test_the_binding_has_the_new_rows():
    import ctypes as C
    import inspect

    import polypolish_amd as pp
    rows = (("pp_depth_bedgraph", 9), ("pp_polish_depth", 4), ("pp_depth_out_bytes", 4), ("pp_depth_out_summary", 4), ("pp_depth_out_write", 2),
            ("pp_depth_out_kernel_ms", 2), ("pp_depth_out_free", 1), ("pp_ctx_set_depth", 4), ("pp_ctx_depth", 2))
    for name, n_args in rows:
        assert name in pp.SIGNATURES and len(pp.SIGNATURES[name][1]) == n_args, name
    order = list(pp.SIGNATURES)
    assert [n for n in order if n in dict(rows)] == [n for n, _ in rows], "in the header's order"
    assert order.index("pp_depth_bedgraph") == order.index("pp_masked_free") + 1 and order.index("pp_ctx_set_depth") == order.index("pp_ctx_set_soft_mask") + 1
    assert pp.SIGNATURES["pp_depth_bedgraph"][0] is C.c_int and pp.SIGNATURES["pp_depth_out_free"][0] is None
    assert "pp_depth_out_stage_ms_" in pp.HOOKS and "pp_depth_geometry_" in pp.HOOKS
    assert issubclass(pp.DepthTrack, pp._Owned) and pp.DepthTrack._free == "pp_depth_out_free"
    for m in ("bytes", "summary", "write", "kernel_ms", "close"):
        assert callable(getattr(pp.DepthTrack, m)), m
    assert callable(pp.Context.depth_bedgraph) and callable(pp.Context.polish_depth) and callable(pp.Context.set_depth) and callable(pp.Context.depth)
    assert callable(pp.depth_geometry)
    for fn in (pp.Context.polish_files, pp.Context.filter_polish_files, pp.polish):
        assert {"depth", "depth_bin", "depth_bgzf"} <= set(inspect.signature(fn).parameters)
