"""pp_filter_thresholds and pp_filter_records on the GPU (pp_filter.hip: k_thr_count / k_thr_hist / k_thr_pick; pp_filter_rec.hip:
k_rec_compact / k_rid_insert / k_rid_find and the grouping of pp_filter_group.h) against the plain models, which the CPU tests
pin to the oracle: (a) the thresholds against filter_model.thresholds on hand-built pairs at the kernels' edge shapes and over
the whole 32-bit range of an insert size, (b) the records against filter_records_model.command -- verdicts byte for byte, counts
and report -- from host and from device memory, (c) the chain filter_records -> gate_records -> polish_raw against the oracle's
filter + polish on the equivalent SAM text.  Needs an MI355X: `-m gpu`."""
import ctypes as C
import os

import numpy as np
import pytest

import filter_model as fm
import filter_records_model as frm
import gate_model as gm
import ingest_model as im
import synth

pytestmark = pytest.mark.gpu
QUIT, ARG, PANIC = 1, 4, 101


@pytest.fixture(scope="module")
def pp():
    import polypolish_amd
    return polypolish_amd


@pytest.fixture(scope="module")
def ctx(pp):
    c = pp.Context(0)
    yield c
    c.close()


# ---- (a) pp_filter_thresholds ---------------------------------------------------------------------------------------------------

ONE = [(1, 0)]                       # a run of 1M: the alignment [start, start + 1)
SELECT_DIGITS = (21, 10)             # the selection's digits are bits [21, 32), [10, 21), [0, 10) of a size (pp_filter.hip)
BOUNDARIES = sorted({3, (1 << 32) - 1, (1 << 32) - 2} | {(1 << b) + d for b in SELECT_DIGITS + (16, 31) for d in (-1, 0, 1)})


def pair(size, o):
    """a read with one alignment in each file on reference 0: insert size `size` (>= 3), orientation o"""
    near, far = (0, 0, 0, ONE), (0, size - 1, 0, ONE)
    if o == 0:
        return ([near], [(0, size - 1, 16, ONE)])
    if o == 1:
        return ([far], [(0, 0, 16, ONE)])
    return ([near], [far]) if o == 2 else ([far], [near])


ZERO = ([(0, 5, 0, [])], [(0, 5, 16, [])])      # no runs, one position: insert size 0 (get_orientation says rf)
# start near 2^32 plus long runs: the usize difference is 2^32 - 2 + 20 * (2^28 - 1) + ... > 2^32 and `as u32` cuts it
TRUNCATED = ([(0, 0, 0, ONE)], [(0, (1 << 32) - 2, 16, [(fm.MAX_RUN, 0)] * 20)])
TRUNCATED_SIZE = ((1 << 32) - 2 + 20 * fm.MAX_RUN) & 0xFFFFFFFF


def _filter_input(pp, inp, keep):
    files = []
    for f in inp["files"]:
        arrs = {k: np.ascontiguousarray(f[k]) for k in ("ref_id", "ref_start", "flags", "cig_off", "n_cig", "cigar", "read", "grp_off", "grp_idx")}
        keep.append(arrs)
        p = {k: (v.ctypes.data if v.size else None) for k, v in arrs.items()}
        files.append(pp.FilterFile(len(arrs["ref_id"]), p["ref_id"], p["ref_start"], p["flags"], p["cig_off"], p["n_cig"], p["cigar"],
                                   len(arrs["cigar"]), p["read"], arrs["grp_off"].ctypes.data, p["grp_idx"], None))
    return pp.FilterInput(inp["n_reads"], (pp.FilterFile * 2)(*files))


def thresholds_job(pp, ctx, inp, orientation, low, high, what=""):
    """begin -> thresholds -> samples -> pairs on one job, each against the model; -> what pp_filter_thresholds gave (a dict, or
    the PolypolishError of a quit the model agrees with), None where the sampling loop panics"""
    L, keep = pp.lib(), []
    fi = _filter_input(pp, inp, keep)
    assert L.pp_filter_begin(ctx._h, C.byref(fi), pp.MEM_HOST) == 0, L.pp_last_error(ctx._h)
    orient, insert, panicked = fm.samples(inp)
    what = (what, orientation, low, high)
    if panicked:
        want = None
    elif orientation != "auto" and orientation not in fm.ORIENTATIONS:     # an unknown name has no sizes (and no index for the model)
        want = fm.Quit(fm.MSG_NO_SIZES if (orient != fm.NOT_SAMPLED).any() else fm.MSG_NO_PAIRS)
    else:
        try:
            want = fm.thresholds(orient, insert, orientation, low, high)
        except fm.Quit as q:
            want = q
    try:
        got = ctx.filter_thresholds(orientation, low, high)
    except pp.PolypolishError as e:
        got = e
    if panicked:
        assert isinstance(got, pp.PolypolishError) and got.code == PANIC, (what, got)
        return None
    if isinstance(want, fm.Quit):
        assert isinstance(got, pp.PolypolishError) and got.code == QUIT and got.msg == want.msg, (what, got, want.msg)
    else:
        assert not isinstance(got, Exception), (what, got)
        counts, correct, lo, hi = want
        assert (got["counts"], got["orientation"], got["low"], got["high"]) == (counts, fm.ORIENTATIONS[correct], lo, hi), (what, got, want)
        assert got["before"] == sum(len(f["ref_id"]) for f in inp["files"]) and got["after"] == 0
    # pp_filter_samples of the same job: the arrays the thresholds were taken from
    n = inp["n_reads"]
    o, i = np.full(max(n, 1), 77, np.uint8), np.full(max(n, 1), 77777, np.uint32)
    assert L.pp_filter_samples(ctx._h, o.ctypes.data, i.ctypes.data) == 0
    assert np.array_equal(o[:n], orient) and np.array_equal(i[:n], insert), what
    if not isinstance(want, fm.Quit):
        w1, w2, v_panic = fm.verdicts(inp, lo, hi, correct)
        g = [np.full(max(len(w), 1), 7, np.uint8) for w in (w1, w2)]
        rc = L.pp_filter_pairs(ctx._h, lo, hi, correct, g[0].ctypes.data, g[1].ctypes.data)
        assert rc == (PANIC if v_panic else 0), what
        if not v_panic:
            assert np.array_equal(g[0][:len(w1)], w1) and np.array_equal(g[1][:len(w2)], w2), what
    return got


PERCENTILES = ((0.1, 99.9), (49.999, 50.001))


def _sizes(kind, n):
    if kind == "equal":
        return [500] * n
    return [BOUNDARIES[(i * 7) % len(BOUNDARIES)] for i in range(n)]


@pytest.mark.parametrize("n", (1, 63, 64, 65, 511, 512, 513, 1025))
def test_thresholds_at_the_edge_shapes(pp, ctx, n):
    for kind in ("equal", "boundaries"):
        reads = [pair(s, 0) for s in _sizes(kind, n)]
        if kind == "boundaries" and n > 1:
            reads[n // 2] = TRUNCATED
        inp = fm.hand_built(reads)
        _, insert, _ = fm.samples(inp)
        assert insert.tolist() == [TRUNCATED_SIZE if rd is TRUNCATED else s for rd, s in zip(reads, _sizes(kind, n))]
        for low, high in PERCENTILES:
            got = thresholds_job(pp, ctx, inp, "auto", low, high, (kind, n))
            if n < 1000 and (low, high) == PERCENTILES[0]:   # the ranks land on the first and on the last of the sorted sizes
                assert (got["low"], got["high"]) == (int(insert.min()), int(insert.max()))
        thresholds_job(pp, ctx, inp, "fr", 10.0, 90.0, (kind, n))


def test_thresholds_over_every_value_of_a_digit_boundary(pp, ctx):
    # every boundary value once, the truncated pair, zeros among the rf pairs: each rank of the sorted list in turn
    reads = [pair(s, 0) for s in BOUNDARIES] + [TRUNCATED] + [ZERO] * 3 + [pair(70000, 1)] * 2
    inp = fm.hand_built(reads)
    n_fr = len(BOUNDARIES) + 1
    for k in range(1, n_fr + 1):
        at = 100.0 * (k - 0.5) / n_fr               # ceil(at / 100 * n_fr) == k: one of the two ranks is k
        got = thresholds_job(pp, ctx, inp, "fr", min(49.9, at), max(50.1, at), k)
        assert sorted(BOUNDARIES + [TRUNCATED_SIZE])[k - 1] in (got["low"], got["high"])
    got = thresholds_job(pp, ctx, inp, "rf", 0.1, 99.9)          # the minority, asked for by name: sizes 0, 0, 0, 70000, 70000
    assert (got["low"], got["high"], got["counts"][1]) == (0, 70000, 5)
    assert thresholds_job(pp, ctx, inp, "rf", 49.9, 60.0)["high"] == 0
    assert thresholds_job(pp, ctx, inp, "auto", 0.1, 99.9)["orientation"] == "fr"


def test_thresholds_on_generated_pairs_of_every_orientation(pp, ctx):
    inp = fm.concat([fm.make_pairs(1, 1500, 0, 300, 900), fm.make_pairs(2, 700, 1, 1 << 15, 1 << 17), fm.make_pairs(3, 300, 2, 1 << 20, 1 << 22),
                     fm.make_pairs(4, 40, 3, 300, 400), fm.generate(5, 800, pos_range=3000, n_contigs=1)])
    for orientation in ("auto",) + fm.ORIENTATIONS:
        for low, high in PERCENTILES + ((25.0, 75.0),):
            thresholds_job(pp, ctx, inp, orientation, low, high)


def test_thresholds_quit_as_the_reference(pp, ctx):
    tie = fm.concat([fm.make_pairs(10, 200, 0, 300, 900), fm.make_pairs(11, 200, 2, 300, 900), fm.make_pairs(12, 150, 1, 300, 900)])
    for inp, orientation, msg in ((tie, "auto", fm.MSG_TIE), (fm.generate(13, 500, cnt=((2, 3), (0, 2))), "auto", fm.MSG_NO_PAIRS),
                                  (fm.generate(14, 0), "auto", fm.MSG_NO_PAIRS), (fm.make_pairs(15, 300, 0, 300, 900), "rr", fm.MSG_NO_SIZES),
                                  (fm.make_pairs(15, 300, 0, 300, 900), "sideways", fm.MSG_NO_SIZES),
                                  (fm.generate(13, 500, cnt=((2, 3), (0, 2))), "sideways", fm.MSG_NO_PAIRS)):
        got = thresholds_job(pp, ctx, inp, orientation, 0.1, 99.9)
        assert isinstance(got, pp.PolypolishError) and (got.code, got.msg) == (QUIT, msg), (orientation, msg, got)
    assert thresholds_job(pp, ctx, tie, "ff", 1.0, 99.0)["orientation"] == "ff"     # (a tie only matters to "auto")
    # the range checks come first, whatever the job holds
    for inp in (tie, fm.generate(14, 0)):
        for low, high, msg in ((0.0, 99.9, fm.MSG_LOW), (50.0, 99.9, fm.MSG_LOW), (-1.0, 200.0, fm.MSG_LOW), (0.1, 50.0, fm.MSG_HIGH), (0.1, 100.0, fm.MSG_HIGH)):
            L, keep = pp.lib(), []
            fi = _filter_input(pp, inp, keep)
            assert L.pp_filter_begin(ctx._h, C.byref(fi), pp.MEM_HOST) == 0
            with pytest.raises(pp.PolypolishError) as e:
                ctx.filter_thresholds("auto", low, high)
            assert (e.value.code, e.value.msg) == (QUIT, msg)


def test_thresholds_panic_on_a_poisoned_sample_and_need_a_job(pp):
    c = pp.Context(0)
    try:
        with pytest.raises(pp.PolypolishError) as e:
            c.filter_thresholds()
        assert e.value.code == ARG
        bad = [(1, fm.OP_UNPARSEABLE)]
        inp = fm.concat([fm.make_pairs(20, 600, 0, 300, 900), fm.hand_built([([(0, 10, 0, [(100, 0)])], [(0, 200, 16, bad)])])])
        assert thresholds_job(pp, c, inp, "auto", 0.1, 99.9) is None
        # an unparseable end nobody needs (the pair sits on two references) is no panic
        inp = fm.concat([fm.make_pairs(20, 600, 0, 300, 900), fm.hand_built([([(0, 10, 0, [(100, 0)])], [(1, 200, 16, bad)])])])
        assert thresholds_job(pp, c, inp, "auto", 0.1, 99.9)["counts"][0] == 600
    finally:
        c.close()


# ---- (b) pp_filter_records ----------------------------------------------------------------------------------------------------------

_built = {}


def case(name):
    """(raws, [(run, model result or exception)]) -- built once, shared, never written to"""
    if name not in _built:
        build, runs = frm.CASES[name]
        raws, out = build(), []
        for run in runs:
            try:
                out.append((run, frm.command(raws, *run)))
            except (fm.Quit, fm.Panic, frm.ArgError) as e:
                out.append((run, e))
        _built[name] = (raws, out)
    return _built[name]


def to_device(pp, raw):
    import torch
    dev = torch.device("cuda:0")
    signed = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64, np.dtype(np.uint8): np.uint8}
    t = {k: torch.from_numpy(np.ascontiguousarray(raw[k], dtype=dt).view(signed[np.dtype(dt)])).to(dev) for k, dt in pp.RAW_FIELDS}
    torch.cuda.synchronize()
    ptrs = {k: (v.data_ptr() or None) for k, v in t.items()}
    ptrs.update(n_rec=len(raw["flag"]), seq_bytes=len(raw["seq"]), n_cig_total=len(raw["cigar"]))
    return ptrs, t


def filter_records(pp, ctx, raws, run, source):
    if source == "host":
        return pp.filter_records(ctx, raws[0], raws[1], *run)
    (p1, k1), (p2, k2) = to_device(pp, raws[0]), to_device(pp, raws[1])
    return pp.filter_records(ctx, p1, p2, *run, mem=pp.MEM_DEVICE)


def check_records(pp, ctx, name, source):
    raws, runs = case(name)
    for run, want in runs:
        what = (name, source) + run
        if isinstance(want, Exception):
            with pytest.raises(pp.PolypolishError) as e:
                filter_records(pp, ctx, raws, run, source)
            if isinstance(want, fm.Quit):
                assert (e.value.code, e.value.msg) == (QUIT, want.msg), what
            else:
                assert e.value.code == (PANIC if isinstance(want, fm.Panic) else ARG), (what, str(e.value))
            continue
        got = filter_records(pp, ctx, raws, run, source)
        assert got["counts"] == want["counts"], (what, got["counts"], want["counts"])
        assert got["report"] == want["report"], (what, got["report"], want["report"])
        for f in range(2):
            assert got["pass"][f].dtype == np.uint8 and got["pass"][f].shape == want["pass"][f].shape, (what, f)
            bad = np.flatnonzero(got["pass"][f] != want["pass"][f])
            assert not len(bad), (what, f"file {f + 1}: verdicts of aligned records {bad[:8].tolist()} differ")


SINGLE_CASES = [k for k in frm.CASES if k not in ("large_a", "tiny", "large_b")]


@pytest.mark.parametrize("source", ("host", "device"))
@pytest.mark.parametrize("name", SINGLE_CASES)
def test_records_against_the_model(pp, ctx, name, source):
    check_records(pp, ctx, name, source)


def test_the_cases_end_as_their_names_say():
    ends = {name: [type(w).__name__ if isinstance(w, Exception) else "ok" for _, w in case(name)[1]] for name in frm.CASES}
    assert ends["file_1_empty"] == ends["file_1_only_unaligned"] == ["Quit", "Quit"] and case("file_1_empty")[1][0][1].msg == frm.MSG_FILE1
    assert ends["file_2_empty"] == ends["file_2_only_unaligned"] == ["Quit", "Quit"] and case("file_2_empty")[1][0][1].msg == fm.MSG_NO_PAIRS
    assert ends["unparseable_where_nobody_compares"] == ["ok", "ok"]
    assert ends["unparseable_in_a_sampled_pair"] == ends["unparseable_in_a_compared_mate"] == ["Panic", "Panic"]
    assert ends["auto_tie"] == ["Quit", "ok", "Quit"] and ends["percentiles_out_of_range"] == ["Quit"] * 4
    for name in ("one_read_300_here_2_there", "two_unknown_references", "a_read_far_apart_in_its_file", "ids_multiples_of_the_table_capacity"):
        assert ends[name] == ["ok", "ok"] and any((p == 0).any() for p in case(name)[1][0][1]["pass"]), name


@pytest.mark.parametrize("source", ("host", "device"))
def test_three_jobs_large_tiny_large_on_one_context(pp, source):
    c = pp.Context(0)
    try:
        for name in ("large_a", "tiny", "large_b", "tiny", "large_a"):
            check_records(pp, c, name, source)
    finally:
        c.close()


@pytest.mark.parametrize("source", ("host", "device"))
def test_a_cigar_range_outside_the_array_is_an_argument_error(pp, ctx, source):
    raws, _ = case("aligned_257")
    for f, rank in ((0, 0), (1, 200)):
        for off in (None, 1 << 62, frm.U64_MAX):
            bad = [{k: v.copy() for k, v in r.items()} for r in raws]
            r = int(frm.aligned(bad[f])[rank])
            bad[f]["cig_off"][r] = len(bad[f]["cigar"]) - int(bad[f]["n_cig"][r]) + 1 if off is None else off
            with pytest.raises(frm.ArgError):
                frm.command(bad)
            with pytest.raises(pp.PolypolishError) as e:
                filter_records(pp, ctx, bad, ("auto", 0.1, 99.9), source)
            assert e.value.code == ARG and f"record {r} of file {f + 1}" in e.value.msg, str(e.value)
    # an UNALIGNED record's range is nobody's business, and the context is fine afterwards
    ok = [{k: v.copy() for k, v in r.items()} for r in raws]
    r = int(np.flatnonzero(ok[0]["flag"] & 4)[0])
    ok[0]["cig_off"][r], ok[0]["n_cig"][r] = 1 << 62, 9
    got = filter_records(pp, ctx, ok, ("auto", 0.1, 99.9), source)
    want = case("aligned_257")[1][0][1]
    assert got["report"] == want["report"] and all(np.array_equal(a, b) for a, b in zip(got["pass"], want["pass"]))


def test_argument_errors_and_a_closed_job(pp, ctx):
    raws, _ = case("aligned_255")
    L = pp.lib()
    with pytest.raises(pp.PolypolishError) as e:
        pp.filter_records(ctx, raws[0], raws[1], mem=pp.MEM_PEER)
    assert e.value.code == ARG
    assert L.pp_filter_records(ctx._h, None, pp.MEM_HOST, b"auto", 0.1, 99.9, None, None, None, None) == ARG
    b = (pp.RawBatch * 2)()
    b[0].n_rec = 5                                          # a non-empty batch without arrays
    assert L.pp_filter_records(ctx._h, b, pp.MEM_HOST, b"auto", 0.1, 99.9, None, None, None, None) == ARG
    b[0].n_rec = 0                                          # two empty batches: file 1 has no alignments
    assert L.pp_filter_records(ctx._h, b, pp.MEM_HOST, b"auto", 0.1, 99.9, None, None, None, None) == QUIT
    assert L.pp_last_error(ctx._h).decode() == frm.MSG_FILE1
    pp.filter_records(ctx, raws[0], raws[1])
    with pytest.raises(pp.PolypolishError) as e:            # the job's arrays went away with the call
        ctx.filter_thresholds()
    assert e.value.code == ARG


def test_kernel_times_name_the_new_kernels(pp):
    c = pp.Context(0)
    try:
        c.set_profiling(True)
        raws, _ = case("one_read_300_here_2_there")
        pp.filter_records(c, raws[0], raws[1])
        kt = pp.KernelTimes()
        assert pp.lib().pp_filter_kernel_times(c._h, C.byref(kt)) == 0
        ms = kt.as_dict()["ms"]
        assert {"samples", "thr_count", "thr_select", "pairs", "rec_compact", "rec_intern", "rec_groups"} <= set(ms), ms
        assert all(0.0 < v < 1000.0 for v in ms.values()), ms
    finally:
        c.close()


# ---- (c) the chain: filter_records -> gate_records -> (prepare) -> polish, against the oracle on the SAM text ----------------------------

@pytest.fixture(scope="module")
def dataset(tmp_path_factory, orc):
    d = tmp_path_factory.mktemp("filter_records_e2e")
    ds = synth.rich_dataset(str(d), seed=23, contig_lens=(4000, 2500), coverage=30, repeat_len=400, repeat_copies=3, zp_frac=0.02)
    contigs = [(c.name, c.assembly) for c in ds["contigs"]]
    sams = [ds["sam1"], ds["sam2"]]
    texts = [open(p, "rb").read() for p in sams]
    ids, raws = {}, []
    for t in texts:                                         # one id per QNAME over BOTH files
        raw, zp = gm.raw_from_text(contigs, t)
        names = [ln.split("\t")[0] for ln in im._lines(t) if ln and ln[0] != "@"]
        assert len(names) == len(raw["flag"]) and "" not in names
        raw["read_id"] = np.array([ids.setdefault(n, (len(ids) * 0x9E3779B97F4A7C15 + 1) & frm.U64_MAX) for n in names], np.uint64)
        raws.append((raw, zp))
    outs = [os.path.join(str(d), f"filtered_{i}.sam") for i in (1, 2)]
    report = orc.filter_files(sams[0], sams[1], outs[0], outs[1])
    verdicts = [fm.failed_lines(open(p, "rb").read()) for p in outs]
    return {"fasta": ds["fasta"], "filtered": outs, "contigs": contigs, "raws": raws, "verdicts": verdicts, "report": report}


def test_chain_equals_the_oracle_s_filter_and_polish_on_the_text(pp, ctx, orc, dataset):
    want = orc.polish_files(dataset["fasta"], dataset["filtered"])
    off = np.concatenate([[0], np.cumsum([len(s) for _, s in dataset["contigs"]])]).astype(np.uint64)
    bases = np.frombuffer("".join(s for _, s in dataset["contigs"]).upper().encode(), np.uint8)
    raws = [r for r, _ in dataset["raws"]]
    got = pp.filter_records(ctx, raws[0], raws[1])
    assert got["report"] == dataset["report"]
    assert any((v == 0).any() for v in dataset["verdicts"])
    passed = []
    for f in range(2):
        # (a line that came with ZP:Z:fail keeps its tag in the oracle's output: its verdict is the caller's zp, not the filter's)
        zp = dataset["raws"][f][1]
        assert np.array_equal(got["pass"][f] & zp, dataset["verdicts"][f] & zp), f
        passed.append(got["pass"][f] & zp)
    for prepare in (False, True):
        res = ctx.polish_raw(off, bases, raws, passed=passed, prepare=prepare)
        assert res["polished"] == im.seqs(want["fasta"]), prepare
        assert tuple(map(sum, zip(*res["counts"]))) == tuple(want["counts"])
        assert ctx.took_direct_path() == prepare
