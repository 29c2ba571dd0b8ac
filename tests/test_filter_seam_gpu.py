"""Seam A on the GPU (pp_filter_begin / pp_filter_samples / pp_filter_pairs: k_filter_reads and k_filter_listed) against the
plain model of tests/filter_model.py, which tests/test_filter_model_cpu.py pins to the oracle on the same configurations:
the orientation and insert size of EVERY read, the verdict of every alignment of both files and the return codes, at the
kernels' edge shapes (64 lanes, 256 threads, two reads a lane, 512 reads and list slots a workgroup), in four input forms
(CIGAR runs or precomputed ends, host or device memory), job after job on one context, and the `filter` command around the
seam from the same inputs as text (both loaders).  Needs an MI355X."""
import ctypes as C
import os

import numpy as np
import pytest

import filter_model as fm
import synth

pytestmark = pytest.mark.gpu

FORMS = (("runs", "host"), ("ends", "host"), ("runs", "device"), ("ends", "device"))
PANIC = 101


@pytest.fixture(scope="module")
def pp():
    import polypolish_amd
    return polypolish_amd


@pytest.fixture(scope="module")
def ctx(pp):
    c = pp.Context(0)
    yield c
    c.close()


# ---- handing an input over ----------------------------------------------------------------------------------------------

def _filter_input(pp, inp, ends, mem, keep):
    """pp_filter_input of a model input: ends = False -> CIGAR runs, True -> precomputed ref_end and no CIGAR array (what
    the device loader hands over); mem = "host" -> numpy arrays, "device" -> torch tensors on the context's GPU.  `keep`
    holds whatever the pointers point into."""
    if mem == "device":
        import torch
        dev = torch.device("cuda:0")

    def ptr(a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        if mem == "host":
            keep.append(a)
            return a.ctypes.data
        t = torch.from_numpy(a.view(np.int32 if a.dtype.itemsize == 4 else np.int64).copy()).to(dev)
        keep.append(t)
        return t.data_ptr() or None
    files = []
    for f in inp["files"]:
        n = len(f["ref_id"])
        has_runs = not ends
        files.append(pp.FilterFile(n, ptr(f["ref_id"]), ptr(f["ref_start"]), ptr(f["flags"]),
                                   ptr(f["cig_off"]) if has_runs else None, ptr(f["n_cig"]) if has_runs else None,
                                   ptr(f["cigar"]) if has_runs else None, len(f["cigar"]) if has_runs else 0,
                                   ptr(f["read"]), ptr(f["grp_off"]), ptr(f["grp_idx"]),
                                   ptr(fm.ends_array(f)) if ends else None))
    if mem == "device":
        torch.cuda.synchronize()
    return pp.FilterInput(inp["n_reads"], (pp.FilterFile * 2)(*files))


class Expected:
    """What the model says about one input: samples, and the verdicts under each of the thresholds."""

    def __init__(self, inp, thresholds):
        self.inp = inp
        self.thresholds = list(thresholds(inp) if callable(thresholds) else thresholds)
        self.orient, self.insert, self.samples_panic = fm.samples(inp)
        self.verdicts = [fm.verdicts(inp, *t) for t in self.thresholds]


def _groups_of(inp, r):
    out = []
    for f in inp["files"]:
        idx = f["grp_idx"][f["grp_off"][r]:f["grp_off"][r + 1]]
        ends = fm.ends_of(f) if len(idx) else []
        out.append([(int(a), int(f["ref_id"][a]), int(f["ref_start"][a]), ends[a], int(f["flags"][a])) for a in idx])
    return out


def _describe(inp, reads):
    return "\n".join(f"  read {r} (slot {r % 512} of workgroup {r // 512}): file 1 {g[0]}  file 2 {g[1]}   [(aln, ref, start, end, flags)]"
                     for r in reads for g in (_groups_of(inp, r),))


def _begin(ctx, pp, inp, form, keep):
    L = pp.lib()
    fi = _filter_input(pp, inp, form[0] == "ends", form[1], keep)
    keep.append(fi)
    rc = L.pp_filter_begin(ctx._h, C.byref(fi), pp.MEM_HOST if form[1] == "host" else pp.MEM_DEVICE)
    assert rc == 0, (rc, L.pp_last_error(ctx._h))


def _check_samples(ctx, pp, exp, what):
    L = pp.lib()
    n = exp.inp["n_reads"]
    orient, insert = np.full(max(n, 1), 77, np.uint8), np.full(max(n, 1), 77777, np.uint32)
    rc = L.pp_filter_samples(ctx._h, orient.ctypes.data, insert.ctypes.data)
    if exp.samples_panic:
        assert rc == PANIC, (what, "pp_filter_samples returned", rc, "the model says the sampling loop panics")
        return False
    assert rc == 0, (what, "pp_filter_samples", rc, L.pp_last_error(ctx._h))
    bad = np.flatnonzero((orient[:n] != exp.orient) | (insert[:n] != exp.insert))
    assert not len(bad), (f"{what}: samples of {len(bad)} reads differ; first: "
                          f"{[(int(r), int(orient[r]), int(insert[r]), int(exp.orient[r]), int(exp.insert[r])) for r in bad[:6]]} "
                          f"[(read, orient, insert, model's orient, model's insert)]\n" + _describe(exp.inp, bad[:6].tolist()))
    return True


def _check_pairs(ctx, pp, exp, k, what):
    L = pp.lib()
    low, high, correct = exp.thresholds[k]
    w1, w2, v_panic = exp.verdicts[k]
    got = np.full(max(len(w1), 1), 7, np.uint8), np.full(max(len(w2), 1), 7, np.uint8)
    rc = L.pp_filter_pairs(ctx._h, low, high, correct, got[0].ctypes.data, got[1].ctypes.data)
    what = f"{what} thresholds ({low}, {high}, {fm.ORIENTATIONS[correct]})"
    if exp.samples_panic or v_panic:    # (the pass over the reads runs the sampling loop whether its result is asked for or not)
        assert rc == PANIC, (what, "pp_filter_pairs returned", rc, "the model says the reference panics")
        return False
    assert rc == 0, (what, "pp_filter_pairs", rc, L.pp_last_error(ctx._h))
    for f, want in enumerate((w1, w2)):
        bad = np.flatnonzero(got[f][:len(want)] != want)
        reads = exp.inp["files"][f]["read"][bad[:6]].tolist()
        assert not len(bad), (f"{what}: {len(bad)} verdicts of file {f + 1} differ; first alignments {bad[:6].tolist()} "
                              f"(got {got[f][bad[:6]].tolist()}, model {want[bad[:6]].tolist()})\n" + _describe(exp.inp, reads))
    return True


def run_job(ctx, pp, exp, form, order, what):
    """One job in one input form.  order: "samples_pairs" (all thresholds after one begin: a later pp_filter_pairs must not
    inherit verdicts), "pairs_only" (no pp_filter_samples), "samples_twice", "begin_each" (a begin per thresholds)."""
    keep = []
    what = f"{what} [{form[0]}, {form[1]} memory, {order}]"
    n_thr = len(exp.thresholds)
    if order == "begin_each":
        for k in range(n_thr):
            _begin(ctx, pp, exp.inp, form, keep)
            _check_samples(ctx, pp, exp, what) and _check_pairs(ctx, pp, exp, k, what)
        return
    # a call that returns PP_ERR_PANIC ends its job (the reference's process has ended there): nothing is asked of it afterwards
    _begin(ctx, pp, exp.inp, form, keep)
    calls = [lambda: _check_samples(ctx, pp, exp, what)] if order != "pairs_only" else []
    if order == "samples_twice":
        calls.append(lambda: _check_samples(ctx, pp, exp, what + " second pp_filter_samples"))
    calls += [lambda k=k: _check_pairs(ctx, pp, exp, k, what) for k in range(n_thr)]
    if order == "pairs_only":           # ... and the samples afterwards are still the samples
        calls.append(lambda: _check_samples(ctx, pp, exp, what + " pp_filter_samples after pp_filter_pairs"))
    calls += [lambda k=k: _check_pairs(ctx, pp, exp, k, what + " again") for k in reversed(range(n_thr))]
    for call in calls:
        if not call():
            return


ORDERS = ("samples_pairs", "pairs_only", "samples_twice", "begin_each")


@pytest.mark.parametrize("name", list(fm.SEAM_CASES))
def test_seam_equals_the_model_in_all_four_input_forms(ctx, pp, name):
    """Every configuration of filter_model.SEAM_CASES (its seed and knobs are in that table under this name): samples of every
    read, verdicts of every alignment, return codes; runs or precomputed ends, host or device memory; every form also in another
    order of the calls."""
    build, thr = fm.SEAM_CASES[name]
    exp = Expected(build(), thr)
    big = exp.inp["n_reads"] > 100_000
    for i, form in enumerate(FORMS):
        for j, order in enumerate(ORDERS):
            if big and j != i:      # (the large job: each form once, each order once)
                continue
            run_job(ctx, pp, exp, form, order, f"case {name} <{fm.knobs(name)}>")


# ---- job after job on one context ---------------------------------------------------------------------------------------

SEQUENCE_POOL = ("reads_1025", "reads_1", "listed_none_1300", "listed_all_1300", "listed_all_1024", "listed_last_1300",
                 "unparseable_in_a_sampled_pair", "unparseable_single_mate_of_several", "unparseable_anywhere", "file1_empty",
                 "file2_empty", "both_empty", "reads_0", "several_vs_none", "group_40_vs_40", "ends_past_2_32", "reads_513",
                 "listed_second_half_700", "pairs_on_other_references", "equal_positions", "unparseable_where_nobody_looks")


def _expected_pool(names):
    return {n: Expected(fm.SEAM_CASES[n][0](), fm.SEAM_CASES[n][1]) for n in names}


def _polish_job(ctx, orc, seed):
    contig_off, bases, recs = synth.fast_records(seed=seed, contig_lens=(6_000, 1_500), coverage=30, read_len=120,
                                                 indel_read_frac=0.05, k_choices=(1, 2), k_probs=(0.9, 0.1))
    got = ctx.polish_records(contig_off, bases, recs)
    want = orc.polish_records(contig_off, bases, recs)
    assert got["polished"] == want["polished"] and np.array_equal(got["offsets"], want["offsets"]), f"polish job, seed {seed}"


def _abandon(ctx, pp, exp, form):
    keep = []
    _begin(ctx, pp, exp.inp, form, keep)    # ... and no pp_filter_samples / pp_filter_pairs
    return keep


def test_filter_jobs_one_after_another_on_one_context(ctx, pp, orc):
    """An ordered list of transitions, every job checked in full: many reads, few, many (grow-only buffers, blk_cnt, the list);
    listed, none listed, listed (filter_n_listed, the any_listed word); PP_ERR_PANIC then a clean job (the poisoned word); a
    pp_filter_begin abandoned before pp_filter_pairs; precomputed ends, runs, precomputed ends; host, device memory; a polish job
    between two filter jobs and a filter job between two polish jobs."""
    big = Expected(fm.generate(5, 40_000, pos_range=100_000), ((100, 900, 0),))
    E = _expected_pool(SEQUENCE_POOL)
    R, H, D, S = "runs", "host", "device", "samples_pairs"
    steps = [
        (big, (R, H), S), (E["reads_1"], (R, H), S), (E["reads_513"], (R, H), "pairs_only"), (big, ("ends", D), "pairs_only"),
        (E["listed_all_1300"], (R, H), S), (E["listed_none_1300"], (R, H), S), (E["listed_all_1024"], (R, H), "pairs_only"),
        (E["listed_none_1300"], (R, D), "pairs_only"), (E["listed_last_1300"], (R, D), S), (E["reads_0"], (R, H), S),
        (E["listed_all_1300"], ("ends", H), S),
        (E["unparseable_in_a_sampled_pair"], (R, H), S), (E["reads_1025"], (R, H), S),
        (E["unparseable_single_mate_of_several"], ("ends", D), S), (E["listed_none_1300"], ("ends", D), S),
        (E["unparseable_anywhere"], (R, D), "pairs_only"), (E["reads_513"], ("ends", H), "pairs_only"),
        "abandon", (E["listed_none_1300"], (R, H), "pairs_only"), "abandon_poisoned", (E["listed_all_1024"], (R, H), "pairs_only"),
        (E["ends_past_2_32"], ("ends", H), S), (E["ends_past_2_32"], (R, H), S), (E["ends_past_2_32"], ("ends", D), S),
        (E["equal_positions"], (R, H), S), (E["equal_positions"], (R, D), S), (E["file1_empty"], (R, H), S),
        (E["listed_all_1300"], (R, D), S), (E["both_empty"], ("ends", D), S), (E["file2_empty"], (R, D), "pairs_only"),
        (E["listed_all_1300"], (R, H), "pairs_only"), "polish", (E["listed_all_1300"], (R, H), S), "polish", "polish",
        (E["unparseable_in_a_sampled_pair"], (R, H), S), "polish", (E["listed_none_1300"], (R, H), S),
    ]
    held = []
    for i, st in enumerate(steps):
        if st == "abandon":
            held = _abandon(ctx, pp, E["listed_all_1300"], (R, D))
        elif st == "abandon_poisoned":
            held = _abandon(ctx, pp, E["unparseable_in_a_sampled_pair"], (R, H))
            # the pass over the reads has run and has set the flag; the job is left there
            _check_samples(ctx, pp, E["unparseable_in_a_sampled_pair"], f"step {i}")
        elif st == "polish":
            _polish_job(ctx, orc, 300 + i)
        else:
            exp, form, order = st
            run_job(ctx, pp, exp, form, order, f"step {i} of the ordered sequence")
    del held


def test_random_sequence_of_filter_jobs_on_one_context(ctx, pp, orc):
    """A seeded random sequence of jobs from the pool (and polish jobs, and abandoned begins), each in a random input form
    and call order, every one checked in full; the seed and the steps so far are printed on failure."""
    seed = 20240611
    rng = np.random.default_rng(seed)
    E = _expected_pool(SEQUENCE_POOL)
    done, held = [], []
    try:
        for i in range(48):
            kind = rng.random()
            if kind < 0.08:
                done.append("polish")
                _polish_job(ctx, orc, 400 + i)
                continue
            name = SEQUENCE_POOL[int(rng.integers(0, len(SEQUENCE_POOL)))]
            form = FORMS[int(rng.integers(0, 4))]
            if kind < 0.16:
                done.append(("abandon", name, form))
                held = _abandon(ctx, pp, E[name], form)
                continue
            order = ORDERS[int(rng.integers(0, 4))]
            done.append((name, form, order))
            run_job(ctx, pp, E[name], form, order, f"job {i} of the random sequence, case {name} <{fm.knobs(name)}>")
    except BaseException:
        print(f"random sequence, seed {seed}; steps so far (the last one failed):")
        for d in done:
            print("  ", d)
        raise
    del held


# ---- the command around the seam, from text -----------------------------------------------------------------------------------

TEXT_FROM_SEAM = ("reads_1025", "listed_all_1300", "equal_positions", "ends_past_2_32", "every_op_many_runs", "file1_empty",
                  "file2_empty", "unparseable_where_nobody_looks", "unparseable_in_a_sampled_pair",
                  "unparseable_mate_behind_the_first_good_pair", "unparseable_pair_on_different_references", "group_40_vs_40")
TEXT_ALL = [("text", n) for n in fm.TEXT_CASES] + [("seam", n) for n in TEXT_FROM_SEAM]


def _text_case(kind, name):
    if kind == "text":
        build, read_name, ref_name, runs = fm.TEXT_CASES[name]
        return build(), dict(read_name=read_name, ref_name=ref_name), runs
    return fm.SEAM_CASES[name][0](), {}, (("auto", 0.1, 99.9), ("fr", 10.0, 90.0), ("rr", 30.0, 60.0))


@pytest.mark.parametrize("kind,name", TEXT_ALL, ids=[n for _, n in TEXT_ALL])
def test_filter_command_from_the_generator_s_texts(ctx, pp, orc, tmp_path, monkeypatch, kind, name):
    """pp_filter_files against the oracle's `filter` on the generator's texts, with the host loader and with the device
    loader: the report and both output files byte for byte, or the same error (a quit: code and message; a panic: the code --
    its text is the Rust runtime's, which neither side reproduces)."""
    inp, naming, runs = _text_case(kind, name)
    paths = fm.write_sams(inp, tmp_path, **naming)
    o1, o2, g1, g2 = (str(tmp_path / n) for n in ("o1.sam", "o2.sam", "g1.sam", "g2.sam"))
    for orientation, low_p, high_p in runs:
        try:
            want, err = orc.filter_files(paths[0], paths[1], o1, o2, orientation, low_p, high_p), None
        except orc.OrcError as e:
            want, err = None, e
        for mode in ("0", "1"):
            what = (name, orientation, low_p, high_p, f"PP_DEVICE_FILTER={mode}")
            monkeypatch.setenv("PP_DEVICE_FILTER", mode)
            if err is not None:
                with pytest.raises(pp.PolypolishError) as ge:
                    ctx.filter_files(paths[0], paths[1], g1, g2, orientation, low_p, high_p)
                assert ge.value.code == err.code, (what, ge.value.code, ge.value.msg, err.code, err.msg)
                if err.code != PANIC:
                    assert ge.value.msg == err.msg, what
                continue
            got = ctx.filter_files(paths[0], paths[1], g1, g2, orientation, low_p, high_p)
            assert got == want, what
            for g, o in ((g1, o1), (g2, o2)):
                with open(g, "rb") as a, open(o, "rb") as b:
                    ga, ob = a.read(), b.read()
                if ga != ob:
                    gl, ol = ga.split(b"\n"), ob.split(b"\n")
                    bad = [(i, x[-40:], y[-40:]) for i, (x, y) in enumerate(zip(gl, ol)) if x != y][:5]
                    raise AssertionError((what, os.path.basename(g), len(gl), len(ol), bad))
            os.remove(g1)
            os.remove(g2)


@pytest.mark.parametrize("kind,name", TEXT_ALL, ids=[n for _, n in TEXT_ALL])
def test_device_loader_equals_the_host_loader(ctx, pp, tmp_path, kind, name):
    """pp_filter_load_device against pp_filter_load on the same texts, array by array (RNAME ids up to renaming; the device
    loader's ends against the ends of the host loader's runs), and both against the generator's arrays."""
    inp, naming, _ = _text_case(kind, name)
    paths = fm.write_sams(inp, tmp_path, **naming)
    try:
        host = pp.FilterLoaded(paths[0], paths[1])
    except pp.PolypolishError as e:
        with pytest.raises(pp.PolypolishError) as de:
            pp.FilterLoadedDevice(ctx, paths[0], paths[1])
        assert (de.value.code, de.value.msg) == (e.code, e.msg)
        return
    dev = pp.FilterLoadedDevice(ctx, paths[0], paths[1])
    try:
        want = fm.canonical(inp)
        assert dev.n_reads == host.n_reads == want["n_reads"]
        assert dev.counts == host.counts
        pairs = set()
        for f in range(2):
            d, h, w = dev.files[f], host.files[f], want["files"][f]
            for k in ("read", "grp_off", "grp_idx", "flags", "ref_start"):
                assert np.array_equal(d[k], h[k]), (name, f, k, np.flatnonzero(d[k] != h[k])[:5] if len(d[k]) == len(h[k]) else (len(d[k]), len(h[k])))
                assert np.array_equal(h[k], w[k]), (name, f, k, "host loader against the generator")
            he = fm.ends_array(h)
            assert np.array_equal(d["ref_end"], he), (name, f, "ref_end", np.flatnonzero(d["ref_end"] != he)[:5])
            assert np.array_equal(he, fm.ends_array(w)), (name, f, "ends against the generator")
            pairs |= set(zip(d["ref_id"].tolist(), h["ref_id"].tolist()))
        assert len({a for a, _ in pairs}) == len(pairs) == len({b for _, b in pairs}), (name, "ref_id is not a renaming")
    finally:
        dev.close()
        host.close()
