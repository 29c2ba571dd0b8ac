"""pp_batch_prepare (include/polypolish_hip.h): any valid batch laid out on the device as the library's ingests lay theirs
out -- window-grouped SEQ rooms, the 4-bit mirror, the window-order mirror as one run -- checked with the numpy invariants of
layout_check.py, polished against the plain batch and the oracle at every position, and followed down the direct path.
The source batches are FOREIGN on purpose: SEQ packed back to back (odd, unaligned seq_off), two records that share one SEQ
range, the seq array ending exactly at the last read's end.  Needs an MI355X: `-m gpu`."""
import ctypes as C

import numpy as np
import pytest

import synth
from layout_check import check_seq4_mirror, check_seq_layout, check_window_order_mirror, same_records

pytestmark = pytest.mark.gpu

POS_KEYS = ("depth", "count_a", "count_c", "count_g", "count_t", "count_other", "valid_thr", "invalid_thr", "status")
WINDOW = 2048
# records per workgroup of the placement kernels (PREP_PER_BLOCK, pp_prepare.hip): the 20,000 records of the second input span
# three of them (8192 + 8192 + 3616), so it did not have to be raised
PREP_PER_BLOCK = 8192
LUT = np.frombuffer(b"ACGT", dtype=np.uint8)


@pytest.fixture(scope="module")
def pp():
    import polypolish_amd
    return polypolish_amd


@pytest.fixture(scope="module")
def ctx(pp):
    c = pp.Context(0)
    yield c
    c.close()


# ---- inputs ------------------------------------------------------------------------------------------------------------
def _shared_range(recs):
    """The records plus a copy of record 0 that SHARES its SEQ range (its own CIGAR runs, appended)."""
    out = {k: np.asarray(v).copy() for k, v in recs.items()}
    co, nc = int(recs["cig_off"][0]), int(recs["n_cig"][0])
    for k in ("contig", "ref_start", "k", "seq_off", "seq_len", "n_cig"):
        out[k] = np.concatenate([out[k], out[k][:1]])
    out["cig_off"] = np.concatenate([out["cig_off"], np.array([len(recs["cigar"])], np.uint64)])
    out["cigar"] = np.concatenate([out["cigar"], recs["cigar"][co:co + nc]])
    return out


def _assert_foreign(recs):
    so, sl = recs["seq_off"].astype(np.int64), recs["seq_len"].astype(np.int64)
    assert len(sl) < 2 or (so % 32 != 0).any(), "SEQ packed back to back: unaligned offsets"
    assert len(sl) == 0 or int((so + sl).max()) == len(recs["seq"]), "the array ends exactly at the last read's end"


def _reads(contig_off, bases, where, seed=0, sub_rate=0.01, k=1, random_seq=False):
    """One-run (M) reads, SEQ packed back to back: where = [(contig, ref_start, seq_len), ...]; the bases of the assembly with
    a few substitutions (random_seq: random bases)."""
    rng = np.random.default_rng(seed)
    seqs = []
    for c, rs, sl in where:
        g = int(contig_off[c]) + rs
        s = LUT[rng.integers(0, 4, sl)] if random_seq else np.asarray(bases[g:g + sl]).copy()
        assert len(s) == sl
        sub = rng.random(sl) < sub_rate
        s[sub] = LUT[rng.integers(0, 4, int(sub.sum()))]
        seqs.append(s)
    sl = np.array([w[2] for w in where], np.uint32)
    n = len(where)
    return {"contig": np.array([w[0] for w in where], np.uint32), "ref_start": np.array([w[1] for w in where], np.uint32),
            "k": np.full(n, k, np.uint32), "seq_off": (np.cumsum(sl.astype(np.uint64)) - sl).astype(np.uint64), "seq_len": sl,
            "cig_off": np.arange(n, dtype=np.uint64), "n_cig": np.ones(n, np.uint32),
            "seq": np.concatenate(seqs) if seqs else np.zeros(0, np.uint8), "cigar": (sl << 4).astype(np.uint32)}


def _assembly(lens, seed):
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    return off, LUT[np.random.default_rng(seed).integers(0, 4, int(off[-1]))]


@pytest.fixture(scope="module")
def input_random(orc):
    """two contigs 3000 + 1200, 1500 reads of random multi-run CIGARs (indels, mixed k)"""
    contig_off, bases, recs = synth.random_cigar_records(seed=11, contig_lens=(3000, 1200), n_reads=1500)
    recs = _shared_range(recs)
    _assert_foreign(recs)
    return contig_off, bases, recs, orc.polish_records(contig_off, bases, recs, positions=True)


@pytest.fixture(scope="module")
def input_fast(orc):
    """50 kbp / 60x: 20,000 records (+ the one that shares a range), three workgroups of the placement kernels"""
    contig_off, bases, recs = synth.fast_records(seed=12, contig_lens=(50_000,), coverage=60, read_len=150, indel_read_frac=0.02,
                                                 k_choices=(1, 2, 3), k_probs=(0.8, 0.1, 0.1))
    assert len(recs["contig"]) == 20_000 and len(recs["contig"]) > 2 * PREP_PER_BLOCK
    recs = _shared_range(recs)
    _assert_foreign(recs)
    return contig_off, bases, recs, orc.polish_records(contig_off, bases, recs, positions=True)


def _seam_case(name):
    if name == "one record":
        off, bases = _assembly([3000], 1)
        return off, bases, _reads(off, bases, [(0, 700, 101)])
    if name == "one window":  # every record in window 1 of three
        off, bases = _assembly([5000], 2)
        rng = np.random.default_rng(2)
        return off, bases, _reads(off, bases, [(0, int(s), 75) for s in rng.integers(2048, 4096 - 75, 300)], seed=2)
    if name == "window edges":  # starts on positions 0 and 2047 of a window, and in the assembly's last (partial) window
        off, bases = _assembly([2 * WINDOW + 700], 3)
        where = [(0, s, 99) for s in (0, 2047, 2048, 4095, 4096, 4096 + 300, 4096 + 601)] * 7
        return off, bases, _reads(off, bases, where, seed=3)
    if name == "contig boundary in a window":  # window 1 (2048..4095) holds records of both contigs
        off, bases = _assembly([3000, 2500], 4)
        rng = np.random.default_rng(4)
        where = [(0, int(s), 120) for s in rng.integers(2048, 3000 - 120, 40)] + [(1, int(s), 120) for s in rng.integers(0, 1096 - 120, 40)]
        where += [(0, 100, 120)] * 6 + [(1, 2300, 120)] * 6
        where = [where[i] for i in rng.permutation(len(where))]
        return off, bases, _reads(off, bases, where, seed=4)
    if name == "read lengths":  # around the room size and the fast class's limit, and one read across three windows
        off, bases = _assembly([12_000], 5)
        where = []
        for sl in (1, 31, 32, 33, 160, 252):
            where += [(0, 1000 + 3 * sl + 17 * j, sl) for j in range(6)]
        where.insert(11, (0, 1500, 5000))
        return off, bases, _reads(off, bases, where, seed=5)
    if name == "8200 windows":  # past the windows a workgroup's LDS holds (PREP_WIN_LDS = 8192): the global-counter kernels
        G = 8200 * WINDOW - 100
        off, bases = np.array([0, G], np.uint64), np.full(G, ord("A"), np.uint8)
        rng = np.random.default_rng(6)
        where = []
        for w in (0, 8191, 8192, 8199):
            where += [(0, int(s), 100) for s in w * WINDOW + rng.integers(0, WINDOW - 200, 90)]
        where = [where[i] for i in rng.permutation(len(where))]
        return off, bases, _reads(off, bases, where, seed=6, random_seq=True)
    raise KeyError(name)


SEAMS = ("one record", "one window", "window edges", "contig boundary in a window", "read lengths", "8200 windows")


# ---- helpers -----------------------------------------------------------------------------------------------------------
def _prepare(pp, ctx, contig_off, recs, source):
    """-> (PreparedBatch, whatever has to stay alive)"""
    if source == "host":
        return pp.prepare_records(ctx, contig_off, recs), None
    import torch
    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(np.ascontiguousarray(recs[k], dtype=dt)).to(dev) for k, dt in pp.REC_FIELDS}
    torch.cuda.synchronize()
    ptrs = {k: v.data_ptr() for k, v in t.items()}
    p = pp.prepare_batch(ctx, contig_off, len(recs["contig"]), ptrs, len(recs["seq"]), len(recs["cigar"]), pp.MEM_DEVICE)
    del t  # the source may be released when the call returns
    torch.cuda.synchronize()
    return p, None


def _check_layout(pp, contig_off, src, prep):
    """every check over ALL records of the batch"""
    n = len(src["contig"])
    h = prep.host()
    assert prep.n_aln == n and prep.n_cig_total == len(src["cigar"]) and prep.seq_bytes == len(h["seq"])
    # (same_records also wants seq arrays of one length: a foreign source has no rooms, so it is compared padded to the
    # prepared array's length -- the records' bytes, which is what it compares, are where they were)
    assert len(h["seq"]) >= len(src["seq"])
    same_records(dict(src, seq=np.concatenate([src["seq"], np.zeros(len(h["seq"]) - len(src["seq"]), np.uint8)])), h)
    check_seq_layout(h, contig_off, used_per_file=[n], grouped=True)
    assert [int(e) for e in h["wo_runs"]] == ([n] if n else [])
    check_window_order_mirror(h, contig_off, [n])
    check_seq4_mirror(pp, h, expect=True)
    return h


def _polish_prepared(pp, ctx, contig_off, bases, preps, positions=False, emit=None, **kw):
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    pp.lib().pp_polish_set_debug(ctx._h, int(positions))
    try:
        ctx.polish_begin(contig_off, bases.ctypes.data, pp.MEM_HOST, **kw)
        if emit is not None:
            ctx.set_emit(emit)
        for p in preps:
            ctx.polish_add_ptrs(p.n_aln, p.ptrs(), p.seq_bytes, p.n_cig_total, pp.MEM_DEVICE)
        ctx.polish_finish()
        polished, offs, stats = ctx.result()
        return {"polished": polished, "offsets": offs, "stats": stats, "positions": ctx.positions() if positions else None}
    finally:
        pp.lib().pp_polish_set_debug(ctx._h, 0)


def _same_everywhere(got, want, what):
    for k in POS_KEYS:
        bad = np.nonzero(want["positions"][k] != got["positions"][k])[0]
        assert len(bad) == 0, (what, k, len(bad), bad[:8], want["positions"][k][bad[:8]], got["positions"][k][bad[:8]])
    assert np.array_equal(got["offsets"], want["offsets"]), what
    assert got["polished"] == want["polished"], what


def _check_parity(pp, ctx, contig_off, bases, recs, prep, want, route=True):
    """polish(prepared) == polish(plain) == the oracle at every position; the prepared batch goes down the direct path, the
    plain one does not"""
    got = _polish_prepared(pp, ctx, contig_off, bases, [prep], positions=True)
    plain = ctx.polish_records(contig_off, bases, recs, positions=True)
    _same_everywhere(got, plain, "prepared against plain")
    _same_everywhere(got, want, "prepared against the oracle")
    del got, plain
    if route:
        fast = _polish_prepared(pp, ctx, contig_off, bases, [prep])
        assert ctx.took_direct_path(), "a prepared batch did not take the direct path"
        assert fast["polished"] == want["polished"] and np.array_equal(fast["offsets"], want["offsets"])
        slow = ctx.polish_records(contig_off, bases, recs)
        assert not ctx.took_direct_path(), "the plain batch took the direct path"
        assert slow["polished"] == want["polished"]


# ---- 1. layout, 3. parity and route ------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["host", "device"])
@pytest.mark.parametrize("which", ["random", "fast"])
def test_layout_parity_and_route(pp, ctx, input_random, input_fast, which, source):
    contig_off, bases, recs, want = input_random if which == "random" else input_fast
    prep, _ = _prepare(pp, ctx, contig_off, recs, source)
    try:
        _check_layout(pp, contig_off, recs, prep)
        _check_parity(pp, ctx, contig_off, bases, recs, prep, want)
    finally:
        prep.close()


# ---- 2. seams ----------------------------------------------------------------------------------------------------------
def test_empty_batch(pp, ctx, orc):
    off, bases = _assembly([3000, 500], 9)
    empty = {k: np.zeros(0, dtype=dt) for k, dt in pp.REC_FIELDS}
    for source in ("host", "device"):
        prep, _ = _prepare(pp, ctx, off, empty, source)
        h = _check_layout(pp, off, empty, prep)
        assert len(h["seq"]) == 0 and len(h["wo"]) == 0 and len(h["seq4"]) == 0
        want = orc.polish_records(off, bases, empty, positions=True)
        _check_parity(pp, ctx, off, bases, empty, prep, want, route=False)
        prep.close()


@pytest.mark.parametrize("name", SEAMS)
def test_seams(pp, ctx, orc, name):
    contig_off, bases, recs = _seam_case(name)
    if len(recs["contig"]) > 1:
        recs = _shared_range(recs)
    _assert_foreign(recs)
    want = orc.polish_records(contig_off, bases, recs, positions=True)
    for source in ("host", "device"):
        prep, _ = _prepare(pp, ctx, contig_off, recs, source)
        try:
            h = _check_layout(pp, contig_off, recs, prep)
            if name == "8200 windows":
                win = (recs["ref_start"].astype(np.int64) // WINDOW)
                assert sorted(set(win.tolist())) == [0, 8191, 8192, 8199]
                assert np.array_equal(h["wo"]["ref_start"].astype(np.int64) // WINDOW, np.sort(win))
            if source == "host":
                _check_parity(pp, ctx, contig_off, bases, recs, prep, want)
        finally:
            prep.close()


# ---- 3. reuse and several batches --------------------------------------------------------------------------------------
def test_resident_reuse_with_other_parameters(pp, ctx, orc, input_fast):
    """the same prepared batch, borrowed by three jobs of one context with different parameters: the oracle's bytes each time"""
    contig_off, bases, recs, _ = input_fast
    prep, _ = _prepare(pp, ctx, contig_off, recs, "host")
    try:
        for kw in (dict(min_depth=5, fraction_valid=0.5, fraction_invalid=0.2), dict(min_depth=40, fraction_valid=0.7, fraction_invalid=0.1),
                   dict(min_depth=1, fraction_valid=0.3, fraction_invalid=0.25)):
            want = orc.polish_records(contig_off, bases, recs, **kw)
            got = _polish_prepared(pp, ctx, contig_off, bases, [prep], **kw)
            assert ctx.took_direct_path(), kw
            assert got["polished"] == want["polished"] and np.array_equal(got["offsets"], want["offsets"]), kw
    finally:
        prep.close()


@pytest.mark.parametrize("which", ["random", "fast"])
def test_two_prepared_batches_in_one_job(pp, ctx, input_random, input_fast, which):
    """the records cut in two, each half prepared on its own, both added to one job: the two runs are joined, the job takes the
    direct path and gives the same bytes"""
    contig_off, bases, recs, want = input_random if which == "random" else input_fast
    n = len(recs["contig"])
    halves = pp.split_records({k: np.ascontiguousarray(recs[k], dtype=dt) for k, dt in pp.REC_FIELDS}, [n // 2 + 1])
    assert len(halves) == 2
    preps = [pp.prepare_records(ctx, contig_off, h) for h in halves]
    try:
        got = _polish_prepared(pp, ctx, contig_off, bases, preps)
        assert ctx.took_direct_path()
        assert got["polished"] == want["polished"] and np.array_equal(got["offsets"], want["offsets"])
        deb = _polish_prepared(pp, ctx, contig_off, bases, preps, positions=True)
        _same_everywhere(deb, want, "two prepared batches against the oracle")
    finally:
        for p in preps:
            p.close()


# ---- 4. errors ---------------------------------------------------------------------------------------------------------
def _outcome(pp, fn):
    try:
        fn()
        return None
    except pp.PolypolishError as e:
        return (e.code, e.msg)


def _small_good():
    return synth.fast_records(seed=21, contig_lens=(6000, 2500), coverage=20, read_len=150, indel_read_frac=0.05)


def _bad_case(kind):
    contig_off, bases, recs = _small_good()
    recs = {k: v.copy() for k, v in recs.items()}
    i = 301
    if kind == "contig out of range":
        recs["contig"][i] = 7
    elif kind == "k = 0":
        recs["k"][i] = 0
    elif kind == "SEQ range outside the array":
        recs["seq_off"][i] = len(recs["seq"]) - 10
    elif kind == "SEQ range beyond 2^40":
        recs["seq_off"][i] = (1 << 40) + 5
    elif kind == "CIGAR/SEQ length mismatch":
        i = int(np.nonzero(recs["n_cig"] == 1)[0][40])
        recs["seq_len"][i] -= 1
    elif kind == "read past its contig's end":
        i = int(np.nonzero((recs["n_cig"] == 1) & (recs["contig"] == 1))[0][10])
        recs["ref_start"][i] = 2500 - 10
    elif kind == "random CIGARs with defects":
        contig_off, bases, recs = synth.random_cigar_records(seed=22, bad_frac=0.1)
    else:
        raise KeyError(kind)
    return contig_off, bases, recs


BAD = ("contig out of range", "k = 0", "SEQ range outside the array", "SEQ range beyond 2^40", "CIGAR/SEQ length mismatch",
       "read past its contig's end", "random CIGARs with defects")


@pytest.mark.parametrize("kind", BAD)
def test_the_polish_reports_the_same_record(pp, ctx, kind):
    """one bad record inside an otherwise good batch: prepare is memory-safe and validates nothing; pp_polish_finish names the same
    record with the same message on the prepared batch as on the plain one"""
    contig_off, bases, recs = _bad_case(kind)
    plain = _outcome(pp, lambda: ctx.polish_records(contig_off, bases, recs))
    assert plain is not None, "the plain batch was accepted"
    for source in ("host", "device"):
        prep, _ = _prepare(pp, ctx, contig_off, recs, source)
        try:
            got = _outcome(pp, lambda: _polish_prepared(pp, ctx, contig_off, bases, [prep]))
            assert got == plain, (source, got, plain)
            h = prep.host()
            for k in ("contig", "ref_start", "k", "seq_len", "cig_off", "n_cig", "cigar"):
                assert np.array_equal(h[k], recs[k]), k
        finally:
            prep.close()
    # the context is as good as before
    contig_off, bases, recs = _small_good()
    assert _outcome(pp, lambda: ctx.polish_records(contig_off, bases, recs)) is None


def test_argument_errors(pp, ctx):
    contig_off, bases, recs = _small_good()
    keep = {k: np.ascontiguousarray(recs[k], dtype=dt) for k, dt in pp.REC_FIELDS}
    ptrs = {k: v.ctypes.data for k, v in keep.items()}
    n, sb, nc = len(keep["contig"]), len(keep["seq"]), len(keep["cigar"])

    def code(off, n_aln, p, seq_bytes, mem):
        try:
            pp.prepare_batch(ctx, off, n_aln, p, seq_bytes, nc, mem).close()
            return pp.OK
        except pp.PolypolishError as e:
            assert e.msg
            return e.code

    assert code(contig_off, n, ptrs, sb, pp.MEM_HOST) == pp.OK
    assert code(np.array([0], np.uint64), n, ptrs, sb, pp.MEM_HOST) == pp.ERR_ARG          # n_contigs == 0
    assert code(np.array([0, 6000, 5000], np.uint64), n, ptrs, sb, pp.MEM_HOST) == pp.ERR_ARG  # descending contig_off
    assert code(contig_off, n, ptrs, sb, pp.MEM_PEER) == pp.ERR_ARG
    assert code(contig_off, n, ptrs, sb, 7) == pp.ERR_ARG
    for name, _ in pp.REC_FIELDS:  # a null array in a non-empty batch
        assert code(contig_off, n, dict(ptrs, **{name: 0}), sb, pp.MEM_HOST) == pp.ERR_ARG, name
    L = pp.lib()
    off = np.ascontiguousarray(contig_off, dtype=np.uint64)
    b = pp.aln_batch(n, ptrs, sb, nc)
    out = C.c_void_p()
    assert L.pp_batch_prepare(None, 2, off.ctypes.data, C.byref(b), pp.MEM_HOST, C.byref(out)) == pp.ERR_ARG
    assert L.pp_batch_prepare(ctx._h, 2, None, C.byref(b), pp.MEM_HOST, C.byref(out)) == pp.ERR_ARG
    assert L.pp_batch_prepare(ctx._h, 2, off.ctypes.data, None, pp.MEM_HOST, C.byref(out)) == pp.ERR_ARG
    assert L.pp_batch_prepare(ctx._h, 2, off.ctypes.data, C.byref(b), pp.MEM_HOST, None) == pp.ERR_ARG
    assert not out.value
    # the limits of pp_polish_begin / pp_polish_add (checked before an array is looked at)
    assert code(np.array([0, 1 << 32], np.uint64), n, ptrs, sb, pp.MEM_HOST) == pp.ERR_LIMIT
    assert code(contig_off, (1 << 32) - 1, ptrs, sb, pp.MEM_HOST) == pp.ERR_LIMIT
    assert code(contig_off, n, ptrs, 1 << 40, pp.MEM_HOST) == pp.ERR_LIMIT


def test_kernel_time_needs_profiling(pp, ctx):
    contig_off, bases, recs = _small_good()
    prep = pp.prepare_records(ctx, contig_off, recs)
    with pytest.raises(pp.PolypolishError) as e:
        prep.kernel_ms()
    assert e.value.code == pp.ERR_ARG
    prep.close()
    ctx.set_profiling(1)
    try:
        prep = pp.prepare_records(ctx, contig_off, recs)
        assert 0.0 < prep.kernel_ms() < 1000.0
        prep.close()
    finally:
        ctx.set_profiling(0)


# ---- 5. sharded --------------------------------------------------------------------------------------------------------
def test_shards_of_a_prepared_batch_take_the_direct_path(pp, ctx, orc):
    """pp_shard_split of a prepared batch under a plan of two ranks, the ranks as two contexts on one GPU: both take the direct
    path, their bytes assemble to the one-context result (and the oracle's)"""
    contig_off, bases, recs = synth.fast_records(seed=31, contig_lens=(150_000, 9_000), coverage=15, read_len=120,
                                                 indel_read_frac=0.1, k_choices=(1, 2, 3), k_probs=(0.7, 0.2, 0.1))
    want = orc.polish_records(contig_off, bases, recs)
    plan = pp.Plan(contig_off, np.bincount(recs["contig"], minlength=2), 2, 65536)
    other = pp.Context(0)
    prep = pp.prepare_records(ctx, contig_off, recs)
    try:
        one = _polish_prepared(pp, ctx, contig_off, bases, [prep])
        assert one["polished"] == want["polished"]
        rank_bytes, rank_offs = [], []
        for rank, c in enumerate((ctx, other)):
            part = pp.ShardPart(c, plan, rank, prep.n_aln, prep.ptrs(), prep.seq_bytes, prep.n_cig_total, pp.MEM_DEVICE)
            assert 0 < part.n_aln < prep.n_aln and list(part.ptrs["wo_runs"]) == [part.n_aln]
            bb = np.ascontiguousarray(bases, dtype=np.uint8)
            c.polish_begin(contig_off, bb.ctypes.data, pp.MEM_HOST)
            c.set_emit(plan.emit_ranges(rank))
            c.polish_add_ptrs(part.n_aln, part.ptrs, part.seq_bytes, part.n_cig_total, pp.MEM_DEVICE)
            c.polish_finish()
            assert c.took_direct_path(), rank
            polished, offs, _ = c.result()
            part.close()
            rank_bytes.append(polished)
            rank_offs.append(offs)
        data, out_off = plan.assemble(rank_bytes, rank_offs)
        assert data == one["polished"] and np.array_equal(out_off, one["offsets"])
    finally:
        prep.close()
        other.close()
        plan.close()
