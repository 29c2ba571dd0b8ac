"""pp_batch_regroup (pp_regroup.hip) against its plain model (tests/regroup_model.py), byte for byte: perm, the nine gathered arrays,
the counts and the carried verdicts.  The sizes stand around the seams of the kernels: a wave, the sort's tile (regroup_geometry),
and 256 / 65,536 records, where the radix sort takes one more pass.  Offsets and lengths are garbage throughout: the link copies them
and never follows them.  Needs an MI355X: `-m gpu`."""
import ctypes as C

import numpy as np
import pytest

import regroup_model as rm

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
def tile(pp):
    t = pp.regroup_geometry()
    assert t >= 256 and t % 64 == 0
    return t


def make_raw(ids, flag=None, seed=0):
    """a raw batch around the ids: every other per-record value random over its whole range (seq_off / cig_off point nowhere)"""
    rng = np.random.default_rng(seed)
    n = len(ids)
    u32 = lambda: rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    u64 = lambda: rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    if flag is None:
        flag = rng.integers(0, 1 << 16, n, dtype=np.uint64).astype(np.uint16) & np.uint16(0xFFFB)     # (all aligned)
    return {"flag": np.asarray(flag, np.uint16), "read_id": np.asarray(ids, np.uint64), "contig": u32(), "ref_start": u32(), "nm": u32(),
            "seq_off": u64(), "seq_len": u32(), "cig_off": u64(), "n_cig": u32(),
            "seq": np.frombuffer(b"ACGTacgtNN*", np.uint8).copy(), "cigar": np.array([16, 33, 48], np.uint32)}


def run(pp, ctx, raw, source="host"):
    """-> (the Regrouped, the device addresses it was given or None, what keeps them alive)"""
    if source == "host":
        return pp.regroup_records(ctx, raw), None, None
    import torch
    dev = torch.device("cuda:0")
    signed = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64, np.dtype(np.uint8): np.uint8}
    t = {k: torch.from_numpy(np.ascontiguousarray(raw[k], dtype=dt).view(signed[np.dtype(dt)])).to(dev) for k, dt in pp.RAW_FIELDS}
    torch.cuda.synchronize()
    ptrs = {k: v.data_ptr() for k, v in t.items()}
    ptrs.update(n_rec=len(raw["flag"]), seq_bytes=len(raw["seq"]), n_cig_total=len(raw["cigar"]))
    return pp.regroup_records(ctx, ptrs, mem=pp.MEM_DEVICE), ptrs, t


def check(pp, ctx, raw, source="host", passed=None):
    """the link on `raw` is the model on `raw`; -> (perm, counts)"""
    want = rm.regroup(raw)
    g, ptrs, keep = run(pp, ctx, raw, source)
    try:
        n = len(raw["flag"])
        assert g.n_rec == n and g.seq_bytes == len(raw["seq"]) and g.n_cig_total == len(raw["cigar"])
        perm = g.perm()
        assert perm.dtype == np.uint32 and np.array_equal(perm, want["perm"]), (perm[:16], want["perm"][:16])
        assert g.counts() == want["counts"]
        got = g.host()
        rm.same_raw(got, want["raw"])
        assert np.array_equal(got["seq"], raw["seq"]) and np.array_equal(got["cigar"], raw["cigar"]), "seq and cigar are not moved"
        view = g.raw()
        if ptrs is not None:
            assert view["seq"] == ptrs["seq"] and view["cigar"] == ptrs["cigar"], "device memory: seq and cigar stay borrowed"
            for k in rm.PER_RECORD:
                assert (view[k] == ptrs[k]) == (want["counts"][1] == 0 or n == 0), (k, "nothing moves: nothing is copied")
        n_al = int(((raw["flag"] & 4) == 0).sum())
        v = np.asarray(passed, np.uint8) if passed is not None else (np.arange(n_al) * 7 % 251).astype(np.uint8)
        assert np.array_equal(g.carry_pass(v), rm.carry_pass(raw["flag"], want["perm"], v))
        return perm, want["counts"]
    finally:
        g.close()
        del keep


def halves(n):
    """pairs: record i and record i + ceil(n / 2) are mates -- in different tiles wherever n has more than one"""
    return np.arange(n, dtype=np.uint64) % np.uint64(max(1, (n + 1) // 2))


def sizes(tile):
    return [0, 1, 2, 63, 64, 65, tile - 1, tile, tile + 1, 2 * tile + 1]


RADIX_SEAMS = (255, 256, 257, 65535, 65536, 65537)


@pytest.mark.parametrize("source", ["host", "device"])
def test_sizes_around_a_wave_and_the_tile(pp, ctx, tile, source):
    for n in sizes(tile):
        rng = np.random.default_rng(n)
        ids = rng.integers(0, max(1, n // 3), n, dtype=np.uint64) + np.uint64(1000)
        flag = np.where(rng.random(n) < 0.2, 4, 0).astype(np.uint16) | (rng.integers(0, 2, n).astype(np.uint16) << 4)
        _, counts = check(pp, ctx, make_raw(ids, flag, seed=n), source)
        assert n < 3 or counts[1] > 0, n


@pytest.mark.parametrize("n", RADIX_SEAMS)
def test_radix_seams_with_distinct_ids_and_with_mates_in_different_tiles(pp, ctx, tile, n):
    rng = np.random.default_rng(n)
    distinct = rng.permutation(n).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    perm, counts = check(pp, ctx, make_raw(distinct, seed=n), "device")
    assert counts == (n, 0) and np.array_equal(perm, np.arange(n, dtype=np.uint32)), "all ids distinct: the identity"
    perm, counts = check(pp, ctx, make_raw(halves(n), seed=n + 1), "device")
    assert counts[0] == (n + 1) // 2 and counts[1] >= n - 3
    assert n <= tile or (n + 1) // 2 >= tile, "mates lie in different tiles"
    check(pp, ctx, make_raw(halves(n), seed=n + 2), "host")


def patterns():
    rng = np.random.default_rng(77)
    n = 20001
    out = {"all_equal": np.full(n, 42, np.uint64),
           "abab": np.arange(n, dtype=np.uint64) % np.uint64(2),
           # every pair reversed: a b b a | c d d c | ...: the second pair of every four comes mate first
           "pairs_reversed": np.uint64(2) * (np.arange(n, dtype=np.uint64) // np.uint64(4)) + np.array([0, 1, 1, 0], np.uint64)[np.arange(n) % 4]}
    size = rng.integers(1, 6, 6000)
    groups = np.repeat(np.arange(len(size), dtype=np.uint64), size)
    out["random_groups_shuffled"] = rng.permutation(groups) + np.uint64(5)
    big = np.arange(20000, dtype=np.uint64) + np.uint64(100)
    big[rng.choice(20000, 5000, replace=False)] = 7
    out["one_group_of_5000"] = big
    return out


@pytest.mark.parametrize("name", ["all_equal", "abab", "pairs_reversed", "random_groups_shuffled", "one_group_of_5000"])
@pytest.mark.parametrize("source", ["host", "device"])
def test_id_patterns(pp, ctx, name, source):
    ids = patterns()[name]
    perm, counts = check(pp, ctx, make_raw(ids, seed=3), source)
    if name == "all_equal":
        assert counts == (1, 0)
    if name == "pairs_reversed":
        assert perm[:8].tolist() == [0, 3, 1, 2, 4, 7, 5, 6]
    if name == "abab":
        assert counts[0] == 2 and perm[:3].tolist() == [0, 2, 4] and perm[-1] == len(ids) - 2
    if name == "one_group_of_5000":
        assert counts[0] == 15001 and counts[1] > 10000


def test_id_values(pp, ctx):
    n = 3000
    base = np.arange(n, dtype=np.uint64) % np.uint64(1000)
    cap = 1024
    while cap < 2 * n + 2:
        cap *= 2
    for ids in (base << np.uint64(33),                                              # ids that differ only above bit 32
                (base << np.uint64(33)) | np.uint64(5),
                base * np.uint64(cap), base * np.uint64(cap * 4),                   # multiples of the table's capacity
                np.where(base % np.uint64(2) == 0, np.uint64(0), np.uint64(0xFFFFFFFFFFFFFFFF)),   # id 0 and id 2^64-1
                np.where(base < 500, base, np.uint64(0xFFFFFFFFFFFFFFFF) - base)):
        _, counts = check(pp, ctx, make_raw(ids.astype(np.uint64), seed=9), "device")
        assert counts[0] == len(np.unique(ids))


@pytest.mark.parametrize("source", ["host", "device"])
def test_unaligned_records_take_part_in_the_order_and_not_in_the_verdicts(pp, ctx, source):
    rng = np.random.default_rng(4)
    n = 9000
    ids = rng.permutation(np.repeat(np.arange(3000, dtype=np.uint64), 3))
    flag = np.zeros(n, np.uint16)
    flag[rng.choice(n, 2500, replace=False)] = 4          # inside groups and between them
    flag[[0, n - 1]] = 4
    flag |= (rng.integers(0, 2, n).astype(np.uint16) << 8)
    passed = (rng.random(int(((flag & 4) == 0).sum())) < 0.7).astype(np.uint8)
    perm, counts = check(pp, ctx, make_raw(ids, flag, seed=5), source, passed)
    assert counts[1] > n // 2
    all_unaligned = np.full(500, 4, np.uint16)
    check(pp, ctx, make_raw(halves(500), all_unaligned, seed=6), source, np.zeros(0, np.uint8))


def test_regrouping_is_idempotent_and_two_calls_give_identical_bytes(pp, ctx):
    raw = make_raw(patterns()["random_groups_shuffled"], seed=8)
    first, _, _ = run(pp, ctx, raw)
    second, _, _ = run(pp, ctx, raw)
    try:
        a, b = first.host(), second.host()
        rm.same_raw(a, b)
        assert np.array_equal(first.perm(), second.perm()) and first.counts() == second.counts()
        again = pp.regroup_records(ctx, first.raw(), mem=pp.MEM_DEVICE)     # the view goes in again as device memory
        try:
            assert again.counts() == (first.counts()[0], 0)
            assert np.array_equal(again.perm(), np.arange(len(raw["flag"]), dtype=np.uint32))
            assert again.raw() == first.raw(), "nothing moves: the view is the input's own arrays"
            rm.same_raw(again.host(), a)
        finally:
            again.close()
    finally:
        first.close()
        second.close()


def test_a_large_job_and_then_a_small_one_on_one_context(pp, ctx):
    rng = np.random.default_rng(10)
    big = rng.permutation(np.repeat(np.arange(100_000, dtype=np.uint64), 2))
    check(pp, ctx, make_raw(big, seed=11), "device")
    check(pp, ctx, make_raw(halves(100), seed=12), "device")
    check(pp, ctx, make_raw(halves(5000), seed=13), "host")


def test_stage_times_need_profiling(pp, ctx):
    raw = make_raw(halves(5000), seed=14)
    g = pp.regroup_records(ctx, raw)
    with pytest.raises(pp.PolypolishError) as e:
        g.kernel_ms()
    assert e.value.code == pp.ERR_ARG
    g.close()
    ctx.set_profiling(True)
    try:
        g = pp.regroup_records(ctx, raw)
        ms = g.stage_ms()
        assert set(ms) == {"intern", "sort", "gather"} and all(v > 0 for v in ms.values())
        assert abs(g.kernel_ms() - sum(ms.values())) < 1e-3
        g.close()
    finally:
        ctx.set_profiling(False)


def test_the_contract_s_argument_errors(pp, ctx):
    L = pp.lib()
    raw = make_raw(halves(100), seed=15)
    b, keep = pp._raw_batch(raw, True, pp.RAW_FIELDS)
    out = C.c_void_p()
    assert L.pp_batch_regroup(None, C.byref(b), pp.MEM_HOST, C.byref(out)) == pp.ERR_ARG
    assert L.pp_batch_regroup(ctx._h, None, pp.MEM_HOST, C.byref(out)) == pp.ERR_ARG
    assert L.pp_batch_regroup(ctx._h, C.byref(b), pp.MEM_HOST, None) == pp.ERR_ARG
    assert L.pp_batch_regroup(ctx._h, C.byref(b), pp.MEM_PEER, C.byref(out)) == pp.ERR_ARG and not out.value
    for name, _ in pp.RAW_FIELDS:
        if name in ("seq", "cigar"):
            continue
        broken, _k = pp._raw_batch(raw, True, pp.RAW_FIELDS)
        setattr(broken, name, None)
        for mem in (pp.MEM_HOST, pp.MEM_DEVICE):      # (refused before anything is read: host addresses do no harm)
            assert L.pp_batch_regroup(ctx._h, C.byref(broken), mem, C.byref(out)) == pp.ERR_ARG and not out.value, (name, mem)
        assert b"null array" in L.pp_last_error(ctx._h)
    huge, _k = pp._raw_batch(raw, True, pp.RAW_FIELDS)
    huge.n_rec = 0xFFFFFFFF
    assert L.pp_batch_regroup(ctx._h, C.byref(huge), pp.MEM_DEVICE, C.byref(out)) == pp.ERR_LIMIT and not out.value
    empty, _k = pp._raw_batch(raw, True, pp.RAW_FIELDS)
    empty.n_rec = 0
    for name, _ in pp.RAW_FIELDS:
        setattr(empty, name, None)
    empty.seq_bytes = empty.n_cig_total = 0
    assert L.pp_batch_regroup(ctx._h, C.byref(empty), pp.MEM_HOST, C.byref(out)) == pp.OK and out.value, "n_rec == 0: an empty object"
    L.pp_regrouped_free(out)
    g = pp.regroup_records(ctx, raw)
    try:
        for wrong in (99, 101, 0):
            with pytest.raises(pp.PolypolishError) as e:
                g.carry_pass(np.ones(wrong, np.uint8))
            assert e.value.code == pp.ERR_ARG and "100 aligned" in str(e.value)
    finally:
        g.close()
    check(pp, ctx, raw)                               # the context is fine afterwards
