"""pp_names on the GPU (pp_names.hip: k_nm_lookup / k_nm_insert / k_nm_rank / k_nm_copy / k_nm_rehash) against the plain model
of tests/names_model.py, which tests/test_names_model_cpu.py pins to the host loader's read numbers.  Every case runs from host
memory and from device memory (torch tensors that are exactly as long as the arrays).  Needs an MI355X: `-m gpu`."""
import ctypes as C

import numpy as np
import pytest

import names_model as nm
import synth

pytestmark = pytest.mark.gpu
ARG = 4
SOURCES = ("host", "device")
U64_MAX = (1 << 64) - 1


@pytest.fixture(scope="module")
def pp():
    import polypolish_amd
    return polypolish_amd


@pytest.fixture(scope="module")
def ctx(pp):
    c = pp.Context(0)
    yield c
    c.close()


def to_device(call):
    """the call's three arrays and room for the ids as tensors of exactly their sizes -> (addresses, tensors to keep)"""
    import torch
    dev = torch.device("cuda:0")
    b, off, ln = call
    t = [torch.from_numpy(np.ascontiguousarray(b, np.uint8)).to(dev), torch.from_numpy(np.ascontiguousarray(off, np.uint64).view(np.int64)).to(dev),
         torch.from_numpy(np.ascontiguousarray(ln, np.uint32).view(np.int32)).to(dev), torch.full((len(off),), -1, dtype=torch.int64, device=dev)]
    torch.cuda.synchronize()
    return tuple(x.data_ptr() or None for x in t), t


def query(pp, table, call, source):
    """pp_names_ids on (bytes, off, len) -> np.uint64 ids"""
    if source == "host":
        return table.ids(call)
    (bp, op, lp, out), keep = to_device(call)
    return table.ids((bp, op, lp), mem=pp.MEM_DEVICE, n=len(call[1]), n_bytes=len(call[0]), out=out)


def run(pp, ctx, calls, source, expect=0, state=None, table=None):
    """every call on one table, each against the model -> (ids per call, the table: the caller closes it)"""
    table = table or pp.Names(ctx, expect)
    state = {} if state is None else state
    out = []
    for call in calls:
        want = np.array(nm.ids(state, nm.names_of(call)), np.uint64)
        got = query(pp, table, call, source)
        assert got.dtype == np.uint64 and got.shape == want.shape
        bad = np.flatnonzero(got != want)
        assert not len(bad), (source, f"names {bad[:8].tolist()}: ids {got[bad[:8]].tolist()}, the model says {want[bad[:8]].tolist()}")
        assert table.count == len(state)
        out.append(got)
    return out, table


# ---- the seams of the wide reads ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("source", SOURCES)
def test_every_alignment_and_length_around_the_eight_byte_loads(pp, ctx, source):
    call, quads, pairs = nm.seam_case()
    # a fresh table (names against names of the call), the same names again (against the pool), and again one and five bytes
    # further on (every off & 7 moves)
    ids, table = run(pp, ctx, [call, call, nm.shifted(call, 1), nm.shifted(call, 5)], source)
    try:
        for got in ids:
            for i1, i2, i3, i4 in quads:
                assert got[i1] == got[i2]                         # two copies, different bytes behind them: one id
                if i3 is not None:
                    assert got[i3] != got[i1] and got[i4] != got[i1] and got[i4] != got[i3]   # last byte changed | one byte shorter
            for i, j in pairs:                                    # one byte of difference at 0, 7, 8, 15
                assert got[i] != got[j]
        assert all(np.array_equal(ids[0], g) for g in ids[1:])
    finally:
        table.close()


@pytest.mark.parametrize("source", SOURCES)
def test_nul_and_high_bytes_the_empty_name_and_a_name_of_10000_bytes(pp, ctx, source):
    call = nm.raw_bytes_case()
    names = nm.names_of(call)
    (got, again), table = run(pp, ctx, [call, nm.shifted(call, 6)], source)
    try:
        assert np.array_equal(got, again)
        first = {n: names.index(n) for n in names}
        assert [int(got[first[n]]) for n in names] == got.tolist()              # equal names, equal ids ...
        assert len(set(got.tolist())) == len(set(names)) == table.count         # ... and only those
        empties = [i for i, n in enumerate(names) if n == b""]
        longs = [i for i, n in enumerate(names) if len(n) == nm.LONG]
        assert len(empties) == 2 and got[empties[0]] == got[empties[1]]
        assert len(longs) == 3 and len({int(got[i]) for i in longs}) == 2       # twice the same, once with its last byte changed
        for i in (empties[0], longs[0], longs[1], names.index(b"a\x00b"), names.index(b"\xff\xfe\x80\x00")):
            assert table.name(int(got[i])) == names[i]
    finally:
        table.close()


@pytest.mark.parametrize("source", SOURCES)
def test_the_last_name_ends_where_the_array_ends(pp, ctx, source):
    # n_bytes is no multiple of 8 and, on the device, the tensor is exactly n_bytes long.  The VALUES are checked here; that no
    # load reaches past n_bytes is a property of word_at (pp_names.hip: an 8-byte load only where eight bytes are left) that is
    # checked by reading the code -- a stray read of a few bytes behind a tensor faults nowhere.
    for call in nm.array_end_cases():
        _, table = run(pp, ctx, [call, call], source)
        last = len(call[1]) - 1
        try:
            assert table.name(int(query(pp, table, call, source)[last])) == nm.names_of(call)[last]
        finally:
            table.close()


# ---- order and determinism -------------------------------------------------------------------------------------------------------------

def _first_appearance(names):
    seen = {}
    return np.array([seen.setdefault(n, len(seen)) for n in names], np.uint64)


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("split", (None, 1, 63, 64, 65, 4999))
def test_ids_follow_first_appearance_whatever_the_calls(pp, ctx, source, split):
    names = nm.order_case()
    want = _first_appearance(names)
    assert int(want.max()) == 1199
    if split is None:       # one call: twice, and with a table sized for a million names
        for expect in (0, 0, 10 ** 6):
            (got,), table = run(pp, ctx, [nm.pack(names, lead=5)], source, expect)
            table.close()
            assert np.array_equal(got, want)
        return
    # calls of `split` names each (up to 5,000 calls): slices of ONE array, uploaded once on the device path
    whole, n = nm.pack(names, lead=5), len(names)
    table, got = pp.Names(ctx), []
    try:
        if source == "device":
            (bp, op, lp, out), keep = to_device(whole)
        for i in range(0, n, split):
            m = min(split, n - i)
            if source == "host":
                got.append(table.ids((whole[0], whole[1][i:i + m], whole[2][i:i + m])))
            else:
                got.append(table.ids((bp, op + 8 * i, lp + 4 * i), mem=pp.MEM_DEVICE, n=m, n_bytes=len(whole[0]), out=out + 8 * i))
        assert np.array_equal(np.concatenate(got), want) and table.count == 1200
    finally:
        table.close()


@pytest.mark.parametrize("source", SOURCES)
def test_4096_copies_of_one_name(pp, ctx, source):
    names = nm.contention_case()
    (got,), table = run(pp, ctx, [nm.pack(names)], source)
    try:
        assert got[:3].tolist() == [0, 1, 2] and (got[3:] == 3).all() and len(got) == 4099 and table.count == 4
    finally:
        table.close()


@pytest.mark.parametrize("source", SOURCES)
def test_more_names_than_one_sweep_of_the_lookup_kernel(pp, ctx, source):
    # k_nm_lookup's workgroups stride over the names: past LOOKUP_SWEEP a lane takes a second name (and its misses add up)
    n = nm.LOOKUP_SWEEP + 70001
    call, want = nm.numbered_case(n, 150000)
    table = pp.Names(ctx)
    try:
        got = query(pp, table, call, source)                    # misses in both sweeps
        assert np.array_equal(got, want) and table.count == int(want.max()) + 1
        assert np.array_equal(query(pp, table, call, source), want)     # hits in both sweeps
    finally:
        table.close()


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("n", (1023, 1024, 1025))
def test_distinct_new_names_around_one_workgroup_of_the_rank_scan(pp, ctx, source, n):
    # k_nm_rank ranks 1,024 names per workgroup (block_scan_excl64<NM_BLOCK>): the new representatives end one short of a
    # workgroup, fill it, and reach into a second one whose base is the column scan's
    call = nm.pack([b"seam_%d" % i for i in range(n)], lead=3)
    (got, again), table = run(pp, ctx, [call, call], source)
    try:
        assert got.tolist() == list(range(n)) and table.count == n
        assert np.array_equal(again, got)
    finally:
        table.close()


@pytest.mark.parametrize("source", SOURCES)
def test_more_workgroups_than_the_column_scan_has_threads(pp, ctx, source):
    # 1,025 workgroups of k_nm_rank: the smallest call at which a thread of the one-workgroup column scan owns two rows of
    # sums (and the threads from 513 on none)
    call, want = nm.numbered_case(1024 * 1024 + 1, 300000)
    table = pp.Names(ctx)
    try:
        got = query(pp, table, call, source)
        assert np.array_equal(got, want) and table.count == int(want.max()) + 1
        assert np.array_equal(query(pp, table, call, source), want) and table.count == int(want.max()) + 1
    finally:
        table.close()


@pytest.mark.parametrize("source", SOURCES)
def test_the_table_grows_and_the_ids_stay(pp, ctx, source):
    calls = [nm.pack(c, lead=1) for c in nm.growth_calls()]
    table, state = pp.Names(ctx, 0), {}
    try:
        first = None
        for call in calls:                                      # 5,000 new names each: 1,024 slots become 65,536
            (got,), _ = run(pp, ctx, [call], source, state=state, table=table)
            first = got if first is None else first
            assert np.array_equal(query(pp, table, calls[0], source), first)        # the first call's names keep the first call's ids
        assert table.count == 20000 and first.tolist() == list(range(5000))
        by_id = {v: k for k, v in state.items()}
        rng = np.random.default_rng(3)
        for i in [0, 19999] + rng.integers(0, 20000, 50).tolist():
            assert table.name(i) == by_id[i], i
    finally:
        table.close()


@pytest.mark.parametrize("source", SOURCES)
def test_the_table_keeps_its_own_copy_of_the_bytes(pp, ctx, source):
    names = nm.order_case(seed=12, n=700, distinct=300)
    call = nm.pack(names, lead=2)
    table = pp.Names(ctx)
    try:
        if source == "host":
            want = table.ids(call)
            call[0][:] = 0                                      # the caller's array may be overwritten when the call has returned
        else:
            (bp, op, lp, out), keep = to_device(call)
            want = table.ids((bp, op, lp), mem=pp.MEM_DEVICE, n=len(call[1]), n_bytes=len(call[0]), out=out)
            import torch
            keep[0].zero_()
            torch.cuda.synchronize()
        assert np.array_equal(want, _first_appearance(names)) and table.count == 300
        got = query(pp, table, nm.pack(names, lead=7), source)  # the same strings from a fresh array
        assert np.array_equal(got, want) and table.count == 300
    finally:
        table.close()


def test_two_tables_on_one_context_and_a_polish_job_between_two_calls(pp, ctx):
    a, b = pp.Names(ctx), pp.Names(ctx, 100)
    try:
        assert a.ids([b"x", b"y", "z"]).tolist() == [0, 1, 2]
        assert b.ids([b"z", b"y"]).tolist() == [0, 1] and (a.count, b.count) == (3, 2)       # they do not see each other
        contig_off, bases, recs = synth.fast_records(seed=5, contig_lens=(6000,), coverage=20, read_len=150)
        want = ctx.polish_records(contig_off, bases, recs)["polished"]
        assert a.ids(["w", "z", "x"]).tolist() == [3, 2, 0] and b.ids([b"x", b"z"]).tolist() == [2, 0]
        assert ctx.polish_records(contig_off, bases, recs)["polished"] == want
        assert (a.name(3), b.name(2), a.count, b.count) == (b"w", b"x", 4, 3)
    finally:
        a.close()
        b.close()


# ---- the contract -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("source", SOURCES)
def test_a_range_outside_the_array_is_an_argument_error_and_changes_nothing(pp, ctx, source):
    names = [b"good_%d" % i for i in range(100)]
    table = pp.Names(ctx)
    try:
        assert table.ids([b"resident", names[70]]).tolist() == [0, 1]
        good = nm.pack(names, lead=3)
        for off, ln in ((len(good[0]) - 4, 5), (U64_MAX, 2), (1 << 63, 1), (len(good[0]) + 1, 1)):      # one past the end | a sum that wraps
            call = (good[0], good[1].copy(), good[2].copy())
            call[1][50], call[2][50] = off, ln
            with pytest.raises(pp.PolypolishError) as e:
                query(pp, table, call, source)
            assert e.value.code == ARG and e.value.bad == 50, str(e.value)
            assert table.count == 2
        call = (good[0], good[1].copy(), good[2].copy())        # of several defects the first index is named
        call[1][[20, 80]] = U64_MAX
        with pytest.raises(pp.PolypolishError) as e:
            query(pp, table, call, source)
        assert e.value.bad == 20 and table.count == 2
        # the good names in front of the defect were not inserted: they get their ids now, in their order
        want = [i + 2 if i < 70 else (1 if i == 70 else i + 1) for i in range(100)]
        assert query(pp, table, good, source).tolist() == want and table.count == 101
        # an empty name reads nothing: its offset is nobody's business
        call = (good[0], np.array([U64_MAX, 0], np.uint64), np.array([0, 0], np.uint32))
        assert query(pp, table, call, source).tolist() == [101, 101]
    finally:
        table.close()


def test_argument_errors(pp, ctx):
    L = pp.lib()
    table = pp.Names(ctx)
    try:
        b, off, ln = nm.pack([b"abc", b"de"])
        ids = np.zeros(2, np.uint64)
        args = (b.ctypes.data, len(b), off.ctypes.data, ln.ctypes.data, 2)
        assert L.pp_names_ids(table._p, *args, pp.MEM_HOST, None, None, None) == ARG                     # neither id64 nor id32
        assert L.pp_names_ids(table._p, *args, pp.MEM_PEER, ids.ctypes.data, None, None) == ARG
        assert L.pp_names_ids(table._p, b.ctypes.data, len(b), None, ln.ctypes.data, 2, pp.MEM_HOST, ids.ctypes.data, None, None) == ARG
        assert L.pp_names_ids(table._p, b.ctypes.data, len(b), off.ctypes.data, None, 2, pp.MEM_HOST, ids.ctypes.data, None, None) == ARG
        assert L.pp_names_ids(table._p, None, len(b), off.ctypes.data, ln.ctypes.data, 2, pp.MEM_HOST, ids.ctypes.data, None, None) == ARG
        assert L.pp_names_ids(None, *args, pp.MEM_HOST, ids.ctypes.data, None, None) == ARG
        assert table.count == 0
        for mem in (pp.MEM_HOST, pp.MEM_DEVICE):                                                          # n == 0 with null arrays
            assert L.pp_names_ids(table._p, None, 0, None, None, 0, mem, None, None, None) == 0
        assert table.count == 0
        # id32 alone, and both: the same values
        id32, both64, both32 = np.zeros(2, np.uint32), np.zeros(2, np.uint64), np.zeros(2, np.uint32)
        assert L.pp_names_ids(table._p, *args, pp.MEM_HOST, None, id32.ctypes.data, None) == 0
        assert L.pp_names_ids(table._p, *args, pp.MEM_HOST, both64.ctypes.data, both32.ctypes.data, None) == 0
        assert id32.tolist() == both64.tolist() == both32.tolist() == [0, 1] and table.count == 2
        # pp_names_name
        out, n = np.zeros(8, np.uint8), C.c_uint32(77)
        assert L.pp_names_name(table._p, 2, out.ctypes.data, 8, C.byref(n)) == ARG                        # id == count
        assert L.pp_names_name(table._p, 0, out.ctypes.data, 2, C.byref(n)) == ARG and n.value == 3      # cap one short: *len is set
        assert L.pp_names_name(table._p, 0, out.ctypes.data, 3, C.byref(n)) == 0 and out[:3].tobytes() == b"abc" and n.value == 3
        assert L.pp_names_name(table._p, 0, out.ctypes.data, 3, None) == ARG
        assert L.pp_names_create(ctx._h, 0, None) == ARG and L.pp_names_count(None) == 0
        L.pp_names_free(None)
    finally:
        table.close()


def test_kernel_ms_needs_profiling(pp, ctx):
    L, ms = pp.lib(), C.c_float(-1.0)
    table = pp.Names(ctx)
    try:
        table.ids([b"a", b"b"])
        assert L.pp_names_kernel_ms(table._p, C.byref(ms)) == ARG
    finally:
        table.close()
    c = pp.Context(0)
    try:
        c.set_profiling(True)
        table = pp.Names(c)
        for names in (nm.order_case(), nm.order_case()):            # inserts and a growth | hits alone
            table.ids(names)
            assert 0.0 < table.kernel_ms() < 1000.0
        table.close()
    finally:
        c.close()
