"""pp_shard_split / pp_shard_count on the GPU (pp_shard_dev.hip: k_split_flag / k_split_place / k_split_meta / k_split_seq /
k_split_cigar / k_split_wo_flag / k_split_wo / k_contig_hist and the scans of pp_dev.h) against the plain model of
tests/shard_model.py, which tests/test_shard_model_cpu.py pins to hand-computed answers and to the host loop.  Every rank's part
of every case is downloaded and compared with the model with exact equality; nothing here is compared with the host loop
(tests/test_gpu_parity.py does that).  Device inputs are torch tensors exactly as long as the arrays.  Needs an MI355X: `-m gpu`."""
import functools
import os
import subprocess

import numpy as np
import pytest

import shard_model as sm
import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
def plan(pp):
    return sm.seam_plan(pp)


def to_device(recs):
    """the batch's arrays (and its mirror) as tensors of exactly their sizes -> (addresses, tensors to keep)"""
    import torch
    dev = torch.device("cuda:0")
    as_int = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32, np.dtype(np.uint8): np.uint8}
    t = {k: torch.from_numpy(np.ascontiguousarray(recs[k], dtype=dt).view(as_int[np.dtype(dt)])).to(dev) for k, dt in sm.FIELDS}
    if "wo" in recs:
        t["wo"] = torch.from_numpy(np.ascontiguousarray(recs["wo"]).view(np.uint8)).to(dev)
    torch.cuda.synchronize()
    ptrs = {k: v.data_ptr() for k, v in t.items()}
    if "wo" in recs and recs.get("wo_runs") is not None:
        ptrs["wo_runs"] = recs["wo_runs"]
    return ptrs, t


def read_part(ctx, part):
    """a device part, downloaded: (batch dict with "seq4", "wo" / "wo_runs" when the part has them, orig)"""
    sizes = {"seq": part.seq_bytes, "cigar": part.n_cig_total}
    got = {name: ctx.download(part.ptrs[name], sizes.get(name, part.n_aln), dt) for name, dt in sm.FIELDS}
    got["seq4"] = ctx.download(part.ptrs.get("seq4"), part.seq_bytes // 2, np.uint8)
    if "wo" in part.ptrs:
        got["wo"] = ctx.download(part.ptrs["wo"], part.n_aln, sm.WO_DTYPE)
    if "wo_runs" in part.ptrs:
        got["wo_runs"] = part.ptrs["wo_runs"]
    return got, ctx.download(part.orig_ptr, part.n_aln, np.uint32)


def without_mirror(want):
    return {k: v for k, v in want.items() if k not in ("wo", "wo_runs")}


def device_agrees(pp, ctx, plan, recs, what, wo_idx_base=0, world=sm.WORLD, want=None):
    """every rank's part, split from device memory, against the model (want: the model's parts where the caller has them)"""
    ptrs, keep = to_device(recs)
    sizes = []
    for r in range(world):
        want_part, want_orig = want[r] if want else sm.split(plan, r, recs, wo_idx_base)
        part = pp.ShardPart(ctx, plan, r, len(recs["contig"]), ptrs, len(recs["seq"]), len(recs["cigar"]), pp.MEM_DEVICE, wo_idx_base)
        try:  # (a part must not outlive its context, not even in the traceback of a failed assertion)
            counts = (part.n_aln, part.seq_bytes, part.n_cig_total)
            has_seq4 = "seq4" in part.ptrs
            got, got_orig = read_part(ctx, part)
        finally:
            part.close()
        assert counts == (len(want_orig), len(want_part["seq"]), len(want_part["cigar"])), (what, r)
        assert has_seq4 or not counts[0], (what, r)
        sm.assert_part(got, got_orig, want_part, want_orig, (what, "rank", r), seq4=True)
        sizes.append(counts[0])
    del keep
    return sizes


def mirrored(recs):
    return dict(recs, wo=sm.mirror(recs), wo_runs=np.array([len(recs["contig"])], dtype=np.uint64))


@functools.lru_cache(maxsize=None)
def size_case(pp, n):
    """case B at n records, with a mirror, and the model's parts (worked out once)"""
    recs = sm.size_batch(n)
    if n:
        recs = mirrored(recs)
    plan = sm.seam_plan(pp)
    return recs, [sm.split(plan, r, recs) for r in range(sm.WORLD)]


def test_case_a_the_seam_batch(pp, ctx, plan):
    recs, _ = sm.seam_batch()
    device_agrees(pp, ctx, plan, recs, "seam")
    device_agrees(pp, ctx, plan, mirrored(recs), "seam with a mirror")


@pytest.mark.parametrize("n", sm.SIZES)
def test_case_b_sizes(pp, ctx, plan, n):
    recs, want = size_case(pp, n)
    assert sum(device_agrees(pp, ctx, plan, recs, n, want=want)) >= n


def test_case_b_one_context_large_small_large(pp, plan):
    """the context's split scratch is grow-only (slots, flags, the mirror's positions): a small split after a large one and
    a large one after that see what the earlier calls left there"""
    c = pp.Context(0)
    try:
        for n, mirror in ((16385, True), (1, True), (257, False), (16385, False), (8193, True), (255, True), (16385, True)):
            recs, want = size_case(pp, n)
            if not mirror:
                recs, want = without_mirror(recs), [(without_mirror(p), o) for p, o in want]
            device_agrees(pp, c, plan, recs, (n, mirror), want=want)
    finally:
        c.close()


def test_case_b_one_rank_takes_everything_and_a_rank_may_take_nothing(pp, ctx, plan):
    recs = sm.size_batch(257)
    one = pp.Plan(sm.CONTIG_OFF, [200, 20, 20, 17], 1, sm.MIN_WINDOW)
    for src in (recs, mirrored(recs)):
        assert device_agrees(pp, ctx, one, src, "world 1", world=1) == [257]
    rows = [r for r in sm.random_rows(400, 11) if r[0] == 0 and r[1] + 120 < 2048]   # window 0 of contig 0 only
    recs = sm.batch(rows)
    for src in (recs, mirrored(recs)):
        assert sorted(device_agrees(pp, ctx, plan, src, "a rank without records")) == [0, 0, len(rows)]


@pytest.mark.parametrize("case", range(9))
def test_case_c_seq_layouts(pp, ctx, plan, case):
    name, recs = sm.layout_cases()[case]
    device_agrees(pp, ctx, plan, recs, name)
    device_agrees(pp, ctx, plan, mirrored(recs), (name, "with a mirror"))


@pytest.mark.parametrize("case", range(9))
def test_case_d_mirrors(pp, ctx, plan, case):
    name, recs, base = sm.mirror_cases()[case]
    device_agrees(pp, ctx, plan, recs, name, wo_idx_base=base)


@pytest.mark.parametrize("n_contigs", sm.COUNT_CONTIGS)
@pytest.mark.parametrize("n", sm.COUNT_SIZES)
def test_case_e_count(pp, ctx, n, n_contigs):
    import torch
    contig, before = sm.count_case(n, n_contigs)
    want = sm.count(contig.tolist(), n_contigs, [int(x) for x in before])
    t = torch.from_numpy(contig.view(np.int32)).to("cuda:0")
    torch.cuda.synchronize()
    got = pp.shard_count(ctx, n, t.data_ptr(), pp.MEM_DEVICE, n_contigs, into=before.copy())
    assert [int(x) for x in got] == want


# ---- what the partition is for: a rank's part and its emit ranges give the bytes all records give ----------------------------------

def polish_part(pp, ctx, contig_off, bases_t, part, emit):
    ctx.polish_begin(contig_off, bases_t.data_ptr(), pp.MEM_DEVICE, 5, 0.5, 0.2)
    ctx.set_emit(emit)
    ctx.polish_add_ptrs(part.n_aln, part.ptrs, part.seq_bytes, part.n_cig_total, pp.MEM_DEVICE)
    ctx.polish_finish()
    polished, offs, _ = ctx.result()
    return polished, offs


def test_parts_at_the_seam_read_lengths_polish_to_the_oracles_bytes(pp, ctx, orc):
    """one valid job of reads of 33, 128 and 257 bases (one trip of k_split_seq's lanes and a partial chunk; exactly one full
    trip; a second trip and a third), indel reads among them, a tiled contig and three ranks: polishing the device part with the
    rank's emit ranges gives the bytes the oracle gives for ALL records with those ranges -- from the records alone and with
    a faithful mirror made elsewhere"""
    import torch
    lens = (30_000, 700, 3_000)
    jobs = [synth.fast_records(seed=41, contig_lens=lens, coverage=8, read_len=L, k_choices=(1, 2, 3), k_probs=(0.8, 0.1, 0.1),
                               indel_read_frac=0.2) for L in (33, 128, 257)]
    contig_off, bases = jobs[0][0], jobs[0][1]
    assert all(np.array_equal(j[1], bases) for j in jobs)
    recs = synth.merge_records(synth.merge_records(jobs[0][2], jobs[1][2], seed=1), jobs[2][2], seed=2)
    n = len(recs["contig"])
    plan = pp.Plan(contig_off, np.bincount(recs["contig"], minlength=3), 3, 2048)
    assert (plan.unit_contig == 0).sum() == 3, "the large contig is tiled"
    eng = synth.oracle_engine(orc)
    want = [eng(contig_off, bases, recs, emit=plan.emit_ranges(r)) for r in range(3)]
    bases_t = torch.from_numpy(np.ascontiguousarray(bases, dtype=np.uint8)).to("cuda:0")
    for src in (recs, dict(recs, wo=pp.window_order_mirror(recs, contig_off), wo_runs=np.array([n], dtype=np.uint64))):
        ptrs, keep = to_device(src)
        for r in range(3):
            part = pp.ShardPart(ctx, plan, r, n, ptrs, len(recs["seq"]), len(recs["cigar"]), pp.MEM_DEVICE)
            try:
                has_wo, n_part = "wo" in part.ptrs, part.n_aln
                polished, offs = polish_part(pp, ctx, contig_off, bases_t, part, plan.emit_ranges(r))
            finally:
                part.close()
            assert has_wo == ("wo" in src) and 0 < n_part < n
            assert polished == want[r]["polished"] and np.array_equal(offs, want[r]["offsets"]), (r, "wo" in src)
        del keep


def test_a_foreign_mirror_stays_foreign_through_the_split():
    """A caller's mirror that does not mirror its records (a wrong k, a moved ref_start, one record named twice and another
    never: the kinds of test_a_foreign_window_order_mirror_is_checked_before_it_is_used that leave seq_off / seq_len alone)
    comes out of pp_shard_split restricted, entry for entry -- the split copies entries, it does not look at the records.  The
    part's mirror must then be as foreign as the source's: the polish compares it with the arrays and leaves it aside (a
    faithful one stands the comparison), and every rank's part with its emit ranges still gives the oracle's bytes -- device parts and host parts alike."""
    code = """
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import torch, synth, polypolish_amd as pp
import test_shard_split_gpu as ts
from oracle import orc
ctx = pp.Context(0)
o, b, r = synth.fast_records(seed=2, contig_lens=(40_000, 7_000), coverage=40, indel_read_frac=0.2)
n = len(r["contig"])
plan = pp.Plan(o, np.bincount(r["contig"], minlength=2), 3, 2048)
assert (plan.unit_contig == 0).sum() == 3
eng = synth.oracle_engine(orc)
want = [eng(o, b, r, emit=plan.emit_ranges(rank)) for rank in range(3)]
bt = torch.from_numpy(np.ascontiguousarray(b, dtype=np.uint8)).to("cuda:0")
for kind in ("faithful", "k", "ref_start", "twice"):
    w = pp.window_order_mirror(r, o)
    if kind == "k": w["k"][3] += 1
    if kind == "ref_start":
        j = int(np.flatnonzero((w["contig"] == 0) & (w["ref_start"] > 5000) & (w["ref_start"] < 6000))[0])   # an interior read
        w["ref_start"][j] += 1
    if kind == "twice": w["file_idx"][7] = w["file_idx"][8]
    src = dict(r, wo=w, wo_runs=np.array([n], dtype=np.uint64))
    ptrs, keep = ts.to_device(src)
    directs = []
    for rank in range(3):
        emit = plan.emit_ranges(rank)
        part = pp.ShardPart(ctx, plan, rank, n, ptrs, len(r["seq"]), len(r["cigar"]), pp.MEM_DEVICE)
        polished, offs = ts.polish_part(pp, ctx, o, bt, part, emit)
        direct = ctx.took_direct_path()
        part.close()
        assert polished == want[rank]["polished"] and np.array_equal(offs, want[rank]["offsets"]), (kind, rank, "device part")
        directs.append(direct)
        got = ctx.polish_records(o, b, pp.shard_split_host(plan, rank, src)[0], emit=emit)
        assert got["polished"] == want[rank]["polished"] and np.array_equal(got["offsets"], want[rank]["offsets"]), (kind, rank, "host part")
    del keep
    assert kind == "faithful" or not all(directs), (kind, directs)   # the rank that was handed the wrong entry left it aside
print("split mirrors ok")
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run(["python", "-c", code], capture_output=True, env=dict(os.environ), timeout=600)
    assert r.returncode == 0 and b"split mirrors ok" in r.stdout, r.stderr.decode()[-2000:]
