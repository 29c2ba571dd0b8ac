"""Parity tests proper: the HIP path (through the C ABI) against the CPU oracle on the same seeded
inputs.  Bit-exact everywhere: polished bytes, contig offsets, per-position f64 depth, counters,
thresholds and vote status; filtered SAM bytes; CLI stdout.  Needs an MI355X: `-m gpu`."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import synth
from layout_check import check_seq4_mirror, check_seq_layout, check_window_order_mirror, same_ingest, same_records

pytestmark = pytest.mark.gpu
C_u64 = ctypes.c_uint64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POS_KEYS = ("depth", "count_a", "count_c", "count_g", "count_t", "count_other", "valid_thr", "invalid_thr", "status")


@pytest.fixture(scope="module")
def pp():
    import polypolish_amd
    return polypolish_amd


@pytest.fixture(scope="module")
def ctx(pp):
    c = pp.Context(0)
    yield c
    c.close()


def _seqs(fasta_bytes):
    return [l for l in fasta_bytes.decode().split("\n") if l and not l.startswith(">")]


def _polish_device_batch(ctx, pp, contig_off, bases, recs, seq4, positions=False, min_depth=5, fraction_valid=0.5,
                         fraction_invalid=0.2, wo=None, emit=None):
    """The records as ONE device-resident batch that is polished in place (what the device tokenizer hands over), with or
    without the 4-bit mirror of the seq array (pp_aln_batch.seq4) and the window-order mirror of the records
    (pp_aln_batch.wo; wo = True: as the host ingest orders it, "shuffled": the same entries in a random order -- the mirror
    is a hint, any permutation of the records must give the same results)."""
    import torch
    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(np.ascontiguousarray(recs[k], dtype=dt)).to(dev) for k, dt in pp.REC_FIELDS}
    tb = torch.from_numpy(np.ascontiguousarray(bases, dtype=np.uint8)).to(dev)
    ptrs = {k: v.data_ptr() for k, v in t.items()}
    if seq4:
        mirror = torch.from_numpy(pp.pack_seq4(recs["seq"])).to(dev)
        ptrs["seq4"] = mirror.data_ptr()
    if wo:
        w = pp.window_order_mirror(recs, contig_off)
        if wo == "shuffled":
            w = w[np.random.default_rng(len(w)).permutation(len(w))]
        wt = torch.from_numpy(np.ascontiguousarray(w).view(np.uint8)).to(dev)
        ptrs["wo"] = wt.data_ptr()
        # the mirror's run table (pp_aln_batch.wo_run_end): with it the job takes the DIRECT path (k_tile reads the bulk of
        # the records straight from the mirror, pp_k_direct.h); "shuffled" claims one run and is none -- the device notices
        # and the job falls back to the bucketing path; "no_runs": the mirror alone (rounds 4's path through k_prep / k_fill)
        if wo != "no_runs" and len(w):
            ptrs["wo_runs"] = [len(w)]
    torch.cuda.synchronize()
    pp.lib().pp_polish_set_debug(ctx._h, int(positions))
    try:
        ctx.polish_begin(contig_off, tb.data_ptr(), pp.MEM_DEVICE, min_depth, fraction_valid, fraction_invalid)
        if emit is not None:
            ctx.set_emit(emit)
        ctx.polish_add_ptrs(len(recs["contig"]), ptrs, len(recs["seq"]), len(recs["cigar"]), pp.MEM_DEVICE)
        ctx.polish_finish()
        polished, offs, stats = ctx.result()
        res = {"polished": polished, "offsets": offs, "stats": stats, "positions": ctx.positions() if positions else None}
    finally:
        pp.lib().pp_polish_set_debug(ctx._h, 0)
    return res


def _compare_records(ctx, orc, contig_off, bases, recs, **kw):
    want = orc.polish_records(contig_off, bases, recs, positions=True, **kw)
    got = ctx.polish_records(contig_off, bases, recs, positions=True, **kw)
    for k in POS_KEYS:
        bad = np.nonzero(want["positions"][k] != got["positions"][k])[0]
        assert len(bad) == 0, (k, len(bad), bad[:8], want["positions"][k][bad[:8]], got["positions"][k][bad[:8]])
    assert np.array_equal(got["offsets"], want["offsets"]), (got["offsets"], want["offsets"])
    assert got["polished"] == want["polished"]
    st = want["positions"]["status"]
    off = [int(x) for x in contig_off]
    for c in range(len(off) - 1):
        assert got["stats"][c]["changed"] == int((st[off[c]:off[c + 1]] == 1).sum())
        assert got["stats"][c]["zero_depth"] == int((want["positions"]["depth"][off[c]:off[c + 1]] == 0.0).sum())
        # the contig's depth sum (mean read depth of the log, polish.rs:173-180,206-227): shares 1/2^j are summed exactly,
        # other shares through the ordered replay, each position rounded to 2^-10
        dsum = float(want["positions"]["depth"][off[c]:off[c + 1]].sum())
        assert abs(got["stats"][c]["depth_sum"] - dsum) <= (off[c + 1] - off[c]) * 2.0 ** -11 + 1e-6 * dsum, (c, got["stats"][c], dsum)
    # without the per-position debug planes the same bytes must come out (different flagging rule; positions where
    # nothing was tallied explicitly skip the vote proper) -- and the same per-contig figures
    plain = ctx.polish_records(contig_off, bases, recs, positions=False, **kw)
    assert plain["polished"] == want["polished"] and np.array_equal(plain["offsets"], want["offsets"])
    for c in range(len(off) - 1):
        assert plain["stats"][c]["changed"] == got["stats"][c]["changed"], c
        assert plain["stats"][c]["zero_depth"] == got["stats"][c]["zero_depth"], c
        dsum = float(want["positions"]["depth"][off[c]:off[c + 1]].sum())
        assert abs(plain["stats"][c]["depth_sum"] - dsum) <= (off[c + 1] - off[c]) * 2.0 ** -11 + 1e-6 * dsum, (c, plain["stats"][c], dsum)
    # the same records as one device batch with the 4-bit mirror of the seq array (the plain class then reads nibbles):
    # per position with the debug planes, bytes and figures without
    if len(recs["contig"]):
        import polypolish_amd as pp
        m = _polish_device_batch(ctx, pp, contig_off, bases, recs, True, positions=True, **kw)
        for k in POS_KEYS:
            bad = np.nonzero(want["positions"][k] != m["positions"][k])[0]
            assert len(bad) == 0, ("seq4", k, len(bad), bad[:8], want["positions"][k][bad[:8]], m["positions"][k][bad[:8]])
        assert m["polished"] == want["polished"]
        m = _polish_device_batch(ctx, pp, contig_off, bases, recs, True, positions=False, **kw)
        assert m["polished"] == want["polished"] and np.array_equal(m["offsets"], want["offsets"])
        for c in range(len(off) - 1):
            assert m["stats"][c]["changed"] == got["stats"][c]["changed"], ("seq4", c)
            assert m["stats"][c]["zero_depth"] == got["stats"][c]["zero_depth"], ("seq4", c)
        # ... and WITHOUT the mirror (a foreign device batch polished in place: the lane-group plain class over the bytes;
        # host batches -- ctx.polish_records above -- get a mirror packed on the device since round 4)
        m = _polish_device_batch(ctx, pp, contig_off, bases, recs, False, positions=True, **kw)
        for k in POS_KEYS:
            bad = np.nonzero(want["positions"][k] != m["positions"][k])[0]
            assert len(bad) == 0, ("bytes", k, len(bad), bad[:8], want["positions"][k][bad[:8]], m["positions"][k][bad[:8]])
        assert m["polished"] == want["polished"]
        m = _polish_device_batch(ctx, pp, contig_off, bases, recs, False, positions=False, **kw)
        assert m["polished"] == want["polished"] and np.array_equal(m["offsets"], want["offsets"])
        # ... and with the window-order mirror of the records (pp_aln_batch.wo): k_prep and k_fill then walk the records
        # through it (gstart / nkeep in mirror order, items numbered by file index, one histogram / cursor update per wave and
        # window), per position with the debug planes and bytes without -- as the ingests order it, and in a random order
        # ... with its run table (the DIRECT path of round 5: k_tile takes the bulk of the records straight from the mirror, the
        # others and the reads that reach into the next window as extras), with the 4-bit mirror (one lane per read) and without
        # (lane groups); in a random order under a run table that is then wrong (the device notices, the job falls back to
        # the bucketing path); and without a run table (round 4's path)
        for order, s4 in ((True, True), (True, False), ("shuffled", False), ("no_runs", True)):
            m = _polish_device_batch(ctx, pp, contig_off, bases, recs, s4, positions=True, wo=order, **kw)
            for k in POS_KEYS:
                bad = np.nonzero(want["positions"][k] != m["positions"][k])[0]
                assert len(bad) == 0, ("wo", order, k, len(bad), bad[:8], want["positions"][k][bad[:8]], m["positions"][k][bad[:8]])
            assert m["polished"] == want["polished"]
            m = _polish_device_batch(ctx, pp, contig_off, bases, recs, s4, positions=False, wo=order, **kw)
            assert m["polished"] == want["polished"] and np.array_equal(m["offsets"], want["offsets"])
            for c in range(len(off) - 1):
                assert m["stats"][c]["changed"] == got["stats"][c]["changed"], ("wo", order, c)
        # What the pileup kernel decides BY ITSELF (debug level 3): a position with depth shares that are not a multiple of
        # the window's fixed-point unit is voted from the interval its depth is known to lie in, and only replayed in
        # file order where a step of the vote (pileup.rs:70-72,114) falls inside it.  Tallies, both thresholds and the
        # status must be the oracle's at EVERY position; the depth of the positions decided that way is the fixed-point
        # one, within reads * 2^-11 of the exact sum (a window's unit is 2^-10 at the coarsest).
        for mirror, order in ((True, None), (False, None), (True, True)):   # (the last one: the direct path)
            m = _polish_device_batch(ctx, pp, contig_off, bases, recs, mirror, positions=3, wo=order, **kw)
            for k in POS_KEYS:
                if k == "depth":
                    continue
                bad = np.nonzero(want["positions"][k] != m["positions"][k])[0]
                assert len(bad) == 0, ("interval", mirror, order, k, len(bad), bad[:8], want["positions"][k][bad[:8]], m["positions"][k][bad[:8]])
            p = want["positions"]
            reads = (p["count_a"].astype(np.int64) + p["count_c"] + p["count_g"] + p["count_t"] + p["count_other"]).astype(np.float64)
            err = np.abs(m["positions"]["depth"] - p["depth"])
            assert (err <= reads * 2.0 ** -11 + 1e-9).all(), ("interval depth", mirror, float(err.max()))
            assert m["polished"] == want["polished"]
    return want, got


RECORD_CASES = {
    "plain_k1": dict(seed=1, contig_lens=(60_000,), coverage=60, indel_read_frac=0.0),
    "indels": dict(seed=2, contig_lens=(40_000, 7_000), coverage=80, indel_read_frac=0.2, n_rate=0.003),
    "dyadic_k": dict(seed=3, contig_lens=(30_000,), coverage=60, k_choices=(1, 2, 4, 8), indel_read_frac=0.02),
    "nondyadic_k": dict(seed=4, contig_lens=(30_000, 2_500), coverage=50, k_choices=(1, 2, 3, 5, 6, 7),
                        k_probs=(0.5, 0.1, 0.1, 0.1, 0.1, 0.1), indel_read_frac=0.05),
    "all_k3": dict(seed=5, contig_lens=(9_000,), coverage=40, k_choices=(3,)),
    "low_depth": dict(seed=6, contig_lens=(50_000,), coverage=6, indel_read_frac=0.05, n_rate=0.01),
    "tiny_contigs": dict(seed=7, contig_lens=(300, 2048, 2049, 500, 4096, 1000), coverage=40, read_len=100,
                         indel_read_frac=0.05),
    "long_reads": dict(seed=8, contig_lens=(40_000,), coverage=30, read_len=5000, indel_read_frac=0.3,
                       sub_rate=0.0005),
    "many_N": dict(seed=9, contig_lens=(20_000,), coverage=30, n_rate=0.2),
    "big_k": dict(seed=10, contig_lens=(20_000,), coverage=40, k_choices=(1, 1024, 2048, 4096, 1000)),
    # every read has an indel: more non-bulk records per block of k_prep than its LDS list holds (they are then handled
    # on the spot), and k_tile's register path for short CIGARs on every item
    "all_indels": dict(seed=11, contig_lens=(60_000,), coverage=100, indel_read_frac=1.0, k_choices=(1, 2, 3)),
    # 5000 contigs: three rounds of the wave's 64-ary contig search, windows that span a dozen contigs
    "many_contigs": dict(seed=12, contig_lens=(300,) * 4990 + (2048, 2049, 4096, 700, 301, 5000, 333, 4097, 310, 999),
                         coverage=25, read_len=100, indel_read_frac=0.05, k_choices=(1, 1, 3)),
}


@pytest.mark.parametrize("name", list(RECORD_CASES))
def test_polish_records_parity(ctx, orc, name):
    contig_off, bases, recs = synth.fast_records(**RECORD_CASES[name])
    want, _ = _compare_records(ctx, orc, contig_off, bases, recs)
    if name in ("plain_k1", "indels"):
        assert (want["positions"]["status"] == 1).sum() > 0
    _compare_records(ctx, orc, contig_off, bases, recs, min_depth=1, fraction_valid=0.6, fraction_invalid=0.05)
    if name in ("nondyadic_k", "all_k3", "big_k"):
        # nearly every position of these jobs has an order-dependent depth: the interval test must settle almost all of
        # them in k_tile (until round 4 every one of them was replayed in file order)
        ctx.set_profiling(1)
        try:
            ctx.polish_records(contig_off, bases, recs)
            replayed = ctx.kernel_times()["n_flagged"]
        finally:
            ctx.set_profiling(0)
        odd = np.isin(recs["k"], (3, 5, 6, 7, 1000, 2048, 4096)).sum()
        # (with k = 3 for every read depth * 0.5 = reads / 6 is an exact .5 at one position in six: there the order of the
        # additions decides the rounding -- but the vote only depends on it where a tally sits exactly on that threshold)
        assert odd > 0 and replayed < 0.03 * int(contig_off[-1]), (name, replayed, int(contig_off[-1]))


@pytest.mark.parametrize("read_len", [12, 31, 33, 160, 161, 192, 193, 250, 252, 253])
def test_read_lengths_across_the_lane_group_widths(ctx, orc, read_len):
    """k_tile sizes its lane groups from the longest fast-class read of the job: 5 lanes x 32 B up to 160
    bases, 6 up to 192, 8 up to 252; longer reads take the slow class.  Every boundary, with a few indels,
    Ns and non-dyadic shares in the mix."""
    contig_off, bases, recs = synth.fast_records(seed=100 + read_len, contig_lens=(12_000, 2_300), coverage=40,
                                                 read_len=read_len, indel_read_frac=0.05, n_rate=0.003,
                                                 k_choices=(1, 1, 1, 2, 3))
    _compare_records(ctx, orc, contig_off, bases, recs)


def _repitch(recs, pitch, lead=0):
    """The same records with every read's bases at lead + i * pitch of a new seq array (the gaps hold a base that differs
    from its neighbours, so that a compare that looks one base too far is seen)."""
    n, L = len(recs["contig"]), int(recs["seq_len"][0])
    assert (recs["seq_len"] == L).all() and pitch >= L
    old = recs["seq"].reshape(n, L)
    seq = np.full(lead + n * pitch + 64, ord("T"), dtype=np.uint8)
    view = seq[lead:lead + n * pitch].reshape(n, pitch)
    view[:, :L] = old
    view[:, L:] = np.where(old[:, -1:] == ord("G"), ord("C"), ord("G"))
    out = dict(recs)
    out["seq"] = seq
    out["seq_off"] = (np.uint64(lead) + np.arange(n, dtype=np.uint64) * np.uint64(pitch))
    return out


@pytest.mark.parametrize("read_len,pitch", [(160, 161), (128, 129), (64, 65), (96, 97), (150, 151), (99, 99), (151, 151), (159, 159)])
def test_reads_that_start_on_odd_bases_of_the_seq_array(ctx, orc, read_len, pitch):
    """With the 4-bit mirror a read that starts on an odd base of the seq array is compared through shifted window
    coordinates (wide4_pass); a length that fills its last 32-base chunk leaves no room for the shift -- fine for a trimmed
    read, whose last base never counts, and handed to the other fast classes for the untrimmed flank in front of an indel
    (wide4_takes).  Odd pitches give every other read an odd start; with a third of the reads carrying an indel, flanks of
    32, 64 and 96 bases in front of one are there."""
    contig_off, bases, recs = synth.fast_records(seed=300 + read_len, contig_lens=(14_000, 2_600), coverage=60, read_len=read_len,
                                                 indel_read_frac=0.35, n_rate=0.002, k_choices=(1, 1, 1, 2, 3))
    recs = _repitch(recs, pitch, lead=1 if pitch % 2 == 0 else 0)
    odd = (recs["seq_off"] & np.uint64(1)) == 1
    assert odd.any() and (~odd).any()
    if read_len >= 99:
        three = recs["n_cig"] == 3
        front = recs["cigar"][recs["cig_off"][three].astype(np.int64)] >> 4
        assert ((front % 32 == 0) & odd[three]).any(), "no untrimmed flank that fills its last chunk from an odd start"
    _compare_records(ctx, orc, contig_off, bases, recs)


def test_mixed_read_lengths_in_one_job(ctx, orc):
    """The longest read picks the group width for everyone: 150-base and 250-base reads together (8 lanes),
    and 150 + 180 (6 lanes)."""
    for other in (250, 180):
        kw = dict(seed=77, contig_lens=(15_000, 3_000), coverage=25, indel_read_frac=0.05, k_choices=(1, 1, 3))
        contig_off, bases, ra = synth.fast_records(read_len=150, **kw)
        contig_off2, bases2, rb = synth.fast_records(read_len=other, **kw)
        assert np.array_equal(bases, bases2)
        _compare_records(ctx, orc, contig_off, bases, synth.merge_records(ra, rb, seed=other))


def test_two_level_bucketing_path(orc, tmp_path):
    """Assemblies beyond 16384 windows (33.5 Mbp per GPU) bucket their work items in two levels (coarse
    buckets, then k_regroup).  PP_BUCKET_LEVELS=2 forces that path on small jobs: same bytes, same stats."""
    code = """
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import torch, synth, polypolish_amd as pp
from oracle import orc
ctx = pp.Context(0)
for kw in (dict(seed=2, contig_lens=(40_000, 7_000), coverage=80, indel_read_frac=0.2, n_rate=0.003),
           dict(seed=4, contig_lens=(30_000, 2_500), coverage=50, k_choices=(1, 2, 3, 5, 6, 7), indel_read_frac=0.05),
           dict(seed=7, contig_lens=(300, 2048, 2049, 500, 4096, 1000), coverage=40, read_len=100, indel_read_frac=0.05)):
    o, b, r = synth.fast_records(**kw)
    want = orc.polish_records(o, b, r, positions=True)
    got = ctx.polish_records(o, b, r, positions=True)
    assert got["polished"] == want["polished"] and np.array_equal(got["offsets"], want["offsets"])
    for k in ("depth", "count_a", "count_c", "count_g", "count_t", "count_other", "status"):
        assert np.array_equal(got["positions"][k], want["positions"][k]), k
print("two-level ok")
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run(["python", "-c", code], capture_output=True, env=dict(os.environ, PP_BUCKET_LEVELS="2"), timeout=600)
    assert r.returncode == 0 and b"two-level ok" in r.stdout, r.stderr.decode()[-2000:]


def test_buffer_growth_takes_one_rerun(tmp_path):
    """A fresh context starts with optimistic capacities (64 tally slabs, 2^20 replay items, 65536 listed positions).  A job
    in which EVERY window has order-dependent depths that all have to be replayed overflows them: the device keeps counting
    what it needs (DE_CAPACITY_LATE), so the host grows everything at once -- two passes, not one per in-flight wave of
    workgroups -- and the result is the oracle's.  Since round 4 the pileup kernel settles such positions itself (interval
    vote), so the plain job is ONE pass with next to nothing replayed; the replay of everything is what --debug does
    (every flagged position through the global list) and what the PP_DEBUG_REPLAY2 hook keeps (through the per-window
    ordered replay): both must still grow their buffers in one rerun."""
    code = """
import os, sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import torch, synth, polypolish_amd as pp
from oracle import orc
o, b, r = synth.fast_records(seed=31, contig_lens=(1_500_000,), coverage=125, k_choices=(1, 3), indel_read_frac=0.01)
want = orc.polish_records(o, b, r, positions=True)
if not os.environ.get("PP_DEBUG_REPLAY2"):
    ctx = pp.Context(0)
    ctx.set_profiling(1)
    got = ctx.polish_records(o, b, r)
    t = ctx.kernel_times()
    assert got["polished"] == want["polished"] and np.array_equal(got["offsets"], want["offsets"])
    assert t["n_passes"] == 1 and t["n_flagged"] < 0.01 * 1_500_000, t   # nothing to grow: the interval vote settles the depths
# per-position records: every order-dependent position is replayed -- through the global list (--debug), or through the
# per-window ordered replay (PP_DEBUG_REPLAY2=1): tally slabs, replay items, listed positions and their scratch overflow together
ctx2 = pp.Context(0)
ctx2.set_profiling(1)
got = ctx2.polish_records(o, b, r, positions=True)
t2 = ctx2.kernel_times()
assert got["polished"] == want["polished"]
assert np.array_equal(got["positions"]["depth"], want["positions"]["depth"])
assert t2["n_passes"] == 2 and t2["n_flagged"] > 1_000_000, t2
got = ctx2.polish_records(o, b, r, positions=True)
assert got["polished"] == want["polished"] and ctx2.kernel_times()["n_passes"] == 1
print("growth ok", t2["n_entries"], t2["n_flagged"])
""" % (ROOT, os.path.join(ROOT, "tests"))
    for hook in ({}, {"PP_DEBUG_REPLAY2": "1"}):
        r = subprocess.run(["python", "-c", code], capture_output=True, timeout=600, env=dict(os.environ, PP_TIMING="1", **hook))
        assert r.returncode == 0 and b"growth ok" in r.stdout, (hook, r.stderr.decode()[-3000:])


def test_ordered_replay_depths_bit_exact_on_both_sort_paths(tmp_path):
    """k_exact2 orders a window's items by file index with a counting sort on the leading index bits, or with a
    bitonic network when the indices are clustered.  PP_DEBUG_REPLAY2=1 keeps k_exact2 in charge while the
    per-position records are collected, so its order-dependent f64 depths are compared bit for bit: (a) indices
    spread over the file, (b) a position-sorted file whose window items have consecutive indices plus one straggler
    at the end of the file (> SORT_BUCKET_MAX items per bucket -> bitonic)."""
    code = """
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import torch, synth, polypolish_amd as pp
from oracle import orc
ctx = pp.Context(0)
def check(o, b, r):
    want = orc.polish_records(o, b, r, positions=True)
    got = ctx.polish_records(o, b, r, positions=True)
    for k in ("depth", "count_a", "count_c", "count_g", "count_t", "status"):
        assert np.array_equal(got["positions"][k], want["positions"][k]), k
    assert got["polished"] == want["polished"]
    return want
o, b, r = synth.fast_records(seed=51, contig_lens=(40_000,), coverage=300, k_choices=(1, 3, 5, 7), indel_read_frac=0.02)
check(o, b, r)
o, b, r = synth.fast_records(seed=52, contig_lens=(600_000,), coverage=60, k_choices=(3, 7), indel_read_frac=0.0)
order = np.argsort(r["ref_start"], kind="stable")
order = np.concatenate([order[:5], order[6:], order[5:6]])   # one read of window 0 becomes the file's last record
for k in ("contig", "ref_start", "k", "seq_len", "n_cig", "seq_off", "cig_off"):
    r[k] = np.ascontiguousarray(r[k][order])
want = check(o, b, r)
assert len(np.unique(want["positions"]["depth"])) > 100
print("replay ok")
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run(["python", "-c", code], capture_output=True, timeout=900, env=dict(os.environ, PP_DEBUG_REPLAY2="1"))
    assert r.returncode == 0 and b"replay ok" in r.stdout, r.stderr.decode()[-3000:]


def test_deep_pileup_on_one_window(ctx, orc):
    # 20,000x on a 3 kbp contig: a single window bucket of ~60k work items
    contig_off, bases, recs = synth.fast_records(seed=21, contig_lens=(3_000,), coverage=20_000, read_len=150,
                                                 indel_read_frac=0.01)
    _compare_records(ctx, orc, contig_off, bases, recs)


def test_empty_and_degenerate_jobs(ctx, orc):
    bases = np.frombuffer(b"ACGT-NNACGTTTGCA" * 200, dtype=np.uint8)
    off = np.array([0, 1000, 3200], dtype=np.uint64)
    empty = {k: np.zeros(0, dtype=dt) for k, dt in (("contig", np.uint32), ("ref_start", np.uint32), ("k", np.uint32),
             ("seq_off", np.uint64), ("seq_len", np.uint32), ("cig_off", np.uint64), ("n_cig", np.uint32),
             ("seq", np.uint8), ("cigar", np.uint32))}
    want, got = _compare_records(ctx, orc, off, bases, empty)  # zero alignments: '-' dropped, all low_depth
    assert b"-" not in got["polished"] and len(got["polished"]) == 3200 - 200
    # homopolymer reads contribute nothing (trim pops everything)
    recs = {"contig": np.zeros(8, np.uint32), "ref_start": np.arange(8, dtype=np.uint32), "k": np.ones(8, np.uint32),
            "seq_off": np.arange(8, dtype=np.uint64) * 20, "seq_len": np.full(8, 20, np.uint32),
            "cig_off": np.arange(8, dtype=np.uint64), "n_cig": np.ones(8, np.uint32),
            "seq": np.frombuffer(b"A" * 160, dtype=np.uint8), "cigar": np.full(8, (20 << 4) | 0, np.uint32)}
    _compare_records(ctx, orc, off, bases, recs)


def _rec(entries):
    """entries: list of (contig, ref_start, k, seq, [(len, op), ...])."""
    seq = b"".join(e[3].encode() for e in entries)
    cig = [((l << 4) | "MIDNSHP=X".index(o)) for e in entries for (l, o) in e[4]]
    n_cig = np.array([len(e[4]) for e in entries], np.uint32)
    seq_len = np.array([len(e[3]) for e in entries], np.uint32)
    return {"contig": np.array([e[0] for e in entries], np.uint32), "ref_start": np.array([e[1] for e in entries], np.uint32),
            "k": np.array([e[2] for e in entries], np.uint32),
            "seq_off": (np.cumsum(seq_len) - seq_len).astype(np.uint64), "seq_len": seq_len,
            "cig_off": (np.cumsum(n_cig) - n_cig).astype(np.uint64), "n_cig": n_cig,
            "seq": np.frombuffer(seq, np.uint8), "cigar": np.array(cig, np.uint32)}


def test_insertion_deletion_and_odd_keys_win_the_vote(ctx, orc):
    ref = "TTGACCGTAGGCTAACGTTAGCATCGGATCCATGCAAGT"
    bases = np.frombuffer(ref.encode(), np.uint8)
    off = np.array([0, len(ref)], np.uint64)
    # 3-base insertion after position 9, deletion of positions 20-21, X and = runs
    ent = [(0, 2, 1, "GACCGTAGACGGCTAACGTTATCGGATCCAT", [(8, "="), (3, "I"), (9, "M"), (2, "D"), (1, "X"), (10, "=")])
           for _ in range(12)]
    want, got = _compare_records(ctx, orc, off, bases, _rec(ent))
    assert len(got["polished"]) == len(ref) + 3 - 2 and (want["positions"]["status"] == 1).sum() >= 3
    # D immediately followed by I (slot rewritten to one base), N bases, a '-' byte in SEQ
    ent = [(0, 5, 1, "CGTAGGNTAACGTTAG-ATCGGATCCATGCAAGT", [(6, "M"), (1, "D"), (1, "I"), (27, "M")]) for _ in range(12)]
    want, got = _compare_records(ctx, orc, off, bases, _rec(ent))
    assert (want["positions"]["status"] == 1).sum() >= 2 and len(got["polished"]) == len(ref) - 1
    # a 200-base insertion (longer than the 1-byte emit code can express)
    big = "ACGT" * 50
    ent = [(0, 2, 1, "GACCGTAG" + big + "GCTAACGTTAGC", [(8, "M"), (200, "I"), (12, "M")]) for _ in range(9)]
    _compare_records(ctx, orc, off, bases, _rec(ent))


def test_f64_order_dependence_on_device(ctx, orc):
    # D4: fifteen k=3 shares sum to 4.999999999999999 -> low_depth at min_depth 5; order of mixed shares matters
    ref = "ACGTACGTACGTTGCA" * 4
    bases = np.frombuffer(ref.encode(), np.uint8)
    off = np.array([0, len(ref)], np.uint64)
    ent = [(0, 0, 3, ref[:32], [(32, "M")]) for _ in range(15)]
    want, got = _compare_records(ctx, orc, off, bases, _rec(ent))
    assert want["positions"]["depth"][0] == 4.999999999999999 and want["positions"]["status"][0] == 2
    rng = np.random.default_rng(0)
    ks = [3, 3, 3, 1, 1, 6, 6, 5, 7, 10, 1, 3, 9, 12, 2]
    for _ in range(4):
        order = rng.permutation(len(ks))
        ent = [(0, 0, ks[i], ref[:32], [(32, "M")]) for i in order]
        _compare_records(ctx, orc, off, bases, _rec(ent))


def test_device_reports_the_first_bad_record(ctx, pp):
    ref = "ACGGTCATTGCAACGGTTATTGCA" * 3
    bases = np.frombuffer(ref.encode(), np.uint8)
    off = np.array([0, len(ref)], np.uint64)
    good = (0, 0, 1, ref[:24], [(24, "M")])
    cases = [
        ((0, 0, 1, ref[:24], [(10, "M"), (4, "N"), (10, "M")]), pp.ERR_QUIT, "unexpected character"),
        ((0, 0, 1, ref[:24], [(23, "M")]), pp.ERR_QUIT, "does not match read sequence"),
        ((0, 60, 1, ref[:24], [(24, "M")]), pp.ERR_PANIC, "past the end"),
        ((5, 0, 1, ref[:24], [(24, "M")]), pp.ERR_QUIT, "not in the assembly"),
        ((0, 0, 0, ref[:24], [(24, "M")]), pp.ERR_ARG, "k = 0"),
        ((0, 0, 1, ref[:24], [(4, "S"), (20, "M")]), pp.ERR_QUIT, "unexpected character"),
        ((0, 0, 1, ref[:24], [(1, "I"), (23, "M")]), pp.ERR_ARG, "start and end"),
    ]
    for bad, code, text in cases:
        with pytest.raises(pp.PolypolishError) as e:
            ctx.polish_records(off, bases, _rec([good, good, bad, good, bad]))
        assert e.value.code == code and text in e.value.msg and "record 2" in e.value.msg, e.value
    # a read overhanging the contig end only by its trimmed tail is fine (the reference never indexes it)
    ent = [(0, len(ref) - 22, 1, ref[-22:] + "GG", [(24, "M")])]
    ctx.polish_records(off, bases, _rec(ent))


def test_committed_end_to_end_fixture(ctx, tmp_path):
    """tests/golden/derived_e2e: the product alone (no oracle in the loop) against committed bytes -- `filter`
    (both loaders), `polish` of its output, the fused command, and `polish --careful -d 3` of the raw SAMs."""
    import hashlib
    import json
    g = os.path.join(ROOT, "tests", "golden", "derived_e2e")
    exp = json.load(open(os.path.join(g, "expected.json")))
    s1, s2, fa = (os.path.join(g, n) for n in ("case_1.sam", "case_2.sam", "case.fasta"))
    want = open(os.path.join(g, "polished_after_filter.fasta"), "rb").read()
    f1, f2 = str(tmp_path / "f1.sam"), str(tmp_path / "f2.sam")
    for mode in ("0", "1"):
        os.environ["PP_DEVICE_FILTER"] = mode
        try:
            assert ctx.filter_files(s1, s2, f1, f2) == exp["filter_report"]
        finally:
            del os.environ["PP_DEVICE_FILTER"]
        assert hashlib.sha256(open(f1, "rb").read()).hexdigest() == exp["filtered_1_sha256"]
        assert hashlib.sha256(open(f2, "rb").read()).hexdigest() == exp["filtered_2_sha256"]
    assert ctx.polish_files(fa, [f1, f2]) == want
    assert ctx.filter_polish_files(fa, s1, s2)[0] == want
    assert ctx.polish_files(fa, [s1, s2], careful=True, min_depth=3) == open(os.path.join(g, "polished_raw_careful_d3.fasta"), "rb").read()


def test_fuzz_cigar_walk_against_the_oracle(ctx, pp, orc):
    """Random multi-operation CIGARs (several indels per read, indels next to each other, X/=, homopolymer ends)
    through the device's CIGAR walk + trim + vote against the oracle; with defects mixed in, the same record must
    be blamed with the same kind of error."""
    import re
    kinds = ("unexpected character", "does not match read sequence", "past the end")
    n_ok = n_err = 0
    for seed in range(40):
        contig_off, bases, recs = synth.random_cigar_records(seed=1000 + seed, bad_frac=0.0 if seed % 2 == 0 else 0.003,
                                                             n_reads=1200 + 40 * seed, max_ops=3 + seed % 6)
        try:
            want = orc.polish_records(contig_off, bases, recs, positions=True)
            we = None
        except orc.OrcError as e:
            want, we = None, e
        if we is None:
            _compare_records(ctx, orc, contig_off, bases, recs)
            n_ok += 1
            continue
        n_err += 1
        with pytest.raises(pp.PolypolishError) as ge:
            ctx.polish_records(contig_off, bases, recs)
        idx = int(re.search(r"aln(\d+)", we.msg).group(1))
        kind = next(k for k in kinds if k in we.msg)
        assert ge.value.code == we.code and kind in ge.value.msg and f"record {idx}" in ge.value.msg, (seed, ge.value, we.msg)
    assert n_ok >= 15 and n_err >= 5, (n_ok, n_err)


def test_one_indel_reads_edge_cases(ctx, pp, orc):
    """Reads with ONE 1-base indel (aM1IbM / aM1DbM) are cut into flank / entry at the indel / flank work items instead of
    being walked (alignment.rs:175-201) -- unless the flank in front is empty or the homopolymer trim
    (alignment.rs:364-378) would reach the indel, which take the general walk (until round 6 a flank of fewer than 8 bases
    did too; such a flank is now a plain piece of 1..7 bases on the direct path).  Every indel position of a 40-base read,
    both kinds, read ends of homopolymers of 1..7 bases (so the trim ends before, at and beyond the indel), starts on both
    sides of a 2048-position window boundary, depth shares 1, 1/2 and 1/3: per-position depth / counts / thresholds /
    status and the bytes against the oracle, with and without the per-position records."""
    rng = np.random.default_rng(11)
    G, L = 6000, 40
    bases = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, G)].copy()
    rec = {k: [] for k in ("contig", "ref_start", "k", "seq_len", "n_cig")}
    seqs, cigs = [], []
    for a in range(1, L - 1):
        for kind in (1, 2):                      # 1 insertion, 2 deletion
            for tail in (1, 2, 3, 5, 7, L - a):  # length of the homopolymer the read ends in (L - a: it reaches the indel)
                for start in (2048 - L // 2, 2048 - a, 2048 - a - 1, 2048 + 5, 4096 - 3):
                    kk = int(rng.choice((1, 1, 2, 3)))
                    b = L - a - (1 if kind == 1 else 0)
                    if b < 1 or start < 0 or start + L + 2 >= G:
                        continue
                    s = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, L)].copy()
                    t = min(tail, L)
                    s[L - t:] = s[L - 1]
                    if L - t - 1 >= 0 and s[L - t - 1] == s[L - 1]:
                        s[L - t - 1] = b"ACGT"[(b"ACGT".index(bytes([s[L - 1]])) + 1) % 4]
                    rec["contig"].append(0); rec["ref_start"].append(start); rec["k"].append(kk)
                    rec["seq_len"].append(L); rec["n_cig"].append(3)
                    seqs.append(s)
                    cigs.append([(a << 4) | 0, (1 << 4) | kind, (b << 4) | 0])
    n = len(seqs)
    assert n > 1500
    order = rng.permutation(n)
    recs = {k: np.array(v, dtype=np.uint32)[order] for k, v in rec.items()}
    recs["seq"] = np.concatenate([seqs[i] for i in order])
    recs["cigar"] = np.array([c for i in order for c in cigs[i]], dtype=np.uint32)
    recs["seq_off"] = (np.arange(n, dtype=np.uint64) * np.uint64(L))
    recs["cig_off"] = (np.arange(n, dtype=np.uint64) * np.uint64(3))
    contig_off = np.array([0, G], dtype=np.uint64)
    _compare_records(ctx, orc, contig_off, bases, recs)
    _compare_records(ctx, orc, contig_off, bases, recs, min_depth=1, fraction_invalid=0.1)


@pytest.mark.parametrize("max_len", [160, 171], ids=["one_lane_per_read", "lane_groups"])
def test_plain_reads_over_the_4bit_mirror_edge_cases(ctx, pp, orc, max_len):
    """The plain class reads its bases from the 4-bit mirror of the seq array when a batch brings one (pp_aln_batch.seq4):
    with a whole read per lane while no read of the job is longer than 160 bases (wide4_pass), with lane groups beyond.
    Reads without indels of every length 8..max_len back to back (so every other one starts on an odd base of the array),
    bytes from A C G T N and the bytes that have no code of their own (R, Y, '-', '.'), tails of one base repeated 1..9
    times -- also of N, of R (shares its code with Y: the trim then goes through the bytes), of a read that IS one
    homopolymer --, an assembly that holds N, R and '-' itself; against the oracle per position (_compare_records runs
    the records with and without the mirror)."""
    rng = np.random.default_rng(23)
    G = 9000
    alpha = np.frombuffer(b"ACGTNRY-.", np.uint8)
    bases = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, G)].copy()
    for ch, cnt in ((b"N", 60), (b"R", 40), (b"-", 30)):
        bases[rng.integers(0, G, cnt)] = ch[0]
    rec = {k: [] for k in ("contig", "ref_start", "k", "seq_len", "n_cig")}
    seqs = []
    for rep in range(4):
        for L in range(8, max_len + 1):
            start = int(rng.integers(0, G - L))
            s = bases[start:start + L].copy()                      # mostly the assembly's own bytes ...
            mut = rng.random(L) < 0.08
            s[mut] = alpha[rng.choice(len(alpha), int(mut.sum()), p=(.2, .2, .2, .2, .08, .04, .04, .02, .02))]
            t = int(rng.integers(1, 10)) if rep != 3 else L        # ... ending in a run of t equal bytes
            tb = alpha[int(rng.choice(len(alpha), p=(.2, .2, .2, .2, .08, .05, .03, .02, .02)))]
            t = min(t, L)
            s[L - t:] = tb
            if L - t - 1 >= 0 and s[L - t - 1] == tb:
                s[L - t - 1] = b"A"[0] if tb != b"A"[0] else b"C"[0]
            rec["contig"].append(0); rec["ref_start"].append(start); rec["k"].append(int(rng.choice((1, 1, 1, 2, 3))))
            rec["seq_len"].append(L); rec["n_cig"].append(1)
            seqs.append(s)
    n = len(seqs)
    order = rng.permutation(n)
    recs = {k: np.array(v, dtype=np.uint32)[order] for k, v in rec.items()}
    lens = recs["seq_len"].astype(np.uint64)
    recs["seq"] = np.concatenate([seqs[i] for i in order])
    recs["seq_off"] = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    recs["cigar"] = ((recs["seq_len"] << 4) | 0).astype(np.uint32)
    recs["cig_off"] = np.arange(n, dtype=np.uint64)
    assert (recs["seq_off"] & 1).sum() > n // 4
    contig_off = np.array([0, G], dtype=np.uint64)
    _compare_records(ctx, orc, contig_off, bases, recs)
    _compare_records(ctx, orc, contig_off, bases, recs, min_depth=1, fraction_invalid=0.05, fraction_valid=0.3)


FILE_CASES = [
    dict(seed=31),
    dict(seed=32, contig_lens=(6000, 1200, 900), coverage=30, repeat_len=400, repeat_copies=3),
    dict(seed=33, contig_lens=(5000,), coverage=50, repeat_len=300, repeat_copies=5, inverted=False, n_rate=0.01),
    dict(seed=34, contig_lens=(2500, 2500), coverage=8, sub_rate=0.02, zp_frac=0.1),
]


@pytest.mark.parametrize("case", FILE_CASES, ids=[f"seed{c['seed']}" for c in FILE_CASES])
def test_polish_files_parity(ctx, orc, tmp_path, case):
    ds = synth.rich_dataset(str(tmp_path), **case)
    sams = [ds["sam1"], ds["sam2"]]
    for kw in (dict(), dict(careful=True), dict(min_depth=2, fraction_invalid=0.1, max_errors=3)):
        want = orc.polish_files(ds["fasta"], sams, **kw)["fasta"]
        got = ctx.polish_files(ds["fasta"], sams, **kw)
        assert got == want, kw


@pytest.mark.parametrize("case", FILE_CASES, ids=[f"seed{c['seed']}" for c in FILE_CASES])
def test_debug_tsv_parity(ctx, orc, tmp_path, case):
    """--debug (src/pileup.rs:137-166, src/polish.rs:230-266): the per-base TSV, byte for byte."""
    ds = synth.rich_dataset(str(tmp_path), **case)
    sams = [ds["sam1"], ds["sam2"]]
    for i, kw in enumerate((dict(), dict(min_depth=2, fraction_invalid=0.1, max_errors=3))):
        want = orc.polish_files(ds["fasta"], sams, debug=True, **kw)
        tsv = str(tmp_path / f"debug{i}.tsv")
        got = ctx.polish_files(ds["fasta"], sams, debug=tsv, **kw)
        assert got == want["fasta"]
        got_tsv = open(tsv, "rb").read()
        if got_tsv != want["debug"]:
            gl, wl = got_tsv.split(b"\n"), want["debug"].split(b"\n")
            bad = [(a, b) for a, b in zip(gl, wl) if a != b][:5]
            raise AssertionError((len(gl), len(wl), bad))
    # the same job without --debug afterwards (different flagging rule) still gives the same FASTA
    assert ctx.polish_files(ds["fasta"], sams) == orc.polish_files(ds["fasta"], sams)["fasta"]


@pytest.mark.parametrize("case", FILE_CASES[1:3], ids=["seed32", "seed33"])
def test_filter_then_polish_parity(ctx, orc, tmp_path, case):
    ds = synth.rich_dataset(str(tmp_path), **case)
    o1, o2, g1, g2 = (str(tmp_path / n) for n in ("o1.sam", "o2.sam", "g1.sam", "g2.sam"))
    for kw in (dict(), dict(orientation="fr", low=5.0, high=95.0), dict(orientation="rf", low=1.0, high=60.0)):
        try:
            want = orc.filter_files(ds["sam1"], ds["sam2"], o1, o2, **kw)
        except orc.OrcError as e:
            with pytest.raises(Exception) as ge:
                ctx.filter_files(ds["sam1"], ds["sam2"], g1, g2, **kw)
            assert ge.value.code == e.code and ge.value.msg == e.msg
            continue
        got = ctx.filter_files(ds["sam1"], ds["sam2"], g1, g2, **kw)
        assert open(g1, "rb").read() == open(o1, "rb").read()
        assert open(g2, "rb").read() == open(o2, "rb").read()
        assert got == want
    orc.filter_files(ds["sam1"], ds["sam2"], o1, o2)
    ctx.filter_files(ds["sam1"], ds["sam2"], g1, g2)
    assert ctx.polish_files(ds["fasta"], [g1, g2]) == orc.polish_files(ds["fasta"], [o1, o2])["fasta"]


@pytest.mark.parametrize("case", FILE_CASES[1:3], ids=["seed32", "seed33"])
def test_fused_filter_polish_equals_the_two_commands(ctx, orc, tmp_path, case):
    """pp_filter_polish_files / `polypolish filter-polish`: the verdicts reach the polish ingest in memory;
    FASTA and (optional) tagged SAMs are byte-identical to the oracle's filter followed by its polish."""
    ds = synth.rich_dataset(str(tmp_path), **case)
    o1, o2, g1, g2 = (str(tmp_path / n) for n in ("o1.sam", "o2.sam", "g1.sam", "g2.sam"))
    want_rep = orc.filter_files(ds["sam1"], ds["sam2"], o1, o2)
    want = orc.polish_files(ds["fasta"], [o1, o2])["fasta"]
    got, rep = ctx.filter_polish_files(ds["fasta"], ds["sam1"], ds["sam2"])
    assert got == want and rep == want_rep
    got, rep = ctx.filter_polish_files(ds["fasta"], ds["sam1"], ds["sam2"], out1=g1, out2=g2, min_depth=3, careful=True)
    assert got == orc.polish_files(ds["fasta"], [o1, o2], min_depth=3, careful=True)["fasta"]
    assert open(g1, "rb").read() == open(o1, "rb").read() and open(g2, "rb").read() == open(o2, "rb").read()
    r = subprocess.run([os.path.join(ROOT, "bin", "polypolish"), "filter-polish", "--in1", ds["sam1"], "--in2", ds["sam2"],
                        ds["fasta"]], capture_output=True)
    assert r.returncode == 0 and r.stdout == want, r.stderr.decode()[-500:]


def test_emit_ranges_match_oracle_slices(ctx, orc):
    """pp_polish_set_emit: every position is still voted with all alignments, but only [lo, hi) of each
    contig contributes bytes and statistics."""
    contig_off, bases, recs = synth.fast_records(seed=71, contig_lens=(30_000, 5_000, 9_000), coverage=50,
                                                 k_choices=(1, 2, 3), indel_read_frac=0.2, n_rate=0.002)
    rng = np.random.default_rng(7)
    lens = np.diff(np.asarray(contig_off, dtype=np.int64))
    for trial in range(4):
        lo = rng.integers(0, lens // 2)
        hi = lo + rng.integers(0, lens - lo + 1)
        if trial == 0:
            lo[:], hi[:] = 0, lens          # everything
        if trial == 1:
            hi[1] = lo[1]                    # an empty range
        emit = np.stack([lo, hi], axis=1)
        want = synth.oracle_engine(orc)(contig_off, bases, recs, emit=emit)
        got = ctx.polish_records(contig_off, bases, recs, emit=emit)
        assert got["polished"] == want["polished"] and np.array_equal(got["offsets"], want["offsets"]), trial
        full = orc.polish_records(contig_off, bases, recs, positions=True)["positions"]
        for c in range(3):
            own = slice(int(contig_off[c] + lo[c]), int(contig_off[c] + hi[c]))
            assert got["stats"][c]["changed"] == int((full["status"][own] == 1).sum())
            assert got["stats"][c]["zero_depth"] == int((full["depth"][own] == 0.0).sum())
    # a rank that owns nothing at all: no bytes, every offset zero
    got = ctx.polish_records(contig_off, bases, recs, emit=np.zeros((3, 2), dtype=np.int64))
    assert got["polished"] == b"" and not np.any(got["offsets"])
    # the next job on the same context emits everything again
    assert ctx.polish_records(contig_off, bases, recs)["polished"] == orc.polish_records(contig_off, bases, recs)["polished"]


@pytest.mark.parametrize("world", [2, 5])
def test_window_tiled_contig_equals_unsharded(ctx, pp, orc, world):
    """Config C5 in miniature on the device: every "rank" polishes the FULL record set with the emit ranges the
    product's planner gives it (k_prep drops the records that do not reach them, k_tile skips foreign windows); the
    ranks' bytes, put together by pp_shard_assemble, are the unsharded polish -- k = 3 shares (ordered f64 depth),
    indels across the cuts and a second small contig included."""
    contig_off, bases, recs = synth.fast_records(seed=61, contig_lens=(14_000, 700), coverage=40, read_len=100,
                                                 k_choices=(1, 1, 2, 3), indel_read_frac=0.2, n_rate=0.003)
    want = orc.polish_records(contig_off, bases, recs)
    plan = pp.Plan(contig_off, np.bincount(recs["contig"], minlength=2), world, 2048)
    assert (plan.unit_contig == 0).sum() == world
    rank_bytes, rank_offs = [], []
    for rank in range(world):
        got = ctx.polish_records(contig_off, bases, recs, emit=plan.emit_ranges(rank))
        rank_bytes.append(got["polished"])
        rank_offs.append(got["offsets"])
    data, out_off = plan.assemble(rank_bytes, rank_offs)
    assert data == want["polished"] and np.array_equal(out_off, want["offsets"])


@pytest.mark.parametrize("long_read", [False, True])
def test_compact_runs_of_sharded_jobs(ctx, pp, orc, long_read):
    """A context of a sharded job runs over a compact assembly of what it owns: whole contigs, and -- on a tiled contig --
    its stretch plus a halo (run_pipeline).  Three ranks over a 400 kbp contig in three windows and two small contigs:
    every rank's part (pp_shard_split) and also ALL records with its emit ranges give the bytes whose assembly is the
    oracle's unsharded polish.  long_read: a 20,000-base alignment across the first cut is longer than the halo -- the
    device notices (DE_HALO) and the job is rerun over the whole assembly, with the same result."""
    contig_off, bases, recs = synth.fast_records(seed=67, contig_lens=(400_000, 3_000, 60_000), coverage=12, read_len=100,
                                                 k_choices=(1, 1, 2, 3), indel_read_frac=0.2, n_rate=0.003)
    plan = pp.Plan(contig_off, np.bincount(recs["contig"], minlength=3), 3, 65536)
    assert (plan.unit_contig == 0).sum() == 3
    if long_read:
        cut = int(plan.unit_hi[0])
        rng = np.random.default_rng(1)
        n_long = 20_000
        extra = {"contig": np.array([0], np.uint32), "ref_start": np.array([cut - 18_000], np.uint32), "k": np.array([1], np.uint32),
                 "seq_off": np.array([0], np.uint64), "seq_len": np.array([n_long], np.uint32), "cig_off": np.array([0], np.uint64),
                 "n_cig": np.array([1], np.uint32), "seq": np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n_long)].copy(),
                 "cigar": np.array([(n_long << 4) | 0], np.uint32)}
        recs = synth.merge_records(recs, extra, seed=3)
    want = orc.polish_records(contig_off, bases, recs)
    for parts in (True, False):
        rank_bytes, rank_offs = [], []
        for rank in range(3):
            mine = pp.shard_split_host(plan, rank, recs)[0] if parts else recs
            got = ctx.polish_records(contig_off, bases, mine, emit=plan.emit_ranges(rank))
            rank_bytes.append(got["polished"])
            rank_offs.append(got["offsets"])
            owned = plan.emit_ranges(rank)
            for c in range(3):  # a contig the rank has no unit of has no bytes there
                if owned[c, 1] == owned[c, 0]:
                    assert got["offsets"][c + 1] == got["offsets"][c]
        data, out_off = plan.assemble(rank_bytes, rank_offs)
        assert data == want["polished"] and np.array_equal(out_off, want["offsets"]), parts


def test_window_grouped_seq_layout_of_the_tokenizer(ctx, pp, orc, tmp_path):
    """PP_SEQ_WINDOW_GROUPED, the default layout of both ingests since round 4: the SEQ bytes of the reads that start in one
    2048-position window are next to each other (per SAM file).  Every record array but seq_off equals the host ingest's,
    every record's bytes are its bytes, the rooms tile the seq array, the windows come in order inside a file's stretch
    (the host ingest keeps file order inside a window, the tokenizer leaves that to its atomics), the batch brings the
    4-bit mirror of its seq array, and the polish of that batch -- and the CLI under every combination of PP_SEQ_LAYOUT /
    PP_SEQ4 / ingest -- gives the oracle's bytes (repeats with SEQ '*' records on both strands, indels, several contigs).
    PP_SEQ_FILE_ORDER on request: array-equal to the host ingest's."""
    ds = synth.rich_dataset(str(tmp_path), seed=97, contig_lens=(30_000, 2_500, 9_000), coverage=25, repeat_len=300,
                            repeat_copies=3, lowercase_frac=0.1)
    sams = [ds["sam1"], ds["sam2"]]
    _, _, off, bases, want, counts = pp.ingest(ds["fasta"], sams)
    _, _, off2, bases2, got, counts2 = pp.ingest_device(ctx, ds["fasta"], sams)      # the default: window-grouped
    _, _, _, _, got1, counts3 = pp.ingest_device(ctx, ds["fasta"], sams, seq_layout=1)
    assert counts == counts2 == counts3 and np.array_equal(off, off2) and np.array_equal(bases, bases2)
    used = [c[1] for c in counts]
    check_seq_layout(want, off, used, grouped=True, file_order_inside=True)
    for g in (got, got1):
        same_records(want, g)
        check_seq_layout(g, off, used, grouped=True)
        check_seq4_mirror(pp, g, expect=True)   # the batch brings the 4-bit mirror of its seq array
    _, _, _, _, flat_h, _ = pp.ingest(ds["fasta"], sams, seq_layout=0)
    _, _, _, _, flat_d, _ = pp.ingest_device(ctx, ds["fasta"], sams, seq_layout=0)
    check_seq_layout(flat_d, off, used, grouped=False)
    check_seq4_mirror(pp, flat_d, expect=True)
    for k in flat_h:
        if k != "wo":
            assert np.array_equal(flat_h[k], flat_d[k]), k
    same_records(want, flat_h)
    for g, inside in ((want, True), (got, False), (flat_h, True), (flat_d, False)):
        check_window_order_mirror(g, off, used, file_order_inside=inside)   # pp_aln_batch.wo of every batch
    res = ctx.polish_records(off, bases, got)
    assert res["polished"] == orc.polish_records(off, bases, want)["polished"]
    exe = os.path.join(ROOT, "bin", "polypolish")
    oracle_fasta = orc.polish_files(ds["fasta"], sams)["fasta"]
    for env in (dict(), dict(PP_SEQ_LAYOUT="window"), dict(PP_SEQ_LAYOUT="file"), dict(PP_SEQ4="0"), dict(PP_SEQ_LAYOUT="file", PP_SEQ4="0"),
                dict(PP_DEVICE_INGEST="0"), dict(PP_DEVICE_INGEST="0", PP_SEQ_LAYOUT="file"), dict(PP_DEVICE_INGEST="0", PP_SEQ4="0"),
                dict(PP_WO="0"), dict(PP_DEVICE_INGEST="0", PP_WO="0"), dict(PP_SEQ_LAYOUT="file", PP_SEQ4="0", PP_WO="0")):
        r = subprocess.run([exe, "polish", ds["fasta"], *sams], capture_output=True, env=dict(os.environ, **env))
        assert r.returncode == 0 and r.stdout == oracle_fasta, (env, r.stderr[-400:])


def test_multi_process_driver_on_one_gpu(orc, tmp_path):
    """`python -m polypolish_amd.distributed polish` with two ranks sharing this GPU (gloo gather): the
    one-process-per-GPU driver end to end, contigs and windows sharded, FASTA identical."""
    ds = synth.rich_dataset(str(tmp_path), seed=81, contig_lens=(140_000, 900, 2_000), coverage=12, repeat_len=300,
                            repeat_copies=3)
    sams = [ds["sam1"], ds["sam2"]]
    env = dict(os.environ, PP_SHARE_GPU="1", PYTHONPATH=ROOT)
    port = 33000 + os.getpid() % 2000
    r = subprocess.run(["python", "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                        "127.0.0.1", "--master-port", str(port), "-m", "polypolish_amd.distributed", "polish",
                        ds["fasta"], *sams], capture_output=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert r.stdout == orc.polish_files(ds["fasta"], sams)["fasta"]


@pytest.mark.parametrize("case", FILE_CASES, ids=[f"seed{c['seed']}" for c in FILE_CASES])
@pytest.mark.parametrize("careful", [False, True])
def test_device_tokenizer_equals_host_ingest(pp, ctx, tmp_path, case, careful, monkeypatch):
    """pp_dev_ingest_*: SAM text tokenized by kernels; the batch must hold the host ingest's records (and therefore what the
    reference's process_one_read would feed the pileup): in the default window-grouped layout the same records and the same
    layout up to the order inside a window, with PP_SEQ_LAYOUT=file (every other case) array by array.  The batch brings
    the 4-bit mirror of its seq array: checked nibble by nibble (secondaries' SEQ filled in from the other strand, lower
    case, bytes other than A/C/G/T)."""
    if careful:
        monkeypatch.setenv("PP_SEQ_LAYOUT", "file")
    ds = synth.rich_dataset(str(tmp_path), lowercase_frac=0.2, **case)
    want, err = same_ingest(pp, ctx, ds["fasta"], [ds["sam1"], ds["sam2"]], max_errors=10, careful=careful)
    assert err is None and len(want[4]["contig"]) > 0


def test_device_tokenizer_details_and_errors(pp, ctx, orc, tmp_path):
    ref = "ACGGTCATTGCAACGGTTATTGCA"
    fa = tmp_path / "a.fasta"
    fa.write_text(f">c d1 d2\n{ref[:10]}\n{ref[10:].lower()}\n>e\nGGGG\n")

    def line(name, flag, rname, pos, cigar, seq, tags="NM:i:0"):
        return f"{name}\t{flag}\t{rname}\t{pos}\t60\t{cigar}\t*\t0\t0\t{seq}\t*\t{tags}\n"
    good = ("@HD\tVN:1\n\n"
            + line("r1", 16, "c", 1, "12M", "acggtcattgca", "AS:i:3\tNM:i:2\tXX:Z:y")
            + line("r1", 256, "c", 13, "0S12M", "*") + line("r1", 272, "c", 13, "5S7M", "*")
            + line("r2", 4, "*", 0, "*", "ACGT", "") + line("r3", 0, "c", 1, "6=1X5=", ref[:12], "NM:i:11")
            + line("r4", 0, "c", 0, "12M", ref[:12], "NM:i:0\tzp:z:FAIL") + line("", 0, "c", 2, "5M", ref[1:6])
            + line("r6", 0, "c", 3, "5M", ref[2:7]) + line("r5", 0, "e", 1, "2M1I1M", "GGAG", "NM:i:1\tNM:i:0\t").rstrip("\n"))
    sam = tmp_path / "a.sam"
    sam.write_text(good)
    want, err = same_ingest(pp, ctx, str(fa), [str(sam)])
    assert err is None and list(want[4]["k"]) == [2, 2, 2, 2, 1]   # the empty QNAME pulls r6 into its group
    many = "".join(line(f"q{i}", 0, "c", 1 + i % 10, "12M", ref[i % 10:i % 10 + 12]) for i in range(3000))
    cases = [
        many + "r\t0\tc\t1\t60\t12M\n" + many,                               # too few columns, line 3001
        many + "r\t0\tc\t1\t60\t12M\t*\t0\t0\t" + ref[:12] + "\t*\n",          # missing NM
        many + line("r", 0, "c", 1, "12Q", ref[:12]) + many,                    # invalid CIGAR
        line("r", 0, "c", 1, "12M", "*") + many,                                # first group has no sequence ...
        line("r", 0, "c", 1, "12M", "*") + many[:5000] + "bad\t0\n" + many,       # ... and wins over a later parse error
        "bad\t0\n" + line("r", 0, "c", 1, "12M", "*") + many,                    # an earlier parse error wins over the group
        many + line("r", 0, "zzz", 1, "12M", ref[:12]),                         # contig not in assembly (EOF flush)
        many + line("r", 0, "c", 1, "*", ref[:12]) + many,                      # empty CIGAR: panic
        line("r", "x", "c", 1, "12M", ref[:12]),                                # FLAG does not parse: panic
        many + line("r", 0, "c", 1, "4294967296M", ref[:12]),                   # run length overflow: panic
        "@HD\tVN:1\n",                                                         # nothing aligned: panic
        "",                                                                     # empty file
        many + line("r", 0, "c", 5000000000, "12M", ref[:12]),                  # start beyond u32: panic
    ]
    seen = set()
    for i, text in enumerate(cases):
        p = tmp_path / f"e{i}.sam"
        p.write_text(text)
        _, err = same_ingest(pp, ctx, str(fa), [str(p)])
        assert err is not None, i
        seen.add(err[0])
    assert seen == {1, 101}
    # two files: the batch grows across calls
    want, err = same_ingest(pp, ctx, str(fa), [str(sam), str(sam)])
    assert err is None and len(want[4]["contig"]) == 10
    # CRLF line ends, with and without a final newline; a file that is one line without newline
    crlf = tmp_path / "crlf.sam"
    crlf.write_bytes(good.replace("\n", "\r\n").encode())
    want, err = same_ingest(pp, ctx, str(fa), [str(crlf)])
    assert err is None and len(want[4]["contig"]) == 5
    crlf.write_bytes((good + "\n").replace("\n", "\r\n").encode())
    assert same_ingest(pp, ctx, str(fa), [str(crlf)])[1] is None
    crlf.write_text(line("solo", 0, "e", 1, "4M", "GGGG").rstrip("\n"))
    want, err = same_ingest(pp, ctx, str(fa), [str(crlf)])
    assert err is None and list(want[4]["seq_len"]) == [4]
    # `polish` without any SAM file is legal (every position low_depth): the CLI through either ingest
    want_fasta = orc.polish_files(str(fa), [])["fasta"]
    for mode in ("1", "0"):
        r = subprocess.run([os.path.join(ROOT, "bin", "polypolish"), "polish", str(fa)], capture_output=True,
                           env=dict(os.environ, PP_DEVICE_INGEST=mode))
        assert r.returncode == 0 and r.stdout == want_fasta, r.stderr.decode()[-500:]


@pytest.mark.parametrize("case", FILE_CASES[:3], ids=["seed31", "seed32", "seed33"])
def test_cli_with_either_ingest(orc, tmp_path, case):
    """`polypolish polish` tokenizes the SAM text on the GPU by default and on the host with PP_DEVICE_INGEST=0;
    same stdout, same log numbers."""
    ds = synth.rich_dataset(str(tmp_path), **case)
    sams = [ds["sam1"], ds["sam2"]]
    want = orc.polish_files(ds["fasta"], sams)
    # (the third: the host ingest with ONE ingest object for all files and no upload while the next file is parsed)
    for env in (dict(PP_DEVICE_INGEST="1"), dict(PP_DEVICE_INGEST="0"), dict(PP_DEVICE_INGEST="0", PP_STREAM_ADDS="0")):
        r = subprocess.run([os.path.join(ROOT, "bin", "polypolish"), "polish", ds["fasta"], *sams], capture_output=True,
                           env=dict(os.environ, **env))
        assert r.returncode == 0 and r.stdout == want["fasta"], (env, r.stderr.decode()[-800:])
        log = r.stderr.decode()
        assert f"{want['counts'][1]:,} alignments kept" in log
    # `polypolish filter` with the load on the device (default) and on the host
    o1, o2, g1, g2 = (str(tmp_path / n) for n in ("o1.sam", "o2.sam", "g1.sam", "g2.sam"))
    rep = orc.filter_files(ds["sam1"], ds["sam2"], o1, o2)
    for mode in ("1", "0"):
        r = subprocess.run([os.path.join(ROOT, "bin", "polypolish"), "filter", "--in1", ds["sam1"], "--in2", ds["sam2"],
                            "--out1", g1, "--out2", g2], capture_output=True, env=dict(os.environ, PP_DEVICE_FILTER=mode))
        assert r.returncode == 0, r.stderr.decode()[-800:]
        assert open(g1, "rb").read() == open(o1, "rb").read() and open(g2, "rb").read() == open(o2, "rb").read()
        assert f"Alignments after filtering:  {rep['after']:,}" in r.stderr.decode()


def test_fuzz_device_parsers_against_the_host_parsers(pp, ctx, tmp_path):
    """Differential fuzzing: SAM files with random defects and oddities must get the same verdict -- identical
    arrays, or the same error code and message -- from the kernels (pp_dev_ingest_*, pp_filter_load_device)
    as from the host parsers, which the CPU tests tie to the oracle."""
    ds = synth.rich_dataset(str(tmp_path), seed=91, contig_lens=(1500, 800), coverage=6, repeat_len=200, repeat_copies=2,
                            zp_frac=0.05, lowercase_frac=0.1)
    base1, base2 = open(ds["sam1"]).read(), open(ds["sam2"]).read()
    rng = np.random.default_rng(2024)
    outcomes = {"ok": 0, "error": 0}
    f1, f2 = str(tmp_path / "f1.sam"), str(tmp_path / "f2.sam")
    for trial in range(500):
        open(f1, "w").write(synth.mutate_sam(base1, rng, int(rng.integers(1, 5))))
        open(f2, "w").write(synth.mutate_sam(base2, rng, int(rng.integers(0, 3))))
        careful = bool(trial % 5 == 0)
        want, err = same_ingest(pp, ctx, ds["fasta"], [f1, f2], max_errors=int(rng.choice([0, 2, 10])), careful=careful)
        outcomes["error" if err else "ok"] += 1
        # the filter's loaders
        try:
            H = pp.FilterLoaded(f1, f2)
            he = None
        except pp.PolypolishError as e:
            H, he = None, (e.code, e.msg)
        try:
            D = pp.FilterLoadedDevice(ctx, f1, f2)
            de = None
        except pp.PolypolishError as e:
            D, de = None, (e.code, e.msg)
        assert de == he, (trial, de, he)
        if H is not None:
            assert D.n_reads == H.n_reads and D.counts == H.counts, trial
            for f in range(2):
                for k in ("flags", "ref_start", "read", "grp_off", "grp_idx"):
                    assert np.array_equal(H.files[f][k], D.files[f][k]), (trial, f, k)
                assert np.array_equal(_host_ref_end(H.files[f]), D.files[f]["ref_end"]), (trial, f)
            H.close(); D.close()
    assert outcomes["ok"] >= 50 and outcomes["error"] >= 50, outcomes


def _host_ref_end(F):
    cig = F["cigar"].astype(np.int64)
    consumes = np.isin(cig & 15, (0, 2, 3, 7, 8))
    cs = np.concatenate([[0], np.cumsum((cig >> 4) * consumes)])
    lo = F["cig_off"].astype(np.int64)
    return (F["ref_start"].astype(np.int64) + cs[lo + F["n_cig"].astype(np.int64)] - cs[lo]).astype(np.uint64)


@pytest.mark.parametrize("case", FILE_CASES, ids=[f"seed{c['seed']}" for c in FILE_CASES])
def test_device_filter_load_equals_host_load(pp, ctx, tmp_path, case):
    """pp_filter_load_device: quick parse, ref_end, QNAME/RNAME interning and the group index as kernels; the
    arrays equal the host loader's (RNAME ids up to renaming)."""
    ds = synth.rich_dataset(str(tmp_path), **case)
    H = pp.FilterLoaded(ds["sam1"], ds["sam2"])
    D = pp.FilterLoadedDevice(ctx, ds["sam1"], ds["sam2"])
    assert D.n_reads == H.n_reads and D.counts == H.counts
    for f in range(2):
        h, d = H.files[f], D.files[f]
        for k in ("flags", "ref_start", "read", "grp_off", "grp_idx"):
            assert np.array_equal(h[k], d[k]), (f, k)
        assert np.array_equal(_host_ref_end(h), d["ref_end"])
    # RNAME ids: the same partition of all records of both files
    hid = np.concatenate([H.files[0]["ref_id"], H.files[1]["ref_id"]]).astype(np.int64)
    did = np.concatenate([D.files[0]["ref_id"], D.files[1]["ref_id"]]).astype(np.int64)
    pairs = set(zip(hid.tolist(), did.tolist()))
    assert len(pairs) == len(set(hid.tolist())) == len(set(did.tolist()))
    H.close(); D.close()


def test_device_filter_load_details_and_errors(pp, ctx, orc, tmp_path):
    def line(name, flag, ref, pos, cigar, rest="*\t0\t0\tACGT\t*"):
        return f"{name}\t{flag}\t{ref}\t{pos}\t60\t{cigar}\t{rest}\n"
    a, b = tmp_path / "a.sam", tmp_path / "b.sam"
    a.write_text("@HD\tVN:1\r\n" + line("x", 0, "c", 10, "5M2D3M") + line("y", 16, "d", 0, "4Mzz3=1Q2X") +
                 line("x", 256, "c", 100, "*") + line("u", 4, "*", 0, "*") + line("z", 0, "c", 7, "10M").rstrip("\n"))
    b.write_text(line("y", 0, "d", 50, "10M") + line("w", 0, "c", 1, "3M") + line("x", 16, "c", 30, "10M"))
    D = pp.FilterLoadedDevice(ctx, str(a), str(b))
    A, B = D.files
    assert D.counts == [(4, 3), (3, 3)] and D.n_reads == 4
    assert list(A["ref_start"]) == [9, 0, 99, 6] and list(A["flags"]) == [0, 16, 256, 0]
    assert list(A["ref_end"]) == [19, 9, 99, 16] and list(B["ref_end"]) == [59, 3, 39]
    assert list(A["read"]) == [0, 1, 0, 2] and list(B["read"]) == [1, 3, 0]
    assert [list(A["grp_idx"][A["grp_off"][r]:A["grp_off"][r + 1]]) for r in range(4)] == [[0, 2], [1], [3], []]
    assert A["ref_id"][0] == A["ref_id"][2] == A["ref_id"][3] == B["ref_id"][1] != A["ref_id"][1] == B["ref_id"][0]
    D.close()
    # the tagged output straight from the text
    out = tmp_path / "o.sam"
    text = a.read_bytes()
    p_, f_ = C_u64(), C_u64()
    err = ctypes.create_string_buffer(600)
    verdicts = np.array([1, 0, 0, 1], np.uint8)
    rc = pp.lib().pp_filter_write_text(text, len(text), verdicts.ctypes.data, 4, str(out).encode(), ctypes.byref(p_), ctypes.byref(f_), err, 600)
    assert rc == 0 and (p_.value, f_.value) == (2, 2)
    lines = out.read_text().split("\n")
    assert lines[0] == "@HD\tVN:1" and lines[-1] == "" and [l.endswith("\tZP:Z:fail") for l in lines[1:6]] == [False, True, True, False, False]

    def both(t1, t2):
        a.write_text(t1); b.write_text(t2)
        try:
            pp.FilterLoaded(str(a), str(b)).close()
            want = (0, "")
        except pp.PolypolishError as e:
            want = (e.code, e.msg)
        try:
            pp.FilterLoadedDevice(ctx, str(a), str(b)).close()
            got = (0, "")
        except pp.PolypolishError as e:
            got = (e.code, e.msg)
        return got, want
    ok = line("r", 0, "c", 1, "4M")
    many = "".join(line(f"r{i}", 0, "c", 1 + i, "4M") for i in range(3000))
    for t1, t2 in [(many + "\n" + ok, ok), (many, many[:9000] + "bad\t0\tc\n" + many), ("@HD\tVN:1\n", ok),
                   (many + "r\t0\tc\t1\n", "zzz"), (ok, "r\tx\tc\t1\t60\t4M\t*\t0\t0\tA\t*\n"),
                   (ok, line("r", 0, "c", 99999999999, "4M"))]:
        got, want = both(t1, t2)
        assert got == want and got[0] != 0, (got, want)
    for t1, t2 in [(many, many), (many, ""), (many, "@HD\tVN:1\n")]:
        got, want = both(t1, t2)
        assert got == want == (0, ""), (got, want)


def test_reference_orientation_vectors_on_device(ctx, pp):
    """T4 (src/filter.rs:384-424) through the filter kernels: orientation and insert size of the eight pairs (all `150M`).
    T3's four CIGARs (src/alignment.rs:402-422) go through k_ref_end in tests/test_reference_vectors_gpu.py."""
    import ctypes as C
    import json
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_unit_vectors.json")))
    cases = gold["T4_orientation"]["cases"]
    n = len(cases)
    names = ("fr", "rf", "ff", "rr")

    def ffile(pos, flags):
        arr = dict(ref_id=np.zeros(n, np.uint32), ref_start=np.array(pos, np.uint32) - 1, flags=np.array(flags, np.uint32),
                   cig_off=np.arange(n, dtype=np.uint64), n_cig=np.ones(n, np.uint32),
                   cigar=np.full(n, (150 << 4) | 0, np.uint32), read=np.arange(n, dtype=np.uint32),
                   grp_off=np.arange(n + 1, dtype=np.uint32), grp_idx=np.arange(n, dtype=np.uint32))
        f = pp.FilterFile(n, arr["ref_id"].ctypes.data, arr["ref_start"].ctypes.data, arr["flags"].ctypes.data,
                          arr["cig_off"].ctypes.data, arr["n_cig"].ctypes.data, arr["cigar"].ctypes.data, n,
                          arr["read"].ctypes.data, arr["grp_off"].ctypes.data, arr["grp_idx"].ctypes.data)
        return f, arr
    f1, k1 = ffile([c[0] for c in cases], [c[2] for c in cases])
    f2, k2 = ffile([c[1] for c in cases], [c[3] for c in cases])
    inp = pp.FilterInput(n, (pp.FilterFile * 2)(f1, f2))
    L = pp.lib()
    assert L.pp_filter_begin(ctx._h, C.byref(inp), pp.MEM_HOST) == 0, L.pp_last_error(ctx._h)
    orient, insert = np.zeros(n, np.uint8), np.zeros(n, np.uint32)
    assert L.pp_filter_samples(ctx._h, orient.ctypes.data, insert.ctypes.data) == 0
    assert [names[o] for o in orient] == [c[4] for c in cases]
    assert list(insert) == [abs(c[0] - c[1]) + 150 for c in cases]


def test_cli_is_a_drop_in(orc, tmp_path):
    ds = synth.rich_dataset(str(tmp_path), seed=41, contig_lens=(5000, 1500), coverage=30, repeat_len=350,
                            repeat_copies=4)
    exe = os.path.join(ROOT, "bin", "polypolish")
    f1, f2, o1, o2 = (str(tmp_path / n) for n in ("f1.sam", "f2.sam", "o1.sam", "o2.sam"))
    r = subprocess.run([exe, "filter", "--in1", ds["sam1"], "--in2", ds["sam2"], "--out1", f1, "--out2", f2],
                       capture_output=True)
    assert r.returncode == 0, r.stderr
    orc.filter_files(ds["sam1"], ds["sam2"], o1, o2)
    assert open(f1, "rb").read() == open(o1, "rb").read() and open(f2, "rb").read() == open(o2, "rb").read()
    dbg = str(tmp_path / "cli_debug.tsv")
    r = subprocess.run([exe, "polish", "-d", "4", "--fraction_invalid=0.15", "--debug", dbg, ds["fasta"], f1, f2],
                       capture_output=True)
    assert r.returncode == 0, r.stderr
    want = orc.polish_files(ds["fasta"], [o1, o2], min_depth=4, fraction_invalid=0.15, debug=True)
    assert r.stdout == want["fasta"]
    assert open(dbg, "rb").read() == want["debug"]
    assert b"positions changed" in r.stderr
    # clap's other spellings of the same command line (src/main.rs:78-108): attached short values, `=`, `--`
    for argv in (["-d4", "-i0.15"], ["-d=4", "--fraction_invalid", "0.15", "--"], ["--min_depth=4", "-i=0.15"]):
        r2 = subprocess.run([exe, "polish"] + argv + [ds["fasta"], f1, f2], capture_output=True)
        assert r2.returncode == 0 and r2.stdout == want["fasta"], (argv, r2.stderr[-300:])
    r = subprocess.run([exe, "polish", "-i", "0.7", ds["fasta"], f1], capture_output=True)
    assert r.returncode == 1 and r.stdout == b"" and b"Error: --fraction_invalid must be less than --fraction_valid" in r.stderr
    r = subprocess.run([exe, "polish", str(tmp_path / "missing.fasta")], capture_output=True)
    assert r.returncode == 1 and b"file does not exist" in r.stderr


def test_the_ways_a_job_ends_give_the_same_bytes(orc, tmp_path):
    """How the results of a job reach the host is a tuning matter (round 6): k_emit's last workgroup writes the metadata block
    into pinned host memory and sets it up for the next job, the host polls (default), waits for the stream (PP_SYNC=wait),
    or the stream copies the block and k_meta_init runs behind it as before (PP_RESULT_COPY=1); the scan kernel in front of
    the emission or not (PP_EMIT_FUSE=0); no steady-state shortcuts (PP_SPECULATE=0 PP_INIT_AHEAD=0).  The switches are read
    once per process: through the CLI, on a job with flagged positions (a repeat: the replays and a second round of the
    emission), stdout against the oracle's."""
    ds = synth.rich_dataset(str(tmp_path), seed=43, contig_lens=(9000, 2500), coverage=40, repeat_len=350, repeat_copies=4)
    exe = os.path.join(ROOT, "bin", "polypolish")
    want = orc.polish_files(ds["fasta"], [ds["sam1"], ds["sam2"]])
    for env in ({}, {"PP_SYNC": "wait"}, {"PP_SYNC": "query"}, {"PP_RESULT_COPY": "1"}, {"PP_EMIT_FUSE": "0"},
                {"PP_SPECULATE": "0", "PP_INIT_AHEAD": "0"}, {"PP_RESULT_COPY": "1", "PP_EMIT_FUSE": "0", "PP_SYNC": "wait"}):
        r = subprocess.run([exe, "polish", ds["fasta"], ds["sam1"], ds["sam2"]], capture_output=True, env=dict(os.environ, **env))
        assert r.returncode == 0, (env, r.stderr[-300:])
        assert r.stdout == want["fasta"], env


def test_job_after_job_on_one_context_with_and_without_flagged_positions(ctx, orc):
    """k_emit's last workgroup sets the metadata block up for the NEXT job only when this one is through and (first round of a
    speculating context) flagged nothing: clean job, job with flagged positions, clean job again, twice -- every one of them
    per position against the oracle."""
    clean = synth.fast_records(seed=81, contig_lens=(40_000, 9_000), coverage=60, indel_read_frac=0.01)
    shared = synth.fast_records(seed=82, contig_lens=(30_000,), coverage=80, k_choices=(1, 3), k_probs=(0.97, 0.03), indel_read_frac=0.01)
    for _ in range(2):
        for contig_off, bases, recs in (clean, clean, shared, clean, shared, shared, clean):
            _compare_records(ctx, orc, contig_off, bases, recs)


def test_configs0_shape_through_the_cli(tmp_path):
    """BASELINE.json configs[0]: one 50 kbp contig, 10,000 x 150 bp paired reads, text in / FASTA out through
    bin/polypolish -- polish (both ingests), filter and the fused command against the oracle's CLI, sha256 of every
    output (the same leg bench.py runs at the other configurations' sizes)."""
    import torch
    import bench
    lens, cov, repeat, _ = bench.config_shape(0)
    out = bench.end_to_end(torch.device("cuda", 0), 0, lens, cov, repeat, seed=4242, keep_dir=str(tmp_path))
    assert out.get("parity") is True, out
    assert "10000 records" in out["files"], out["files"]


def test_configs2_from_text_at_full_size(tmp_path):
    """BASELINE.json configs[2] END TO END FROM SAM TEXT at full size (5 Mbp, 200x, a 5-kbp segment in five copies on both
    strands): real all-hits files -- every read inside a copy as a primary record plus four secondary records with
    SEQ / QUAL '*' (src/alignment.rs:290-295,311-322 fill them, reverse-complemented on the inverted copies) -- through
    `polish` (k = 5 groups, order-dependent f64 depth), `filter` (alignment_pass_qc's n x m loop over the copies,
    src/filter.rs:352-377), `filter` followed by `polish`, and the fused command; sha256 against the oracle's CLI."""
    import torch
    import bench
    lens, cov, repeat, _ = bench.config_shape(2)
    out = bench.end_to_end(torch.device("cuda", 0), 2, lens, cov, repeat, seed=4244, keep_dir=str(tmp_path))
    assert out.get("parity") is True, out
    assert out["filter_then_polish"]["parity"], out
    assert out["filter"]["records_failed_in_file_1"] > 1000, out["filter"]  # the filter had something to reject


def test_configs3_from_sam_files_beyond_4_gib(tmp_path):
    """BASELINE.json configs[3] (100-contig metagenome, 100x) END TO END FROM SAM TEXT at a reduced size whose two SAM files
    are still larger than 4 GiB each: byte offsets into a file's text, newline positions and the tokenizer's scans pass
    2^32 (pp_tokenize.hip indexes the text with 64-bit offsets; a 32-bit slip would scramble every record of the second half
    of a file).  `polish` through the device tokenizer and through the host ingest against the oracle's CLI, sha256."""
    import torch
    import bench
    lens, cov, repeat, _ = bench.config_shape(3, genome=38_000_000)
    out = bench.end_to_end(torch.device("cuda", 0), 3, lens, cov, repeat, seed=4245, keep_dir=str(tmp_path))
    assert out.get("parity") is True, out
    assert out["text_bytes"] / 2 > 2 ** 32 + 2 ** 27, out["text_bytes"]   # each of the two files well past 4 GiB
    assert out["polish"]["parity"] and out["polish_host_ingest"]["parity"], out
    for p in os.listdir(tmp_path):   # 9 GB of text: gone before the next test
        os.unlink(os.path.join(tmp_path, p))


def test_assembly_of_4_gbp_is_refused_cleanly(ctx, pp):
    """Positions are 32-bit in this version: an assembly of 2^32-4096 bp or more is refused by pp_polish_begin with
    PP_ERR_LIMIT before anything is read or allocated (the reference's Vec<PileupBase>, src/pileup.rs:178-187, has no
    such limit -- a documented deviation), and the context stays usable."""
    import ctypes as C
    L = pp.lib()
    prm = pp.Params(5, 0.5, 0.2)
    for G, ok in (((1 << 32) - 4096, False), (1 << 32, False), (1 << 33, False)):
        off = (C.c_uint64 * 2)(0, G)
        rc = L.pp_polish_begin(ctx._h, 1, off, C.c_void_p(0x1000), pp.MEM_DEVICE, C.byref(prm))
        assert rc == 5 and b"2^32-4096" in L.pp_last_error(ctx._h), (G, rc)
    contig_off, bases, recs = synth.fast_records(seed=2, contig_lens=(4000,), coverage=20)
    got = ctx.polish_records(contig_off, bases, recs)
    assert len(got["polished"]) == 4000


def test_plain_c_host_over_the_abi(orc, tmp_path):
    """examples/polish_min.c: a C99 program that sees nothing but include/polypolish_hip.h (host ingest -> seam B ->
    its own FASTA printing) produces the oracle's bytes."""
    ds = synth.rich_dataset(str(tmp_path), seed=43, contig_lens=(6000, 1200, 300), coverage=25, repeat_len=300,
                            repeat_copies=3, lowercase_frac=0.1)
    want = orc.polish_files(ds["fasta"], [ds["sam1"], ds["sam2"]])
    r = subprocess.run([os.path.join(ROOT, "bin", "polish_min"), ds["fasta"], ds["sam1"], ds["sam2"]], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()[-800:]
    assert r.stdout == want["fasta"]


def _interior_matches(whole, start, piece, slack=1500):
    """The interior of a sub-job's polished bytes must be the full job's bytes for the same stretch of the assembly;
    where that stretch starts in the full output depends on the indels repaired in front of it, so it is searched for
    within +- slack of its assembly coordinate."""
    return whole.find(piece, max(0, start - slack), start + len(piece) + slack) >= 0


@pytest.mark.parametrize("recipe", ["survey", "subs"])
def test_full_size_properties(ctx, pp, orc, recipe):
    """BASELINE.json configs[1] size (5 Mbp, 200x): size-independent properties + exact parity on a window.  'survey' is
    SURVEY 8d's recipe (substitutions, deletions and insertions planted in the assembly, half of the indels in
    homopolymers, reads aligned to the assembly with I / D runs: the case Polypolish exists for, alignment.rs:175-201,
    349-378); 'subs' (substitutions only) keeps coordinates fixed, which is what the idempotence check needs."""
    import torch
    import bench
    dev = torch.device("cuda", 0)
    job = bench.make_job(dev, G=5_000_000, coverage=200, seed=7, recipe=recipe)
    torch.cuda.synchronize()
    bench.run_job(ctx, pp, job)
    a, offs, stats = ctx.result()
    bench.run_job(ctx, pp, job)
    b, _, _ = ctx.result()
    assert a == b, "two runs of the same job differ (atomics must not leak into the result)"
    assert bench.recovered(job, a, offs), f"{bench.recovered(job, a, offs, count=True)} planted assembly errors were not repaired"
    n_err = sum(job["planted"][k] for k in ("substitutions", "deletions", "insertions"))
    assert stats[0]["changed"] >= n_err > 300
    if recipe == "survey":
        p = job["planted"]
        assert min(p["substitutions"], p["deletions"], p["insertions"]) > 100 and p["indels_in_homopolymers"] > 100
        assert len(a) == len(job["truth"]) == job["G"] + p["deletions"] - p["insertions"]
    else:
        # idempotence: polishing the polished assembly with the same reads changes nothing
        job2 = dict(job)
        job2["bases"] = torch.frombuffer(bytearray(a), dtype=torch.uint8).to(dev)
        job2.pop("_prepared", None)
        bench.run_job(ctx, pp, job2)
        c, _, st2 = ctx.result()
        assert c == a and st2[0]["changed"] == 0
    # partition invariance + exact oracle parity on a window of the contig
    lo, hi = 1_000_000, 1_300_000
    sub = bench.subset_job(job, lo, hi)
    torch.cuda.synchronize()
    bench.run_job(ctx, pp, sub)
    s, _, _ = ctx.result()
    want = orc.polish_records(np.array([0, hi - lo], np.uint64), sub["bases"].cpu().numpy(), bench.to_host_records(sub))
    assert s == want["polished"]
    assert _interior_matches(a, lo + 400, s[400:-400])


@pytest.mark.parametrize("config", [2, 3, 4])
def test_full_size_configs(ctx, pp, orc, config):
    """BASELINE.json configs[2], [3], [4] at FULL size on one GPU (records resident, SURVEY 8d's recipe with planted
    indels), through whatever bucketing path their size picks by itself (configs[3] / [4] are beyond 16384 windows):
    determinism, recovery of every planted assembly error (the truth's bytes AND lengths, contig by contig), and exact
    oracle parity + partition invariance on sampled 300 kbp windows (for configs[2] one of them holds a repeat locus:
    five records of share 1/5 per read, on both strands, order-dependent f64 depth)."""
    import torch
    import bench
    dev = torch.device("cuda", 0)
    lens, cov, repeat, _ = bench.config_shape(config)
    job = bench.make_job(dev, contig_lens=lens, coverage=cov, seed=42 + config + 1, repeat=repeat)
    torch.cuda.synchronize()
    coff = job["contig_off"].astype(np.int64)
    bench.run_job(ctx, pp, job)
    a, offs, stats = ctx.result()
    bench.run_job(ctx, pp, job)
    b, _, _ = ctx.result()
    assert a == b, "two runs of the same job differ (atomics must not leak into the result)"
    assert bench.recovered(job, a, offs), f"{bench.recovered(job, a, offs, count=True)} planted assembly errors were not repaired"
    n_err = sum(job["planted"][k] for k in ("substitutions", "deletions", "insertions"))
    assert sum(s["changed"] for s in stats) >= 0.9 * n_err > 300
    # sampled windows: exact oracle parity of the sub-job, and its interior equals the full job's bytes there
    big = int(np.argmax(np.diff(coff)))
    clen = int(coff[big + 1] - coff[big])
    samples = [(big, clen // 3, min(clen, clen // 3 + 300_000)), (len(coff) - 2, 0, min(int(coff[-1] - coff[-2]), 300_000))]
    if repeat:
        samples.append((0, job["repeat_loci"][2] - 100_000, job["repeat_loci"][2] + 200_000))
    offs = np.asarray(offs, dtype=np.int64)
    for c, lo, hi in samples:
        sub = bench.subset_job(job, lo, hi, contig=c)
        torch.cuda.synchronize()
        bench.run_job(ctx, pp, sub)
        s, _, _ = ctx.result()
        want = orc.polish_records(np.array([0, hi - lo], np.uint64), sub["bases"].cpu().numpy(), bench.to_host_records(sub))
        assert s == want["polished"], (config, c, lo, hi)
        assert _interior_matches(a, int(offs[c]) + lo + 400, s[400:-400], slack=20_000), (config, c, lo, hi)


def test_batches_added_one_after_the_other_equal_one_batch(ctx, pp, orc):
    """pp_polish_add several times per job (the reference streams its SAM files, alignment.rs:238-265): any cut of the
    records into batches gives the bytes, depths and statuses of the single batch -- host batches, device batches
    (the first one borrowed in place, then gathered) and a mix; a bad record in a later batch is reported with
    its index in the whole job, and the first one in file order wins."""
    import torch
    o, b, r = synth.fast_records(seed=21, contig_lens=(30_000, 5_000), coverage=40, indel_read_frac=0.1,
                                 k_choices=(1, 1, 2, 3), n_rate=0.003)
    want = orc.polish_records(o, b, r, positions=True)
    n = len(r["contig"])
    for cuts in ([n // 2], [1, 2, n - 1], [n // 3, n // 3 + 1, 2 * n // 3], [0, n]):
        got = ctx.polish_records(o, b, r, positions=True, cuts=cuts)
        assert got["polished"] == want["polished"] and np.array_equal(got["offsets"], want["offsets"]), cuts
        for k in POS_KEYS:
            assert np.array_equal(got["positions"][k], want["positions"][k]), (cuts, k)
    # device-resident batches and a host batch in between
    dev = torch.device("cuda", 0)
    parts = pp.split_records({k: np.ascontiguousarray(r[k], dtype=dt) for k, dt in pp.REC_FIELDS}, [n // 4, n // 2])
    dt = {"contig": torch.int32, "ref_start": torch.int32, "k": torch.int32, "seq_off": torch.int64, "seq_len": torch.int32,
          "cig_off": torch.int64, "n_cig": torch.int32, "seq": torch.uint8, "cigar": torch.int32}
    tens = [{k: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else (v.view(np.int32) if v.dtype == np.uint32 else v))
             .to(dev).to(dt[k]) for k, v in p.items()} for p in parts]
    bases_d = torch.from_numpy(np.ascontiguousarray(b)).to(dev)
    torch.cuda.synchronize()
    for kinds in ((1, 1, 1), (1, 0, 1), (0, 1, 0)):
        ctx.polish_begin(o, bases_d.data_ptr(), pp.MEM_DEVICE)
        for p, t, kd in zip(parts, tens, kinds):
            if kd:
                ctx.polish_add_ptrs(len(p["contig"]), {k: v.data_ptr() for k, v in t.items()}, t["seq"].numel(), t["cigar"].numel(),
                                    pp.MEM_DEVICE)
            else:
                ctx.polish_add_ptrs(len(p["contig"]), {k: v.ctypes.data for k, v in p.items()}, len(p["seq"]), len(p["cigar"]),
                                    pp.MEM_HOST)
        ctx.polish_finish()
        polished, offs, _ = ctx.result()
        assert polished == want["polished"] and np.array_equal(offs, want["offsets"]), kinds
    # errors: record 3 of the second batch and record 1 of the third are bad -> the job reports index n1 + 3
    ref = "ACGGTCATTGCAACGGTTATTGCA" * 3
    bases2 = np.frombuffer(ref.encode(), np.uint8)
    off2 = np.array([0, len(ref)], np.uint64)
    good = (0, 0, 1, ref[:24], [(24, "M")])
    bad = (0, 0, 1, ref[:24], [(23, "M")])
    recs = _rec([good] * 5 + [good, good, good, bad, good] + [good, bad])
    with pytest.raises(pp.PolypolishError) as e:
        ctx.polish_records(off2, bases2, recs, cuts=[5, 10])
    assert e.value.code == pp.ERR_QUIT and "does not match read sequence" in e.value.msg and "record 8" in e.value.msg, e.value


def test_rccl_gather_through_the_library(ctx, pp, orc):
    """pp_comm_* / pp_polish_gather with a communicator of ONE rank (all a one-GPU box can hold): librccl loads,
    ncclCommInitRank + ncclAllGather run on the context's stream, and rank 0's buffer receives the polished bytes
    with the per-contig offsets."""
    import torch
    o, b, r = synth.fast_records(seed=33, contig_lens=(20_000, 3_000), coverage=30, indel_read_frac=0.1)
    want = orc.polish_records(o, b, r)
    c2 = pp.Context(0)
    try:
        c2.comm_init(0, 1, pp.comm_unique_id())
        got = c2.polish_records(o, b, r)
        assert got["polished"] == want["polished"]
        buf = torch.zeros(len(want["polished"]) + 4096, dtype=torch.uint8, device="cuda:0")
        lens, offs = c2.gather(buf.data_ptr(), buf.numel())
        assert int(lens[0]) == len(want["polished"]) and np.array_equal(offs[0], want["offsets"])
        assert bytes(buf[:int(lens[0])].cpu().numpy()) == want["polished"]
    finally:
        c2.close()


@pytest.mark.parametrize("config", [1, 3, 4])
def test_bench_shards_the_real_configs_across_ranks(tmp_path, config):
    """bench.py --gpus 2 --config 3 / 4 (reduced size) with both ranks on this GPU: the native planner, the records split
    on the device, the compact runs and the assembly of the gathered bytes give exactly the bytes ONE GPU produces for
    the whole job (gather_verified).  config 1 = the driver's own multi-GPU launch (weak scaling: every rank its own
    contig; the gathered bytes are the ranks' bytes)."""
    import json
    env = dict(os.environ, PP_BENCH_SHARE_GPU="1", PYTHONPATH=ROOT)
    port = 35000 + os.getpid() % 2000 + config
    r = subprocess.run(["python", "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                        "127.0.0.1", "--master-port", str(port), "bench.py", "--gpus", "2", "--config", str(config),
                        "--genome", "3000000", "--steps", "2", "--warmup", "1", "--full"], capture_output=True, env=env, cwd=ROOT,
                       timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    line = json.loads([l for l in r.stdout.decode().splitlines() if l.startswith("{")][-1])
    assert line["gather_verified"] is True and line["n_gpus"] == 2 and line["scaling"] == ("weak" if config == 1 else "strong"), line
    assert ("window-tile" if config == 4 else "contig-shard") in line["config"]["parallelism"]
    # a multi-GPU record can be read: every rank's kernels and the compute / gather halves of its steps, and (strong
    # scaling) what the whole job takes on one GPU
    assert [r["rank"] for r in line["per_rank"]] == [0, 1] and all("tile" in r["kernel_ms_per_step"] for r in line["per_rank"])
    sp = line["multi_gpu_split"]
    assert sp["compute_ms_per_step_max"] > 0 and sp["gather_ms_per_step_max"] >= 0
    assert (sp["compute_only_speedup"] is None) == (config == 1)
    if config == 1:
        assert line["planted_errors_recovered"] is True and abs(line["value"] * line["ms_per_step"] / 1e3 - 6.0) < 0.01  # 2 x 3 Mbp per step


@pytest.mark.parametrize("n_ctx", [2, 3])
def test_cli_polishes_on_several_contexts_in_one_process(orc, tmp_path, n_ctx):
    """bin/polypolish polish with PP_SHARE_GPU=n: n contexts (here all on this GPU, on a multi-GPU box one per device).
    Default: every context uploads and tokenizes its own slice of each SAM file (cut at read-group boundaries), the
    records are split on the device and travel context to context; PP_DEVICE_INGEST=0: one host parse, host split, every
    context is sent its part.  Either way the assembled FASTA and the per-contig figures of the log are those of the
    single-context run / the oracle.  The dataset has repeats (groups of three records with SEQ '*', k = 3)."""
    ds = synth.rich_dataset(str(tmp_path), seed=83, contig_lens=(140_000, 900, 2_000, 30_000), coverage=12, repeat_len=300,
                            repeat_copies=3)
    sams = [ds["sam1"], ds["sam2"]]
    exe = os.path.join(ROOT, "bin", "polypolish")
    single = subprocess.run([exe, "polish", ds["fasta"], *sams], capture_output=True, env=dict(os.environ, PP_DEVICE="0"),
                            timeout=600)
    want = orc.polish_files(ds["fasta"], sams)["fasta"]
    stat = lambda err: [l for l in err.decode().splitlines() if "changed" in l or "depth of zero" in l or "mean read depth" in l
                        or "alignments" in l]
    for ingest in ("1", "0"):
        multi = subprocess.run([exe, "polish", ds["fasta"], *sams], capture_output=True,
                               env=dict(os.environ, PP_SHARE_GPU=str(n_ctx), PP_DEVICE_INGEST=ingest), timeout=600)
        assert multi.returncode == 0, (ingest, multi.stderr.decode()[-2000:])
        assert multi.stdout == want == single.stdout, ingest
        assert stat(multi.stderr) == stat(single.stderr) and len(stat(multi.stderr)) > 12, ingest


def test_one_process_driver_gathers_over_the_communicator_and_survives_a_rank_that_never_joins(orc, tmp_path):
    """VERDICT r5 item 8 / ADVICE r4.  The one-process multi-GPU driver's RCCL route (PP_GATHER=rccl: pp_comm_init from one
    thread per context, pp_polish_gather's AllGather of sizes + one group of Send / Recv, one D2H) has never run with more
    than one rank -- RCCL refuses two ranks on one device.  With tests/fake_rccl.cpp as the communicator library (PP_RCCL_LIB:
    the same nine entry points, ranks as threads of one process on one device) it runs here with 2 and 3 contexts and gives
    the oracle's bytes.  And a rank that fails before it joins (FAKE_RCCL_FAIL_RANK: its ncclCommInitRank returns an error, the
    others wait for it as RCCL's would, for good) no longer keeps the command: pp_comm_init gives up after PP_COMM_TIMEOUT
    seconds, the driver falls back to the route where every device copies its share out, same bytes."""
    import time
    ds = synth.rich_dataset(str(tmp_path), seed=91, contig_lens=(120_000, 2_000, 40_000), coverage=12, repeat_len=300, repeat_copies=3)
    sams = [ds["sam1"], ds["sam2"]]
    exe = os.path.join(ROOT, "bin", "polypolish")
    fake = os.path.join(str(tmp_path), "librccl_fake.so")
    b = subprocess.run(["hipcc", "-shared", "-fPIC", "-std=c++17", os.path.join(ROOT, "tests", "fake_rccl.cpp"), "-o", fake],
                       capture_output=True, timeout=300)
    assert b.returncode == 0, b.stderr.decode()[-2000:]
    want = orc.polish_files(ds["fasta"], sams)["fasta"]
    for n_ctx in (2, 3):
        r = subprocess.run([exe, "polish", ds["fasta"], *sams], capture_output=True, timeout=300,
                           env=dict(os.environ, PP_SHARE_GPU=str(n_ctx), PP_GATHER="rccl", PP_RCCL_LIB=fake, PP_TIMING="1"))
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        assert b"ONE RCCL gather" in r.stderr, r.stderr.decode()[-2000:]
        assert r.stdout == want, n_ctx
    t0 = time.time()
    r = subprocess.run([exe, "polish", ds["fasta"], *sams], capture_output=True, timeout=120,
                       env=dict(os.environ, PP_SHARE_GPU="3", PP_GATHER="rccl", PP_RCCL_LIB=fake, PP_TIMING="1", FAKE_RCCL_FAIL_RANK="1",
                                PP_COMM_TIMEOUT="3"))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert b"every device copies its share out" in r.stderr and r.stdout == want
    assert time.time() - t0 < 60


@pytest.mark.parametrize("world", [3, 8])
def test_device_split_equals_host_split(ctx, pp, orc, world):
    """pp_shard_split on a device batch (kernels: flag, scans, gather of the SoA / SEQ bytes / CIGAR runs) gives the part
    the host loop gives, array by array incl. orig, on a job with whole-contig units and a tiled contig, indel reads and two
    records that touch no unit; and polishing a rank's part with its emit ranges gives the bytes of polishing ALL records
    with them (device engine)."""
    import ctypes as C
    import torch
    contig_off, bases, recs = synth.fast_records(seed=24, contig_lens=(90_000, 700, 12_000, 5_000), coverage=30, read_len=120,
                                                 k_choices=(1, 2, 3), k_probs=(0.8, 0.1, 0.1), indel_read_frac=0.2)
    recs = {k: v.copy() for k, v in recs.items()}
    n = len(recs["contig"])
    plan = pp.Plan(contig_off, np.bincount(recs["contig"], minlength=4), world, 4096)
    odd = {k: v.copy() for k, v in recs.items()}
    odd["contig"][5] = 77
    odd["ref_start"][9] = 10 ** 7
    dev = torch.device("cuda", 0)
    keep = {k: torch.from_numpy(np.ascontiguousarray(odd[k], dtype=dt).view(np.int64 if dt == np.uint64 else (np.int32 if dt == np.uint32 else np.uint8))).to(dev)
            for k, dt in pp.REC_FIELDS}
    torch.cuda.synchronize()
    L = pp.lib()
    total = 0
    def parts_agree(src, keep_t, r):
        want, want_orig = pp.shard_split_host(plan, r, src)
        ptrs_t = {k: v.data_ptr() for k, v in keep_t.items() if k != "wo"}
        if "wo" in keep_t:
            ptrs_t["wo"] = keep_t["wo"].data_ptr()
        part = pp.ShardPart(ctx, plan, r, n, ptrs_t, keep_t["seq"].numel(), keep_t["cigar"].numel(), pp.MEM_DEVICE)
        # the window-order mirror goes along into the part: the source's entries of the part's records, in the source's order,
        # renumbered -- on the device as on the host
        assert ("wo" in part.ptrs) == ("wo" in want) == ("wo" in src and len(want_orig) > 0), r
        if "wo" in want:
            w = np.zeros(part.n_aln, dtype=pp.WO_DTYPE)
            assert L.pp_ctx_download(ctx._h, w.ctypes.data, part.ptrs["wo"], w.nbytes) == 0
            assert all(np.array_equal(w[k], want["wo"][k]) for k in pp.WO_DTYPE.names), r
            check_window_order_mirror(want, contig_off, [len(want_orig)])
        assert part.n_aln == len(want_orig) and part.seq_bytes == len(want["seq"]) and part.n_cig_total == len(want["cigar"]), r
        sizes = {"seq": part.seq_bytes, "cigar": part.n_cig_total}
        for name, dt in pp.REC_FIELDS:
            cnt = int(sizes.get(name, part.n_aln))
            got = np.zeros(cnt, dtype=dt)
            if cnt:
                assert L.pp_ctx_download(ctx._h, got.ctypes.data, part.ptrs[name], got.nbytes) == 0
            assert np.array_equal(got, want[name]), (r, name)
        orig = np.zeros(part.n_aln, dtype=np.uint32)
        if part.n_aln:
            assert L.pp_ctx_download(ctx._h, orig.ctypes.data, part.orig_ptr, orig.nbytes) == 0
        assert np.array_equal(orig, want_orig), r
        # a device part brings the 4-bit mirror of its seq array
        assert "seq4" in part.ptrs
        m = np.zeros((part.seq_bytes + 1) // 2, dtype=np.uint8)
        if m.size:
            assert L.pp_ctx_download(ctx._h, m.ctypes.data, part.ptrs["seq4"], m.nbytes) == 0
            assert np.array_equal(m[:part.seq_bytes // 2], pp.pack_seq4(want["seq"])[:part.seq_bytes // 2]), r
        cnt_part = part.n_aln
        part.close()
        return want, cnt_part
    for r in range(world):
        total += parts_agree(odd, keep, r)[1]
    assert n <= total < 1.2 * n
    # The same from a batch laid out as the library's ingests lay one out (rooms of PP_SEQ_ALIGN bytes, the SEQ bytes NOT in
    # the order of the records: here shuffled, as window-grouping shuffles them): a part keeps the order of the source's seq
    # array -- a window-grouped batch gives window-grouped parts -- on the device (a scan over the array's 32-byte slots)
    # as on the host (a sort), and the two agree array by array.
    rng = np.random.default_rng(5)
    sl = odd["seq_len"].astype(np.int64)
    room = (sl + 31) & ~31
    perm = rng.permutation(n)
    place = np.zeros(n, dtype=np.int64)
    place[perm] = np.cumsum(room[perm]) - room[perm]
    shuf = {k: v.copy() for k, v in odd.items()}
    shuf["seq"] = np.zeros(int(room.sum()), dtype=np.uint8)
    for i in range(n):
        shuf["seq"][place[i]:place[i] + sl[i]] = odd["seq"][int(odd["seq_off"][i]):int(odd["seq_off"][i]) + sl[i]]
    shuf["seq_off"] = place.astype(np.uint64)
    keep2 = {k: torch.from_numpy(np.ascontiguousarray(shuf[k], dtype=dt).view(np.int64 if dt == np.uint64 else (np.int32 if dt == np.uint32 else np.uint8))).to(dev)
             for k, dt in pp.REC_FIELDS}
    torch.cuda.synchronize()
    shuf["wo"] = pp.window_order_mirror(shuf, contig_off)   # (the odd records 5 and 9 included: a mirror holds every record)
    keep2["wo"] = torch.from_numpy(np.ascontiguousarray(shuf["wo"]).view(np.uint8)).to(dev)
    torch.cuda.synchronize()
    for r in range(world):
        want, _ = parts_agree(shuf, keep2, r)
        if len(want["contig"]) > 1:  # the part's SEQ bytes follow the source's seq array, not the records
            src_order = np.argsort(shuf["seq_off"][pp.shard_split_host(plan, r, shuf)[1]], kind="stable")
            assert (np.diff(want["seq_off"][src_order].astype(np.int64)) > 0).all(), r
    cnt = pp.shard_count(ctx, n, keep["contig"].data_ptr(), pp.MEM_DEVICE, 4, {k: v.data_ptr() for k, v in keep.items()})
    assert np.array_equal(cnt.astype(np.int64), np.bincount(odd["contig"][odd["contig"] < 4], minlength=4))
    for r in range(world):  # the property the partition exists for, on the device engine
        part, _ = pp.shard_split_host(plan, r, recs)
        e = plan.emit_ranges(r)
        a = ctx.polish_records(contig_off, bases, part, emit=e)
        b = ctx.polish_records(contig_off, bases, recs, emit=e)
        assert a["polished"] == b["polished"] and np.array_equal(a["offsets"], b["offsets"]), r


def test_several_contexts_report_the_first_bad_record_of_the_job(orc, tmp_path):
    """Records with defects that only the CIGAR walk finds, on a job sharded over three contexts: every context numbers
    the records it was sent, the job's error is the one about the FIRST bad record in file order with its job-wide
    number -- the message of the single-context run (src/alignment.rs:238-303: the reference streams)."""
    ref = "ACGGTCATTGCAACGGTTATTGCAGGCTTAACGTAGCTAGGCTTAGCATCGATCAGGCTAACGTTAGCCTAGAT" * 120
    fa = tmp_path / "a.fasta"
    fa.write_text(">c\n" + ref + "\n>d\n" + ref[:3000] + "\n")
    rng = np.random.default_rng(3)

    def line(name, ctg, pos, cigar, n, tags="NM:i:0"):
        return f"{name}\t0\t{ctg}\t{pos}\t60\t{cigar}\t*\t0\t0\t{ref[pos - 1:pos - 1 + n]}\t*\t{tags}\n"
    recs = [line(f"g{i}", "c" if i % 5 else "d", 1 + int(rng.integers(0, 2900 if i % 5 == 0 else 8700)), "40M", 40) for i in range(4000)]
    exe = os.path.join(ROOT, "bin", "polypolish")
    err = lambda r: [l for l in r.stderr.decode().splitlines() if l.startswith("Error:")]
    for at in ((700, 3100), (3100, 700), (2000,)):
        lines = list(recs)
        for j, a in enumerate(at):
            lines[a] = line(f"bad{j}", "c", 8000 - 7000 * j, "10M4N26M" if j == 0 else "39M", 36 if j == 0 else 40)
        sam = tmp_path / "bad.sam"
        sam.write_text("".join(lines))
        single = subprocess.run([exe, "polish", str(fa), str(sam)], capture_output=True, env=dict(os.environ, PP_DEVICE="0"))
        assert single.returncode == 1 and f"alignment record {min(at)}".encode() in single.stderr, single.stderr[-300:]
        for ingest in ("1", "0"):
            multi = subprocess.run([exe, "polish", str(fa), str(sam)], capture_output=True,
                                   env=dict(os.environ, PP_SHARE_GPU="3", PP_DEVICE_INGEST=ingest))
            assert multi.returncode == 1 and multi.stdout == b""
            assert err(multi) == err(single), (at, ingest, multi.stderr[-400:])
    # The defect in a SECOND file: the 4000 good records in the first one, the bad record among a few hundred of the second
    # -- and the same with a line the parsers refuse further down that file: the records in front of it are then replayed,
    # the first context taking the first file's batch whole, and the walk's error about the bad record stands.
    first, second = tmp_path / "first.sam", tmp_path / "second.sam"
    first.write_text("".join(recs))
    tail = list(recs[:300])
    tail[120] = line("bad0", "c", 8000, "10M4N26M", 36)
    for parse_bad in ("", "p\t0\tc\t9\t60\t40M\n"):
        second.write_text("".join(tail[:200]) + parse_bad + "".join(tail[200:]))
        cmd = [exe, "polish", str(fa), str(first), str(second)]
        single = subprocess.run(cmd, capture_output=True, env=dict(os.environ, PP_DEVICE="0"))
        assert single.returncode == 1 and len(err(single)) == 1 and "alignment record" in err(single)[0], single.stderr[-300:]
        for ingest in ("1", "0"):
            multi = subprocess.run(cmd, capture_output=True, env=dict(os.environ, PP_SHARE_GPU="3", PP_DEVICE_INGEST=ingest))
            assert multi.returncode == 1 and multi.stdout == b""
            assert err(multi) == err(single), (bool(parse_bad), ingest, multi.stderr[-400:])


def test_two_defects_are_reported_in_streaming_order(orc, tmp_path):
    """A file with TWO independent defects: one that only the CIGAR walk finds (the device: an N run inside the CIGAR, a
    CIGAR shorter than SEQ) and one the parse finds (too few columns, a missing NM tag).  The reference streams and
    stops at whichever comes first -- with the read group that is still pending at a failing line NOT yet processed
    (alignment.rs:238-303).  Exit code and the kind of message must be the oracle's, with either ingest, also when
    the two defects sit in different SAM files."""
    ref = "ACGGTCATTGCAACGGTTATTGCAGGCTTAACGTAGCTAGGCTTAGCATCGATCAGGCTAACGTTAGCCTAGAT" * 4
    fa = tmp_path / "a.fasta"
    fa.write_text(">c\n" + ref + "\n")

    def line(name, pos, cigar, n, tags="NM:i:0"):
        return f"{name}\t0\tc\t{pos}\t60\t{cigar}\t*\t0\t0\t{ref[pos - 1:pos - 1 + n]}\t*\t{tags}\n"
    good = [line(f"g{i}", 1 + 3 * i, "40M", 40) for i in range(30)]
    walk_bad = line("w", 5, "10M4N26M", 36)        # passes the gates (M at both ends), the walk rejects the N
    walk_bad2 = line("w2", 7, "39M", 40)            # CIGAR does not match SEQ
    parse_bad = "p\t0\tc\t9\t60\t40M\n"             # too few columns
    parse_bad2 = line("p2", 11, "40M", 40, tags="XS:i:1")   # aligned but no NM tag
    exe = os.path.join(ROOT, "bin", "polypolish")
    orc_exe = os.path.join(ROOT, "oracle", "_build", "pp_oracle")
    cases = {
        "walk_then_parse": [good[:10] + [walk_bad] + good[10:20] + [parse_bad] + good[20:]],
        "parse_then_walk": [good[:10] + [parse_bad] + good[10:20] + [walk_bad] + good[20:]],
        "walk_in_the_pending_group": [good[:10] + [walk_bad, parse_bad2] + good[10:]],   # w is pending when p2 fails
        "walk_flushed_by_the_failing_line": [good[:10] + [walk_bad2, good[10], parse_bad] + good[11:]],
        "walk_in_file_1_parse_in_file_2": [good[:10] + [walk_bad] + good[10:], good[:5] + [parse_bad2] + good[5:]],
        "parse_in_file_1_walk_in_file_2": [good[:10] + [parse_bad] + good[10:], good[:5] + [walk_bad] + good[5:]],
    }
    kinds = (b"unexpected character", b"does not match read sequence", b"too few columns", b"missing NM tag")
    for name, files in cases.items():
        paths = []
        for i, lines in enumerate(files):
            p = tmp_path / f"{name}_{i}.sam"
            p.write_text("@SQ\tSN:c\tLN:%d\n" % len(ref) + "".join(lines))
            paths.append(str(p))
        want = subprocess.run([orc_exe, "polish", str(fa)] + paths, capture_output=True)
        assert want.returncode != 0, name
        want_kind = [k for k in kinds if k in want.stderr]
        assert len(want_kind) == 1, (name, want.stderr)
        # (the third: the records in front of the defect, the earlier file's included, sit in ONE host ingest object)
        for ingest in (dict(PP_DEVICE_INGEST="1"), dict(PP_DEVICE_INGEST="0"), dict(PP_DEVICE_INGEST="0", PP_STREAM_ADDS="0")):
            got = subprocess.run([exe, "polish", str(fa)] + paths, capture_output=True, env=dict(os.environ, **ingest))
            assert got.returncode == want.returncode and got.stdout == b"", (name, ingest, got.stderr)
            assert want_kind[0] in got.stderr, (name, ingest, want.stderr, got.stderr)


def test_one_percent_of_the_reads_with_three_scattered_alignments(ctx, orc):
    """The replay's worst case: at 200x, 1 % of the reads have three alignments (share 1/3,
    order-dependent f64 depth) scattered over the contig, so EVERY window has positions whose depth depends on the
    order of the additions -- ties at x.5 of depth * fraction_valid included.  Per-position f64 depth, thresholds,
    status and bytes against the oracle; the small and the large instance of the replay kernel both run (the second
    contig is 3x as deep)."""
    contig_off, bases, recs = synth.fast_records(seed=71, contig_lens=(300_000,), coverage=200, k_choices=(1, 3),
                                                 k_probs=(0.99, 0.01), indel_read_frac=0.01)
    want, got = _compare_records(ctx, orc, contig_off, bases, recs)
    nd_touched = int((want["positions"]["depth"] != np.floor(want["positions"]["depth"])).sum())
    assert nd_touched > 100_000
    contig_off, bases, recs = synth.fast_records(seed=72, contig_lens=(30_000,), coverage=900, k_choices=(1, 3),
                                                 k_probs=(0.97, 0.03), indel_read_frac=0.01)
    _compare_records(ctx, orc, contig_off, bases, recs)   # ~13 K items per window: the 128 KiB instance


def _with_hot_region(seed, length, coverage, hot_lo, hot_hi, hot_coverage, **hot_kw):
    """fast_records over one contig plus a pile of extra reads that start in [hot_lo, hot_hi) (same truth and assembly:
    the generator draws them first from the seed) -- a collapsed repeat."""
    contig_off, bases, base = synth.fast_records(seed=seed, contig_lens=(length,), coverage=coverage, indel_read_frac=0.01)
    off2, bases2, deep = synth.fast_records(seed=seed, contig_lens=(length,), coverage=hot_coverage, **hot_kw)
    assert np.array_equal(bases, bases2)
    keep = np.nonzero((deep["ref_start"] >= hot_lo) & (deep["ref_start"] < hot_hi))[0]
    hot = dict(deep)
    for k in ("contig", "ref_start", "k", "seq_len", "n_cig", "seq_off", "cig_off"):
        hot[k] = np.ascontiguousarray(deep[k][keep])
    return contig_off, bases, synth.merge_records(base, hot, seed=seed)


def test_heavy_windows_are_split_over_helper_blocks(ctx, pp, orc):
    """Collapsed repeats (BASELINE configs[2] in miniature): a few windows hold many times the average number of items.
    They are listed as heavy: k_tile tallies each of them with eight helper blocks that meet in a global slab, and
    the ordered replay (shares 1/3 and 1/5 in the pile) runs with one block per 256 positions.  Everything per
    position against the oracle, twice on the same context (the slabs clean themselves), then (b) a pile too deep for
    the sub-range blocks to sort (they hand their positions to the thread-serial replay) and (c) the same job cut
    into emit ranges through the pile."""
    contig_off, bases, recs = _with_hot_region(81, 40_000, 100, 19_000, 23_000, 1500, k_choices=(1, 3, 5),
                                               k_probs=(0.6, 0.2, 0.2), indel_read_frac=0.02)
    starts = recs["ref_start"].astype(np.int64)
    w_first, w_last = starts // 2048, (starts + 149) // 2048
    per_window = np.bincount(w_first, minlength=20) + np.bincount(w_last[w_last != w_first], minlength=20)
    assert per_window.max() > 16384 and np.median(per_window) < 2000   # heavy, and beyond the one-block replay
    for _ in range(2):
        want, got = _compare_records(ctx, orc, contig_off, bases, recs)
    assert len(np.unique(want["positions"]["depth"][19_000:23_000])) > 500
    # (c) emit ranges that cut through the pile
    full = want["polished"]
    pieces = []
    for lo, hi in ((0, 20_480), (20_480, 21_000), (21_000, 40_000)):
        r = ctx.polish_records(contig_off, bases, recs, emit=np.array([[lo, hi]]))
        pieces.append(r["polished"])
    assert b"".join(pieces) == full
    # (b) one window at ~6000x: ~80 K items, more than 10 K for each of its sub-range blocks
    contig_off, bases, recs = _with_hot_region(82, 30_000, 60, 10_240, 12_100, 6000, k_choices=(1, 3), k_probs=(0.9, 0.1),
                                               indel_read_frac=0.0)
    _compare_records(ctx, orc, contig_off, bases, recs)


def test_filter_only_fails_on_an_unparseable_cigar_when_it_needs_it(tmp_path):
    """get_ref_end is lazy (src/alignment.rs:138-149: run lengths are parsed when an alignment's end is asked for): a
    CIGAR with a length beyond 64 bits is only fatal -- a panic, exit 101 -- if that alignment takes part in a pair
    comparison (src/filter.rs:189-218, 352-377).  Lone alignments and single alignments that are never paired up (the
    mate on another contig) pass through untouched.  Output bytes and exit codes against the oracle's CLI, both loaders."""
    exe = os.path.join(ROOT, "bin", "polypolish")
    orc_exe = os.path.join(ROOT, "oracle", "_build", "pp_oracle")
    huge = "9" * 25 + "M"
    head = "@SQ\tSN:c\tLN:100000\n@SQ\tSN:d\tLN:100000\n"

    def line(name, flag, pos, cigar="50M", ref="c"):
        return f"{name}\t{flag}\t{ref}\t{pos}\t60\t{cigar}\t*\t0\t0\t{'A' * 50}\t{'I' * 50}\tNM:i:0\n"
    pairs1 = "".join(line(f"p{i}", 0, 100 + 7 * i) for i in range(40))
    pairs2 = "".join(line(f"p{i}", 16, 400 + 7 * i) for i in range(40))
    cases = {
        # a read whose mate has no alignment: never compared
        "lone": (pairs1 + line("lone", 0, 50, huge), pairs2, 0),
        # a read with ONE alignment and a mate: passes without a comparison (filter.rs:361-363) -- but it takes part in
        # the threshold sampling (one alignment per read, same reference): evaluated there
        "sampled": (pairs1 + line("s", 0, 50, huge), pairs2 + line("s", 16, 300), 101),
        # two alignments for the read, the mate's only alignment is fine: both ends are needed for the comparison
        "compared": (pairs1 + line("m", 0, 50, huge) + line("m", 256, 900), pairs2 + line("m", 16, 350), 101),
        # one alignment each, on different contigs: not sampled (filter.rs:160), and each passes as its read's only
        # alignment without a comparison
        "different_reference": (pairs1 + line("x", 0, 50, huge), pairs2 + line("x", 16, 300, ref="d"), 0),
    }
    for name, (t1, t2, want_rc) in cases.items():
        a, b = tmp_path / f"{name}_1.sam", tmp_path / f"{name}_2.sam"
        a.write_text(head + t1)
        b.write_text(head + t2)
        outs = {}
        for who, binary, env in (("oracle", orc_exe, {}), ("host", exe, {}), ("device", exe, {"PP_DEVICE_FILTER": "1"})):
            o1, o2 = tmp_path / f"{name}_{who}_1.out", tmp_path / f"{name}_{who}_2.out"
            r = subprocess.run([binary, "filter", "--in1", str(a), "--in2", str(b), "--out1", str(o1), "--out2", str(o2)],
                               capture_output=True, env=dict(os.environ, **env))
            assert r.returncode == want_rc, (name, who, r.returncode, r.stderr.decode()[-600:])
            outs[who] = (o1.read_bytes(), o2.read_bytes()) if want_rc == 0 else None
        assert outs["host"] == outs["oracle"] and outs["device"] == outs["oracle"], name


def test_device_front_ends_hand_non_ascii_text_to_the_host_parsers(orc, tmp_path):
    """The device tokenizer and the device filter loader only notice THAT a file holds bytes outside ASCII (newline pass);
    which lines are valid UTF-8 -- the reference refuses the others -- is the host parsers' call: the drivers fall back.
    CLI against the oracle's CLI: valid UTF-8 in a tag changes nothing, an invalid byte ends the load."""
    ds = synth.rich_dataset(str(tmp_path), seed=96, contig_lens=(1500,), coverage=8)
    exe = os.path.join(ROOT, "bin", "polypolish")
    orc_exe = os.path.join(ROOT, "oracle", "_build", "pp_oracle")
    base1 = open(ds["sam1"], "rb").read().split(b"\n")
    body = [i for i, l in enumerate(base1) if l and not l.startswith(b"@")]
    for name, blob, ok in (("valid", "日本".encode(), True), ("invalid", b"\xff", False)):
        i = body[len(body) // 2]
        f1 = tmp_path / f"{name}_1.sam"
        f1.write_bytes(b"\n".join(base1[:i] + [base1[i] + b"\tXX:Z:" + blob] + base1[i + 1:]))
        want = subprocess.run([orc_exe, "polish", ds["fasta"], str(f1), ds["sam2"]], capture_output=True)
        assert (want.returncode == 0) == ok
        logs = {}
        for ingest in ("1", "0"):
            got = subprocess.run([exe, "polish", ds["fasta"], str(f1), ds["sam2"]], capture_output=True,
                                 env=dict(os.environ, PP_DEVICE_INGEST=ingest))
            assert got.returncode == want.returncode and got.stdout == want.stdout, (name, ingest, got.stderr[-500:])
            if not ok:
                assert b"unable to load alignments" in got.stderr and b"unable to load alignments" in want.stderr
            logs[ingest] = [l for l in got.stderr.split(b"\n") if not l.startswith(b"Time to run")]
        # the run log (polish.rs:41-90, 109-134, 206-227) is the same whether the file went through the device tokenizer
        # and came back (the hand-over resumes the log at that file) or through the host parsers from the start
        assert logs["1"] == logs["0"], name
        if ok:
            assert any(l.startswith(b"Finished!") for l in logs["1"]) and sum(b"alignments from" in l for l in logs["1"]) == 2
        outs = {}
        for who, binary, env in (("oracle", orc_exe, {}), ("host", exe, {}), ("device", exe, {"PP_DEVICE_FILTER": "1"})):
            o1, o2 = tmp_path / f"{name}_{who}_1.out", tmp_path / f"{name}_{who}_2.out"
            r = subprocess.run([binary, "filter", "--in1", str(f1), "--in2", ds["sam2"], "--out1", str(o1), "--out2", str(o2)],
                               capture_output=True, env=dict(os.environ, **env))
            assert (r.returncode == 0) == ok, (name, who, r.stderr[-500:])
            outs[who] = (o1.read_bytes(), o2.read_bytes()) if ok else r.returncode
        assert outs["host"] == outs["oracle"] == outs["device"], name


def test_replays_are_left_out_after_a_clean_job_and_come_back_when_needed(ctx, orc):
    """A context whose job before flagged nothing for the exact replays (k_exact2 / k_exact) leaves their launches out, and
    runs them -- and the emission once more -- when this job's metadata say something was flagged after all
    (run_pipeline, round 5).  A clean job, then one with order-dependent depths and insertions, then a clean one again:
    every one of them bit-identical to the oracle, whichever way it went."""
    clean = synth.fast_records(seed=71, contig_lens=(30_000,), coverage=40, indel_read_frac=0.0, n_rate=0.0)
    odd = synth.fast_records(seed=72, contig_lens=(30_000, 2_500), coverage=50, k_choices=(1, 2, 3, 5, 6, 7),
                             k_probs=(0.5, 0.1, 0.1, 0.1, 0.1, 0.1), indel_read_frac=0.2, n_rate=0.01)
    import polypolish_amd as pp
    for contig_off, bases, recs in (clean, clean, odd, odd, clean, odd):
        want = orc.polish_records(contig_off, bases, recs)
        got = ctx.polish_records(contig_off, bases, recs)
        assert got["polished"] == want["polished"] and np.array_equal(got["offsets"], want["offsets"])
        m = _polish_device_batch(ctx, pp, contig_off, bases, recs, True, wo=True)   # ... and over the direct path
        assert m["polished"] == want["polished"] and np.array_equal(m["offsets"], want["offsets"])


def test_a_foreign_window_order_mirror_is_checked_before_it_is_used(orc, tmp_path):
    """pp_aln_batch.wo is a hint: every result is the same with and without it (include/polypolish_hip.h).  A mirror that is not
    one of the library's own (its ingests', pp_shard_split's -- a registry of their address ranges) is compared with the arrays
    it mirrors before anything reads the records through it: every entry a record of the batch, none twice, every field the
    record's.  A faithful mirror passes -- in run order (the direct path), shuffled, without a run
    table --; one that names a record twice, one out of range, one with a wrong field (an altered ref_start, a wrong k) is
    left aside and the job gives the oracle's bytes over the bucketing path, never other bytes, never an error
    (/root/reference src/alignment.rs:297-303: every good alignment is applied exactly as parsed)."""
    code = """
import sys, os, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import torch, synth, polypolish_amd as pp
import test_gpu_parity as tg
from oracle import orc
ctx = pp.Context(0)
o, b, r = synth.fast_records(seed=2, contig_lens=(40_000, 7_000), coverage=40, indel_read_frac=0.2)
want = orc.polish_records(o, b, r)["polished"]
real = pp.window_order_mirror
for order in (True, "shuffled", "no_runs"):
    assert tg._polish_device_batch(ctx, pp, o, b, r, True, wo=order)["polished"] == want
    assert ctx.took_direct_path() == (order is True), order
def broken(kind):
    def make(recs, off):
        w = real(recs, off)
        if kind == "twice": w["file_idx"][7] = w["file_idx"][8]
        if kind == "range": w["file_idx"][5] = len(w) + 3
        if kind == "field": w["ref_start"][11] += 1
        if kind == "k": w["k"][3] += 1
        if kind == "seq_off": w["seq_off"][9] += 32
        return w
    return make
for kind in ("twice", "range", "field", "k", "seq_off"):
    pp.window_order_mirror = broken(kind)
    for order in (True, "no_runs"):
        got = tg._polish_device_batch(ctx, pp, o, b, r, True, wo=order)
        assert got["polished"] == want, (kind, order)
        assert not ctx.took_direct_path(), (kind, order)
print("mirror check ok")
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run(["python", "-c", code], capture_output=True, env=dict(os.environ), timeout=600)
    assert r.returncode == 0 and b"mirror check ok" in r.stdout, r.stderr.decode()[-2000:]


def test_extras_room_is_capped_and_a_deep_window_takes_the_bucketing_path(orc):
    """the direct path gives every window the same room for extras, so one deep window would set it for all of
    them.  The room is capped (PP_XENT_BUDGET bytes for all windows together, never below the job's own estimate); a window
    that needs more sends the job over the bucketing path -- same bytes, no error.  Here the budget is one byte and most reads
    carry an indel (every piece of such a read is an extra)."""
    code = """
import sys, os, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import torch, synth, polypolish_amd as pp
import test_gpu_parity as tg
from oracle import orc
ctx = pp.Context(0)
o, b, r = synth.fast_records(seed=5, contig_lens=(30_000,), coverage=300, indel_read_frac=0.9)
want = orc.polish_records(o, b, r)["polished"]
got = tg._polish_device_batch(ctx, pp, o, b, r, True, wo=True)
assert got["polished"] == want
assert not ctx.took_direct_path()
print("capped ok")
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run(["python", "-c", code], capture_output=True, env=dict(os.environ, PP_XENT_BUDGET="1"), timeout=600)
    assert r.returncode == 0 and b"capped ok" in r.stdout, r.stderr.decode()[-2000:]


def test_a_record_whose_seq_lies_outside_the_seq_array_is_refused(ctx, pp):
    """seq_off + seq_len beyond seq_bytes was only caught where it passed 2^40.  Both paths refuse the record (the
    caller broke the batch's contract: PP_ERR_ARG), naming it."""
    o, b, r = synth.fast_records(seed=8, contig_lens=(20_000,), coverage=20)
    r = dict(r)
    r["seq_off"] = r["seq_off"].copy()
    r["seq_off"][17] = len(r["seq"]) - 5
    for wo in (True, None):
        with pytest.raises(pp.PolypolishError) as e:
            _polish_device_batch(ctx, pp, o, b, r, True, wo=wo)
        assert e.value.code == pp.ERR_ARG and "record 17" in e.value.msg and "seq array" in e.value.msg, e.value.msg


def test_filter_seam_verdicts_with_and_without_the_sampling_call(ctx, pp):
    """Seam A at the ABI: pp_filter_pairs right after pp_filter_begin (the pass over the reads has not run yet) gives the
    verdicts pp_filter_begin -> pp_filter_samples -> pp_filter_pairs gives, and both are alignment_pass_qc
    (src/filter.rs:352-377) restated here in plain loops -- reads with 0..3 alignments per file, two contigs, I/D/S runs."""
    import ctypes as C
    rng = np.random.default_rng(77)
    n_reads = 3000

    def make_file():
        cnt = rng.choice([0, 1, 1, 1, 2, 3], n_reads)
        grp_off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
        n = int(grp_off[-1])
        perm = rng.permutation(n).astype(np.uint32)          # file order differs from group order
        read = np.empty(n, np.uint32)
        read[perm] = np.repeat(np.arange(n_reads, dtype=np.uint32), cnt)
        runs, off = [], []
        for _ in range(n):
            off.append(len(runs))
            m = int(rng.integers(1, 4))
            for j in range(m):
                runs.append((int(rng.integers(1, 120)) << 4) | int(rng.choice([0, 0, 1, 2, 4, 7, 8])))
        arr = dict(ref_id=rng.integers(0, 2, n).astype(np.uint32), ref_start=rng.integers(0, 5000, n).astype(np.uint32),
                   flags=rng.choice([0, 16], n).astype(np.uint32), cig_off=np.array(off, np.uint64),
                   n_cig=np.diff(np.array(off + [len(runs)])).astype(np.uint32), cigar=np.array(runs, np.uint32), read=read,
                   grp_off=grp_off, grp_idx=perm)
        f = pp.FilterFile(n, arr["ref_id"].ctypes.data, arr["ref_start"].ctypes.data, arr["flags"].ctypes.data,
                          arr["cig_off"].ctypes.data, arr["n_cig"].ctypes.data, arr["cigar"].ctypes.data, len(runs),
                          arr["read"].ctypes.data, arr["grp_off"].ctypes.data, arr["grp_idx"].ctypes.data)
        end = arr["ref_start"].astype(np.int64).copy()
        for a in range(n):
            for op in arr["cigar"][off[a]:off[a] + arr["n_cig"][a]]:
                if (op & 15) in (0, 2, 3, 7, 8):
                    end[a] += op >> 4
        arr["end"] = end
        return f, arr
    f1, a1 = make_file()
    f2, a2 = make_file()
    inp = pp.FilterInput(n_reads, (pp.FilterFile * 2)(f1, f2))
    low, high, correct = 100, 900, 0

    def orientation(fl1, s1, e1, fl2, s2, e2):               # filter.rs:189-209
        fw1, fw2 = not fl1 & 16, not fl2 & 16
        p1, p2 = (s1 if fw1 else e1), (s2 if fw2 else e2)
        if fw1 != fw2:
            return 0 if ((fw1 if p1 < p2 else fw2)) else 1
        return (2 if p1 < p2 else 3) if fw1 else (2 if p2 < p1 else 3)

    def verdicts(me, other):
        out = np.ones(len(me["read"]), np.uint8)
        for r in range(n_reads):
            mine = me["grp_idx"][me["grp_off"][r]:me["grp_off"][r + 1]]
            mates = other["grp_idx"][other["grp_off"][r]:other["grp_off"][r + 1]]
            if len(mine) <= 1 or len(mates) == 0:
                continue
            for a in mine:
                ok = 0
                for b in mates:
                    s1, e1, s2, e2 = int(me["ref_start"][a]), int(me["end"][a]), int(other["ref_start"][b]), int(other["end"][b])
                    ins = max(s1, e1, s2, e2) - min(s1, e1, s2, e2)
                    if me["ref_id"][a] == other["ref_id"][b] and low <= ins <= high and \
                            orientation(int(me["flags"][a]), s1, e1, int(other["flags"][b]), s2, e2) == correct:
                        ok = 1
                        break
                out[a] = ok
        return out
    want = verdicts(a1, a2), verdicts(a2, a1)
    assert 0 < want[0].sum() < len(want[0])
    L = pp.lib()
    for with_samples in (False, True, False):
        got = np.full(f1.n_aln, 7, np.uint8), np.full(f2.n_aln, 7, np.uint8)
        assert L.pp_filter_begin(ctx._h, C.byref(inp), pp.MEM_HOST) == 0, L.pp_last_error(ctx._h)
        if with_samples:
            orient, insert = np.zeros(n_reads, np.uint8), np.zeros(n_reads, np.uint32)
            assert L.pp_filter_samples(ctx._h, orient.ctypes.data, insert.ctypes.data) == 0
            uniq = (np.diff(a1["grp_off"]) == 1) & (np.diff(a2["grp_off"]) == 1)
            assert ((orient != 255) <= uniq).all() and (orient != 255).sum() > 100
        assert L.pp_filter_pairs(ctx._h, low, high, correct, got[0].ctypes.data, got[1].ctypes.data) == 0
        assert (got[0] == want[0]).all() and (got[1] == want[1]).all()


@pytest.mark.parametrize("long_read", [False, True])
def test_sharded_jobs_take_the_direct_path(ctx, pp, orc, long_read):
    """A rank of a sharded job whose batch brings the window-order mirror AND its runs takes the direct path too (over the
    job's own coordinates: k_tile / k_emit only over the windows it works on): three ranks over a 400 kbp contig in three
    windows and two small contigs, (a) every rank's host part -- pp_shard_split restricts the mirror and its run table --
    (b) all records with the rank's emit ranges, (c) the part split on the device from a resident batch; the ranks' bytes
    assemble to the oracle's unsharded polish, and every run says it took the direct path.  long_read: a 20,000-base
    alignment across the first cut (no compact run, so no halo to outgrow).  Two runs (two SAM files) in the mirror."""
    import torch
    contig_off, bases, recs = synth.fast_records(seed=68, contig_lens=(400_000, 3_000, 60_000), coverage=12, read_len=100,
                                                 k_choices=(1, 1, 2, 3), indel_read_frac=0.2, n_rate=0.003)
    plan = pp.Plan(contig_off, np.bincount(recs["contig"], minlength=3), 3, 65536)
    if long_read:
        cut = int(plan.unit_hi[0])
        rng = np.random.default_rng(2)
        n_long = 20_000
        extra = {"contig": np.array([0], np.uint32), "ref_start": np.array([cut - 18_000], np.uint32), "k": np.array([1], np.uint32),
                 "seq_off": np.array([0], np.uint64), "seq_len": np.array([n_long], np.uint32), "cig_off": np.array([0], np.uint64),
                 "n_cig": np.array([1], np.uint32), "seq": np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n_long)].copy(),
                 "cigar": np.array([(n_long << 4) | 0], np.uint32)}
        recs = synth.merge_records(recs, extra, seed=4)
    n = len(recs["contig"])
    per_file = [n // 2, n - n // 2]
    recs = dict(recs)
    recs["wo"] = pp.window_order_mirror(recs, contig_off, used_per_file=per_file)
    recs["wo_runs"] = np.cumsum(per_file).astype(np.uint64)
    want = orc.polish_records(contig_off, bases, recs)
    dev = torch.device("cuda:0")
    t = {k: torch.from_numpy(np.ascontiguousarray(recs[k], dtype=dt)).to(dev) for k, dt in pp.REC_FIELDS}
    t["wo"] = torch.from_numpy(np.ascontiguousarray(recs["wo"]).view(np.uint8)).to(dev)
    tb = torch.from_numpy(np.ascontiguousarray(bases, dtype=np.uint8)).to(dev)
    torch.cuda.synchronize()
    dptrs = {k: v.data_ptr() for k, v in t.items()}
    dptrs["wo_runs"] = recs["wo_runs"]
    for how in ("host part", "all records", "device part"):
        rank_bytes, rank_offs = [], []
        for rank in range(3):
            emit = plan.emit_ranges(rank)
            if how == "host part":
                mine = pp.shard_split_host(plan, rank, recs)[0]
                assert len(mine["wo"]) == len(mine["contig"]) and len(mine["wo_runs"]) == 2 and int(mine["wo_runs"][-1]) == len(mine["contig"])
                got = ctx.polish_records(contig_off, bases, mine, emit=emit)
            elif how == "all records":
                got = ctx.polish_records(contig_off, bases, recs, emit=emit)
            else:
                part = pp.ShardPart(ctx, plan, rank, n, dptrs, len(recs["seq"]), len(recs["cigar"]), pp.MEM_DEVICE)
                assert list(part.ptrs["wo_runs"]) == list(pp.shard_split_host(plan, rank, recs)[0]["wo_runs"])
                ctx.polish_begin(contig_off, tb.data_ptr(), pp.MEM_DEVICE, 5, 0.5, 0.2)
                ctx.set_emit(emit)
                ctx.polish_add_ptrs(part.n_aln, part.ptrs, part.seq_bytes, part.n_cig_total, pp.MEM_DEVICE)
                ctx.polish_finish()
                polished, offs, stats = ctx.result()
                got = {"polished": polished, "offsets": offs}
                part.close()
            assert ctx.took_direct_path(), (how, rank)
            rank_bytes.append(got["polished"])
            rank_offs.append(got["offsets"])
        data, out_off = plan.assemble(rank_bytes, rank_offs)
        assert data == want["polished"] and np.array_equal(out_off, want["offsets"]), how


def test_newline_index_of_a_text_of_very_short_lines(orc, tmp_path):
    """A SAM text with far more lines than records -- 300,000 four-byte header lines in front of them, more newlines than one
    per 64 bytes of text -- through both device text front ends (polish: the tokenizer; filter: the device loader), against
    the oracle's bytes."""
    ds = synth.rich_dataset(str(tmp_path), seed=131, contig_lens=(20_000, 3_000), coverage=20, repeat_len=200, repeat_copies=2)
    sams = []
    for i, src in enumerate((ds["sam1"], ds["sam2"])):
        dst = str(tmp_path / f"short_{i + 1}.sam")
        with open(src, "rb") as f:
            body = f.read()
        head_end = 0
        while body[head_end:head_end + 1] == b"@":
            head_end = body.index(b"\n", head_end) + 1
        with open(dst, "wb") as f:
            f.write(body[:head_end] + b"@CO\n" * 300_000 + body[head_end:])
        sams.append(dst)
    assert os.path.getsize(sams[0]) // 64 + 1024 < 300_000
    exe = os.path.join(ROOT, "bin", "polypolish")
    want = orc.polish_files(ds["fasta"], sams)["fasta"]
    r = subprocess.run([exe, "polish", ds["fasta"], *sams], capture_output=True)
    assert r.returncode == 0 and r.stdout == want, r.stderr[-400:]
    o1, o2 = str(tmp_path / "f1.sam"), str(tmp_path / "f2.sam")
    w1, w2 = str(tmp_path / "w1.sam"), str(tmp_path / "w2.sam")
    orc.filter_files(sams[0], sams[1], w1, w2)
    r = subprocess.run([exe, "filter", "--in1", sams[0], "--in2", sams[1], "--out1", o1, "--out2", o2], capture_output=True,
                       env=dict(os.environ, PP_DEVICE_FILTER="1"))
    assert r.returncode == 0, r.stderr[-400:]
    assert open(o1, "rb").read() == open(w1, "rb").read() and open(o2, "rb").read() == open(w2, "rb").read()
