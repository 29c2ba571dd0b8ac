"""One polish context, job after job.  A pp_ctx is reused -- the bench's timed steps, a rank's shares, pp_polish_files in a
loop -- and much of what a job does depends on state the job before left on the context: the pinned metadata block and the
serial k_emit's last workgroup writes behind it, the metadata block set up ahead for the next job, speculation on the replays,
the k_tile instance picked by the last job's longest read, the room for extras, the grids sized by the last job's winners,
the cached contig table and emit ranges.  Every job here is checked against the oracle's result for that job: polished
bytes, contig offsets and per-contig figures, and, with the debug planes, every per-position record.  Needs an MI355X."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import synth
from test_gpu_parity import POS_KEYS, RECORD_CASES, _polish_device_batch, _rec, _with_hot_region

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = (5, 0.5, 0.2)  # min_depth, fraction_valid, fraction_invalid
PARAMS = (DEFAULT, (1, 0.6, 0.05), (8, 0.7, 0.3))


# ---- jobs ---------------------------------------------------------------------------------------------------------------

def _exact_reads(seed, contig_lens, coverage, read_len=150):
    """Reads drawn from the truth without errors, over an assembly that IS the truth: nothing changes unless planted."""
    return synth.fast_records(seed=seed, contig_lens=contig_lens, coverage=coverage, read_len=read_len, sub_rate=0.0,
                              n_rate=0.0, asm_sub_rate=0.0, indel_read_frac=0.0)


def _planted(seed, contig_lens, coverage, contig, n_subs):
    """_exact_reads with n_subs substitutions planted in one contig of the assembly, well inside it (depth >= min_depth
    there), and none elsewhere: exactly n_subs changed positions in that contig."""
    off, bases, recs = _exact_reads(seed, contig_lens, coverage)
    bases = bases.copy()
    lo, hi = int(off[contig]), int(off[contig + 1])
    for p in np.linspace(lo + 300, hi - 300, n_subs).astype(np.int64):
        bases[p] = {ord("A"): ord("C"), ord("C"): ord("G"), ord("G"): ord("T"), ord("T"): ord("A")}[int(bases[p])]
    return off, bases, recs


@functools.lru_cache(maxsize=None)
def _hot_contig(seed):
    return _with_hot_region(seed, 40_000, 100, 19_000, 23_000, 1500, k_choices=(1, 3, 5), k_probs=(0.6, 0.2, 0.2),
                            indel_read_frac=0.02)


def _hot_with_contigs(seed, n_small):
    """A collapsed repeat (heavy windows: see test_heavy_windows_are_split_over_helper_blocks) in contig 0, followed by
    n_small small contigs of their own."""
    off, bases, hot = _hot_contig(seed)
    s_off, s_bases, small = synth.fast_records(seed=seed + n_small, contig_lens=(2_000,) * n_small, coverage=30)
    small = dict(small, contig=small["contig"] + np.uint32(1))
    return (np.concatenate([off, s_off[1:] + off[-1]]).astype(np.uint64), np.concatenate([bases, s_bases]),
            synth.merge_records(hot, small, seed=seed))


def _bad_job():
    """Two bad records (the first one is record 2) among good ones: the device refuses the job
    (test_device_reports_the_first_bad_record)."""
    ref = "ACGGTCATTGCAACGGTTATTGCA" * 3
    good = (0, 0, 1, ref[:24], [(24, "M")])
    bad = (0, 0, 1, ref[:24], [(23, "M")])  # CIGAR shorter than the read
    return (np.array([0, len(ref)], np.uint64), np.frombuffer(ref.encode(), np.uint8), _rec([good, good, bad, good, bad]))


SHAPES = {
    "clean": lambda: synth.fast_records(seed=101, contig_lens=(30_000,), coverage=40, indel_read_frac=0.0, n_rate=0.0),
    "clean2": lambda: synth.fast_records(seed=102, contig_lens=(24_000, 9_000), coverage=50, indel_read_frac=0.01),
    "odd_ins": lambda: synth.fast_records(seed=103, contig_lens=(30_000, 2_500), coverage=50, k_choices=(1, 2, 3, 5, 6, 7),
                                          k_probs=(0.5, 0.1, 0.1, 0.1, 0.1, 0.1), indel_read_frac=0.2, n_rate=0.01),
    "all_indels": lambda: synth.fast_records(seed=104, contig_lens=(20_000,), coverage=60, indel_read_frac=1.0, k_choices=(1, 2, 3)),
    "one_contig": lambda: synth.fast_records(seed=105, contig_lens=(20_000,), coverage=40, read_len=100, indel_read_frac=0.05),
    "contigs20": lambda: synth.fast_records(seed=106, contig_lens=tuple(1_000 + 97 * i for i in range(20)), coverage=30,
                                            read_len=100, indel_read_frac=0.05, k_choices=(1, 1, 3)),
    "contigs300": lambda: synth.fast_records(seed=107, contig_lens=(300,) * 300, coverage=25, read_len=100, indel_read_frac=0.05),
    "many2000": lambda: synth.fast_records(seed=108, contig_lens=(300,) * 2_000, coverage=20, read_len=100, indel_read_frac=0.05),
    "short100": lambda: synth.fast_records(seed=109, contig_lens=(20_000, 5_000), coverage=40, read_len=100, indel_read_frac=0.05),
    "long250": lambda: synth.fast_records(seed=110, contig_lens=(25_000,), coverage=40, read_len=250, indel_read_frac=0.05),
    "deep3k": lambda: synth.fast_records(seed=111, contig_lens=(3_000,), coverage=5_000, read_len=150, indel_read_frac=0.02,
                                         k_choices=(1, 1, 3)),
    "heavy": lambda: _hot_contig(112),
    "shallow": lambda: synth.fast_records(seed=113, contig_lens=(15_000,), coverage=8, indel_read_frac=0.05, n_rate=0.01),
    "tiny_contigs": lambda: synth.fast_records(**RECORD_CASES["tiny_contigs"]),
    "all_k3": lambda: synth.fast_records(**RECORD_CASES["all_k3"]),
    "many_N": lambda: synth.fast_records(**RECORD_CASES["many_N"]),
    "big_k": lambda: synth.fast_records(**RECORD_CASES["big_k"]),
    "bad": _bad_job,
}


@functools.lru_cache(maxsize=None)
def _job(name):
    return SHAPES[name]()


def _expected(orc, job, params=DEFAULT):
    """The oracle's result for a job, with its per-position records and per-contig figures."""
    off, bases, recs = job
    md, fv, fi = params
    w = orc.polish_records(off, bases, recs, min_depth=md, fraction_valid=fv, fraction_invalid=fi, positions=True)
    o = [int(x) for x in off]
    pos = w["positions"]
    w["contig_len"] = [o[c + 1] - o[c] for c in range(len(o) - 1)]
    w["changed"] = [int((pos["status"][o[c]:o[c + 1]] == 1).sum()) for c in range(len(o) - 1)]
    w["zero_depth"] = [int((pos["depth"][o[c]:o[c + 1]] == 0.0).sum()) for c in range(len(o) - 1)]
    w["depth_sum"] = [float(pos["depth"][o[c]:o[c + 1]].sum()) for c in range(len(o) - 1)]
    # How far the per-contig depth sum (the log's mean read depth) may lie from the oracle's: a window tallies shares 1/k in
    # units of 2^-b, b = min(20, 31 - bit length of its work items) (DEPTH_FX_BITS, win_fx_bits), a share that is not a
    # multiple of the unit rounded to the nearest one, at every position the read covers; a replayed position is rounded to
    # 2^-10.  A window has at most two items per record, so b is at least the job-wide figure below.
    b = min(20, 31 - int(2 * len(recs["contig"]) + 1).bit_length())
    k = recs["k"].astype(np.int64)
    inexact = ((k & (k - 1)) != 0) | (k > (1 << b))
    span = np.bincount(recs["contig"][inexact], weights=recs["seq_len"][inexact].astype(np.float64), minlength=len(o) - 1)
    w["depth_slack"] = [float(span[c]) * 2.0 ** -(b + 1) + w["contig_len"][c] * 2.0 ** -11 + 1e-6 * w["depth_sum"][c]
                        for c in range(len(o) - 1)]
    return w


@functools.lru_cache(maxsize=None)
def _want(orc, name, params=DEFAULT):
    return _expected(orc, _job(name), params)


# ---- running a job one way or another, and checking it --------------------------------------------------------------

ROUTES = ("host", "host_wo", "device_wo", "device_bucket", "device_bytes", "sharded")


def _run(ctx, name, route, params=DEFAULT, debug=False):
    """One job on ctx.  host: host records (the mirror packed on the device); host_wo: ... with the window-order mirror and its
    run table (the direct path); device_wo: one device batch with the 4-bit and the window-order mirror and its run table (the
    direct path); device_bucket: the same batch without the window-order mirror (the bucketing path); device_bytes: ... and
    without the 4-bit mirror; sharded: three ranks' emit ranges (pp_shard_plan) one after the other, put together."""
    import polypolish_amd as pp
    off, bases, recs = _job(name)
    md, fv, fi = params
    kw = dict(min_depth=md, fraction_valid=fv, fraction_invalid=fi)
    if route == "host":
        return ctx.polish_records(off, bases, recs, positions=debug, **kw)
    if route == "host_wo":
        r = dict(recs)
        r["wo"] = pp.window_order_mirror(recs, off)
        r["wo_runs"] = [len(recs["contig"])]
        return ctx.polish_records(off, bases, r, positions=debug, **kw)
    if route in ("device_wo", "device_bucket", "device_bytes"):
        return _polish_device_batch(ctx, pp, off, bases, recs, route != "device_bytes", positions=debug,
                                    wo=route == "device_wo", **kw)
    assert route == "sharded" and not debug
    nc = len(off) - 1
    plan = pp.Plan(off, np.bincount(recs["contig"], minlength=nc), 3, 2048)
    rank_bytes, rank_offs = [], []
    stats = [dict(changed=0, zero_depth=0, depth_sum=0.0) for _ in range(nc)]
    for rank in range(3):
        got = ctx.polish_records(off, bases, recs, emit=plan.emit_ranges(rank), **kw)
        rank_bytes.append(got["polished"])
        rank_offs.append(got["offsets"])
        for c in range(nc):  # (the ranks' emit ranges cover every position once: their figures add up to the contig's)
            for k in stats[c]:
                stats[c][k] += got["stats"][c][k]
    data, out_off = plan.assemble(rank_bytes, rank_offs)
    return {"polished": data, "offsets": out_off, "stats": stats, "positions": None}


def _check(got, want, where):
    assert got["polished"] == want["polished"], (f"{where}: polished bytes differ ({len(got['polished'])} vs "
                                                 f"{len(want['polished'])} bytes)")
    assert np.array_equal(np.asarray(got["offsets"], np.uint64), want["offsets"]), (f"{where}: contig offsets differ",
                                                                                     got["offsets"][:8], want["offsets"][:8])
    nc = len(want["changed"])
    chg = [got["stats"][c]["changed"] for c in range(nc)]
    zd = [got["stats"][c]["zero_depth"] for c in range(nc)]
    bad = [c for c in range(nc) if chg[c] != want["changed"][c] or zd[c] != want["zero_depth"][c]]
    assert not bad, (f"{where}: per-contig changed / zero_depth differ at contigs {bad[:8]}",
                     [(chg[c], want["changed"][c], zd[c], want["zero_depth"][c]) for c in bad[:8]])
    for c in range(nc):
        d, w = got["stats"][c]["depth_sum"], want["depth_sum"][c]
        assert abs(d - w) <= want["depth_slack"][c], f"{where}: contig {c} depth sum {d} vs {w} (slack {want['depth_slack'][c]})"
    if got.get("positions") is not None:
        for k in POS_KEYS:
            diff = np.nonzero(want["positions"][k] != got["positions"][k])[0]
            assert len(diff) == 0, (f"{where}: per-position {k} differs at {len(diff)} positions", diff[:8],
                                    want["positions"][k][diff[:8]], got["positions"][k][diff[:8]])


class Sequence:
    """Jobs on one context, each checked against the oracle; every assertion names the step and the jobs before it."""

    def __init__(self, ctx, orc, label, seed=None):
        self.ctx, self.orc, self.label, self.seed, self.history = ctx, orc, label, seed, []

    def where(self):
        head = f"{self.label}" + (f" (seed {self.seed})" if self.seed is not None else "")
        steps = "\n  ".join(self.history)
        return f"{head}, step {len(self.history)} of:\n  {steps}"

    def step(self, name, route="host", params=DEFAULT, debug=False, direct=None):
        self.history.append(f"{len(self.history) + 1}: {name} route={route} params={params} debug={debug}")
        if name == "bad":
            return self.refused(route)
        got = _run(self.ctx, name, route, params, debug)
        _check(got, _want(self.orc, name, params), self.where())
        if direct is not None:
            assert self.ctx.took_direct_path() == direct, f"{self.where()}: direct path {self.ctx.took_direct_path()}, expected {direct}"
        return got

    def refused(self, route):
        import polypolish_amd as pp
        with pytest.raises(pp.PolypolishError) as e:
            _run(self.ctx, "bad", route)
        # (host records: the first bad record is named; a device batch names one of them)
        assert e.value.code == pp.ERR_QUIT and ("record 2" if route == "host" else "record") in e.value.msg, f"{self.where()}: {e.value}"


@pytest.fixture(scope="module")
def ctx():
    import polypolish_amd as pp
    c = pp.Context(0)
    yield c
    c.close()


# ---- a. the serial k_emit writes behind the copy, where a smaller job polls ----------------------------------------------

def _stale_slot_cases(orc):
    """For s in 2..5, on a fresh context each: job A (20 contigs, exactly s changed positions in contig 6) and then job B
    (1 contig).  B polls word 50 + 4 * 1 + 1 = 55 of the pinned block for its serial; A's copy left there contig 6's
    `changed` (word 17 + 20 + 3 * 6): s.  A's one launch of k_emit is serial 1, B's first is 2 (one more per rerun of A), so
    for one s at least the word A left passes for B's serial unless it is cleared.  Then with A's heavy windows in the
    place B polls (A has 1 + d contigs: B's word lies in A's list of heavy windows for d in 1..8).  Returns the failures."""
    import polypolish_amd as pp
    fails = []

    def check(ctx, name, job, want_res, history):
        off, bases, recs = job
        got = ctx.polish_records(off, bases, recs)
        try:
            _check(got, want_res, f"{name} after {history}")
        except AssertionError as e:
            fails.append(str(e)[:600])

    def want_of(job):
        return dict(_expected(orc, job), positions=None)

    job_b = _exact_reads(202, (5_000,), 20)
    want_b = want_of(job_b)
    for s in range(2, 6):
        job_a = _planted(201, tuple(2_000 + 10 * c for c in range(20)), 20, 6, s)
        want_a = want_of(job_a)
        # the two figures the case rests on
        assert want_a["changed"][6] == s and sum(want_a["changed"]) == s, (s, want_a["changed"])
        assert want_b["offsets"][1] != want_a["offsets"][1], "B's polished length must differ from A's contig 0"
        ctx = pp.Context(0)
        try:
            check(ctx, f"job A (s = {s})", job_a, want_a, "a fresh context")
            check(ctx, f"job B (s = {s})", job_b, want_b, f"job A (20 contigs, {s} changed in contig 6)")
        finally:
            ctx.close()
    for d in (2, 5, 8):
        job_a = _hot_with_contigs(203, d)
        ctx = pp.Context(0)
        try:
            check(ctx, f"heavy job A ({1 + d} contigs)", job_a, want_of(job_a), "a fresh context")
            check(ctx, "job B", job_b, want_b, f"heavy job A ({1 + d} contigs)")
        finally:
            ctx.close()
    return fails


STALE_CHILD = """
import json, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import torch
from oracle import orc
import test_context_sequence_gpu as t
fails = t._stale_slot_cases(orc)
print("STALE-SLOT " + json.dumps(fails))
"""


@pytest.mark.parametrize("env", [{}, {"PP_SYNC": "wait"}, {"PP_RESULT_COPY": "1"}], ids=["poll", "sync_wait", "result_copy"])
def test_a_smaller_job_does_not_take_a_word_of_the_job_before_for_its_serial(orc, env):
    """How the host learns that a job is through is read once per process (PP_SYNC, PP_RESULT_COPY): each way in a child
    process of its own."""
    code = STALE_CHILD % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, env=dict(os.environ, **env), timeout=900)
    assert r.returncode == 0, (env, r.returncode, r.stderr.decode()[-3000:])
    line = [l for l in r.stdout.decode().splitlines() if l.startswith("STALE-SLOT ")]
    assert line, (env, r.stdout.decode()[-2000:])
    fails = json.loads(line[-1][len("STALE-SLOT "):])
    assert not fails, (env, "\n".join(fails))


# ---- b. transitions that each cross one piece of carried state --------------------------------------------------------

def test_contig_count_moves_the_polled_slot_and_regrows_the_pinned_block(ctx, orc):
    q = Sequence(ctx, orc, "contig counts")
    for name in ("one_contig", "contigs20", "one_contig", "many2000", "one_contig", "contigs300", "contigs20", "many2000",
                 "clean"):
        q.step(name, "host")
        q.step(name, "device_wo")


def test_read_length_hint_reruns_in_the_middle_of_a_sequence(ctx, orc):
    """maxlen_hint picks k_tile's instance from the job before: 250 bp reads after 100 bp ones rerun (DE_GW_HINT)."""
    q = Sequence(ctx, orc, "read lengths")
    for name in ("short100", "long250", "short100", "short100", "long250", "long250", "short100"):
        q.step(name, "device_wo")
    for name in ("short100", "long250", "short100"):
        q.step(name, "host")
        q.step(name, "host", debug=True)


def test_deep_and_heavy_jobs_between_shallow_ones(ctx, orc):
    """Room for extras (xcap: grow-only, capped per job) and heavy windows, then a shallow job, then deep again."""
    q = Sequence(ctx, orc, "depth")
    for name in ("shallow", "deep3k", "shallow", "deep3k", "heavy", "shallow", "heavy", "deep3k", "clean"):
        q.step(name, "device_wo")
    for name in ("deep3k", "shallow", "heavy", "shallow"):
        q.step(name, "host")


def test_speculation_and_multi_byte_winners_from_one_job_to_the_next(ctx, orc):
    """A clean job makes the next one speculate (no replays until its metadata say otherwise); k_emit's grid follows the
    multi-byte winners of the job before (last_multi), k_exact's the positions it listed (last_listed)."""
    q = Sequence(ctx, orc, "speculation")
    for route in ("host", "device_wo"):
        for name in ("clean", "clean", "odd_ins", "clean", "all_indels", "clean", "all_indels", "odd_ins", "all_indels", "clean"):
            q.step(name, route)


def test_same_assembly_with_other_thresholds(ctx, orc):
    """The contig table is kept when it is the same; the metadata block set up ahead is keyed by the fractions too."""
    q = Sequence(ctx, orc, "thresholds")
    for route in ("host", "device_wo"):
        for params in (DEFAULT, DEFAULT, PARAMS[1], PARAMS[2], PARAMS[1], DEFAULT, (5, 0.5, 0.3), (5, 0.55, 0.2), DEFAULT):
            q.step("odd_ins", route, params)


def test_every_route_after_every_other_on_one_assembly(ctx, orc):
    """Direct path, bucketing path, host records, a sharded job's emit ranges (and its compact run) and back."""
    q = Sequence(ctx, orc, "routes")
    order = ("device_wo", "device_bucket", "host", "sharded", "host", "device_wo", "sharded", "device_wo", "host_wo",
             "device_bytes", "sharded", "device_bucket", "device_wo")
    for name in ("clean2", "contigs20"):
        for route in order:
            q.step(name, route, direct=True if route in ("device_wo", "host_wo") else None)


def test_debug_planes_on_and_off(ctx, orc):
    q = Sequence(ctx, orc, "debug planes")
    for route in ("host", "device_wo", "device_bucket"):
        for debug in (True, False, True, True, False, False):
            q.step("odd_ins", route, debug=debug)


def test_a_refused_job_leaves_the_context_usable(ctx, orc):
    q = Sequence(ctx, orc, "refused job")
    for bad_route in ("host", "device_wo", "device_bucket"):
        q.step("clean2", "device_wo", direct=True)
        q.step("bad", bad_route)
        q.step("clean2", "device_wo", direct=True)
        q.step("clean2", "device_wo", direct=True)
        q.step("bad", bad_route)
        q.step("odd_ins", "host", debug=True)


def test_a_prepared_job_repeated_then_another_then_it_again(ctx, orc):
    """The bench's steady state: the same prepared job (resident device batch, mirrors trusted) step after step."""
    import torch
    import polypolish_amd as pp
    dev = torch.device("cuda:0")
    prepared, keep = {}, []
    for name in ("clean2", "odd_ins"):
        off, bases, recs = _job(name)
        t = {k: torch.from_numpy(np.ascontiguousarray(recs[k], dtype=dt)).to(dev) for k, dt in pp.REC_FIELDS}
        t["seq4"] = torch.from_numpy(pp.pack_seq4(recs["seq"])).to(dev)
        t["wo"] = torch.from_numpy(np.ascontiguousarray(pp.window_order_mirror(recs, off)).view(np.uint8)).to(dev)
        tb = torch.from_numpy(np.ascontiguousarray(bases, dtype=np.uint8)).to(dev)
        keep.append((t, tb))
        ptrs = {k: v.data_ptr() for k, v in t.items()}
        ptrs["wo_runs"] = [len(recs["contig"])]
        prepared[name] = ctx.prepared_job(off, tb.data_ptr(), pp.MEM_DEVICE, len(recs["contig"]), ptrs, len(recs["seq"]),
                                          len(recs["cigar"]), pp.MEM_DEVICE)
    torch.cuda.synchronize()
    q = Sequence(ctx, orc, "prepared job")
    ctx.trust_mirrors(True)
    try:
        for name in ("clean2",) * 5 + ("odd_ins",) + ("clean2",) * 3 + ("odd_ins",) * 3 + ("clean2",):
            q.history.append(f"{len(q.history) + 1}: {name} prepared")
            prepared[name]()
            polished, offs, stats = ctx.result()
            _check({"polished": polished, "offsets": offs, "stats": stats}, _want(orc, name), q.where())
            assert ctx.took_direct_path(), q.where()
    finally:
        ctx.trust_mirrors(False)
    # ... and an ordinary job behind them
    q.step("odd_ins", "host", debug=True)


# ---- c. a seeded random sequence --------------------------------------------------------------------------------------

POOL = ("clean", "clean2", "odd_ins", "all_indels", "contigs20", "contigs300", "short100", "long250", "heavy", "shallow",
        "tiny_contigs", "all_k3", "many_N", "big_k")
SEED = 20261016


def test_seeded_random_sequence_of_jobs(ctx, orc):
    """About 40 (shape, route, thresholds, debug planes) steps on one context; a failure names the seed and the steps
    before it, so the sequence can be replayed."""
    rng = np.random.default_rng(SEED)
    q = Sequence(ctx, orc, "random sequence", seed=SEED)
    for _ in range(42):
        if rng.random() < 0.05:
            q.step("bad", str(rng.choice(("host", "device_wo"))))
            continue
        name = str(rng.choice(POOL))
        route = str(rng.choice(ROUTES))
        params = PARAMS[int(rng.choice(3, p=(0.6, 0.2, 0.2)))]
        debug = route != "sharded" and bool(rng.random() < 0.3)
        q.step(name, route, params, debug)
