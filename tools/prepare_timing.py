#!/usr/bin/env python3
"""What pp_batch_prepare buys a caller's batch, and what it costs -- not part of bench.py.

The job is bench.py's configs[1] (tools/synthjob.make_job: 5 Mbp / 200x, resident in HBM).  Three routes, in one process, on one
context, measured in alternating rounds, medians over the timed steps (host clock around begin + add + finish, which ends in a
synchronisation of the stream):

  plain_ms     the job in FILE ORDER with no 4-bit mirror and no window-order mirror (the batch behind bench.py's
               roofline_file_order_seq) through pp_polish_add: what a caller's own batch gets today -- the bucketing path
  prepared_ms  the same records after pp_batch_prepare, WITHOUT pp_ctx_trust_mirrors_: the direct path through the public ABI
  resident_ms  synthjob's own window-grouped batch with its mirrors, trusted: exactly what bench.py's headline runs
  prepare_ms   pp_prepared_kernel_ms: HIP events around the prepare's kernels (device source)
  prepare_frac_of_roofline   the prepare's algorithmic bytes (per record 36 B of fields read, 32 B of mirror written, seq_len
               read, 1.5 x room written) over prepare_ms, as a fraction of 8 TB/s
  break_even_jobs            prepare_ms / (plain_ms - prepared_ms): polishes of one resident batch after which the prepare has
               paid for itself

Prints one JSON line (and writes it to --out).  Needs an MI355X: there is no CPU path."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

PEAK_GBS = 8000.0  # MI355X HBM3E


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=10, help="timed steps per route and round")
    ap.add_argument("--rounds", type=int, default=3, help="alternating rounds (steps x rounds >= 20)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--prepares", type=int, default=7, help="timed pp_batch_prepare calls (after two untimed ones)")
    ap.add_argument("--genome", type=int, default=5_000_000)
    ap.add_argument("--coverage", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.steps * args.rounds < 20:
        ap.error("at least 20 timed steps per route")

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("prepare_timing.py needs an MI355X (no CPU path)")
    import polypolish_amd as pp
    import synthjob

    device = torch.device("cuda:0")
    # bench.py's configs[1] job, seed included (config 1, rank 0)
    job = synthjob.make_job(device, contig_lens=[args.genome], coverage=args.coverage, read_len=150, seed=42 + 1 + 1,
                            indel_read_frac=synthjob.SURVEY_INDEL_READ_FRAC, recipe="survey")
    resident = synthjob.with_wo(synthjob.with_seq4(job))
    plain = synthjob.with_wo(synthjob.with_seq4(synthjob.file_ordered(job), on=False), on=False)
    torch.cuda.synchronize()
    ctx = pp.Context(0)
    n = plain["n_aln"]
    r = plain["recs"]
    plain_ptrs = {k: v.data_ptr() for k, v in r.items()}

    # ---- the prepare itself ----
    ctx.set_profiling(1)
    prep_ms = []
    prep = None
    for i in range(2 + args.prepares):
        if prep is not None:
            prep.close()
        prep = pp.prepare_batch(ctx, plain["contig_off"], n, plain_ptrs, r["seq"].numel(), r["cigar"].numel(), pp.MEM_DEVICE)
        if i >= 2:
            prep_ms.append(prep.kernel_ms())
    ctx.set_profiling(0)
    prepare_ms = statistics.median(prep_ms)
    seq_len = r["seq_len"].long()
    rooms = int(((seq_len + 31) & ~31).sum().item())
    assert rooms == prep.seq_bytes
    prepare_bytes = n * (36 + 32) + int(seq_len.sum().item()) + rooms + rooms // 2

    def job_of(j, ptrs, n_aln, seq_bytes, n_cig):
        return ctx.prepared_job(j["contig_off"], j["bases"].data_ptr(), pp.MEM_DEVICE, n_aln, ptrs, seq_bytes, n_cig, pp.MEM_DEVICE, 5, 0.5, 0.2)

    res_ptrs = {k: v.data_ptr() for k, v in resident["recs"].items()}
    res_ptrs.update(seq4=resident["seq4"].data_ptr(), wo=resident["wo"].data_ptr(), wo_runs=resident["wo_runs"])
    routes = {
        "plain": (job_of(plain, plain_ptrs, n, r["seq"].numel(), r["cigar"].numel()), False),
        "prepared": (job_of(plain, prep.ptrs(), prep.n_aln, prep.seq_bytes, prep.n_cig_total), False),
        "resident": (job_of(resident, res_ptrs, resident["n_aln"], resident["recs"]["seq"].numel(), resident["recs"]["cigar"].numel()), True),
    }
    ms = {k: [] for k in routes}
    direct, polished = {}, {}
    for rnd in range(args.rounds):
        for name, (run, trust) in routes.items():
            ctx.trust_mirrors(trust)
            for _ in range(args.warmup if rnd == 0 else 2):
                run()
            ctx.sync()
            for _ in range(args.steps):
                t0 = time.perf_counter()
                run()
                ctx.sync()
                ms[name].append(1e3 * (time.perf_counter() - t0))
            direct[name] = ctx.took_direct_path()
            if rnd == 0:
                polished[name] = ctx.result()[0]
    ctx.trust_mirrors(False)
    med = {k: statistics.median(v) for k, v in ms.items()}
    gain = med["plain"] - med["prepared"]
    out = {
        "tool": "tools/prepare_timing.py",
        "workload": f"configs[1]: {args.genome / 1e6:g} Mbp / {args.coverage}x, {n} records resident in HBM",
        "steps_per_route": args.steps * args.rounds, "rounds": args.rounds,
        "plain_ms": round(med["plain"], 4), "prepared_ms": round(med["prepared"], 4), "resident_ms": round(med["resident"], 4),
        "prepared_over_resident": round(med["prepared"] / med["resident"], 4),
        "spread_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
        "prepare_ms": round(prepare_ms, 4), "prepare_ms_min_max": [round(min(prep_ms), 4), round(max(prep_ms), 4)],
        "prepare_algorithmic_bytes": prepare_bytes,
        "prepare_frac_of_roofline": round(prepare_bytes / (prepare_ms * 1e-3) / 1e9 / PEAK_GBS, 4),
        "break_even_jobs": round(prepare_ms / gain, 2) if gain > 0 else None,
        "took_direct_path": {k: bool(v) for k, v in direct.items()},
        "same_polished_bytes": bool(polished["plain"] == polished["prepared"] == polished["resident"]),
    }
    prep.close()
    ctx.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
