"""Multi-GPU polish, one process per GPU: contigs (and windows of a large contig) shard across ranks with no
data-path collective; the only exchange is the collection of the polished bytes on rank 0.

Everything that decides or moves data is in libpolypolish_hip.so (include/polypolish_hip.h, "multi-GPU"):

  pp_shard_plan_create   whole contigs by longest-processing-time on their alignment counts; a contig that carries
                         more than one rank's share (config C5: one 250 Mbp contig) is cut into windows on 2048-bp
                         boundaries, one per rank
  pp_shard_split         the records that reach a rank's units: its contigs' records, on a tiled contig its window's
                         records plus those that reach in from the neighbours (an alignment only touches its own
                         contig's positions ref_start + j: src/alignment.rs:297-303, src/pileup.rs:189-200)
  pp_polish_set_emit     a rank polishes those records with the ranges of its units: the device works on its windows
                         only.  Every owned position sees all of its alignments in file order, so the order-dependent
                         f64 depth stays exact (src/pileup.rs:64), and the read group's share 1/k
                         (src/alignment.rs:288) was fixed by the ingest before anything was partitioned
  pp_polish_gather       ncclAllGather of byte counts + one group of ncclSend / ncclRecv into rank 0 (RCCL over xGMI)
  pp_shard_assemble      the ranks' bytes back in FASTA order

This module is the launcher glue for `python -m torch.distributed.run ... -m polypolish_amd.distributed polish ...`:
it hands the ncclUniqueId around and prints the FASTA.  With PP_SHARE_GPU=1 (tests on a one-GPU box: RCCL refuses two
ranks on one device) and in the CPU tests the bytes travel as torch.distributed objects over gloo instead.
"""
from __future__ import annotations

import numpy as np


def gather_objects(polished: bytes, offs, rank: int, world: int):
    """Transport for tests / shared-GPU runs: every rank's (bytes, contig_out_off) to rank 0 over torch.distributed
    (gloo).  Returns (list of bytes, list of offset arrays) on rank 0, (None, None) elsewhere."""
    if world == 1:
        return [polished], [np.asarray(offs, dtype=np.uint64)]
    import torch.distributed as dist
    got = [None] * world if rank == 0 else None
    dist.gather_object((polished, np.asarray(offs, dtype=np.uint64)), got, dst=0)
    if rank != 0:
        return None, None
    return [g[0] for g in got], [g[1] for g in got]


DEBUG_HEADER = b"name\tpos\tbase\tdepth\tinvalid\tvalid\tpileup\tstatus\tnew_base\n"  # src/polish.rs:230-245


def write_debug_parts(path, plan, rank, world, fmt, at=len(DEBUG_HEADER)):
    """--debug across ranks: every rank formats the lines of the plan's units it owns (`fmt(lo, hi)` -> bytes, positions of
    the concatenated assembly), the ranks' lengths are all-gathered, and every rank writes its parts with pwrite at their
    places behind the first `at` bytes of the file (rank 0 created it and wrote the header).  Units come contig by contig,
    a tiled contig's windows in position order: the file is in assembly order, every position once."""
    import os
    off = np.asarray(plan.contig_off, dtype=np.uint64)
    units = range(len(plan.unit_rank))
    mine = {u: fmt(int(off[plan.unit_contig[u]] + plan.unit_lo[u]), int(off[plan.unit_contig[u]] + plan.unit_hi[u]))
            for u in units if int(plan.unit_rank[u]) == rank}
    lens = {u: len(b) for u, b in mine.items()}
    if world > 1:
        import torch.distributed as dist
        seen = [None] * world
        dist.all_gather_object(seen, lens)
        for s in seen:
            lens.update(s)
    where = {}
    for u in units:
        where[u] = at
        at += lens.get(u, 0)
    fd = os.open(path, os.O_WRONLY)
    try:
        for u, b in mine.items():
            view, o = memoryview(b), where[u]
            while len(view):
                k = os.pwrite(fd, view, o)
                view, o = view[k:], o + k
    finally:
        os.close(fd)


def polish_sharded(engine, names, descs, contig_off, bases, recs, rank, world, gather=None, min_window=0, locate=None,
                   after=None, **params):
    """Sharded polish.  `engine(contig_off, bases, recs, emit=..., **params)` polishes the records it is given restricted
    to the emit ranges and returns {"polished": bytes, "offsets": array} (Context.polish_records on a GPU; the oracle in
    the CPU tests).  A rank gives it only the records that reach its units (pp_shard_split).  `gather(polished, offsets)`
    collects every rank's result on rank 0 (default: gloo objects).  `locate(exc)` (optional) returns the rank-local
    number of the record an engine failure is about: the ranks then agree on the job's FIRST bad record (the reference
    streams, so that is the one it reports) and all of them raise.  `after(plan)` (optional) runs on every rank once every
    engine has succeeded, before the gather (the --debug TSV: write_debug_parts).  Rank 0 returns the FASTA text of the
    whole assembly (src/polish.rs:196-203), other ranks None."""
    import polypolish_amd as pp
    contig_off = np.asarray(contig_off, dtype=np.uint64)
    n_contigs = len(contig_off) - 1
    counts = np.bincount(np.asarray(recs["contig"], dtype=np.int64), minlength=n_contigs)[:n_contigs]
    plan = pp.Plan(contig_off, counts, world, min_window)
    mine, orig = pp.shard_split_host(plan, rank, recs)
    res, failure = None, None
    try:
        res = engine(contig_off, bases, mine, emit=plan.emit_ranges(rank), **params)
    except Exception as e:  # noqa: BLE001 -- whatever the engine raises travels to every rank
        local = locate(e) if locate else None
        failure = (int(orig[local]) if local is not None and local < len(orig) else -1, e)
    if world > 1:
        import torch.distributed as dist
        seen = [None] * world
        dist.all_gather_object(seen, None if failure is None else (failure[0], type(failure[1]).__name__, str(failure[1]),
                                                                   getattr(failure[1], "code", 1)))
        bad = [(s[0], r, s) for r, s in enumerate(seen) if s is not None]
        if bad:
            _, r, s = min(bad)
            if failure is not None and r == rank:
                raise failure[1]
            raise pp.PolypolishError(s[3], s[2])
    elif failure is not None:
        raise failure[1]
    if after is not None:
        after(plan)
    if gather is None:
        gather = lambda b, o: gather_objects(b, o, rank, world)  # noqa: E731
    all_bytes, all_offs = gather(res["polished"], res["offsets"])
    if rank != 0:
        return None
    data, out_off = plan.assemble(all_bytes, all_offs)
    out = []
    for c in range(n_contigs):
        out.append(b">" + names[c].encode() + ((b" " + descs[c].encode()) if descs[c] else b"") + b" polypolish\n"
                   + data[int(out_off[c]):int(out_off[c + 1])] + b"\n")
    return b"".join(out)


def main(argv=None):
    """`polypolish polish` across the GPUs of one node, one process per GPU:

        python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 \\
            -m polypolish_amd.distributed polish [options] assembly.fasta a_1.sam a_2.sam > polished.fasta

    Options as the reference's (src/main.rs:78-108).  Every rank runs the host ingest (the 1/k shares are fixed before
    anything is partitioned), polishes its contigs / windows on its own GPU, the polished bytes go to rank 0 over RCCL
    and rank 0 prints the FASTA.  --debug PATH: rank 0 creates the file and writes its header before polishing; every
    rank formats the TSV lines of the positions it emits on its GPU (Context.debug_tsv), the ranks' lengths are
    all-gathered and every rank writes its lines at their offset (pwrite) -- no TSV travels between ranks.
    PP_SHARE_GPU=1 (testing on a one-GPU box): all ranks use GPU 0 and the bytes travel over gloo."""
    import argparse
    import ctypes as C
    import os
    import sys
    import torch
    import torch.distributed as dist
    import polypolish_amd as pp
    ap = argparse.ArgumentParser(prog="polypolish_amd.distributed")
    ap.add_argument("command", choices=["polish"])
    ap.add_argument("-i", "--fraction_invalid", type=float, default=0.2)
    ap.add_argument("-v", "--fraction_valid", type=float, default=0.5)
    ap.add_argument("-m", "--max_errors", type=int, default=10)
    ap.add_argument("-d", "--min_depth", type=int, default=5)
    ap.add_argument("--careful", action="store_true")
    ap.add_argument("--debug", default=None)
    ap.add_argument("--text_chain", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--wrap", default=None)
    ap.add_argument("--out_bgzf", action="store_true")
    ap.add_argument("--index", action="store_true")
    ap.add_argument("--vcf", default=None)
    ap.add_argument("--vcf_bgzf", action="store_true")
    ap.add_argument("--bed", default=None)
    ap.add_argument("--bed_bgzf", action="store_true")
    ap.add_argument("--soft_mask", action="store_true")
    ap.add_argument("--bed_status", default=None)
    ap.add_argument("--depth", default=None)
    ap.add_argument("--depth_bin", default=None)
    ap.add_argument("--depth_bgzf", action="store_true")
    ap.add_argument("--vcf_tbi", action="store_true")
    ap.add_argument("--bed_tbi", action="store_true")
    ap.add_argument("--depth_tbi", action="store_true")
    ap.add_argument("assembly")
    ap.add_argument("sam", nargs="*")
    a = ap.parse_args(argv)
    if a.vcf is not None or a.vcf_bgzf:    # (a rank's share has no defined runs at its edges: pp_polish_vcf)
        raise SystemExit("Error: --vcf runs on one GPU: polish with `polypolish polish --vcf`, or without --vcf")
    for flag, given in (("--bed", a.bed is not None or a.bed_bgzf), ("--soft_mask", a.soft_mask), ("--bed_status", a.bed_status is not None)):
        if given:    # (the status plane of a rank is its share's: pp_polish_bed)
            raise SystemExit(f"Error: {flag} runs on one GPU: polish with `polypolish polish {flag}`, or without {flag}")
    if a.depth is not None or a.depth_bin is not None or a.depth_bgzf:    # (the depth plane of a rank is its share's: pp_polish_depth)
        raise SystemExit("Error: --depth runs on one GPU: polish with `polypolish polish --depth`, or without --depth")
    for flag, given in (("--vcf_tbi", a.vcf_tbi), ("--bed_tbi", a.bed_tbi), ("--depth_tbi", a.depth_tbi)):
        if given:    # (the index of a track that runs on one GPU: pp_tabix_index)
            raise SystemExit(f"Error: {flag} runs on one GPU: polish with `polypolish polish {flag}`, or without {flag}")
    for flag, given in (("--out", a.out is not None), ("--wrap", a.wrap is not None), ("--out_bgzf", a.out_bgzf), ("--index", a.index)):
        if given:    # (rank 0 writes the FASTA here as the ranks' bytes arrive; the device link makes it on one context)
            raise SystemExit(f"Error: {flag} is not available here: rank 0 writes the FASTA itself; polish with `polypolish polish {flag}`, "
                             f"which also runs on several GPUs (PP_GPUS)")
    if a.text_chain:    # (one context per command, as for BAM)
        raise SystemExit("Error: SAM text on the record chain (--text_chain) runs on one GPU: polish it with `polypolish polish --text_chain`, "
                         "or without --text_chain")
    # BAM input runs on one GPU (`polypolish polish`, Context.polish_files): the ranks here share the host ingest of SAM text
    for path in a.sam:
        if not os.path.isfile(path):
            continue
        try:
            kind = pp.aln_file_kind(path)
        except pp.PolypolishError as e:
            raise SystemExit(f"Error: {e.msg}")
        if kind != pp.ALN_SAM:
            raise SystemExit(f"Error: BAM input (\"{path}\") runs on one GPU: polish it with `polypolish polish`, or convert it to SAM text")
    # stdout carries the FASTA and nothing else: libraries that chat on fd 1 (gloo's "[Gloo] Rank ..." lines)
    # are pointed at stderr for the whole run
    sys.stdout.flush()
    fasta_fd = os.dup(1)
    os.dup2(2, 1)
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    share = os.environ.get("PP_SHARE_GPU") == "1"
    if not torch.cuda.is_available():
        raise SystemExit("Error: no usable MI355X (HIP) device -- this build has no CPU path")
    dev = 0 if share else local
    torch.cuda.set_device(dev)
    if world > 1:
        dist.init_process_group("gloo")  # control plane only: the unique id and (shared-GPU runs) the bytes
    try:
        names, descs, off, bases, recs, _ = pp.ingest(a.assembly, a.sam, max_errors=a.max_errors, careful=a.careful)
        after = None
        if a.debug:  # create_debug_file, src/polish.rs:230-245: created (header written) before polishing, by rank 0
            created = True
            if rank == 0:
                try:
                    with open(a.debug, "wb") as f:
                        f.write(DEBUG_HEADER)
                except OSError:
                    created = False
            if world > 1:
                flag = [created]
                dist.broadcast_object_list(flag, src=0)
                created = flag[0]
            if not created:
                if rank != 0:
                    raise SystemExit(1)
                raise pp.PolypolishError(pp.ERR_QUIT, f'unable to create "{a.debug}"')
        ctx = pp.Context(dev)
        if a.debug:
            def after(plan):
                write_debug_parts(a.debug, plan, rank, world, lambda lo, hi: ctx.debug_tsv(names, lo, hi))
        gather = None
        if world > 1 and not share:
            ident = [pp.comm_unique_id() if rank == 0 else None]
            dist.broadcast_object_list(ident, src=0)
            ctx.comm_init(rank, world, ident[0])

            def gather(polished, offs):  # RCCL: the bytes are still on the device (pp_polish_result_device)
                buf = torch.empty(int(off[-1]) + int(off[-1]) // 8 + (1 << 20), dtype=torch.uint8, device=f"cuda:{dev}") \
                    if rank == 0 else None
                lens, offs_all = ctx.gather(buf.data_ptr() if rank == 0 else None, buf.numel() if rank == 0 else 0)
                if rank != 0:
                    return None, None
                host = buf.cpu().numpy()
                starts = np.concatenate([[0], np.cumsum(lens.astype(np.int64))])
                return [host[int(starts[r]):int(starts[r + 1])].tobytes() for r in range(world)], list(offs_all)
        def locate(exc):  # the rank-local record a device error of the CIGAR walk is about
            rec, kind = C.c_uint64(), C.c_uint32()
            return int(rec.value) if pp.lib().pp_polish_error_record(ctx._h, C.byref(rec), C.byref(kind)) else None
        out = polish_sharded(ctx.polish_records, names, descs, off, bases, recs, rank, world, gather=gather, locate=locate,
                             after=after, min_depth=a.min_depth, fraction_valid=a.fraction_valid,
                             fraction_invalid=a.fraction_invalid, debug=bool(a.debug))
    except pp.PolypolishError as e:
        sys.stderr.write(f"\nError: {e.msg}\n")
        raise SystemExit(101 if e.code == pp.ERR_PANIC else 1)
    if rank == 0:
        view = memoryview(out)
        while len(view):
            view = view[os.write(fasta_fd, view):]
    os.close(fasta_fd)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
