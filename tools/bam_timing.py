#!/usr/bin/env python3
"""What pp_bam_records costs on a configs[1]-shaped input: the records of tools/synthjob.py's SAM pair (make_job(pairs=True): every
record, the ones the gates reject and the unaligned ones too, secondary records with l_seq 0) encoded to uncompressed BAM bytes by
a vectorised numpy encoder, one byte array per file, resident in HBM (an allocation of exactly its length).  Prints one JSON line:
  pass_a_ms / scans_ms / pass_b_ms   HIP-event time of k_bam_scan | k_bam_place x 2 + k_colscan<3> | k_bam_expand, summed over the two
                 files (best of --repeat)
  bam_bytes      the bytes of the two arrays;  pass_a_gbps = bam_bytes over pass A's time (it touches every record, not every byte)
  pass_b_bytes   what pass B reads and writes: SEQ nibbles in, rooms out, CIGAR words both ways, 44 bytes of per-record arrays
  pass_b_gbps    ... over its own time
  names_ms       pp_names_ids over the decode's name ranges into its read_id array (the next link; both files, one table)
  gate_seq_copy_gbps   k_gate_seq on the decoded batch, the same machine and run: bytes as tools/gate_timing.py counts them
  tokenizer_stages_ms  (--text) the device tokenizer's own stage timers on the SAM text of the same job
--out FILE writes the line to FILE as well.  Measurement only: no threshold is attached to any of it."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import polypolish_amd as pp  # noqa: E402
import synthjob  # noqa: E402

NIBBLE = b"=ACMGRSVTWYHKDBN"
CORE = np.dtype([("block_size", "<u4"), ("ref_id", "<i4"), ("pos", "<i4"), ("l_read_name", "u1"), ("mapq", "u1"), ("bin", "<u2"),
                 ("n_cigar_op", "<u2"), ("flag", "<u2"), ("l_seq", "<u4"), ("next_ref", "<i4"), ("next_pos", "<i4"), ("tlen", "<i4")])


def encode_bam(S, lo, hi, chunk=1 << 18):
    """records [lo, hi) of the job's SAM pair -> (bytes: np.uint8, rec_off: np.uint64).  QNAME "r<read>"; NM:C / NM:S / NM:I on the
    aligned records; QUAL 0xFF.  Records are grouped by their shape (name digits, CIGAR words, l_seq, aux bytes): all records of a
    shape are rows of one 2-D array, filled column-wise, and scattered to their offsets in chunks."""
    col = lambda k, t: S[k][lo:hi].cpu().numpy().astype(t)  # noqa: E731
    flag, read, contig, pos, nm = col("flag", np.int64), col("read", np.int64), col("contig", np.int64), col("ref_start", np.int64), col("nm", np.int64)
    seq_off, seq_len, cig_off, n_cig = col("seq_off", np.int64), col("seq_len", np.int64), col("cig_off", np.int64), col("n_cig", np.int64)
    seq_all, cig_all = S["seq"].cpu().numpy(), S["cigar"].cpu().numpy().astype(np.uint32)
    lut = np.full(256, 255, np.uint8)
    for i, c in enumerate(NIBBLE):
        lut[c] = lut[bytes([c]).lower()[0]] = i
    unal = (flag & 4) != 0
    nd = np.ones(len(read), np.int64)
    for k in range(1, 10):
        nd += read >= 10 ** k
    aux_len = np.where(unal, 0, np.where(nm < 256, 4, np.where(nm < 65536, 5, 7)))
    size = 36 + (nd + 2) + 4 * n_cig + (seq_len + 1) // 2 + seq_len + aux_len
    off = np.cumsum(size) - size
    out = np.zeros(int(size.sum()), np.uint8)
    key = ((nd * 8 + n_cig) * 4096 + seq_len) * 8 + aux_len
    assert n_cig.max() < 8 and seq_len.max() < 4096, "a shape key of this tool's does not hold the records"
    shapes, which = np.unique(key, return_inverse=True)
    order = np.argsort(which, kind="stable")
    bounds = np.searchsorted(which[order], np.arange(len(shapes) + 1))
    for s in range(len(shapes)):
        members = order[bounds[s]:bounds[s + 1]]
        d, nc, sl, al = (int(x[members[0]]) for x in (nd, n_cig, seq_len, aux_len))
        R = int(size[members[0]])
        for at in range(0, len(members), chunk):
            ix = members[at:at + chunk]
            m = len(ix)
            rows = np.zeros((m, R), np.uint8)
            core = np.zeros(m, CORE)
            core["block_size"], core["l_read_name"], core["mapq"], core["bin"], core["n_cigar_op"], core["l_seq"] = R - 4, d + 2, 60, 4680, nc, sl
            core["ref_id"] = np.where(unal[ix], -1, contig[ix])
            core["pos"] = np.where(unal[ix], -1, pos[ix])
            core["flag"], core["next_ref"], core["next_pos"] = flag[ix], -1, -1
            rows[:, :36] = core.view(np.uint8).reshape(m, 36)
            rows[:, 36] = ord("r")
            for j in range(d):
                rows[:, 36 + d - j] = 48 + (read[ix] // 10 ** j) % 10
            p = 36 + d + 2
            if nc:
                rows[:, p:p + 4 * nc] = cig_all[cig_off[ix][:, None] + np.arange(nc)].view(np.uint8).reshape(m, 4 * nc)
                p += 4 * nc
            if sl:
                codes = lut[seq_all[seq_off[ix][:, None] + np.arange(sl)]]
                assert codes.max() < 16, "a SEQ character without a nibble"
                if sl & 1:
                    codes = np.concatenate([codes, np.zeros((m, 1), np.uint8)], axis=1)
                rows[:, p:p + (sl + 1) // 2] = (codes[:, 0::2] << 4) | codes[:, 1::2]
                p += (sl + 1) // 2
                rows[:, p:p + sl] = 0xFF
                p += sl
            if al:
                rows[:, p], rows[:, p + 1], rows[:, p + 2] = ord("N"), ord("M"), {4: ord("C"), 5: ord("S"), 7: ord("I")}[al]
                for j in range(al - 3):
                    rows[:, p + 3 + j] = (nm[ix] >> (8 * j)) & 0xFF
            out[(off[ix][:, None] + np.arange(R)).ravel()] = rows.ravel()
    return out, off.astype(np.uint64)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mbp", type=float, default=5.0, help="assembly size (configs[1]: 5)")
    ap.add_argument("--coverage", type=int, default=200)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--text", action="store_true", help="also write the SAM text and run the device tokenizer on it (tools/gate_timing.py)")
    ap.add_argument("--out", help="also write the JSON line to this file")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    job = synthjob.make_job(dev, contig_lens=(int(a.mbp * 1e6),), coverage=a.coverage, seed=a.seed, pairs=True, unaligned_frac=1e-3)
    torch.cuda.synchronize()
    S = job["sam"]
    n, half = S["n"], S["half"]
    files = []
    for lo, hi in ((0, half), (half, n)):
        b, off = encode_bam(S, lo, hi)
        tb, to = torch.from_numpy(b).to(dev), torch.from_numpy(off.view(np.int64)).to(dev)
        files.append((tb, to, len(b), len(off)))
        print(f"[bam_timing] records [{lo}, {hi}) encoded: {len(b)} bytes", file=sys.stderr, flush=True)
        del b, off
    torch.cuda.synchronize()
    ctx = pp.Context(0)
    ctx.set_profiling(1)
    best = None
    for _ in range(max(1, a.repeat)):
        ms, names_ms, b_bytes, gate_ms, gate_bytes = [0.0, 0.0, 0.0], 0.0, 0, 0.0, 0
        table = pp.Names(ctx)
        for tb, to, n_bytes, n_rec in files:
            rec = pp.BamRecords(ctx, (tb.data_ptr(), n_bytes), (to.data_ptr(), n_rec), None, pp.MEM_DEVICE)
            ms = [x + y for x, y in zip(ms, rec._stage_ms("pp_bam_stage_ms_", ("pass_a", "scans", "pass_b")).values())]
            ln = ctx.download(rec._ptrs["seq_len"], rec.n_rec, np.uint32).astype(np.int64)
            b_bytes += int(((ln + 1) // 2).sum()) + rec.seq_bytes + 8 * rec.n_cig_total + 44 * rec.n_rec
            table.ids(**rec.names(), mem=pp.MEM_DEVICE, out=rec.read_id_ptr)
            names_ms += table.kernel_ms()
            g = pp.gate_records(ctx, rec.raw(), mem=pp.MEM_DEVICE)
            gate_ms += g._stage_ms("pp_gated_stage_ms_", ("gates", "placement", "copy"))["copy"]
            h_len = ctx.download(g._ptrs["seq_len"], g.n_aln, np.uint32)
            gate_bytes += int(h_len.sum(dtype=np.int64)) + g.seq_bytes + 8 * g.n_cig_total
            g.close()
            rec.close()
        table.close()
        if best is None or sum(ms) < best["pass_a_ms"] + best["scans_ms"] + best["pass_b_ms"]:
            bam_bytes = sum(f[2] for f in files)
            best = {"pass_a_ms": round(ms[0], 4), "scans_ms": round(ms[1], 4), "pass_b_ms": round(ms[2], 4), "records": int(n),
                    "bam_bytes": bam_bytes, "pass_a_gbps": round(bam_bytes / 1e9 / (ms[0] / 1e3), 1), "pass_b_bytes": b_bytes,
                    "pass_b_gbps": round(b_bytes / 1e9 / (ms[2] / 1e3), 1), "names_ms": round(names_ms, 4),
                    "gate_seq_copy_ms": round(gate_ms, 4), "gate_seq_copy_gbps": round(gate_bytes / 1e9 / (gate_ms / 1e3), 1) if gate_ms else None}
    out = {"input": f"{a.mbp:g} Mbp x {a.coverage}, {n} records in two files as uncompressed BAM (seed {a.seed})", **best}
    if a.text:
        import gate_timing
        with tempfile.TemporaryDirectory(prefix="pp_bam_", dir=os.environ.get("TMPDIR", "/tmp")) as tmp:
            out["tokenizer_stages_ms"] = gate_timing.tokenizer_stages(job, tmp)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
