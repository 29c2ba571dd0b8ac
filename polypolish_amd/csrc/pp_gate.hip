// pp_gate.hip -- pp_batch_gate: process_one_read (alignment.rs:275-322) over a caller's RAW alignment records, on the device.
//
// pp_aln_batch asks for the records AFTER the reference's read gates: unaligned records dropped, adjacent records of one read
// grouped, --careful applied, the three gates applied, k = the good alignments of the read, SEQ "*" filled from the read's first
// alignment that has a sequence, everything upper-cased.  Behind SAM text that is pp_ingest.cpp on the host and k_tok_group /
// k_tok_meta / k_tok_seq of pp_tokenize.hip on the device, welded to the text.  This is the fourth producer: the same rules over
// the arrays of a pp_raw_batch, for a caller who parses SAM or BAM itself, holds an aligner's output, or comes out of seam A.
// All of it is work per RECORD -- a read of thousands of alignments (all hits in a repeat) is no lane's loop:
//   k_gate_aligned   rank of every record among the aligned ones (FLAG & 4 takes part in nothing): the workgroups' sums, a scan of
//                    them, then the list rec_of[aligned rank] = raw index.  Every scan here is one of pp_dev.h's: the DPP wave
//                    scan with a carry per workgroup through LDS, k_tscan / k_colscan over the workgroups' sums
//   k_gate_groups    a record opens a group when its read_id differs from the aligned record in front: group of every record,
//                    first record of every group, the same two passes
//   k_gate_judge     the contract (SEQ / CIGAR range inside the arrays, before anything is read through it), the empty CIGAR,
//                    the three gates.  A group's number of good records and its source (the first record with a sequence) are
//                    ONE counter and ONE atomicMin per group, fed once per wave and group: the lanes of a wave that share a group
//                    are a stretch of it, found with ballots, and a group that lies inside one wave is stored without atomics
//   k_gate_place     "no sequence" for the groups that found no source; then out index, room and CIGAR offset of every good
//                    record by scans (rooms and runs in 64 bits), and the record's fields to their place
//   k_gate_seq       the hot kernel: eight lanes per good record, 16 bytes per lane and trip out of the source at any alignment,
//                    upper-cased four bytes at a time, 16-byte aligned stores into the room; the source array's last bytes byte by
//                    byte; a "*" record on the other strand byte by byte, reversed and complemented.  The eight lanes also copy
//                    the record's CIGAR runs.
// The first failing group in file order wins (atomicMin on the raw index of the group's first record << 8 | kind, as the polish
// reports its first offending record).
#include "pp_dev.h"

struct pp_gated : DevOwner {
    using DevOwner::DevOwner;
    AlnArrays a;
    u32 *orig = nullptr;  // the raw index of every gated record
    pp_aln_batch view{};
    pp_sam_counts counts{};
    StageMs<3> t;         // ranks, groups, gates and scans | placement | SEQ and CIGAR copy
};

namespace {

constexpr u32 GATE_BLOCK = 1024;  // records per workgroup of the scanning kernels
constexpr u32 GATE_NONE = 0xFFFFFFFFu;
constexpr u64 GATE_RC = 1ull << 63;  // desc[]: the source's bytes go in reversed and complemented (seq_off < 2^40)
// status[0]: raw index of the failing group's first record << 8 | kind -- "no sequence" is asked first (alignment.rs:277-281)
enum : u32 { GE_NO_SEQUENCE = 1, GE_EMPTY_CIGAR = 2 };
// status[1]: raw index of a record that breaks the contract << 8 | kind
enum : u32 { GA_SEQ_RANGE = 1, GA_CIG_RANGE = 2 };

struct GateRaw {  // the raw batch (device memory)
    const uint16_t *flag;
    const u64 *read_id, *seq_off, *cig_off;
    const u32 *contig, *ref_start, *nm, *seq_len, *n_cig, *cigar;
    const u8 *seq;
    u64 seq_bytes, n_cig_total;
};
struct GateOut {
    u32 *contig, *ref_start, *k, *seq_len, *n_cig, *orig;
    u64 *seq_off, *cig_off, *desc;  // desc: where the source has the record's bytes | GATE_RC
};

// blk_off == nullptr: the workgroups' numbers of aligned records; else rec_of[aligned rank] = raw index
__global__ __launch_bounds__(GATE_BLOCK) void k_gate_aligned(u32 n_rec, const uint16_t *__restrict__ flag, const u32 *__restrict__ blk_off,
                                                             u32 *__restrict__ blk_sum, u32 *__restrict__ rec_of) {
    __shared__ u32 s_w[GATE_BLOCK / 64];
    const u64 r = (u64)blockIdx.x * GATE_BLOCK + threadIdx.x;
    const u32 al = (r < n_rec && !(flag[r] & 4u)) ? 1u : 0u;
    u32 total;
    const u32 ex = block_scan_excl<GATE_BLOCK>(al, s_w, &total);
    if (!blk_off) {
        if (threadIdx.x == 0) blk_sum[blockIdx.x] = total;
        return;
    }
    if (al) rec_of[blk_off[blockIdx.x] + ex] = (u32)r;
}

// blk_off == nullptr: the workgroups' numbers of group starts; else grp_of[a], grp_first[g] (and grp_first[n_groups] = n_al)
__global__ __launch_bounds__(GATE_BLOCK) void k_gate_groups(u32 n_al, const u32 *__restrict__ rec_of, const u64 *__restrict__ read_id,
                                                            const u32 *__restrict__ blk_off, u32 *__restrict__ blk_sum,
                                                            u32 *__restrict__ grp_of, u32 *__restrict__ grp_first) {
    __shared__ u32 s_w[GATE_BLOCK / 64];
    const u64 a = (u64)blockIdx.x * GATE_BLOCK + threadIdx.x;
    const u32 start = (a < n_al && (a == 0 || read_id[rec_of[a]] != read_id[rec_of[a - 1]])) ? 1u : 0u;
    u32 total;
    const u32 ex = block_scan_excl<GATE_BLOCK>(start, s_w, &total);
    if (!blk_off) {
        if (threadIdx.x == 0) blk_sum[blockIdx.x] = total;
        return;
    }
    if (a >= n_al) return;
    const u32 g = blk_off[blockIdx.x] + ex + start - 1u;  // (record 0 opens group 0)
    grp_of[a] = g;
    if (start) grp_first[g] = (u32)a;
    if (a == (u64)n_al - 1u) grp_first[g + 1u] = n_al;
}

__global__ __launch_bounds__(256) void k_gate_judge(u32 n_al, GateRaw R, const u32 *__restrict__ rec_of, const u32 *__restrict__ grp_of,
                                                    const u32 *__restrict__ grp_first, u32 max_errors, int careful,
                                                    const u8 *__restrict__ pass, u64 n_pass, u8 *__restrict__ good,
                                                    u32 *__restrict__ g_cnt, u32 *__restrict__ g_src, u64 *__restrict__ status) {
    const u32 a = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    const bool in = a < n_al;
    u32 g = GATE_NONE, gf = 0, ge = 0;
    bool ok = false, has_seq = false;
    if (in) {
        g = grp_of[a];
        gf = grp_first[g];
        ge = grp_first[g + 1u];
        if (!(careful && ge - gf > 1u)) {  // (--careful: nothing of such a group is used, nothing of it is looked at)
            const u32 r = rec_of[a], sl = R.seq_len[r], nc = R.n_cig[r];
            const u64 co = R.cig_off[r];
            const bool seq_ok = sl == 0 || inside(R.seq_off[r], sl, R.seq_bytes);
            const bool cig_ok = nc == 0 || inside(co, nc, R.n_cig_total);
            if (!seq_ok) report(status + 1, ((u64)r << 8) | GA_SEQ_RANGE);
            else if (!cig_ok) report(status + 1, ((u64)r << 8) | GA_CIG_RANGE);
            has_seq = sl > 0;
            if (nc == 0) report(status, ((u64)rec_of[gf] << 8) | GE_EMPTY_CIGAR);  // empty expanded CIGAR: the reference panics
            else if (cig_ok) {
                const u32 f = R.cigar[co] & 15u, l = R.cigar[co + nc - 1u] & 15u;
                const bool ends_ok = (f == PP_OP_M || f == PP_OP_EQ) && (l == PP_OP_M || l == PP_OP_EQ);
                // pass: the filter's verdict for this aligned record (a record beyond the verdicts that are there passes: the
                // host says PP_ERR_ARG for the wrong count once the records are found free of defects)
                ok = ends_ok && R.nm[r] <= max_errors && (!pass || (u64)a >= n_pass || pass[a] != 0);
            }
        }
        good[a] = ok ? 1 : 0;
    }
    // The wave's lanes that share a group are a stretch of it: its last lane speaks for the stretch.
    const u32 gp = (u32)__shfl_up((int)g, 1, 64), gn = (u32)__shfl_down((int)g, 1, 64);
    const bool head = lane == 0 || g != gp, tail = in && (lane == 63u || g != gn);
    const u64 heads = __ballot(head), goods = __ballot(ok), seqs = __ballot(has_seq);
    if (tail) {
        const u64 upto = lane == 63u ? ~0ull : ((1ull << (lane + 1u)) - 1ull);
        const u32 hl = 63u - (u32)__clzll((long long)(heads & upto));  // (lane 0 is a head)
        const u64 m = upto & ~((1ull << hl) - 1ull);
        const u32 cnt = (u32)__popcll(goods & m);
        const u64 s = seqs & m;
        const u32 src = s ? a - lane + (u32)(__ffsll((long long)s) - 1) : GATE_NONE;
        if (a - (lane - hl) == gf && a + 1u == ge) {  // the whole group: nobody else writes its words
            g_cnt[g] = cnt;
            g_src[g] = src;
        } else {
            if (cnt) atomicAdd(&g_cnt[g], cnt);
            if (s) atomicMin(&g_src[g], src);
        }
    }
}

// PLACE == false: "no sequence" for the groups without a source, and the workgroups' sums of good records, rooms (in units of
// PP_SEQ_ALIGN bytes) and CIGAR runs (blk3: three words per workgroup).  PLACE == true: blk3 holds their exclusive scan, and
// every good record goes to its place.
template <bool PLACE>
__global__ __launch_bounds__(GATE_BLOCK) void k_gate_place(u32 n_al, GateRaw R, const u32 *__restrict__ rec_of, const u32 *__restrict__ grp_of,
                                                           const u32 *__restrict__ grp_first, const u8 *__restrict__ good,
                                                           const u32 *__restrict__ g_cnt, const u32 *__restrict__ g_src, int careful,
                                                           u64 *__restrict__ blk3, GateOut O, u64 *__restrict__ status) {
    __shared__ u32 s_w[GATE_BLOCK / 64];
    __shared__ u64 s_w64[GATE_BLOCK / 64];
    const u64 a = (u64)blockIdx.x * GATE_BLOCK + threadIdx.x;
    u32 is_good = 0, units = 0, nc = 0, r = 0, g = 0, sl = 0, src_a = GATE_NONE;
    if (a < n_al) {
        g = grp_of[a];
        r = rec_of[a];
        if (!PLACE && grp_first[g] == (u32)a) {  // the group's first record speaks for it
            const u32 size = grp_first[g + 1u] - (u32)a;
            if (!(careful && size > 1u) && g_src[g] == GATE_NONE) report(status, ((u64)r << 8) | GE_NO_SEQUENCE);
        }
        if (good[a]) {
            is_good = 1;
            nc = R.n_cig[r];
            sl = R.seq_len[r];
            if (sl == 0) {  // SEQ "*": the group's source (a group without one fails: nothing is placed)
                src_a = g_src[g];
                if (src_a != GATE_NONE) sl = R.seq_len[rec_of[src_a]];
            }
            units = (u32)room_units(sl);
        }
    }
    u32 t_cnt;
    u64 t_units, t_cig;
    const u32 ex_cnt = block_scan_excl<GATE_BLOCK>(is_good, s_w, &t_cnt);
    const u64 ex_units = block_scan_excl64<GATE_BLOCK>(units, s_w64, &t_units);
    const u64 ex_cig = block_scan_excl64<GATE_BLOCK>(nc, s_w64, &t_cig);
    u64 *const mine = blk3 + 3ull * blockIdx.x;
    if (!PLACE) {
        if (threadIdx.x == 0) { mine[0] = t_cnt; mine[1] = t_units; mine[2] = t_cig; }
        return;
    }
    if (!is_good) return;
    const u64 o = mine[0] + ex_cnt;
    const u32 rs = src_a == GATE_NONE ? r : rec_of[src_a];
    const bool rc = rs != r && ((R.flag[r] ^ R.flag[rs]) & 16u) != 0;
    O.contig[o] = R.contig[r];
    O.ref_start[o] = R.ref_start[r];
    O.k[o] = g_cnt[g];
    O.seq_len[o] = sl;
    O.n_cig[o] = nc;
    O.seq_off[o] = (mine[1] + ex_units) * (u64)PP_SEQ_ALIGN;
    O.cig_off[o] = mine[2] + ex_cig;
    O.orig[o] = r;
    O.desc[o] = R.seq_off[rs] | (rc ? GATE_RC : 0ull);
}

// upper-cases the four ASCII bytes of a word: bit 7 of every byte in 'a'..'z', shifted down to the 0x20 that is taken off
__device__ __forceinline__ u32 upper4(u32 w) {
    const u32 x = w & 0x7F7F7F7Fu;
    const u32 m = (x + 0x1F1F1F1Fu) & ~(x + 0x05050505u) & ~w & 0x80808080u;
    return w - (m >> 2);
}

// The SEQ bytes into their rooms and the CIGAR runs to their place: eight lanes per good record.  Every source range was found
// inside the source array by k_gate_judge; a 16-byte load that would reach past the array's end is taken byte by byte.
__global__ __launch_bounds__(256) void k_gate_seq(u32 n_good, const u32 *__restrict__ seq_len, const u64 *__restrict__ seq_off,
                                                  const u64 *__restrict__ desc, const u32 *__restrict__ n_cig, const u64 *__restrict__ cig_off,
                                                  const u32 *__restrict__ orig, const u64 *__restrict__ src_cig_off,
                                                  const u32 *__restrict__ src_cigar, const u8 *__restrict__ src, u64 src_bytes,
                                                  u8 *__restrict__ seq, u32 *__restrict__ cigar) {
    const u64 t = (u64)blockIdx.x * 256u + threadIdx.x;
    const u32 s = (u32)t & 7u;
    if ((t >> 3) >= n_good) return;
    const u32 o = (u32)(t >> 3);
    const u64 n = seq_len[o], room = room_bytes(n);
    const u64 d = desc[o], at0 = d & ~GATE_RC;
    const bool rc = (d & GATE_RC) != 0;
    u8 *const out = seq + seq_off[o];  // a multiple of PP_SEQ_ALIGN
    for (u64 i = 16u * s; i < room; i += 128u) {
        u32 w0 = 0, w1 = 0, w2 = 0, w3 = 0;
        if (i < n) {
            const u32 live = (u32)min((u64)16, n - i);  // bytes of this chunk that belong to the read (>= 1)
            if (!rc && at0 + i + 16u <= src_bytes) {
                uint4 v;
                __builtin_memcpy(&v, src + at0 + i, 16);  // (any alignment: one global_load_dwordx4)
                const u64 lo = live >= 8u ? ~0ull : ((1ull << (8u * live)) - 1ull);
                const u64 hi = live >= 16u ? ~0ull : (live > 8u ? ((1ull << (8u * (live - 8u))) - 1ull) : 0ull);
                w0 = upper4(v.x & (u32)lo); w1 = upper4(v.y & (u32)(lo >> 32));
                w2 = upper4(v.z & (u32)hi); w3 = upper4(v.w & (u32)(hi >> 32));
            } else {
                // the last bytes of the source array, or a "*" record on the other strand (rare): byte by byte
                u64 a = 0, b = 0;
                for (u32 j = 0; j < live; j++) {
                    u8 c = rc ? src[at0 + (n - 1u - (i + j))] : src[at0 + i + j];
                    if (c >= (u8)'a' && c <= (u8)'z') c = (u8)(c - 32);
                    if (rc) c = comp_upper(c);
                    if (j < 8u) a |= (u64)c << (8u * j); else b |= (u64)c << (8u * (j - 8u));
                }
                w0 = (u32)a; w1 = (u32)(a >> 32); w2 = (u32)b; w3 = (u32)(b >> 32);
            }
        }
        *(uint4 *)(out + i) = make_uint4(w0, w1, w2, w3);
    }
    const u32 nc = n_cig[o];
    const u32 *const cs = src_cigar + src_cig_off[orig[o]];
    u32 *const cd = cigar + cig_off[o];
    for (u32 j = s; j < nc; j += 8u) cd[j] = cs[j];
}

}  // namespace

extern "C" void pp_gated_free(pp_gated *g) { delete g; }

extern "C" void pp_gated_batch(const pp_gated *g, pp_aln_batch *out, const uint32_t **orig) {
    if (out) *out = g ? g->view : pp_aln_batch{};
    if (orig) *orig = g ? g->orig : nullptr;
}

extern "C" void pp_gated_counts(const pp_gated *g, pp_sam_counts *out) {
    if (out) *out = g ? g->counts : pp_sam_counts{};
}

extern "C" int pp_gated_kernel_ms(const pp_gated *g, float *ms) {
    return g ? g->t.total(g->ctx, "pp_gated_kernel_ms", "when the batch was gated", ms) : PP_ERR_ARG;
}

// (internal hook, not part of the header: tools/gate_timing.py) the same time by stage: gates and scans | placement | SEQ and CIGAR copy
extern "C" int pp_gated_stage_ms_(const pp_gated *g, float *ms3) { return g ? g->t.stages(ms3) : PP_ERR_ARG; }

extern "C" int pp_batch_gate(pp_ctx *ctx, const pp_raw_batch *raw, int mem, uint32_t max_errors, int careful, const uint8_t *pass,
                             uint64_t n_pass, pp_gated **out, uint64_t *bad_record) {
    if (!ctx) return PP_ERR_ARG;
    if (int rdy = pp_ctx_wait(ctx)) return rdy;
    if (bad_record) *bad_record = ~0ull;
    if (!raw || !out) return ctx->fail(PP_ERR_ARG, "pp_batch_gate: null argument");
    *out = nullptr;
    int rc;
    if ((rc = raw_check(ctx, "pp_batch_gate", raw, mem, RAW_ALL | RAW_SEQ_LIMIT))) return rc;
    PP_HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const u32 n_rec = (u32)raw->n_rec;

    std::unique_ptr<pp_gated> P(new pp_gated(ctx));
    // a batch without aligned records gates to an empty batch -- unless it came with verdicts for records it does not have
    auto empty = [&]() -> int {
        PP_HIPCHK(ctx, hipStreamSynchronize(st));
        if (pass && n_pass != 0)
            return ctx->fail(PP_ERR_ARG, "pp_batch_gate: %llu filter verdicts for 0 aligned records", (unsigned long long)n_pass);
        *out = P.release();
        return PP_OK;
    };
    if (n_rec == 0) return empty();

    CallScratch T;
    StageTimer timer(ctx, ctx->profiling != 0);
    // ---- the source on the device ----
    pp_raw_batch D;
    if ((rc = raw_on_device(ctx, T, mem, raw, RAW_ALL, &D))) return rc;
    const GateRaw R{D.flag, (const u64 *)D.read_id, (const u64 *)D.seq_off, (const u64 *)D.cig_off, D.contig, D.ref_start, D.nm, D.seq_len, D.n_cig,
                    D.cigar, D.seq, D.seq_bytes, D.n_cig_total};

    // ---- the aligned records ----
    const u32 nb_r = (n_rec + GATE_BLOCK - 1u) / GATE_BLOCK;
    void *d_blk, *d_blkoff, *d_rec_of;
    if ((rc = T.get(ctx, &d_blk, (size_t)nb_r * 4)) || (rc = T.get(ctx, &d_blkoff, ((size_t)nb_r + 1) * 4)) || (rc = T.get(ctx, &d_rec_of, (size_t)n_rec * 4)))
        return rc;
    if ((rc = timer.begin(0))) return rc;
    hipLaunchKernelGGL(k_gate_aligned, dim3(nb_r), dim3(GATE_BLOCK), 0, st, n_rec, R.flag, (const u32 *)nullptr, (u32 *)d_blk, (u32 *)nullptr);
    hipLaunchKernelGGL(k_tscan<u32>, dim3(1), dim3(1024), 0, st, (const u32 *)d_blk, (u64)nb_r, (u32 *)d_blkoff);
    hipLaunchKernelGGL(k_gate_aligned, dim3(nb_r), dim3(GATE_BLOCK), 0, st, n_rec, R.flag, (const u32 *)d_blkoff, (u32 *)d_blk, (u32 *)d_rec_of);
    if ((rc = timer.end())) return rc;
    PP_HIPCHK(ctx, hipGetLastError());
    u32 n_al = 0;
    if ((rc = fetch(ctx, (const u32 *)d_blkoff + nb_r, &n_al))) return rc;
    if (n_al == 0) return empty();

    // ---- groups, gates, sums ----
    const u32 nb = (n_al + GATE_BLOCK - 1u) / GATE_BLOCK;
    const u64 n_pass_dev = pass ? std::min<u64>(n_pass, n_al) : 0;
    void *d_gblk, *d_gblkoff, *d_grp_of, *d_grp_first, *d_good, *d_gcnt, *d_gsrc, *d_blk3, *d_blk3off, *d_status;
    const u8 *d_pass = nullptr;  // (the verdicts are host memory whatever the batch is)
    if ((rc = T.get(ctx, &d_gblk, (size_t)nb * 4)) || (rc = T.get(ctx, &d_gblkoff, ((size_t)nb + 1) * 4)) || (rc = T.get(ctx, &d_grp_of, (size_t)n_al * 4)) ||
        (rc = T.get(ctx, &d_grp_first, ((size_t)n_al + 1) * 4)) || (rc = T.get(ctx, &d_good, (size_t)n_al)) || (rc = T.get(ctx, &d_gcnt, (size_t)n_al * 4)) ||
        (rc = T.get(ctx, &d_gsrc, (size_t)n_al * 4)) || (rc = T.get(ctx, &d_blk3, (size_t)nb * 24)) || (rc = T.get(ctx, &d_blk3off, ((size_t)nb + 1) * 24)) ||
        (rc = T.get(ctx, &d_status, 16)))
        return rc;
    if (pass && (rc = on_device(ctx, T, PP_MEM_HOST, pass, (size_t)n_pass_dev, &d_pass))) return rc;
    if ((rc = timer.begin(0))) return rc;
    PP_HIPCHK(ctx, hipMemsetAsync(d_gcnt, 0, (size_t)n_al * 4, st));
    PP_HIPCHK(ctx, hipMemsetAsync(d_gsrc, 0xFF, (size_t)n_al * 4, st));
    PP_HIPCHK(ctx, hipMemsetAsync(d_status, 0xFF, 16, st));
    hipLaunchKernelGGL(k_gate_groups, dim3(nb), dim3(GATE_BLOCK), 0, st, n_al, (const u32 *)d_rec_of, R.read_id, (const u32 *)nullptr, (u32 *)d_gblk,
                       (u32 *)nullptr, (u32 *)nullptr);
    hipLaunchKernelGGL(k_tscan<u32>, dim3(1), dim3(1024), 0, st, (const u32 *)d_gblk, (u64)nb, (u32 *)d_gblkoff);
    hipLaunchKernelGGL(k_gate_groups, dim3(nb), dim3(GATE_BLOCK), 0, st, n_al, (const u32 *)d_rec_of, R.read_id, (const u32 *)d_gblkoff, (u32 *)d_gblk,
                       (u32 *)d_grp_of, (u32 *)d_grp_first);
    hipLaunchKernelGGL(k_gate_judge, dim3((n_al + 255u) / 256u), dim3(256), 0, st, n_al, R, (const u32 *)d_rec_of, (const u32 *)d_grp_of,
                       (const u32 *)d_grp_first, (u32)max_errors, careful ? 1 : 0, d_pass, n_pass_dev, (u8 *)d_good, (u32 *)d_gcnt,
                       (u32 *)d_gsrc, (u64 *)d_status);
    GateOut O{};
    hipLaunchKernelGGL(k_gate_place<false>, dim3(nb), dim3(GATE_BLOCK), 0, st, n_al, R, (const u32 *)d_rec_of, (const u32 *)d_grp_of,
                       (const u32 *)d_grp_first, (const u8 *)d_good, (const u32 *)d_gcnt, (const u32 *)d_gsrc, careful ? 1 : 0, (u64 *)d_blk3, O,
                       (u64 *)d_status);
    hipLaunchKernelGGL(k_colscan<3>, dim3(1), dim3(1024), 0, st, (const u64 *)d_blk3, (u64)nb, (u64 *)d_blk3off);
    if ((rc = timer.end())) return rc;
    PP_HIPCHK(ctx, hipGetLastError());
    u64 status[2] = {~0ull, ~0ull}, totals[3] = {0, 0, 0};
    u32 n_groups = 0;
    if ((rc = fetch(ctx, d_status, status, 2)) || (rc = fetch(ctx, (const u64 *)d_blk3off + 3ull * nb, totals, 3)) ||
        (rc = fetch(ctx, (const u32 *)d_gblkoff + nb, &n_groups)))
        return rc;
    if (status[1] != ~0ull) {
        if (bad_record) *bad_record = status[1] >> 8;
        return ctx->fail(PP_ERR_ARG, "pp_batch_gate: the %s range of record %llu does not lie inside the batch's %s array",
                         (status[1] & 0xFFu) == GA_SEQ_RANGE ? "SEQ" : "CIGAR", (unsigned long long)(status[1] >> 8),
                         (status[1] & 0xFFu) == GA_SEQ_RANGE ? "seq" : "cigar");
    }
    if (status[0] != ~0ull) {
        if (bad_record) *bad_record = status[0] >> 8;
        if ((status[0] & 0xFFu) == GE_NO_SEQUENCE)
            return ctx->fail(PP_ERR_QUIT, "no alignments for read record %llu contain sequence", (unsigned long long)(status[0] >> 8));
        return ctx->fail(PP_ERR_PANIC, "an alignment of read record %llu has an empty CIGAR (the reference panics on its first run)",
                         (unsigned long long)(status[0] >> 8));
    }
    if (pass && n_pass != n_al)
        return ctx->fail(PP_ERR_ARG, "pp_batch_gate: %llu filter verdicts for %llu aligned records", (unsigned long long)n_pass, (unsigned long long)n_al);
    const u32 n_good = (u32)totals[0];
    const u64 total = totals[1] * (u64)PP_SEQ_ALIGN, n_cig_out = totals[2];
    if (total >= (1ull << 40)) return ctx->fail(PP_ERR_LIMIT, "more than 2^40 SEQ bytes in one gated batch");
    P->counts.alignments = n_al;
    P->counts.used = n_good;
    P->counts.reads = n_groups;

    // ---- the result ----
    AlnArrays &A = P->a;
    if ((rc = A.alloc_records(*P, n_good)) || (rc = P->alloc(A.seq, (size_t)total + 64)) || (rc = P->alloc(A.cigar, (size_t)n_cig_out)) ||
        (rc = P->alloc(P->orig, n_good)))
        return rc;
    PP_HIPCHK(ctx, hipMemsetAsync(A.seq + total, 0, 64, st));
    void *d_desc;  // (the call's: nothing of the object points to it)
    if ((rc = T.get(ctx, &d_desc, (size_t)n_good * 8))) return rc;
    O = GateOut{A.contig, A.ref_start, A.k, A.seq_len, A.n_cig, P->orig, A.seq_off, A.cig_off, (u64 *)d_desc};
    if ((rc = timer.begin(1))) return rc;
    if (n_good)
        hipLaunchKernelGGL(k_gate_place<true>, dim3(nb), dim3(GATE_BLOCK), 0, st, n_al, R, (const u32 *)d_rec_of, (const u32 *)d_grp_of,
                           (const u32 *)d_grp_first, (const u8 *)d_good, (const u32 *)d_gcnt, (const u32 *)d_gsrc, careful ? 1 : 0, (u64 *)d_blk3off, O,
                           (u64 *)d_status);
    if ((rc = timer.end()) || (rc = timer.begin(2))) return rc;
    if (n_good)
        hipLaunchKernelGGL(k_gate_seq, dim3((unsigned)(((u64)n_good * 8u + 255u) / 256u)), dim3(256), 0, st, n_good, (const u32 *)A.seq_len,
                           (const u64 *)A.seq_off, (const u64 *)d_desc, (const u32 *)A.n_cig, (const u64 *)A.cig_off, (const u32 *)P->orig, R.cig_off,
                           R.cigar, R.seq, R.seq_bytes, A.seq, A.cigar);
    if ((rc = timer.end())) return rc;
    PP_HIPCHK(ctx, hipGetLastError());
    PP_HIPCHK(ctx, hipStreamSynchronize(st));  // the source may be released, the scratch goes away
    if ((rc = P->t.take(timer))) return rc;
    P->view = A.view(n_good, total, n_cig_out);
    *out = P.release();
    return PP_OK;
}
