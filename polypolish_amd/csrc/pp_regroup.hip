// pp_regroup.hip -- pp_batch_regroup: the records of ONE file brought together read by read, on the device, in front of pp_batch_gate.
//
// The gate restates the reference's streaming rule (alignment.rs:255-263): a read is a run of adjacent aligned records with one
// QNAME.  A coordinate-sorted file scatters a read's records; this link lays them out again as a name-grouped file has them: groups
// in the order of their first record, file order inside a group.  perm[j] = the raw record that stands at place j, which is the
// STABLE order of the records by rep[i] = the first record that carries record i's read_id.
//   k_rid_insert / k_rid_find   (pp_filter_group.h) rep[] through an open-addressing table over the 64-bit ids, as pp_filter_records
//   k_rg_hist      (pp_rg_sort.h, shared with pp_bam_sort) a least-significant-digit radix sort of the indices by rep[], 8 bits a
//   k_rg_scatter   pass, as many passes as n_rec - 1 has bytes; stable and without atomics in the ranks.  The cost is linear in n_rec
//                  whatever the groups' sizes (one group of all records included: every pass then moves every key to where it was)
//   k_rg_count     groups (rep[i] == i) and moved records (perm[j] != j)
//   k_rg_gather    the nine per-record arrays through perm: coalesced writes, random reads.  seq and cigar are not moved:
//                  seq_off / cig_off are indirections already
//   k_rg_aligned   (pp_rg_sort.h) !(flag & 4) of the raw and of the regrouped records; their scans give k_rg_map: aligned rank behind
//   k_rg_map       -> aligned rank in front, which carries the filter's verdicts over (pp_regrouped_pass)
// Offsets and lengths are copied, never followed: nothing in the records can make the call read outside its arrays.
#include "pp_filter_group.h"
#include "pp_rg_sort.h"

#include <cstring>

struct pp_regrouped : DevOwner {  // owns the upload of a host batch, the gathered arrays of a batch whose records moved, and perm
    using DevOwner::DevOwner;
    pp_raw_batch view{};
    u32 *perm = nullptr;
    uint64_t n_groups = 0, n_moved = 0, n_aligned = 0;
    std::vector<uint32_t> amap;  // aligned rank in the regrouped batch -> aligned rank in raw (empty: the identity)
    StageMs<3> t;                // intern | sort | gather, counts and the verdict map
};

namespace {

// counts[0] += groups, counts[1] += moved records: the waves' ballots meet in LDS, one atomic per workgroup and counter (a wave each
// on two words was 1.3 ms of contention on 6.7 M records)
__global__ __launch_bounds__(RG_BLOCK) void k_rg_count(u32 n, const u32 *__restrict__ rep, const u32 *__restrict__ perm, u64 *__restrict__ counts) {
    __shared__ u32 s_n[RG_WAVES][2];
    const u64 i = (u64)blockIdx.x * RG_BLOCK + threadIdx.x;
    const bool in = i < n;
    const u64 g = __ballot(in && rep[i] == (u32)i), m = __ballot(in && perm[i] != (u32)i);
    if ((threadIdx.x & 63u) == 0) {
        s_n[threadIdx.x >> 6][0] = (u32)__popcll(g);
        s_n[threadIdx.x >> 6][1] = (u32)__popcll(m);
    }
    __syncthreads();
    if (threadIdx.x < 2u) {
        u32 sum = 0;
#pragma unroll
        for (u32 w = 0; w < RG_WAVES; w++) sum += s_n[w][threadIdx.x];
        if (sum) atomicAdd(&counts[threadIdx.x], (u64)sum);
    }
}

struct RgArrays { const void *in[9]; void *out[9]; };

__global__ __launch_bounds__(256) void k_rg_gather(u32 n, const u32 *__restrict__ perm, RgArrays A) {
    const u64 j = (u64)blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    const u32 p = perm[j];
    ((uint16_t *)A.out[0])[j] = ((const uint16_t *)A.in[0])[p];
    ((u64 *)A.out[1])[j] = ((const u64 *)A.in[1])[p];
    ((u32 *)A.out[2])[j] = ((const u32 *)A.in[2])[p];
    ((u32 *)A.out[3])[j] = ((const u32 *)A.in[3])[p];
    ((u32 *)A.out[4])[j] = ((const u32 *)A.in[4])[p];
    ((u64 *)A.out[5])[j] = ((const u64 *)A.in[5])[p];
    ((u32 *)A.out[6])[j] = ((const u32 *)A.in[6])[p];
    ((u64 *)A.out[7])[j] = ((const u64 *)A.in[7])[p];
    ((u32 *)A.out[8])[j] = ((const u32 *)A.in[8])[p];
}

enum : int { RG_INTERN = 0, RG_SORT = 1, RG_GATHER = 2 };

}  // namespace

extern "C" void pp_regrouped_free(pp_regrouped *g) { delete g; }

extern "C" void pp_regrouped_raw(const pp_regrouped *g, pp_raw_batch *out) {
    if (out) *out = g ? g->view : pp_raw_batch{};
}

extern "C" const uint32_t *pp_regrouped_perm(const pp_regrouped *g) { return g ? g->perm : nullptr; }

extern "C" void pp_regrouped_counts(const pp_regrouped *g, uint64_t *n_groups, uint64_t *n_moved) {
    if (n_groups) *n_groups = g ? g->n_groups : 0;
    if (n_moved) *n_moved = g ? g->n_moved : 0;
}

extern "C" int pp_regrouped_pass(const pp_regrouped *g, const uint8_t *pass, uint64_t n_pass, uint8_t *out) {
    if (!g) return PP_ERR_ARG;
    if (n_pass != g->n_aligned)
        return g->ctx->fail(PP_ERR_ARG, "pp_regrouped_pass: %llu filter verdicts for %llu aligned records", (unsigned long long)n_pass,
                            (unsigned long long)g->n_aligned);
    if (n_pass && (!pass || !out)) return g->ctx->fail(PP_ERR_ARG, "pp_regrouped_pass: null argument");
    if (g->amap.empty()) {
        if (n_pass && out != pass) memmove(out, pass, (size_t)n_pass);
        return PP_OK;
    }
    for (uint64_t a = 0; a < n_pass; a++) out[a] = pass[g->amap[a]];
    return PP_OK;
}

extern "C" int pp_regrouped_kernel_ms(const pp_regrouped *g, float *ms) {
    return g ? g->t.total(g->ctx, "pp_regrouped_kernel_ms", "when the batch was regrouped", ms) : PP_ERR_ARG;
}

// (internal hooks, not part of the header: tools/regroup_timing.py, tests/test_regroup_gpu.py) the same time by stage: intern | sort |
// gather; and the sort's tile, so that the tests can place their sizes around it
extern "C" int pp_regrouped_stage_ms_(const pp_regrouped *g, float *ms3) { return g ? g->t.stages(ms3) : PP_ERR_ARG; }
extern "C" void pp_regroup_geometry_(uint32_t *tile) {
    if (tile) *tile = RG_TILE;
}

extern "C" int pp_batch_regroup(pp_ctx *ctx, const pp_raw_batch *raw, int mem, pp_regrouped **out) {
    if (!ctx) return PP_ERR_ARG;
    if (int rdy = pp_ctx_wait(ctx)) return rdy;
    if (!raw || !out) return ctx->fail(PP_ERR_ARG, "pp_batch_regroup: null argument");
    *out = nullptr;
    int rc;
    if ((rc = raw_check(ctx, "pp_batch_regroup", raw, mem, RAW_READS))) return rc;
    if (mem == PP_MEM_HOST && ((raw->seq_bytes && !raw->seq) || (raw->n_cig_total && !raw->cigar)))  // (seq and cigar are read to be copied only)
        return ctx->fail(PP_ERR_ARG, "pp_batch_regroup: null array in a non-empty batch");
    PP_HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const u32 n = (u32)raw->n_rec;

    std::unique_ptr<pp_regrouped> P(new pp_regrouped(ctx));
    // ---- the source on the device: a host batch is uploaded into memory of the object ----
    if ((rc = raw_on_device(ctx, *P, mem, raw, RAW_ALL, &P->view))) return rc;
    const pp_raw_batch src = P->view;
    if ((rc = P->alloc(P->perm, n))) return rc;
    if (n == 0) {
        PP_HIPCHK(ctx, hipStreamSynchronize(st));
        *out = P.release();
        return PP_OK;
    }
    const uint16_t *const d_flag = src.flag;
    const u64 *const d_id = (const u64 *)src.read_id;

    CtxScratch T(ctx, ctx->g_rec, "pp_batch_regroup");
    StageTimer timer(ctx, ctx->profiling != 0);
    const unsigned gb = (unsigned)(((u64)n + 255u) / 256u);
    // ---- rep[i]: the first record with record i's id ----
    u64 cap = 1024;  // (a power of two, 2^32 at the most: the mask is 32 bits)
    while (cap < 2ull * n + 2ull && cap < (1ull << 32)) cap <<= 1;
    void *d_slots, *d_rep, *d_isrep;
    if ((rc = T.get(ctx, &d_slots, (size_t)cap * 4)) || (rc = T.get(ctx, &d_rep, (size_t)n * 4)) || (rc = T.get(ctx, &d_isrep, (size_t)n * 4))) return rc;
    if ((rc = timer.begin(RG_INTERN))) return rc;
    PP_HIPCHK(ctx, hipMemsetAsync(d_slots, 0, (size_t)cap * 4, st));
    hipLaunchKernelGGL(k_rid_insert, dim3(gb), dim3(256), 0, st, (u64)n, d_id, (u32 *)d_slots, (u32)(cap - 1));
    hipLaunchKernelGGL(k_rid_find, dim3(gb), dim3(256), 0, st, (u64)n, d_id, (const u32 *)d_slots, (u32)(cap - 1), (u32 *)d_rep, (u32 *)d_isrep);
    if ((rc = timer.end())) return rc;
    PP_HIPCHK(ctx, hipGetLastError());

    // ---- perm: the indices, sorted by rep, stable ----
    u32 *const d_perm = P->perm;
    int passes = 0;
    for (u32 top = n - 1u; top; top >>= 8) passes++;
    const u32 n_tiles = (u32)(((u64)n + RG_TILE - 1u) / RG_TILE);
    const u64 n_cnt = 256ull * n_tiles;
    void *d_key[2] = {nullptr, nullptr}, *d_idx = nullptr, *d_cnt = nullptr, *d_off = nullptr;
    if (passes) {
        if ((rc = T.get(ctx, &d_key[0], (size_t)n * 4)) || (rc = T.get(ctx, &d_cnt, (size_t)n_cnt * 4)) || (rc = T.get(ctx, &d_off, (size_t)(n_cnt + 1) * 4)))
            return rc;
        if (passes > 1 && ((rc = T.get(ctx, &d_key[1], (size_t)n * 4)) || (rc = T.get(ctx, &d_idx, (size_t)n * 4)))) return rc;
    }
    if ((rc = timer.begin(RG_SORT))) return rc;
    if (!passes) hipLaunchKernelGGL(k_rg_iota, dim3(gb), dim3(256), 0, st, n, d_perm);
    {
        // the indices go to and fro between the scratch and perm, so that the last pass writes perm
        const u32 *key_in = (const u32 *)d_rep, *idx_in = nullptr;
        for (int p = 0; p < passes; p++) {
            const bool to_perm = ((passes - 1 - p) & 1) == 0;
            u32 *const key_out = (u32 *)d_key[p & 1], *const idx_out = to_perm ? d_perm : (u32 *)d_idx;
            hipLaunchKernelGGL(k_rg_hist<u32>, dim3(n_tiles), dim3(RG_BLOCK), 0, st, n, key_in, 8u * p, n_tiles, (u32 *)d_cnt);
            if ((rc = scan_u32<u32>(ctx, T.sums(), T.sums_off(), (const u32 *)d_cnt, n_cnt, (u32 *)d_off))) return rc;
            hipLaunchKernelGGL(k_rg_scatter<u32>, dim3(n_tiles), dim3(RG_BLOCK), 0, st, n, key_in, idx_in, 8u * p, n_tiles, (const u32 *)d_off, key_out, idx_out);
            key_in = key_out;
            idx_in = idx_out;
        }
    }
    if ((rc = timer.end())) return rc;
    PP_HIPCHK(ctx, hipGetLastError());

    // ---- groups, moved records, aligned records ----
    void *d_counts, *d_aln, *d_rank_raw;
    if ((rc = T.get(ctx, &d_counts, 16)) || (rc = T.get(ctx, &d_aln, (size_t)n * 4)) || (rc = T.get(ctx, &d_rank_raw, ((size_t)n + 1) * 4))) return rc;
    if ((rc = timer.begin(RG_GATHER))) return rc;
    PP_HIPCHK(ctx, hipMemsetAsync(d_counts, 0, 16, st));
    hipLaunchKernelGGL(k_rg_count, dim3(n_tiles * RG_ROUNDS), dim3(RG_BLOCK), 0, st, n, (const u32 *)d_rep, (const u32 *)d_perm, (u64 *)d_counts);
    hipLaunchKernelGGL(k_rg_aligned, dim3(gb), dim3(256), 0, st, n, d_flag, (const u32 *)nullptr, (u32 *)d_aln);
    if ((rc = scan_u32<u32>(ctx, T.sums(), T.sums_off(), (const u32 *)d_aln, (u64)n, (u32 *)d_rank_raw))) return rc;
    if ((rc = timer.end())) return rc;
    PP_HIPCHK(ctx, hipGetLastError());
    u64 counts[2] = {0, 0};
    u32 n_al = 0;
    if ((rc = fetch(ctx, d_counts, counts, 2)) || (rc = fetch(ctx, (const u32 *)d_rank_raw + n, &n_al))) return rc;
    P->n_groups = counts[0];
    P->n_moved = counts[1];
    P->n_aligned = n_al;

    // ---- the view: the source's own arrays when nothing moves, else the nine arrays through perm ----
    if (P->n_moved) {
        RawArrays G;  // (the object's from the start: an early return frees them with it)
        if ((rc = G.alloc_records(*P, n))) return rc;
        const RgArrays A{{src.flag, src.read_id, src.contig, src.ref_start, src.nm, src.seq_off, src.seq_len, src.cig_off, src.n_cig},
                         {G.flag, G.read_id, G.contig, G.ref_start, G.nm, G.seq_off, G.seq_len, G.cig_off, G.n_cig}};
        void *d_rank_new, *d_amap;
        if ((rc = T.get(ctx, &d_rank_new, ((size_t)n + 1) * 4)) || (rc = T.get(ctx, &d_amap, (size_t)std::max<u32>(1, n_al) * 4))) return rc;
        if ((rc = timer.begin(RG_GATHER))) return rc;
        hipLaunchKernelGGL(k_rg_gather, dim3(gb), dim3(256), 0, st, n, (const u32 *)d_perm, A);
        hipLaunchKernelGGL(k_rg_aligned, dim3(gb), dim3(256), 0, st, n, d_flag, (const u32 *)d_perm, (u32 *)d_aln);
        if ((rc = scan_u32<u32>(ctx, T.sums(), T.sums_off(), (const u32 *)d_aln, (u64)n, (u32 *)d_rank_new))) return rc;
        hipLaunchKernelGGL(k_rg_map, dim3(gb), dim3(256), 0, st, n, d_flag, (const u32 *)d_perm, (const u32 *)d_rank_raw, (const u32 *)d_rank_new,
                           (u32 *)d_amap);
        if ((rc = timer.end())) return rc;
        PP_HIPCHK(ctx, hipGetLastError());
        P->amap.resize(n_al);
        if (n_al && (rc = fetch(ctx, d_amap, P->amap.data(), n_al))) return rc;
        PP_HIPCHK(ctx, hipStreamSynchronize(st));
        for (const void *q : A.in) P->release(q);  // (the stream is synchronised: an uploaded source array has been read and gives way)
        P->view = G.view(n, src.seq_bytes, src.n_cig_total);
        P->view.seq = src.seq;  // (not moved)
        P->view.cigar = src.cigar;
    }
    PP_HIPCHK(ctx, hipStreamSynchronize(st));
    if ((rc = P->t.take(timer))) return rc;
    *out = P.release();
    return PP_OK;
}

extern "C" int pp_ctx_set_regroup(pp_ctx *ctx, int on) {
    if (!ctx) return PP_ERR_ARG;
    ctx->regroup = on != 0;
    return PP_OK;
}

// (internal, the file drivers: pp_driver.cpp, pp_driver_bam.cpp)
extern "C" int pp_ctx_regroup_(const pp_ctx *ctx) { return ctx && ctx->regroup ? 1 : 0; }

extern "C" int pp_ctx_set_text_chain(pp_ctx *ctx, int on) {
    if (!ctx) return PP_ERR_ARG;
    ctx->text_chain = on != 0;
    return PP_OK;
}

// (internal, the file drivers: pp_driver.cpp, pp_filter_host.cpp)
extern "C" int pp_ctx_text_chain_(const pp_ctx *ctx) { return ctx && ctx->text_chain ? 1 : 0; }
