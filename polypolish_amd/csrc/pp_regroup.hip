// pp_regroup.hip -- pp_batch_regroup: the records of ONE file brought together read by read, on the device, in front of pp_batch_gate.
//
// The gate restates the reference's streaming rule (alignment.rs:255-263): a read is a run of adjacent aligned records with one
// QNAME.  A coordinate-sorted file scatters a read's records; this link lays them out again as a name-grouped file has them: groups
// in the order of their first record, file order inside a group.  perm[j] = the raw record that stands at place j, which is the
// STABLE order of the records by rep[i] = the first record that carries record i's read_id.
//   k_rid_insert / k_rid_find   (pp_filter_group.h) rep[] through an open-addressing table over the 64-bit ids, as pp_filter_records
//   k_rg_hist      a least-significant-digit radix sort of the indices by rep[], 8 bits a pass, as many passes as n_rec - 1 has
//   k_rg_scatter   bytes.  A pass: every tile of RG_TILE keys counts its 256 digits (LDS); the counts, laid out digit by digit and
//                  inside a digit tile by tile, are scanned (scan_u32) into the place of every (digit, tile)'s first key; the scatter
//                  ranks a key among the equal digits of its tile WITHOUT atomics -- lanes below it in its wave's round (64-bit
//                  ballots, one per digit bit), the wave's earlier rounds, the tile's earlier waves (their counts through LDS) -- so
//                  that a pass is stable and the order never depends on how atomics land.  The cost is linear in n_rec whatever the
//                  groups' sizes (one group of all records included: every pass then moves every key to where it was)
//   k_rg_count     groups (rep[i] == i) and moved records (perm[j] != j)
//   k_rg_gather    the nine per-record arrays through perm: coalesced writes, random reads.  seq and cigar are not moved:
//                  seq_off / cig_off are indirections already
//   k_rg_aligned   !(flag & 4) of the raw and of the regrouped records; their scans give k_rg_map: aligned rank behind -> aligned
//   k_rg_map       rank in front, which carries the filter's verdicts over (pp_regrouped_pass)
// Offsets and lengths are copied, never followed: nothing in the records can make the call read outside its arrays.
#include "pp_filter_group.h"

#include <cstring>

struct pp_regrouped {
    pp_ctx *ctx = nullptr;
    // flag read_id contig ref_start nm seq_off seq_len cig_off n_cig | seq cigar (PP_MEM_HOST) | perm
    void *d[12] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    pp_raw_batch view{};
    uint64_t n_groups = 0, n_moved = 0, n_aligned = 0;
    std::vector<uint32_t> amap;  // aligned rank in the regrouped batch -> aligned rank in raw (empty: the identity)
    bool timed = false;
    float ms[3] = {0.f, 0.f, 0.f};  // intern | sort | gather, counts and the verdict map
};

namespace {

constexpr u32 RG_BLOCK = 1024;                    // 16 waves ...
constexpr u32 RG_ROUNDS = 4;                      // ... each takes 4 x 64 adjacent keys: round by round, lane by lane
constexpr u32 RG_TILE = RG_BLOCK * RG_ROUNDS;     // keys per workgroup
constexpr u32 RG_WAVES = RG_BLOCK / 64u;
constexpr u32 RG_SIZE[9] = {2, 8, 4, 4, 4, 8, 4, 8, 4};  // bytes per element of the nine arrays

// the place of the key that lane `lane` of wave `wave` takes in round `j` of its tile
__device__ __forceinline__ u64 rg_index(u32 wave, u32 j, u32 lane) {
    return (u64)blockIdx.x * RG_TILE + wave * (64u * RG_ROUNDS) + j * 64u + lane;
}

__global__ __launch_bounds__(256) void k_rg_iota(u32 n, u32 *__restrict__ perm) {
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    if (i < n) perm[i] = (u32)i;
}

// cnt[digit * n_tiles + tile] = the tile's keys with that digit
__global__ __launch_bounds__(RG_BLOCK) void k_rg_hist(u32 n, const u32 *__restrict__ key, u32 shift, u32 n_tiles, u32 *__restrict__ cnt) {
    __shared__ u32 s_h[256];
    if (threadIdx.x < 256u) s_h[threadIdx.x] = 0;
    __syncthreads();
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (u32 j = 0; j < RG_ROUNDS; j++) {
        const u64 i = rg_index(wave, j, lane);
        if (i < n) atomicAdd(&s_h[(key[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 256u) cnt[(u64)threadIdx.x * n_tiles + blockIdx.x] = s_h[threadIdx.x];
}

// off[digit * n_tiles + tile] = where the tile's first key with that digit goes.  idx_in == nullptr: the keys stand in index order
// (the first pass).
__global__ __launch_bounds__(RG_BLOCK) void k_rg_scatter(u32 n, const u32 *__restrict__ key_in, const u32 *__restrict__ idx_in, u32 shift,
                                                         u32 n_tiles, const u32 *__restrict__ off, u32 *__restrict__ key_out,
                                                         u32 *__restrict__ idx_out) {
    __shared__ u32 s_c[RG_WAVES][256];  // keys of wave w with digit d so far; then the place of the wave's first such key
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (u32 t = threadIdx.x; t < RG_WAVES * 256u; t += RG_BLOCK) (&s_c[0][0])[t] = 0;
    __syncthreads();
    const u64 below = (1ull << lane) - 1ull;
    u32 key[RG_ROUNDS], at[RG_ROUNDS];  // at: the key's rank among its wave's keys with its digit
    bool live[RG_ROUNDS];
#pragma unroll
    for (u32 j = 0; j < RG_ROUNDS; j++) {
        const u64 i = rg_index(wave, j, lane);
        live[j] = i < n;
        key[j] = live[j] ? key_in[i] : 0u;
        const u32 d = (key[j] >> shift) & 255u;
        u64 peers = __ballot(live[j]);  // the round's live lanes with this lane's digit
#pragma unroll
        for (u32 b = 0; b < 8; b++) {
            const u64 m = __ballot((d >> b) & 1u);
            peers &= ((d >> b) & 1u) ? m : ~m;
        }
        // every lane reads the wave's count, then the digit's first lane adds the round's: a barrier between the two and behind
        // them (all waves make all rounds), so that neither the hardware nor the compiler may take one for the other
        at[j] = s_c[wave][d] + (u32)__popcll(peers & below);
        __syncthreads();
        if (live[j] && (peers & below) == 0) s_c[wave][d] += (u32)__popcll(peers);
        __syncthreads();
    }
    if (threadIdx.x < 256u) {  // a digit each: the waves in order, on top of the tile's place
        u32 run = off[(u64)threadIdx.x * n_tiles + blockIdx.x];
#pragma unroll
        for (u32 w = 0; w < RG_WAVES; w++) {
            const u32 c = s_c[w][threadIdx.x];
            s_c[w][threadIdx.x] = run;
            run += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (u32 j = 0; j < RG_ROUNDS; j++) {
        if (!live[j]) continue;
        const u64 i = rg_index(wave, j, lane);
        const u32 to = s_c[wave][(key[j] >> shift) & 255u] + at[j];
        if (to < n) {  // (it is: the places come from the counts of these very keys)
            key_out[to] = key[j];
            idx_out[to] = idx_in ? idx_in[i] : (u32)i;
        }
    }
}

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

// perm == nullptr: the raw records' own order
__global__ __launch_bounds__(256) void k_rg_aligned(u32 n, const uint16_t *__restrict__ flag, const u32 *__restrict__ perm, u32 *__restrict__ is_aln) {
    const u64 j = (u64)blockIdx.x * 256u + threadIdx.x;
    if (j < n) is_aln[j] = (flag[perm ? perm[j] : (u32)j] & 4u) ? 0u : 1u;
}

__global__ __launch_bounds__(256) void k_rg_map(u32 n, const uint16_t *__restrict__ flag, const u32 *__restrict__ perm, const u32 *__restrict__ rank_raw,
                                                const u32 *__restrict__ rank_new, u32 *__restrict__ amap) {
    const u64 j = (u64)blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    const u32 p = perm[j];
    if (!(flag[p] & 4u)) amap[rank_new[j]] = rank_raw[p];
}

// the call's scratch: the context's grow-only buffers (pp_ctx::g_rec) in the order of the requests, as pp_filter_records keeps its own
struct Scratch {
    pp_ctx *ctx;
    size_t k = 2;  // ([0], [1]: scan_u32's block sums)
    pp::DevBuf &sums() { return ctx->g_rec[0]; }
    pp::DevBuf &sums_off() { return ctx->g_rec[1]; }
    int get(pp_ctx *, void **out, size_t bytes) {
        *out = nullptr;
        if (k >= sizeof ctx->g_rec / sizeof ctx->g_rec[0]) return ctx->fail(PP_ERR_HIP, "pp_batch_regroup: out of buffer slots");
        if (int rc = pp::dev_ensure(ctx, ctx->g_rec[k], bytes ? bytes : 16)) return rc;
        *out = ctx->g_rec[k++].p;
        return PP_OK;
    }
};

enum : int { RG_INTERN = 0, RG_SORT = 1, RG_GATHER = 2 };

}  // namespace

extern "C" void pp_regrouped_free(pp_regrouped *g) {
    if (!g) return;
    if (g->ctx) (void)hipSetDevice(g->ctx->device);
    for (void *q : g->d)
        if (q) (void)hipFree(q);
    delete g;
}

extern "C" void pp_regrouped_raw(const pp_regrouped *g, pp_raw_batch *out) {
    if (out) *out = g ? g->view : pp_raw_batch{};
}

extern "C" const uint32_t *pp_regrouped_perm(const pp_regrouped *g) { return g ? (const uint32_t *)g->d[11] : nullptr; }

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
    if (!g || !ms) return PP_ERR_ARG;
    if (!g->timed) return g->ctx->fail(PP_ERR_ARG, "pp_regrouped_kernel_ms: the context had no profiling on when the batch was regrouped (pp_ctx_set_profiling)");
    *ms = g->ms[0] + g->ms[1] + g->ms[2];
    return PP_OK;
}

// (internal hooks, not part of the header: tools/regroup_timing.py, tests/test_regroup_gpu.py) the same time by stage: intern | sort |
// gather; and the sort's tile, so that the tests can place their sizes around it
extern "C" int pp_regrouped_stage_ms_(const pp_regrouped *g, float *ms3) {
    if (!g || !ms3 || !g->timed) return PP_ERR_ARG;
    for (int i = 0; i < 3; i++) ms3[i] = g->ms[i];
    return PP_OK;
}
extern "C" void pp_regroup_geometry_(uint32_t *tile) {
    if (tile) *tile = RG_TILE;
}

extern "C" int pp_batch_regroup(pp_ctx *ctx, const pp_raw_batch *raw, int mem, pp_regrouped **out) {
    if (!ctx) return PP_ERR_ARG;
    if (int rdy = pp_ctx_wait(ctx)) return rdy;
    if (!raw || !out) return ctx->fail(PP_ERR_ARG, "pp_batch_regroup: null argument");
    *out = nullptr;
    if (mem != PP_MEM_HOST && mem != PP_MEM_DEVICE)
        return ctx->fail(PP_ERR_ARG, "pp_batch_regroup: the batch must be host memory or memory of the context's device");
    if (raw->n_rec >= 0xFFFFFFFFull) return ctx->fail(PP_ERR_LIMIT, "more than 2^32-1 alignments in one batch");
    const void *src[9] = {raw->flag, raw->read_id, raw->contig, raw->ref_start, raw->nm, raw->seq_off, raw->seq_len, raw->cig_off, raw->n_cig};
    if (raw->n_rec)
        for (const void *q : src)
            if (!q) return ctx->fail(PP_ERR_ARG, "pp_batch_regroup: null array in a non-empty batch");
    if (mem == PP_MEM_HOST && ((raw->seq_bytes && !raw->seq) || (raw->n_cig_total && !raw->cigar)))
        return ctx->fail(PP_ERR_ARG, "pp_batch_regroup: null array in a non-empty batch");
    PP_HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const u32 n = (u32)raw->n_rec;

    pp_regrouped *P = new pp_regrouped;
    P->ctx = ctx;
    std::unique_ptr<pp_regrouped, void (*)(pp_regrouped *)> guard(P, pp_regrouped_free);  // (every early return releases what was made so far)
    P->view = *raw;
    int rc;
    // ---- the source on the device: a host batch is uploaded into memory of the object ----
    if (mem == PP_MEM_HOST) {
        P->view = pp_raw_batch{};
        P->view.n_rec = n;
        P->view.seq_bytes = raw->seq_bytes;
        P->view.n_cig_total = raw->n_cig_total;
        const void *from[11] = {src[0], src[1], src[2], src[3], src[4], src[5], src[6], src[7], src[8], raw->seq, raw->cigar};
        size_t bytes[11];
        for (int a = 0; a < 9; a++) bytes[a] = (size_t)n * RG_SIZE[a];
        bytes[9] = (size_t)raw->seq_bytes;
        bytes[10] = (size_t)raw->n_cig_total * 4;
        for (int a = 0; a < 11; a++) {
            PP_HIPCHK(ctx, hipMalloc(&P->d[a], bytes[a] ? bytes[a] : 16));
            if (bytes[a]) PP_HIPCHK(ctx, hipMemcpyAsync(P->d[a], from[a], bytes[a], hipMemcpyHostToDevice, st));
            if (a < 9) src[a] = P->d[a];
        }
        pp_raw_batch &V = P->view;
        V.flag = (const uint16_t *)P->d[0]; V.read_id = (const uint64_t *)P->d[1]; V.contig = (const u32 *)P->d[2];
        V.ref_start = (const u32 *)P->d[3]; V.nm = (const u32 *)P->d[4]; V.seq_off = (const uint64_t *)P->d[5];
        V.seq_len = (const u32 *)P->d[6]; V.cig_off = (const uint64_t *)P->d[7]; V.n_cig = (const u32 *)P->d[8];
        V.seq = (const u8 *)P->d[9]; V.cigar = (const u32 *)P->d[10];
    }
    if (n == 0) {
        PP_HIPCHK(ctx, hipMalloc(&P->d[11], 16));
        PP_HIPCHK(ctx, hipStreamSynchronize(st));
        guard.release();
        *out = P;
        return PP_OK;
    }
    const uint16_t *const d_flag = (const uint16_t *)src[0];
    const u64 *const d_id = (const u64 *)src[1];

    Scratch T{ctx};
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
    PP_HIPCHK(ctx, hipMalloc(&P->d[11], (size_t)n * 4));
    u32 *const d_perm = (u32 *)P->d[11];
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
            hipLaunchKernelGGL(k_rg_hist, dim3(n_tiles), dim3(RG_BLOCK), 0, st, n, key_in, 8u * p, n_tiles, (u32 *)d_cnt);
            if ((rc = scan_u32<u32>(ctx, T.sums(), T.sums_off(), (const u32 *)d_cnt, n_cnt, (u32 *)d_off))) return rc;
            hipLaunchKernelGGL(k_rg_scatter, dim3(n_tiles), dim3(RG_BLOCK), 0, st, n, key_in, idx_in, 8u * p, n_tiles, (const u32 *)d_off, key_out, idx_out);
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
        RgArrays A{};
        void *fresh[9] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        struct Drop {  // (the arrays the gather fills belong to the object only once it holds them)
            void **p;
            ~Drop() { for (int a = 0; a < 9; a++) if (p[a]) (void)hipFree(p[a]); }
        } drop{fresh};
        for (int a = 0; a < 9; a++) {
            PP_HIPCHK(ctx, hipMalloc(&fresh[a], (size_t)n * RG_SIZE[a]));
            A.in[a] = src[a];
            A.out[a] = fresh[a];
        }
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
        for (int a = 0; a < 9; a++) {  // (an uploaded source array has been read: it gives way)
            if (P->d[a]) (void)hipFree(P->d[a]);
            P->d[a] = fresh[a];
            fresh[a] = nullptr;
        }
        pp_raw_batch &V = P->view;
        V.flag = (const uint16_t *)P->d[0]; V.read_id = (const uint64_t *)P->d[1]; V.contig = (const u32 *)P->d[2];
        V.ref_start = (const u32 *)P->d[3]; V.nm = (const u32 *)P->d[4]; V.seq_off = (const uint64_t *)P->d[5];
        V.seq_len = (const u32 *)P->d[6]; V.cig_off = (const uint64_t *)P->d[7]; V.n_cig = (const u32 *)P->d[8];
    }
    PP_HIPCHK(ctx, hipStreamSynchronize(st));
    if (timer.on) {
        if ((rc = timer.sums(P->ms, 3))) return rc;
        P->timed = true;
    }
    guard.release();
    *out = P;
    return PP_OK;
}

extern "C" int pp_ctx_set_regroup(pp_ctx *ctx, int on) {
    if (!ctx) return PP_ERR_ARG;
    ctx->regroup = on != 0;
    return PP_OK;
}

// (internal, the file drivers: pp_driver.cpp, pp_driver_bam.cpp)
extern "C" int pp_ctx_regroup_(const pp_ctx *ctx) { return ctx && ctx->regroup ? 1 : 0; }
