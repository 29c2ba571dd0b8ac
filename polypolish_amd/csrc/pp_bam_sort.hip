// pp_bam_sort.hip -- pp_bam_sort: the coordinate order of BAM records, on the device.  The link in front of pp_bam_tagged_head for a
// caller who wants the filtered file sorted: from the uncompressed BAM bytes and the records' offsets it makes perm (output record j is
// input record perm[j]), the offsets in that order, and on the host the header that says SO:coordinate (pp_bam_sort_host.h).
//
// The key of a record is 64 bits: high word ref_id, or 0xFFFFFFFF for ref_id == -1 (unplaced records come last); low word
// (uint32)(pos + 1) << 1 | reverse strand.  perm is the STABLE order by that key: reference, position, strand, input order.
//   k_bs_key      one lane per record: the record's range (pp_bam_host::step_kind: the walk's own verdict, nothing read through an
//                 offset before it is checked, no sum that could wrap), then ref_id, pos and flag from the 32 bytes of the fixed part,
//                 four bytes at a time at any alignment.  A defect is status[0] = record << 8 | kind by atomicMin: the first record in
//                 index order wins.  The OR and the AND of all keys (LDS, then one atomic per workgroup) tell which of the eight bytes
//                 differ between any two keys: a byte in which all agree needs no pass
//   k_rg_hist     (pp_rg_sort.h) one least-significant-digit pass per differing byte, stable and without atomics in the ranks: two
//   k_rg_scatter  calls give identical bytes
//   k_bs_gather   rec_off through perm, and the records that changed place
//   k_rg_aligned  (pp_rg_sort.h) the aligned-rank map behind pp_bam_sorted_pass, as pp_regrouped_pass has it
//   k_rg_map
// No byte outside [0, n_bytes) is loaded: a record's fields are read only once its 4 + block_size >= 36 bytes were found inside the array.
#include "pp_bam_sort_host.h"
#include "pp_rg_sort.h"

#include <cstring>

extern "C" char *pp_bam_msg_buf_(size_t *cap);  // pp_bam.hip: the per-thread message behind pp_bam_last_error()

struct pp_bam_sorted : DevOwner {  // owns perm and the offsets in its order
    using DevOwner::DevOwner;
    u32 *perm = nullptr;
    u64 *rec_off = nullptr;
    std::vector<uint8_t> head;   // HOST: the rewritten header
    uint64_t n_rec = 0, n_moved = 0, n_unplaced = 0, n_aligned = 0;
    std::vector<uint32_t> amap;  // aligned rank in sorted order -> aligned rank in input order (empty: the identity)
    StageMs<3> t;                // keys | sort | gather, counts and the verdict map
};

namespace {

enum : u32 { BS_POS = 8, BS_REF = 9 };  // behind pp_bam_host's W_*: pos < -1; ref_id < -1 or >= n_ref
enum : int { BS_KEYS = 0, BS_SORT = 1, BS_GATHER = 2 };

__device__ __forceinline__ u32 ld32(const u8 *__restrict__ p, u64 at) {  // four bytes at any alignment, inside a checked range
    u32 w;
    __builtin_memcpy(&w, p + at, 4);
    return w;
}

// status: [0] the first defect, [1] the OR of all keys, [2] their AND, [3] the records with ref_id == -1
__global__ __launch_bounds__(256) void k_bs_key(u32 n_rec, const u8 *__restrict__ B, u64 N, const u64 *__restrict__ rec_off, u32 n_ref,
                                                u64 *__restrict__ key, uint16_t *__restrict__ flag, u64 *__restrict__ status) {
    __shared__ u64 s_or, s_and;
    __shared__ u32 s_un;
    if (threadIdx.x == 0) { s_or = 0; s_and = ~0ull; s_un = 0; }
    __syncthreads();
    const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
    if (r < n_rec) {
        const u64 o = rec_off[r];
        const u64 left = o <= N ? N - o : 0;  // (an offset behind the array: the walk's "ends inside the block_size word")
        const u32 bs = left >= 4 ? ld32(B, o) : 0u;
        u32 kind = pp_bam_host::step_kind(left, bs);
        u64 k = 0;
        u32 f = 0;
        if (!kind) {  // the 36 bytes from o on lie inside the array
            const int32_t ref = (int32_t)ld32(B, o + 4u), pos = (int32_t)ld32(B, o + 8u);
            f = (u32)B[o + 18u] | (u32)B[o + 19u] << 8;
            if (pos < -1) kind = BS_POS;
            else if (ref < -1 || (ref >= 0 && (u32)ref >= n_ref)) kind = BS_REF;
            else {
                k = (u64)(ref >= 0 ? (u32)ref : 0xFFFFFFFFu) << 32 | (u64)((((u32)pos + 1u) << 1) | ((f >> 4) & 1u));
                atomicOr(&s_or, k);
                atomicAnd(&s_and, k);
                if (ref < 0) atomicAdd(&s_un, 1u);
            }
        }
        if (kind) report(status, (r << 8) | kind);
        key[r] = k;
        flag[r] = (uint16_t)f;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicOr(status + 1, s_or);
        atomicAnd(status + 2, s_and);
        if (s_un) atomicAdd(status + 3, (u64)s_un);
    }
}

// out[j] = rec_off[perm[j]]; *moved += the places j with perm[j] != j (a ballot and one atomic per wave)
__global__ __launch_bounds__(256) void k_bs_gather(u32 n, const u32 *__restrict__ perm, const u64 *__restrict__ rec_off, u64 *__restrict__ out,
                                                   u64 *__restrict__ moved) {
    const u64 j = (u64)blockIdx.x * 256u + threadIdx.x;
    u32 p = (u32)j;
    if (j < n) {
        p = perm[j];
        out[j] = rec_off[p];
    }
    const u64 m = __ballot(j < n && p != (u32)j);
    if ((threadIdx.x & 63u) == 0 && m) atomicAdd(moved, (u64)__popcll(m));
}

}  // namespace

extern "C" void pp_bam_sorted_free(pp_bam_sorted *s) { delete s; }

extern "C" const uint32_t *pp_bam_sorted_perm(const pp_bam_sorted *s) { return s ? s->perm : nullptr; }

extern "C" const uint64_t *pp_bam_sorted_rec_off(const pp_bam_sorted *s) { return s ? (const uint64_t *)s->rec_off : nullptr; }

extern "C" void pp_bam_sorted_head(const pp_bam_sorted *s, const uint8_t **head, uint64_t *n_head) {
    if (head) *head = s && !s->head.empty() ? s->head.data() : nullptr;
    if (n_head) *n_head = s ? s->head.size() : 0;
}

extern "C" void pp_bam_sorted_counts(const pp_bam_sorted *s, uint64_t *n_moved, uint64_t *n_unplaced) {
    if (n_moved) *n_moved = s ? s->n_moved : 0;
    if (n_unplaced) *n_unplaced = s ? s->n_unplaced : 0;
}

extern "C" int pp_bam_sorted_pass(const pp_bam_sorted *s, const uint8_t *pass, uint64_t n_pass, uint8_t *out) {
    if (!s) return PP_ERR_ARG;
    if (n_pass != s->n_aligned)
        return s->ctx->fail(PP_ERR_ARG, "pp_bam_sorted_pass: %llu filter verdicts for %llu aligned records", (unsigned long long)n_pass,
                            (unsigned long long)s->n_aligned);
    if (n_pass && (!pass || !out)) return s->ctx->fail(PP_ERR_ARG, "pp_bam_sorted_pass: null argument");
    if (s->amap.empty()) {
        if (n_pass && out != pass) memmove(out, pass, (size_t)n_pass);
        return PP_OK;
    }
    for (uint64_t a = 0; a < n_pass; a++) out[a] = pass[s->amap[a]];
    return PP_OK;
}

extern "C" int pp_bam_sorted_kernel_ms(const pp_bam_sorted *s, float *ms) {
    return s ? s->t.total(s->ctx, "pp_bam_sorted_kernel_ms", "when the records were sorted", ms) : PP_ERR_ARG;
}

// (internal hook, not part of the header: tools/bam_sort_timing.py) the same time by stage: keys | sort | gather.  The sort's tile is
// pp_regroup_geometry_'s.
extern "C" int pp_bam_sorted_stage_ms_(const pp_bam_sorted *s, float *ms3) { return s ? s->t.stages(ms3) : PP_ERR_ARG; }

extern "C" int pp_bam_sort(pp_ctx *ctx, const uint8_t *bytes, uint64_t n_bytes, uint64_t records_at, const uint64_t *rec_off, uint64_t n_rec,
                           int mem, pp_bam_sorted **out, uint64_t *bad_record) {
    if (!ctx) return PP_ERR_ARG;
    if (int rdy = pp_ctx_wait(ctx)) return rdy;
    if (bad_record) *bad_record = ~0ull;
    if (!out) return ctx->fail(PP_ERR_ARG, "pp_bam_sort: null argument");
    *out = nullptr;
    if (mem != PP_MEM_HOST && mem != PP_MEM_DEVICE)
        return ctx->fail(PP_ERR_ARG, "pp_bam_sort: the bytes must be host memory or memory of the context's device");
    if ((n_bytes && !bytes) || (n_rec && !rec_off)) return ctx->fail(PP_ERR_ARG, "pp_bam_sort: null bytes with n_bytes > 0, or null rec_off with n_rec > 0");
    if (records_at > n_bytes) return ctx->fail(PP_ERR_ARG, "pp_bam_sort: records_at %llu lies behind the %llu bytes", (unsigned long long)records_at, (unsigned long long)n_bytes);
    if (n_rec >= 0xFFFFFFFFull) return ctx->fail(PP_ERR_LIMIT, "more than 2^32-1 alignments in one batch");
    if (n_bytes >= (1ull << 40)) return ctx->fail(PP_ERR_LIMIT, "pp_bam_sort: 2^40 or more bytes in one call");
    PP_HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const u32 n = (u32)n_rec;
    int rc;

    std::unique_ptr<pp_bam_sorted> P(new pp_bam_sorted(ctx));
    P->n_rec = n_rec;
    // ---- the header: on the host, from bytes[0, records_at) ----
    u32 n_ref = 0;
    {
        std::vector<u8> fetched;  // ... downloaded, where the bytes are the device's
        const u8 *h_bytes = (const u8 *)bytes;
        if (mem == PP_MEM_DEVICE) {
            try {
                fetched.resize((size_t)records_at);
            } catch (const std::bad_alloc &) {
                return ctx->fail(PP_ERR_LIMIT, "pp_bam_sort: no host memory for a header of %llu bytes", (unsigned long long)records_at);
            }
            if (records_at && (rc = fetch(ctx, bytes, fetched.data(), (size_t)records_at))) return rc;
            h_bytes = fetched.data();
        }
        size_t cap = 0;
        char *msg = pp_bam_msg_buf_(&cap);
        if (cap) msg[0] = 0;
        if ((rc = pp_bam_sort_host::head_sorted(h_bytes, records_at, &P->head, &n_ref, msg, cap))) return ctx->fail(rc, "%s", msg);
    }
    if ((rc = P->alloc(P->perm, n)) || (rc = P->alloc(P->rec_off, n))) return rc;
    if (n == 0) {
        PP_HIPCHK(ctx, hipStreamSynchronize(st));
        *out = P.release();
        return PP_OK;
    }

    CallScratch U;  // the copy of host bytes and offsets: released when the call returns
    CtxScratch T(ctx, ctx->g_rec, "pp_bam_sort");
    StageTimer timer(ctx, ctx->profiling != 0);
    const u8 *d_bytes = nullptr;
    const u64 *d_rec_off = nullptr;
    if ((rc = on_device(ctx, U, mem, (const u8 *)bytes, (size_t)n_bytes, &d_bytes)) || (rc = on_device(ctx, U, mem, (const u64 *)rec_off, (size_t)n, &d_rec_off)))
        return rc;
    const unsigned gb = (unsigned)(((u64)n + 255u) / 256u);
    const u32 n_tiles = (u32)(((u64)n + RG_TILE - 1u) / RG_TILE);
    const u64 n_cnt = 256ull * n_tiles;

    // ---- the keys, the flags, the first defect ----
    void *d_key[2], *d_flag, *d_status;
    if ((rc = T.get(ctx, &d_key[0], (size_t)n * 8)) || (rc = T.get(ctx, &d_key[1], (size_t)n * 8)) || (rc = T.get(ctx, &d_flag, (size_t)n * 2)) ||
        (rc = T.get(ctx, &d_status, 32)))
        return rc;
    const u64 status0[4] = {~0ull, 0ull, ~0ull, 0ull};
    PP_HIPCHK(ctx, hipMemcpyAsync(d_status, status0, sizeof status0, hipMemcpyHostToDevice, st));
    if ((rc = timer.begin(BS_KEYS))) return rc;
    hipLaunchKernelGGL(k_bs_key, dim3(gb), dim3(256), 0, st, n, d_bytes, (u64)n_bytes, d_rec_off, n_ref, (u64 *)d_key[0], (uint16_t *)d_flag, (u64 *)d_status);
    if ((rc = timer.end())) return rc;
    PP_HIPCHK(ctx, hipGetLastError());
    u64 status[4] = {~0ull, 0, 0, 0};
    if ((rc = fetch(ctx, d_status, status, 4))) return rc;
    if (status[0] != ~0ull) {
        const u64 r = status[0] >> 8;
        const u32 kind = (u32)(status[0] & 0xFFu);
        if (bad_record) *bad_record = r;
        return ctx->fail(PP_ERR_ARG, "pp_bam_sort: record %llu %s", (unsigned long long)r,
                         kind == pp_bam_host::W_CUT ? "has an offset outside the bytes, or the bytes end inside its block_size"
                         : kind == pp_bam_host::W_SMALL ? "has a block_size below the 32 bytes of its fixed part"
                         : kind == pp_bam_host::W_PAST ? "runs past the end of the bytes"
                         : kind == BS_POS ? "has a position below -1" : "has a reference id that the header does not have");
    }
    P->n_unplaced = status[3];

    // ---- perm: the indices sorted by key, stable; a pass per byte in which two keys differ ----
    u32 shifts[8], passes = 0;
    for (u32 b = 0; b < 8u; b++)
        if (((status[1] ^ status[2]) >> (8u * b)) & 0xFFull) shifts[passes++] = 8u * b;
    u32 *const d_perm = P->perm;
    void *d_idx = nullptr, *d_cnt = nullptr, *d_off = nullptr;
    if (passes && ((rc = T.get(ctx, &d_cnt, (size_t)n_cnt * 4)) || (rc = T.get(ctx, &d_off, (size_t)(n_cnt + 1) * 4)) || (rc = T.get(ctx, &d_idx, (size_t)n * 4))))
        return rc;
    if ((rc = timer.begin(BS_SORT))) return rc;
    if (!passes) hipLaunchKernelGGL(k_rg_iota, dim3(gb), dim3(256), 0, st, n, d_perm);
    {
        // the indices go to and fro between the scratch and perm, so that the last pass writes perm
        const u32 *idx_in = nullptr;
        for (u32 p = 0; p < passes; p++) {
            const bool to_perm = ((passes - 1u - p) & 1u) == 0;
            const u64 *const key_in = (const u64 *)d_key[p & 1u];
            u64 *const key_out = (u64 *)d_key[(p + 1u) & 1u];
            u32 *const idx_out = to_perm ? d_perm : (u32 *)d_idx;
            hipLaunchKernelGGL(k_rg_hist<u64>, dim3(n_tiles), dim3(RG_BLOCK), 0, st, n, key_in, shifts[p], n_tiles, (u32 *)d_cnt);
            if ((rc = scan_u32<u32>(ctx, T.sums(), T.sums_off(), (const u32 *)d_cnt, n_cnt, (u32 *)d_off))) return rc;
            hipLaunchKernelGGL(k_rg_scatter<u64>, dim3(n_tiles), dim3(RG_BLOCK), 0, st, n, key_in, idx_in, shifts[p], n_tiles, (const u32 *)d_off, key_out, idx_out);
            idx_in = idx_out;
        }
    }
    if ((rc = timer.end())) return rc;
    PP_HIPCHK(ctx, hipGetLastError());

    // ---- the offsets in that order, the moved records, the aligned records ----
    void *d_moved, *d_aln, *d_rank_raw;
    if ((rc = T.get(ctx, &d_moved, 8)) || (rc = T.get(ctx, &d_aln, (size_t)n * 4)) || (rc = T.get(ctx, &d_rank_raw, ((size_t)n + 1) * 4))) return rc;
    if ((rc = timer.begin(BS_GATHER))) return rc;
    PP_HIPCHK(ctx, hipMemsetAsync(d_moved, 0, 8, st));
    hipLaunchKernelGGL(k_bs_gather, dim3(gb), dim3(256), 0, st, n, (const u32 *)d_perm, d_rec_off, P->rec_off, (u64 *)d_moved);
    hipLaunchKernelGGL(k_rg_aligned, dim3(gb), dim3(256), 0, st, n, (const uint16_t *)d_flag, (const u32 *)nullptr, (u32 *)d_aln);
    if ((rc = scan_u32<u32>(ctx, T.sums(), T.sums_off(), (const u32 *)d_aln, (u64)n, (u32 *)d_rank_raw))) return rc;
    if ((rc = timer.end())) return rc;
    PP_HIPCHK(ctx, hipGetLastError());
    u64 moved = 0;
    u32 n_al = 0;
    if ((rc = fetch(ctx, d_moved, &moved)) || (rc = fetch(ctx, (const u32 *)d_rank_raw + n, &n_al))) return rc;
    P->n_moved = moved;
    P->n_aligned = n_al;

    // ---- the verdict map, where a record moved ----
    if (moved && n_al) {
        void *d_rank_new, *d_amap;
        if ((rc = T.get(ctx, &d_rank_new, ((size_t)n + 1) * 4)) || (rc = T.get(ctx, &d_amap, (size_t)n_al * 4))) return rc;
        if ((rc = timer.begin(BS_GATHER))) return rc;
        hipLaunchKernelGGL(k_rg_aligned, dim3(gb), dim3(256), 0, st, n, (const uint16_t *)d_flag, (const u32 *)d_perm, (u32 *)d_aln);
        if ((rc = scan_u32<u32>(ctx, T.sums(), T.sums_off(), (const u32 *)d_aln, (u64)n, (u32 *)d_rank_new))) return rc;
        hipLaunchKernelGGL(k_rg_map, dim3(gb), dim3(256), 0, st, n, (const uint16_t *)d_flag, (const u32 *)d_perm, (const u32 *)d_rank_raw,
                           (const u32 *)d_rank_new, (u32 *)d_amap);
        if ((rc = timer.end())) return rc;
        PP_HIPCHK(ctx, hipGetLastError());
        P->amap.resize(n_al);
        if ((rc = fetch(ctx, d_amap, P->amap.data(), n_al))) return rc;
    }
    PP_HIPCHK(ctx, hipStreamSynchronize(st));  // host inputs may be released
    if ((rc = P->t.take(timer))) return rc;
    *out = P.release();
    return PP_OK;
}
