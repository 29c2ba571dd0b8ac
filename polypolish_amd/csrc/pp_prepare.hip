// pp_prepare.hip -- pp_batch_prepare: ANY valid pp_aln_batch laid out as the library's ingests lay theirs out, on the device.
//
// The direct path of the polish (pp_k_direct.h) wants a batch whose SEQ bytes sit in rooms of PP_SEQ_ALIGN bytes, window-grouped,
// with the 4-bit mirror of the seq array, the window-order mirror of the records and its run table.  The two SAM-text ingests
// write that layout from their parse records; a caller who holds alignments but no SAM text (a binding that parses SAM or BAM
// itself, anything that edits or filters records) had no way to it through the public ABI.  This is the third producer: it
// works from the nine arrays of a batch and from nothing else.
//   k_prep_home    per record: the window it starts in (wo_home, pp_wo_home.h: the rule k_prepd reads the mirror by) and its
//                  room in units of PP_SEQ_ALIGN bytes -- none for a record whose SEQ range lies outside the source array
//   k_prep_hist / k_prep_cols / k_prep_place
//                  the multisplit of the records into their windows without global atomics on hot addresses, after the
//                  tokenizer's k_tok_win_hist / _cols / _place: an LDS histogram of (records << 40 | units) per window and
//                  workgroup, a column scan over the workgroups, LDS cursors.  A record's entry of the mirror and its room
//                  come from ONE counter, so a window's rooms follow each other in the order of its entries.  Beyond
//                  PREP_WIN_LDS windows: one global counter per window (k_prep_count_g / k_prep_place_g) -- there are enough
//                  of them then.  k_prep_place has the record's fields in registers (coalesced reads, file order): it copies
//                  them to the output arrays and writes the record's 32-byte mirror entry.
//   k_prep_copy    the hot kernel, in MIRROR order: a workgroup's entries own one contiguous stretch of seq and seq4, its
//                  16-byte chunks are dealt to the lanes (a 150-base read is ten of them), each chunk is fetched from wherever
//                  the source has it (any alignment), zero-filled past the read, stored, and packed into the 4-bit mirror
//                  while it is in registers.
// One run covers the whole batch (wo_run_end = {n_aln}): inside a run only the windows have to ascend, and the kernels order a
// position's alignments by file index -- which the entries carry -- so a batch of two SAM files needs no runs of its own.
// Nothing is validated that the polish reports later: the call only has to be memory-safe, and a record it cannot read keeps
// a seq_off outside the prepared array, so that pp_polish_finish names it exactly as on the plain batch.
#include "pp_dev.h"
#include "pp_wo_home.h"

struct pp_prepared : DevOwner {
    using DevOwner::DevOwner;
    AlnArrays a;
    u8 *seq4 = nullptr;         // the 4-bit mirror of a.seq
    pp_wo_rec *wo = nullptr;    // the window-order mirror of the records
    uint64_t run_end = 0;       // the mirror's one run (pp_aln_batch.wo_run_end: HOST memory)
    pp_aln_batch view{};
    StageMs<1> t;
};

namespace {

constexpr u32 PREP_WIN_LDS = 8192;    // windows whose counters fit a workgroup's LDS (64 KiB); beyond: global counters
constexpr u32 PREP_PER_BLOCK = 8192;  // records per workgroup of k_prep_hist / k_prep_place (more when there would be > 1024 rows)
constexpr u32 PREP_COPY_E = 256;      // mirror entries per workgroup of k_prep_copy
constexpr u64 PREP_UNITS_MASK = (1ull << 40) - 1ull;
constexpr u64 PREP_NO_SRC = ~0ull;    // src_off of a record that gets no bytes
// why a batch cannot be laid out (flag word, set on the device: the placement then writes nothing)
constexpr u32 PREP_LIM_BYTES = 1u, PREP_LIM_WIN_RECORDS = 2u, PREP_LIM_WIN_BYTES = 4u;
constexpr u64 PREP_MAX_UNITS = (1ull << 40) / PP_SEQ_ALIGN;  // 2^40 SEQ bytes, in rooms' units
constexpr u64 PREP_MAX_WIN_RECORDS = 1ull << 24;

struct PrepSrc {  // the source batch (device memory)
    const u32 *contig, *ref_start, *k, *seq_len, *n_cig, *cigar;
    const u64 *seq_off, *cig_off;
    u64 seq_bytes, n_cig_total;
};
struct PrepOut {
    u32 *contig, *ref_start, *k, *seq_len, *n_cig;
    u64 *seq_off, *cig_off;
    pp_wo_rec *wo;
    u64 *src_off, *dst_pos;  // per mirror entry: where the source has the record's bytes (PREP_NO_SRC: nowhere) | where its room starts
};

__global__ __launch_bounds__(256) void k_prep_home(u32 n, const u32 *__restrict__ contig, const u32 *__restrict__ ref_start,
                                                   const u64 *__restrict__ seq_off, const u32 *__restrict__ seq_len,
                                                   const u64 *__restrict__ contig_off, u32 n_contigs, u32 n_win, u64 seq_bytes,
                                                   u32 *__restrict__ win, u32 *__restrict__ units, u64 *__restrict__ total) {
    __shared__ u64 s_sum;
    if (threadIdx.x == 0) s_sum = 0;
    __syncthreads();
    const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u64 u = 0;
    if (r < n) {
        const u32 c = contig[r];
        // (a contig index out of range has no home: with the last window)
        win[r] = c < n_contigs ? pp::wo_home(contig_off[c], ref_start[r], n_win) : n_win - 1u;
        const u32 sl = seq_len[r];
        if (inside(seq_off[r], sl, seq_bytes)) u = room_units(sl);
        units[r] = (u32)u;  // (<= 2^27)
    }
    for (int o = 32; o > 0; o >>= 1) u += (u64)__shfl_down((long long)u, o, 64);
    if ((threadIdx.x & 63u) == 0 && u) atomicAdd(&s_sum, u);
    __syncthreads();
    if (threadIdx.x == 0 && s_sum) atomicAdd(total, s_sum);
}

__global__ __launch_bounds__(1024) void k_prep_hist(const u32 *__restrict__ win, const u32 *__restrict__ units, u32 n, u32 per_block,
                                                    u32 n_win, u64 *__restrict__ mat) {
    __shared__ u64 hist[PREP_WIN_LDS];
    for (u32 w = threadIdx.x; w < n_win; w += 1024u) hist[w] = 0;
    __syncthreads();
    const u64 lo = (u64)blockIdx.x * per_block, hi = min((u64)n, lo + per_block);
    for (u64 r = lo + threadIdx.x; r < hi; r += 1024u) atomicAdd(&hist[win[r]], (1ull << 40) | (u64)units[r]);
    __syncthreads();
    for (u32 w = threadIdx.x; w < n_win; w += 1024u) mat[(u64)blockIdx.x * n_win + w] = hist[w];
}

// the limits of one window, and of the batch (the sums of a batch beyond them are not to be trusted: nothing is placed then)
__device__ __forceinline__ void prep_limits(u64 records, u64 win_units, const u64 *total, u32 *flag) {
    const u32 f = (*total >= PREP_MAX_UNITS ? PREP_LIM_BYTES : 0u) | (records >= PREP_MAX_WIN_RECORDS ? PREP_LIM_WIN_RECORDS : 0u) |
                  (win_units > 0xFFFFFFFFull ? PREP_LIM_WIN_BYTES : 0u);
    if (f) atomicOr(flag, f);
}

// one wave per window: exclusive scan of its column over the workgroups (in place), the totals to wunits / wcount
__global__ __launch_bounds__(256) void k_prep_cols(u32 n_win, u32 n_blocks, u64 *__restrict__ mat, u32 *__restrict__ wunits,
                                                   u32 *__restrict__ wcount, const u64 *__restrict__ total, u32 *__restrict__ flag) {
    const u32 w = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (w >= n_win) return;
    u64 carry = 0, recs = 0, uts = 0;  // (recs / uts: this lane's share of the column, added up apart -- the packed sum may wrap)
    for (u32 b0 = 0; b0 < n_blocks; b0 += 64u) {
        const u32 b = b0 + lane;
        const u64 v = b < n_blocks ? mat[(u64)b * n_win + w] : 0ull;
        recs += v >> 40;
        uts += v & PREP_UNITS_MASK;
        u64 inc = v;
        for (int o = 1; o < 64; o <<= 1) {
            const u64 t = (u64)__shfl_up((long long)inc, o, 64);
            if ((int)lane >= o) inc += t;
        }
        if (b < n_blocks) mat[(u64)b * n_win + w] = carry + inc - v;
        carry += (u64)__shfl((long long)inc, 63, 64);
    }
    for (int o = 32; o > 0; o >>= 1) {
        recs += (u64)__shfl_down((long long)recs, o, 64);
        uts += (u64)__shfl_down((long long)uts, o, 64);
    }
    if (lane == 0) {
        prep_limits(recs, uts, total, flag);
        wunits[w] = (u32)uts;
        wcount[w] = (u32)recs;
    }
}

// more windows than LDS holds: global counters per window (the records of a window apart from its units: no field can run over)
__global__ __launch_bounds__(256) void k_prep_count_g(const u32 *__restrict__ win, const u32 *__restrict__ units, u32 n,
                                                      u64 *__restrict__ wunits64, u32 *__restrict__ wcount) {
    const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const u32 w = win[r];
    atomicAdd(&wcount[w], 1u);
    if (units[r]) atomicAdd(&wunits64[w], (u64)units[r]);
}
// ... their limits; the counters become the cursors of k_prep_place_g (zeroed)
__global__ __launch_bounds__(256) void k_prep_split_g(u32 n_win, u64 *__restrict__ wunits64, u32 *__restrict__ wunits,
                                                      const u32 *__restrict__ wcount, const u64 *__restrict__ total, u32 *__restrict__ flag) {
    const u32 w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_win) return;
    const u64 uts = wunits64[w];
    prep_limits(wcount[w], uts, total, flag);
    wunits[w] = (u32)uts;
    wunits64[w] = 0;
}

// One record to its place: `old` = its window's counter before the record took its entry and its room (records << 40 | units).
// The fields go to the output arrays as they are, seq_off rewritten; the mirror entry as two 16-byte stores of one 32-byte line.
__device__ __forceinline__ void prep_place_one(u64 r, u32 w, u64 old, const u64 *__restrict__ wbase, const u32 *__restrict__ wcbase,
                                               const PrepSrc &S, const PrepOut &O) {
    const u64 slot = (u64)wcbase[w] + (old >> 40);
    const u64 pos = (wbase[w] + (old & PREP_UNITS_MASK)) * (u64)PP_SEQ_ALIGN;
    const u32 contig = S.contig[r], ref_start = S.ref_start[r], k = S.k[r], sl = S.seq_len[r], nc = S.n_cig[r];
    const u64 so = S.seq_off[r], co = S.cig_off[r];
    const bool readable = inside(so, sl, S.seq_bytes);
    // A record that cannot be read stays unreadable: beyond 2^40 where it was (the polish reports the overflow), else ending
    // exactly at 2^40 -- outside any prepared array, whatever is appended in front of it (it reports the range)
    const bool beyond = so > (1ull << 40) || so + sl > (1ull << 40);
    const u64 new_so = readable ? pos : (beyond ? so : (1ull << 40) - sl);
    const u32 op0 = (nc == 1u && co < S.n_cig_total) ? S.cigar[co] : (u32)PP_WO_MULTI_RUN;
    O.contig[r] = contig; O.ref_start[r] = ref_start; O.k[r] = k; O.seq_len[r] = sl; O.n_cig[r] = nc;
    O.seq_off[r] = new_so; O.cig_off[r] = co;
    uint4 *const e = (uint4 *)(O.wo + slot);
    e[0] = make_uint4(contig, ref_start, k, sl);
    e[1] = make_uint4((u32)new_so, (u32)(new_so >> 32), op0, (u32)r);
    O.src_off[slot] = (readable && sl) ? so : PREP_NO_SRC;
    O.dst_pos[slot] = pos;
}

__global__ __launch_bounds__(1024) void k_prep_place(const u32 *__restrict__ win, const u32 *__restrict__ units, u32 n, u32 per_block,
                                                     u32 n_win, const u64 *__restrict__ mat, const u64 *__restrict__ wbase,
                                                     const u32 *__restrict__ wcbase, const u32 *__restrict__ flag, PrepSrc S, PrepOut O) {
    __shared__ u64 cur[PREP_WIN_LDS];
    if (*flag) return;  // (uniform: a batch beyond the limits)
    for (u32 w = threadIdx.x; w < n_win; w += 1024u) cur[w] = mat[(u64)blockIdx.x * n_win + w];
    __syncthreads();
    const u64 lo = (u64)blockIdx.x * per_block, hi = min((u64)n, lo + per_block);
    for (u64 r = lo + threadIdx.x; r < hi; r += 1024u) {
        const u32 w = win[r];
        const u64 old = atomicAdd(&cur[w], (1ull << 40) | (u64)units[r]);
        prep_place_one(r, w, old, wbase, wcbase, S, O);
    }
}
__global__ __launch_bounds__(256) void k_prep_place_g(const u32 *__restrict__ win, const u32 *__restrict__ units, u32 n,
                                                      u64 *__restrict__ wcur, const u64 *__restrict__ wbase, const u32 *__restrict__ wcbase,
                                                      const u32 *__restrict__ flag, PrepSrc S, PrepOut O) {
    if (*flag) return;
    const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const u32 w = win[r];
    const u64 old = atomicAdd(&wcur[w], (1ull << 40) | (u64)units[r]);
    prep_place_one(r, w, old, wbase, wcbase, S, O);
}

// The SEQ bytes into their rooms, and their 4-bit mirror.  A workgroup takes PREP_COPY_E consecutive entries of the mirror:
// their rooms are one stretch [d0, d1) of the seq array (the rooms follow each other in mirror order; an entry without bytes
// has no room), dealt to the lanes in chunks of 16 bytes -- consecutive lanes store consecutive chunks.  A chunk's entry is
// found by bisection over the entries' starts in LDS.  A chunk past the read's end loads nothing; the last bytes of the source
// array are read byte by byte (a 16-byte load there would reach past seq_bytes).
__global__ __launch_bounds__(256) void k_prep_copy(u32 n, const pp_wo_rec *__restrict__ wo, const u64 *__restrict__ src_off,
                                                   const u64 *__restrict__ dst_pos, const u8 *__restrict__ src, u64 src_bytes,
                                                   u8 *__restrict__ seq, u8 *__restrict__ seq4) {
    __shared__ u64 s_dst[PREP_COPY_E + 1], s_src[PREP_COPY_E];
    __shared__ u32 s_len[PREP_COPY_E];
    const u64 e0 = (u64)blockIdx.x * PREP_COPY_E;
    const u32 cnt = (u32)min((u64)PREP_COPY_E, (u64)n - e0), t = threadIdx.x;
    if (t < cnt) {
        const u32 len = wo[e0 + t].seq_len;
        const u64 so = src_off[e0 + t], dp = dst_pos[e0 + t];
        s_len[t] = len; s_src[t] = so; s_dst[t] = dp;
        if (t == cnt - 1u) s_dst[cnt] = dp + (so == PREP_NO_SRC ? 0ull : room_bytes(len));
    }
    __syncthreads();
    const u64 d0 = s_dst[0], n_chunks = (s_dst[cnt] - d0) >> 4;
    for (u64 c = t; c < n_chunks; c += blockDim.x) {
        const u64 d = d0 + (c << 4);
        u32 lo = 0, hi = cnt;  // the last entry that starts at or in front of d (entries without a room start where the next one does)
        while (hi - lo > 1u) {
            const u32 mid = (lo + hi) >> 1;
            if (s_dst[mid] <= d) lo = mid; else hi = mid;
        }
        const u64 i = d - s_dst[lo];  // offset inside the room (a multiple of 16)
        const u32 len = s_len[lo];
        u32 w[4] = {0, 0, 0, 0};
        if (i < len && s_src[lo] != PREP_NO_SRC) {  // (masked lanes do not load)
            const u64 at = s_src[lo] + i;
            const u32 live = (u32)min((u64)16, (u64)len - i);  // bytes of this chunk that belong to the read (>= 1)
            if (at + 16u <= src_bytes) {
                uint4 v;
                __builtin_memcpy(&v, src + at, 16);  // (any alignment: one global_load_dwordx4)
                w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const u32 have = live > 4u * q ? min(4u, live - 4u * q) : 0u;
                    w[q] &= have == 4u ? 0xFFFFFFFFu : ((1u << (8u * have)) - 1u);
                }
            } else {
                for (u32 j = 0; j < live; j++) w[j >> 2] |= (u32)src[at + j] << (8u * (j & 3u));
            }
        }
        *(uint4 *)(seq + d) = make_uint4(w[0], w[1], w[2], w[3]);
        *(uint2 *)(seq4 + (d >> 1)) = pack4_16(w);
    }
}

}  // namespace

extern "C" void pp_prepared_free(pp_prepared *p) {
    if (p) pp_mirror_forget_(p);
    delete p;
}

extern "C" void pp_prepared_batch(const pp_prepared *p, pp_aln_batch *out) {
    if (!out) return;
    if (!p) { *out = pp_aln_batch{}; return; }
    *out = p->view;
}

extern "C" int pp_prepared_kernel_ms(const pp_prepared *p, float *ms) {
    return p ? p->t.total(p->ctx, "pp_prepared_kernel_ms", "when the batch was prepared", ms) : PP_ERR_ARG;
}

extern "C" int pp_batch_prepare(pp_ctx *ctx, uint32_t n_contigs, const uint64_t *contig_off, const pp_aln_batch *b, int mem,
                                pp_prepared **out) {
    if (!ctx) return PP_ERR_ARG;
    if (int rdy = pp_ctx_wait(ctx)) return rdy;
    if (!contig_off || !b || !out || n_contigs == 0) return ctx->fail(PP_ERR_ARG, "pp_batch_prepare: null argument or no contigs");
    *out = nullptr;
    if (mem != PP_MEM_HOST && mem != PP_MEM_DEVICE)
        return ctx->fail(PP_ERR_ARG, "pp_batch_prepare: the batch must be host memory or memory of the context's device");
    for (uint32_t c = 0; c < n_contigs; c++)
        if (contig_off[c + 1] < contig_off[c]) return ctx->fail(PP_ERR_ARG, "pp_batch_prepare: contig offsets decrease at contig %u", c);
    const u64 G = contig_off[n_contigs];
    if (G >= 0xFFFFFFFFull - 4096ull)
        return ctx->fail(PP_ERR_LIMIT, "assembly of %llu bp exceeds the 2^32-4096 bp limit of this version", (unsigned long long)G);
    if (b->n_aln >= 0xFFFFFFFFull) return ctx->fail(PP_ERR_LIMIT, "more than 2^32-1 alignments in one batch");
    if (b->seq_bytes >= (1ull << 40)) return ctx->fail(PP_ERR_LIMIT, "more than 2^40 SEQ bytes in one batch");
    if (b->n_aln && (!b->contig || !b->ref_start || !b->k || !b->seq_off || !b->seq_len || !b->cig_off || !b->n_cig || !b->seq || !b->cigar))
        return ctx->fail(PP_ERR_ARG, "pp_batch_prepare: null array in a non-empty batch");
    PP_HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const u32 n = (u32)b->n_aln;
    const u32 n_win = (u32)std::max<u64>(1, (G + pp::TILE - 1) / pp::TILE);

    std::unique_ptr<pp_prepared> P(new pp_prepared(ctx));
    AlnArrays &A = P->a;
    if (n == 0) {  // an empty batch prepares to an empty batch
        P->view = A.view(0, 0, b->n_cig_total);
        PP_HIPCHK(ctx, hipStreamSynchronize(st));
        *out = P.release();
        return PP_OK;
    }

    CallScratch T;
    StageTimer timer(ctx, ctx->profiling != 0);
    int rc;
    // ---- the source on the device ----
    pp_aln_batch D;
    if ((rc = aln_on_device(ctx, T, mem, b, &D))) return rc;
    const PrepSrc S{D.contig, D.ref_start, D.k, D.seq_len, D.n_cig, D.cigar, (const u64 *)D.seq_off, (const u64 *)D.cig_off, D.seq_bytes, D.n_cig_total};
    // ---- the result's arrays (seq and seq4 once their size is known) ----
    if ((rc = A.alloc_records(*P, n)) || (rc = P->alloc(A.cigar, (size_t)b->n_cig_total)) || (rc = P->alloc(P->wo, n))) return rc;
    if (b->n_cig_total) PP_HIPCHK(ctx, hipMemcpyAsync(A.cigar, S.cigar, (size_t)b->n_cig_total * 4, hipMemcpyDeviceToDevice, st));
    // ---- scratch ----
    const bool lds = n_win <= PREP_WIN_LDS;
    const u32 per_block = std::max<u32>(PREP_PER_BLOCK, (u32)((((u64)n + 1023u) / 1024u + 1023u) & ~1023ull));  // (at most 1024 rows)
    const u32 nb = (n + per_block - 1u) / per_block;
    void *d_cofs, *d_win, *d_units, *d_mat, *d_wunits, *d_wcount, *d_wbase, *d_wcbase, *d_src, *d_dst, *d_word;
    if ((rc = T.get(ctx, &d_cofs, ((size_t)n_contigs + 1) * 8)) || (rc = T.get(ctx, &d_win, (size_t)n * 4)) || (rc = T.get(ctx, &d_units, (size_t)n * 4)) ||
        (rc = T.get(ctx, &d_mat, (lds ? (size_t)nb : (size_t)1) * n_win * 8)) || (rc = T.get(ctx, &d_wunits, ((size_t)n_win + 1) * 4)) ||
        (rc = T.get(ctx, &d_wcount, ((size_t)n_win + 1) * 4)) || (rc = T.get(ctx, &d_wbase, ((size_t)n_win + 1) * 8)) ||
        (rc = T.get(ctx, &d_wcbase, ((size_t)n_win + 1) * 4)) || (rc = T.get(ctx, &d_src, (size_t)n * 8)) || (rc = T.get(ctx, &d_dst, (size_t)n * 8)) ||
        (rc = T.get(ctx, &d_word, 16)))
        return rc;
    u64 *const d_total = (u64 *)d_word;
    u32 *const d_flag = (u32 *)((u64 *)d_word + 1);
    PP_HIPCHK(ctx, hipMemcpyAsync(d_cofs, contig_off, ((size_t)n_contigs + 1) * 8, hipMemcpyHostToDevice, st));
    PP_HIPCHK(ctx, hipMemsetAsync(d_word, 0, 16, st));
    const PrepOut O{A.contig, A.ref_start, A.k, A.seq_len, A.n_cig, A.seq_off, A.cig_off, P->wo, (u64 *)d_src, (u64 *)d_dst};

    if ((rc = timer.begin(0))) return rc;
    // ---- placement ----
    const unsigned g256 = (unsigned)(((u64)n + 255u) / 256u);
    hipLaunchKernelGGL(k_prep_home, dim3(g256), dim3(256), 0, st, n, S.contig, S.ref_start, S.seq_off, S.seq_len, (const u64 *)d_cofs, n_contigs,
                       n_win, (u64)b->seq_bytes, (u32 *)d_win, (u32 *)d_units, d_total);
    if (lds) {
        hipLaunchKernelGGL(k_prep_hist, dim3(nb), dim3(1024), 0, st, (const u32 *)d_win, (const u32 *)d_units, n, per_block, n_win, (u64 *)d_mat);
        hipLaunchKernelGGL(k_prep_cols, dim3((n_win + 3u) / 4u), dim3(256), 0, st, n_win, nb, (u64 *)d_mat, (u32 *)d_wunits, (u32 *)d_wcount,
                           (const u64 *)d_total, d_flag);
    } else {
        PP_HIPCHK(ctx, hipMemsetAsync(d_mat, 0, (size_t)n_win * 8, st));
        PP_HIPCHK(ctx, hipMemsetAsync(d_wcount, 0, ((size_t)n_win + 1) * 4, st));
        hipLaunchKernelGGL(k_prep_count_g, dim3(g256), dim3(256), 0, st, (const u32 *)d_win, (const u32 *)d_units, n, (u64 *)d_mat, (u32 *)d_wcount);
        hipLaunchKernelGGL(k_prep_split_g, dim3((n_win + 255u) / 256u), dim3(256), 0, st, n_win, (u64 *)d_mat, (u32 *)d_wunits, (const u32 *)d_wcount,
                           (const u64 *)d_total, d_flag);
    }
    // (one workgroup each: a window's units are u32, their sum is kept in 64 bits)
    hipLaunchKernelGGL(k_tscan<u64>, dim3(1), dim3(1024), 0, st, (const u32 *)d_wunits, (u64)n_win, (u64 *)d_wbase);
    hipLaunchKernelGGL(k_tscan<u32>, dim3(1), dim3(1024), 0, st, (const u32 *)d_wcount, (u64)n_win, (u32 *)d_wcbase);
    if (lds)
        hipLaunchKernelGGL(k_prep_place, dim3(nb), dim3(1024), 0, st, (const u32 *)d_win, (const u32 *)d_units, n, per_block, n_win, (const u64 *)d_mat,
                           (const u64 *)d_wbase, (const u32 *)d_wcbase, (const u32 *)d_flag, S, O);
    else
        hipLaunchKernelGGL(k_prep_place_g, dim3(g256), dim3(256), 0, st, (const u32 *)d_win, (const u32 *)d_units, n, (u64 *)d_mat, (const u64 *)d_wbase,
                           (const u32 *)d_wcbase, (const u32 *)d_flag, S, O);
    if ((rc = timer.end())) return rc;
    struct { u64 units, flag; } got{0, 0};  // d_total | d_flag
    if ((rc = fetch(ctx, d_word, &got))) return rc;
    const u32 flag = (u32)got.flag;
    if (flag & PREP_LIM_BYTES) return ctx->fail(PP_ERR_LIMIT, "more than 2^40 SEQ bytes in one prepared batch");
    if (flag & PREP_LIM_WIN_RECORDS) return ctx->fail(PP_ERR_LIMIT, "more than 2^24 alignments start in one 2048-position window");
    if (flag & PREP_LIM_WIN_BYTES) return ctx->fail(PP_ERR_LIMIT, "more than 2^37 SEQ bytes start in one 2048-position window");
    // ---- the SEQ bytes and their 4-bit mirror ----
    const u64 total = got.units * (u64)PP_SEQ_ALIGN;  // a sum of rooms
    if ((rc = P->alloc(A.seq, (size_t)total + 64)) || (rc = P->alloc(P->seq4, (size_t)(total / 2) + 96))) return rc;
    PP_HIPCHK(ctx, hipMemsetAsync(A.seq + total, 0, 64, st));
    PP_HIPCHK(ctx, hipMemsetAsync(P->seq4 + total / 2, 0, 96, st));
    if ((rc = timer.begin(0))) return rc;
    if (total)
        hipLaunchKernelGGL(k_prep_copy, dim3((unsigned)(((u64)n + PREP_COPY_E - 1u) / PREP_COPY_E)), dim3(256), 0, st, n, (const pp_wo_rec *)P->wo,
                           (const u64 *)d_src, (const u64 *)d_dst, D.seq, (u64)b->seq_bytes, A.seq, P->seq4);
    if ((rc = timer.end())) return rc;
    PP_HIPCHK(ctx, hipGetLastError());
    PP_HIPCHK(ctx, hipStreamSynchronize(st));  // the source may be released, the scratch goes away
    if ((rc = P->t.take(timer))) return rc;
    pp_aln_batch &V = P->view = A.view(n, total, b->n_cig_total);
    V.seq4 = P->seq4;
    V.wo = P->wo;
    P->run_end = n;
    V.wo_n_runs = 1;
    V.wo_run_end = &P->run_end;
    pp_mirror_register_(P.get(), V.wo, (size_t)n * sizeof(pp_wo_rec));  // one of the library's own: pp_polish_add takes it unchecked
    *out = P.release();
    return PP_OK;
}
