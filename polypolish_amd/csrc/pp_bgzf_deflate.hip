// pp_bgzf_deflate.hip -- pp_bgzf_deflate, pp_bam_out_deflate: bytes in device memory compressed into BGZF blocks, on the device.  The
// compressor of the record chain: what pp_bam_tagged frames as level-0 BGZF leaves here at about a fifth of the size.  The bytes are cut
// every 65,280; each piece becomes one BGZF block around ONE DEFLATE block (BFINAL = 1).  tests/bgzf_deflate_model.py defines the
// bytes: every rule is a function of the piece's bytes alone, never of the order in which lanes, waves or atomics run (the LDS atomics
// below are max and add over integers: the same result in any order).  The format's rules and the serial steps are in pp_bgzf_host.h,
// shared with the host twin deflate_block(); this file is the parallel part around them.
//   k_df_piece    ONE WORKGROUP OF 256 LANES PER PIECE (a grid of at most DF_GRID workgroups walks the pieces; a workgroup's tokens
//                 live in its own slot of scratch).  The piece stays in global memory (it is read a few times within microseconds:
//                 L2); LDS holds the hash table (32 KB: 2^13 entries of 32 bits, LDS has no 16-bit atomic max), one strip's matches,
//                 the histograms and the plan: 43 KB, three workgroups per CU.
//                   strips   lane t is position s0 + t: it reads T[h], the workgroup meets, every lane puts its position in with an
//                            atomic max, and the lanes whose position the parse can still reach (not below the carried next free
//                            position) compare at their candidate, eight bytes at a time, at most 258 bytes
//                   parse    wave 0, 64 positions at a time: the ballot of the lanes that hold a match gives the next match at or
//                            behind the cursor; the literals in front of it leave together, then the match, and the cursor skips its
//                            length.  At most one round per position (64 per window, DF_STRIP per strip); tokens and histograms are
//                            written as they are found
//                   plan     the used symbols are ranked by (count, symbol) by all lanes; lane 0 runs df_plan over LDS: the merges
//                            (at most 285 steps), the repair (fewer steps than symbols), the header's runs (at most 316 items of at
//                            most 138 lengths), the three costs, the choice, the codes
//                   bits     stored: the bytes are copied.  Otherwise the words of the stream are cleared, and the header's items
//                            and the tokens go out 256 at a time: the workgroup scan of their bit lengths (pp_dev.h) gives every
//                            item its place, an atomic OR per 32-bit word it touches puts it there (at most three)
//                   CRC32    every lane the byte table over its slice of the piece, the slices' values shifted to the piece's end
//                            (pp_crc.h) and XORed
//                 The block's stream goes to the piece's slot of a temporary array (65,344 bytes apart), its length, CRC32 and form
//                 to meta[].
//   k_colscan     (pp_dev.h) the blocks' sizes to their offsets: blk_off[], the EOF block's offset last
//   k_df_place    one workgroup per block: header with the real BSIZE, the stream, CRC32, ISIZE at the block's place, any alignment
// No cross-workgroup wait anywhere.  No byte outside the caller's [0, n_bytes) is loaded: a 4-byte load at i is issued only where
// i + 4 <= n, a compare of k bytes only where k <= n - i, and the candidate lies in front of i.
#include "pp_bgzf_host.h"
#include "pp_crc.h"
#include "pp_dev.h"
#include "pp_fasta_out_host.h"

#include <cstring>

struct pp_bgzf_out : DevOwner {
    using DevOwner::DevOwner;
    u8 *d_out = nullptr;       // DEVICE: the file
    u64 *d_blk_off = nullptr;  // DEVICE: n_blk + 1 offsets
    uint64_t n_out = 0, n_blk = 0;
    uint64_t counts[3] = {0, 0, 0};  // stored | fixed | dynamic
    StageMs<3> t;              // the pieces | the scan | the placing
};

namespace {

namespace hb = pp_bgzf_host;

constexpr u32 DF_BLOCK = hb::DF_STRIP;  // lanes per workgroup: one per position of a strip
constexpr u32 PAY = hb::STORE_PAYLOAD;
constexpr u32 SLOT = 65344;             // bytes between two pieces' streams in the temporary array: PAY + 5 and up to a multiple of 64
constexpr u32 DF_GRID = 1024;           // workgroups of k_df_piece, each with a token slot of PAY words
static_assert(DF_BLOCK == 256 && SLOT % 64 == 0 && SLOT >= PAY + 5 + 3, "the strip is the workgroup; a slot holds a stored stream, in whole words");

__device__ __forceinline__ u32 ld32(const u8 *__restrict__ p, u32 at) {  // four bytes at any alignment, inside a checked range
    u32 w;
    __builtin_memcpy(&w, p + at, 4);
    return w;
}

__device__ __forceinline__ u64 ld64(const u8 *__restrict__ p, u32 at) {
    u64 w;
    __builtin_memcpy(&w, p + at, 8);
    return w;
}

// v (nbits <= 48 of them, nothing above) into the stream at bit `at`: only words that get a set bit are touched
__device__ __forceinline__ void put_bits(u32 *words, u32 at, u64 v, u32 nbits) {
    (void)nbits;
    const u32 sh = at & 31u;
    u32 *const p = words + (at >> 5);
    const u64 lo = v << sh;
    const u32 hi = sh ? (u32)(v >> (64u - sh)) : 0u;
    if ((u32)lo) atomicOr(p, (u32)lo);
    if ((u32)(lo >> 32)) atomicOr(p + 1, (u32)(lo >> 32));
    if (hi) atomicOr(p + 2, hi);
}

// (not inlined: the serial part keeps its registers to itself)
__device__ __attribute__((noinline)) void plan_piece(hb::DfPlan *P, u32 n) { hb::df_plan(P, n); }

struct PieceArgs {
    const u8 *base;  // piece p's bytes start at base + p * stride + head
    u64 stride, head;
    u64 total;       // the bytes of all pieces
    u64 n_pieces;
    u32 *tok;        // gridDim.x slots of PAY tokens
    u8 *tmp;         // n_pieces slots of SLOT bytes
    uint4 *meta;     // per piece: the stream's bytes, CRC32, ISIZE, form
    u64 *size;       // per piece: the block's bytes
    u64 *counts;     // stored | fixed | dynamic
};

__global__ __launch_bounds__(DF_BLOCK, 3) void k_df_piece(PieceArgs A) {
    __shared__ u32 s_tab[1u << hb::DF_HB];  // position + 1 of the last 4-gram with this hash in the strips in front; 0: none
    __shared__ hb::DfPlan s_plan;
    __shared__ uint16_t s_len[DF_BLOCK], s_dist[DF_BLOCK];  // the strip's counted matches: length (0: none), distance - 1
    __shared__ u8 s_byte[DF_BLOCK];                         // ... and its bytes
    __shared__ u32 s_crc[256];
    __shared__ u32 s_w[DF_BLOCK / 64];
    __shared__ u32 s_next, s_ntok;
    const u32 t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    crc_table_fill(s_crc, t, DF_BLOCK);
    u32 *const tok = A.tok + (u64)blockIdx.x * PAY;
    for (u64 piece = blockIdx.x; piece < A.n_pieces; piece += gridDim.x) {
        const u8 *__restrict__ const src = A.base + piece * A.stride + A.head;
        const u32 n = (u32)min((u64)PAY, A.total - piece * (u64)PAY);
        for (u32 i = t; i < (1u << hb::DF_HB); i += DF_BLOCK) s_tab[i] = 0;
        for (u32 i = t; i < hb::DF_NSYM; i += DF_BLOCK) s_plan.hist[i] = 0;
        if (t == 0) { s_next = 0; s_plan.m_lit = 0; s_plan.m_dist = 0; }
        __syncthreads();

        // ---- the strips: candidates, matches, the parse ----
        u32 pos = 0, ntok = 0;  // (wave 0's) the next free position, the tokens so far
        for (u32 s0 = 0; s0 < n; s0 += DF_BLOCK) {
            const u32 i = s0 + t;
            const bool has = i < n && n - i >= 4u;
            u32 w = 0, h = 0, cand = 0;
            if (has) {
                w = ld32(src, i);
                h = hb::df_hash(w);
                cand = s_tab[h];
            } else if (i < n) w = src[i];
            const u32 next = s_next;
            __syncthreads();  // every lane has read the table as the strips in front left it
            if (has) atomicMax(&s_tab[h], i + 1u);
            u32 L = 0, D = 0;
            if (has && cand && i >= next && i - (cand - 1u) <= hb::DF_MAX_DIST) {
                const u32 c = cand - 1u, cap = min(hb::DF_MAX_MATCH, n - i);  // c < i: every load below ends at or in front of i + cap <= n
                D = i - c - 1u;
                if (ld32(src, c) == w) {
                    L = 4;
                    bool open = true;
                    while (open && L + 8u <= cap) {
                        const u64 x = ld64(src, c + L) ^ ld64(src, i + L);
                        if (x) { L += (u32)__builtin_ctzll(x) >> 3; open = false; }
                        else L += 8u;
                    }
                    while (open && L < cap) {
                        if (src[c + L] != src[i + L]) open = false;
                        else L++;
                    }
                }
            }
            s_len[t] = (uint16_t)L;  // (0 or >= 4)
            s_dist[t] = (uint16_t)D;
            s_byte[t] = (u8)w;
            __syncthreads();
            if (wave == 0) {
                for (u32 win = 0; win < DF_BLOCK / 64u; win++) {
                    const u32 base = s0 + 64u * win;
                    if (base >= n) break;
                    const u32 p = base + lane, lim = min(64u, n - base);
                    const u32 myL = p < n ? s_len[64u * win + lane] : 0u, myD = s_dist[64u * win + lane];
                    const u32 byte = s_byte[64u * win + lane];
                    const u64 m = __ballot(myL != 0);
                    u32 cur = pos > base ? pos - base : 0u;
                    while (cur < lim) {  // every round moves the cursor on
                        const u64 mm = m >> cur;
                        const u32 end = mm ? min(cur + (u32)__builtin_ctzll(mm), lim) : lim;
                        if (lane >= cur && lane < end) {  // the literals in front of the next match
                            tok[ntok + (lane - cur)] = byte;
                            atomicAdd(&s_plan.hist[byte], 1u);
                        }
                        ntok += end - cur;
                        cur = end;
                        if (cur < lim) {  // ... and the match
                            const u32 l = __shfl(myL, (int)cur, 64), d = __shfl(myD, (int)cur, 64);
                            if (lane == 0) {
                                tok[ntok] = hb::DF_MATCH | (l - 3u) << 16 | d;
                                atomicAdd(&s_plan.hist[257u + hb::df_len_sym(l)], 1u);
                                atomicAdd(&s_plan.hist[hb::DF_NLIT + hb::df_dist_sym(d + 1u)], 1u);
                            }
                            ntok++;
                            cur += l;
                        }
                    }
                    if (base + cur > pos) pos = base + cur;
                }
                if (lane == 0) s_next = pos;
            }
            __syncthreads();
        }
        if (t == 0) { s_ntok = ntok; s_plan.hist[256] = 1; }
        __syncthreads();

        // ---- the plan: the used symbols in (count, symbol) order by all lanes, the rest by lane 0 ----
        for (u32 s = t; s < hb::DF_NSYM; s += DF_BLOCK) {
            const u32 lo = s < hb::DF_NLIT ? 0u : hb::DF_NLIT, hi = s < hb::DF_NLIT ? hb::DF_NLIT : hb::DF_NSYM, c = s_plan.hist[s];
            if (!c) continue;
            u32 r = 0;
            for (u32 u = lo; u < hi; u++) {
                const u32 cu = s_plan.hist[u];
                r += (cu && (cu < c || (cu == c && u < s))) ? 1u : 0u;
            }
            s_plan.order[lo + r] = (uint16_t)(s - lo);
            atomicAdd(lo ? &s_plan.m_dist : &s_plan.m_lit, 1u);
        }
        __syncthreads();
        if (t == 0) plan_piece(&s_plan, n);
        __syncthreads();

        // ---- the stream ----
        const u32 type = s_plan.type, stream = (s_plan.bits + 7u) / 8u, n_tok = s_ntok;
        u8 *const slot = A.tmp + piece * (u64)SLOT;
        u32 *const words = (u32 *)slot;
        if (type == hb::DF_STORED) {
            for (u32 j = t; j < 5u + n; j += DF_BLOCK) slot[j] = j < 5u ? hb::store_head_byte(18u + j, n) : src[j - 5u];
        } else {
            for (u32 j = t; j < (stream + 3u) / 4u; j += DF_BLOCK) words[j] = 0;
            __threadfence();
            __syncthreads();
            if (t == 0) put_bits(words, 0, 1u | type << 1, 3);
            u32 at = 3;
            const u32 n_head = type == hb::DF_DYNAMIC ? hb::df_header_items(&s_plan) : 0u;
            for (u32 k0 = 0; k0 < n_head + n_tok; k0 += DF_BLOCK) {  // the header's items, then the tokens
                const u32 k = k0 + t;
                u32 nb = 0, total;
                u64 v = 0;
                if (k < n_head) v = hb::df_header_item(&s_plan, k, &nb);
                else if (k < n_head + n_tok) v = hb::df_token_bits(&s_plan, tok[k - n_head], &nb);
                const u32 ex = block_scan_excl<DF_BLOCK>(nb, s_w, &total);
                if (nb) put_bits(words, at + ex, v, nb);
                at += total;
            }
            if (t == 0) put_bits(words, at, s_plan.code[256], s_plan.clen[256]);
        }

        // ---- CRC32: lane t's slice, shifted by the bytes behind it ----
        const u32 per = (n + DF_BLOCK - 1u) / DF_BLOCK, lo = min(n, t * per), hi = min(n, lo + per);
        u32 c = 0;
        if (hi > lo) {
            c = 0xFFFFFFFFu;
            for (u32 i = lo; i < hi; i++) c = crc_byte(s_crc, c, src[i]);
            c = multmodp(x8n_modp(n - hi), ~c);
        }
        for (int o = 32; o > 0; o >>= 1) c ^= __shfl_xor(c, o, 64);
        if (lane == 0) s_w[wave] = c;
        __syncthreads();
        if (t == 0) {
            u32 crc = 0;
            for (u32 i = 0; i < DF_BLOCK / 64u; i++) crc ^= s_w[i];
            A.meta[piece] = make_uint4(stream, crc, n, type);
            A.size[piece] = 18ull + stream + 8ull;
            atomicAdd(A.counts + type, 1ull);
        }
        __syncthreads();  // (LDS is used again for the next piece)
    }
}

__global__ __launch_bounds__(DF_BLOCK) void k_df_place(const u8 *__restrict__ tmp, const uint4 *__restrict__ meta, const u64 *__restrict__ blk_off, u64 n_pieces,
                                                        u8 *__restrict__ out) {
    const u64 b = blockIdx.x;
    u8 *const dst = out + blk_off[b];
    if (b == n_pieces) {
        if (threadIdx.x < hb::EOF_SIZE) dst[threadIdx.x] = hb::eof_byte(threadIdx.x);
        return;
    }
    const uint4 m = meta[b];
    const u8 *__restrict__ const slot = tmp + b * (u64)SLOT;
    const u32 stream = m.x, total = 18u + stream + 8u;
    for (u32 j = threadIdx.x; j < total; j += DF_BLOCK) {
        u8 v;
        if (j < 18u) v = hb::head_byte(j, total);
        else if (j < 18u + stream) v = slot[j - 18u];
        else v = (u8)((j < 22u + stream ? m.y : m.z) >> (8u * ((j - 18u - stream) & 3u)));
        dst[j] = v;
    }
}

// the pieces at base + p * stride + head, `total` bytes in all, to an object
int deflate_pieces(pp_ctx *ctx, const u8 *base, u64 stride, u64 head, u64 total, pp_bgzf_out **out) {
    hipStream_t st = ctx->stream;
    std::unique_ptr<pp_bgzf_out> P(new pp_bgzf_out(ctx));
    CallScratch T;
    StageTimer timer(ctx, ctx->profiling != 0);
    int rc;
    const u64 n_pieces = (total + PAY - 1u) / PAY;
    const u32 grid = (u32)std::min<u64>(n_pieces, DF_GRID);
    void *d_tok, *d_tmp, *d_meta, *d_size, *d_counts;
    if ((rc = T.get(ctx, &d_tok, (size_t)grid * PAY * 4)) || (rc = T.get(ctx, &d_tmp, (size_t)n_pieces * SLOT)) || (rc = T.get(ctx, &d_meta, (size_t)n_pieces * 16)) ||
        (rc = T.get(ctx, &d_size, (size_t)n_pieces * 8)) || (rc = T.get(ctx, &d_counts, 24)))
        return rc;
    if ((rc = P->alloc(P->d_blk_off, (size_t)n_pieces + 1))) return rc;
    PP_HIPCHK(ctx, hipMemsetAsync(d_counts, 0, 24, st));
    if ((rc = timer.begin(0))) return rc;
    if (n_pieces)
        hipLaunchKernelGGL(k_df_piece, dim3(grid), dim3(DF_BLOCK), 0, st,
                           PieceArgs{base, stride, head, total, n_pieces, (u32 *)d_tok, (u8 *)d_tmp, (uint4 *)d_meta, (u64 *)d_size, (u64 *)d_counts});
    if ((rc = timer.end()) || (rc = timer.begin(1))) return rc;
    hipLaunchKernelGGL(k_colscan<1>, dim3(1), dim3(1024), 0, st, (const u64 *)d_size, n_pieces, (u64 *)P->d_blk_off);
    if ((rc = timer.end())) return rc;
    PP_HIPCHK(ctx, hipGetLastError());
    u64 eof_at = 0;
    if ((rc = fetch(ctx, (const u64 *)P->d_blk_off + n_pieces, &eof_at)) || (rc = fetch(ctx, d_counts, P->counts, 3))) return rc;
    P->n_blk = n_pieces;
    P->n_out = eof_at + hb::EOF_SIZE;
    if ((rc = P->alloc(P->d_out, (size_t)P->n_out))) return rc;
    if ((rc = timer.begin(2))) return rc;
    hipLaunchKernelGGL(k_df_place, dim3((unsigned)(n_pieces + 1u)), dim3(DF_BLOCK), 0, st, (const u8 *)d_tmp, (const uint4 *)d_meta, (const u64 *)P->d_blk_off,
                       n_pieces, (u8 *)P->d_out);
    if ((rc = timer.end())) return rc;
    PP_HIPCHK(ctx, hipGetLastError());
    PP_HIPCHK(ctx, hipStreamSynchronize(st));  // host inputs may be released, the scratch goes away
    if ((rc = P->t.take(timer))) return rc;
    *out = P.release();
    return PP_OK;
}

}  // namespace

extern "C" void pp_bgzf_out_free(pp_bgzf_out *o) { delete o; }

extern "C" void pp_bgzf_out_bytes(const pp_bgzf_out *o, const uint8_t **dev, uint64_t *n_bytes) {
    if (dev) *dev = o ? o->d_out : nullptr;
    if (n_bytes) *n_bytes = o ? o->n_out : 0;
}

extern "C" const uint64_t *pp_bgzf_out_blk_off(const pp_bgzf_out *o, uint64_t *n_blk) {
    if (n_blk) *n_blk = o ? o->n_blk : 0;
    return o ? (const uint64_t *)o->d_blk_off : nullptr;
}

extern "C" void pp_bgzf_out_counts(const pp_bgzf_out *o, uint64_t *stored, uint64_t *fixed, uint64_t *dynamic) {
    if (stored) *stored = o ? o->counts[0] : 0;
    if (fixed) *fixed = o ? o->counts[1] : 0;
    if (dynamic) *dynamic = o ? o->counts[2] : 0;
}

extern "C" int pp_bgzf_out_kernel_ms(const pp_bgzf_out *o, float *ms) {
    return o ? o->t.total(o->ctx, "pp_bgzf_out_kernel_ms", "when the bytes were compressed", ms) : PP_ERR_ARG;
}

// (internal hook, not part of the header: tools/bgzf_deflate_timing.py) the same time by stage: the pieces | the scan | the placing
extern "C" int pp_bgzf_out_stage_ms_(const pp_bgzf_out *o, float *ms3) { return o ? o->t.stages(ms3) : PP_ERR_ARG; }

extern "C" int pp_bgzf_out_write(const pp_bgzf_out *o, const char *path) {
    if (!o || !o->ctx) return PP_ERR_ARG;
    if (!path) return o->ctx->fail(PP_ERR_ARG, "pp_bgzf_out_write: null argument");
    return pp::write_device_file(o->ctx, "pp_bgzf_out_write", o->d_out, o->n_out, path);
}

// the .gzi index of the file (pp_fasta_out_host.h: gzi): the blocks' offsets are downloaded, the pairs written on the host
extern "C" int pp_bgzf_out_gzi(const pp_bgzf_out *z, pp_bytes *gzi) {
    if (!z || !z->ctx) return PP_ERR_ARG;
    pp_ctx *ctx = z->ctx;
    if (!gzi) return ctx->fail(PP_ERR_ARG, "pp_bgzf_out_gzi: null argument");
    static_assert(pp_fasta_out_host::GZI_PIECE == PAY, "the index counts the uncompressed bytes in the compressor's pieces");
    gzi->data = nullptr;
    gzi->len = 0;
    PP_HIPCHK(ctx, hipSetDevice(ctx->device));
    std::vector<uint64_t> off((size_t)z->n_blk + 1);
    if (int rc = fetch(ctx, z->d_blk_off, off.data(), off.size())) return rc;
    std::string s;
    pp_fasta_out_host::gzi(off.data(), z->n_blk, s);
    gzi->data = (uint8_t *)malloc(s.size() + 1);
    if (!gzi->data) return ctx->fail(PP_ERR_HIP, "pp_bgzf_out_gzi: out of host memory");
    memcpy(gzi->data, s.data(), s.size());
    gzi->len = s.size();
    return PP_OK;
}

extern "C" int pp_bgzf_deflate(pp_ctx *ctx, const uint8_t *bytes, uint64_t n_bytes, int mem, pp_bgzf_out **out) {
    if (!ctx) return PP_ERR_ARG;
    if (int rdy = pp_ctx_wait(ctx)) return rdy;
    if (!out) return ctx->fail(PP_ERR_ARG, "pp_bgzf_deflate: null argument");
    *out = nullptr;
    if (mem != PP_MEM_HOST && mem != PP_MEM_DEVICE) return ctx->fail(PP_ERR_ARG, "pp_bgzf_deflate: the bytes must be host memory or memory of the context's device");
    if (n_bytes && !bytes) return ctx->fail(PP_ERR_ARG, "pp_bgzf_deflate: null bytes with n_bytes > 0");
    if (n_bytes >= (1ull << 40)) return ctx->fail(PP_ERR_LIMIT, "pp_bgzf_deflate: 2^40 or more bytes in one call");
    PP_HIPCHK(ctx, hipSetDevice(ctx->device));
    CallScratch T;  // the copy of host bytes: released when the call returns
    const u8 *d_bytes = nullptr;
    if (int rc = on_device(ctx, T, mem, (const u8 *)bytes, (size_t)n_bytes, &d_bytes)) return rc;
    return deflate_pieces(ctx, d_bytes, PAY, 0, n_bytes, out);
}

// the payloads of the level-0 file: block b's at b * 65,311 + 23
extern "C" int pp_bam_out_deflate(pp_ctx *ctx, const pp_bam_out *o, pp_bgzf_out **out) {
    if (!ctx) return PP_ERR_ARG;
    if (int rdy = pp_ctx_wait(ctx)) return rdy;
    if (!out) return ctx->fail(PP_ERR_ARG, "pp_bam_out_deflate: null argument");
    *out = nullptr;
    if (!o) return ctx->fail(PP_ERR_ARG, "pp_bam_out_deflate: null argument");
    const uint8_t *file = nullptr;
    uint64_t n_file = 0, n_blocks = 0;
    pp_bam_out_bytes(o, &file, &n_file);
    pp_bam_out_counts(o, nullptr, nullptr, &n_blocks);
    PP_HIPCHK(ctx, hipSetDevice(ctx->device));
    return deflate_pieces(ctx, file, hb::STORE_BLOCK, hb::STORE_HEAD, n_file - hb::EOF_SIZE - (u64)hb::STORE_EXTRA * n_blocks, out);
}
