// pp_bgzf.hip -- pp_bgzf_inflate: the blocks of a BGZF file (every BAM file on disk is one) inflated on the device into one dense
// array, which pp_bam_records takes as PP_MEM_DEVICE bytes.  A BGZF block is a gzip member of at most 64 KiB on either side: a header
// with a BC extra subfield that holds BSIZE, one raw DEFLATE stream with no dictionary from the block in front, CRC32 and ISIZE.
// The BSIZE chain is serial by the format and is walked on the host (pp_bgzf_walk, pp_bgzf_host.h); everything per block runs here:
//   k_bgzf_head     one lane per block: the header at blk_off[b] -- the same function the host walk runs, each field checked before
//                   anything is read through it -- then the payload's place and ISIZE; a defect is status = block << 8 | kind by
//                   atomicMin: the first block in index order wins.  The exclusive scan of the ISIZEs (scan_u32, pp_dev.h) gives
//                   every block its room [out_off[b], out_off[b + 1]).
//   k_bgzf_inflate  ONE WAVE per block.  The symbol loop is serial by the format, so all 64 lanes run it on the same values (table
//                   entries and compressed words go through readfirstlane / readlane, the scalar unit does the arithmetic) and the
//                   wave helps where there is width: it holds 512 bytes of the compressed stream in two registers per lane (a
//                   refill is a readlane; the next 256 bytes are loaded while the current ones are decoded), it builds the decode
//                   tables from the code lengths (counts by LDS atomics, ranks by ballots, table fill per symbol), it copies stored
//                   blocks 16 bytes per lane and matches a byte per lane.  Tables in LDS: 10 bits of first-level lookup for
//                   literal/length, 8 for distance, codes longer than that by the canonical count/offset search over the sorted
//                   symbols.  Match sources are read back from the block's own room in global memory: a wave reads only what it
//                   wrote itself, behind a workgroup-scope fence that is issued only when the source is newer than the last fence.
//                   A match with distance < length replicates: byte i is byte i % distance of the distance bytes in front, all of
//                   which exist before the match starts.
//                   EVERY LOOP IS BOUNDED BY THE INPUT: each symbol takes at least one bit, and after each symbol the bit position
//                   is compared with the payload's end and the output position with ISIZE.  A malformed stream ends with a status
//                   code; nothing is written outside the block's room.  The kernel has no barrier instruction in it.
//   k_bgzf_crc      one wave per block: every lane runs the byte-table CRC32 (table in LDS) over its 64th of the block's output, the
//                   lanes' values are combined pairwise by multiplication by x^(8 n) mod P (zlib's crc32_combine: a 32-entry table
//                   of x^(2^k); pp_crc.h, shared with the BGZF writer of pp_bam_out.hip), lane 0 compares with the footer.  A kernel of its own: its time is a stage of pp_bgzf_kernel_ms.
// No byte outside [0, n_bytes) is loaded: a wide load is issued only where the payload has that many bytes left.
#include "pp_bgzf_host.h"
#include "pp_crc.h"
#include "pp_dev.h"

extern "C" char *pp_bam_msg_buf_(size_t *cap);  // pp_bam.hip: the per-thread message behind pp_bam_last_error()

struct pp_bgzf : DevOwner {
    using DevOwner::DevOwner;
    u8 *d_out = nullptr;          // DEVICE: the inflated bytes
    uint64_t n_out = 0;
    pp_bam_offs *offs = nullptr;  // pp_bgzf_bam_walk's record offsets (DEVICE)
    StageMs<3> t;                 // header, scan and inflate | CRC | the kernels of pp_bgzf_bam_walk
};

namespace {

namespace hb = pp_bgzf_host;

// status: index of a defective block << 8 | kind; the header's kinds (pp_bgzf_host.h) come first
enum : u32 { BZ_BTYPE = 16, BZ_STORED = 17, BZ_CODES = 18, BZ_SYMBOL = 19, BZ_DISTANCE = 20, BZ_LONG = 21, BZ_PAST = 22, BZ_SHORT = 23, BZ_CRC = 24 };

constexpr u32 LIT_BITS = 10, DIST_BITS = 8, CL_BITS = 7;
constexpr u32 MAX_LENS = 320;  // 288 + 32 code lengths at most (HLIT <= 286, HDIST <= 30 are checked)

__constant__ uint16_t LEN_BASE[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
__constant__ uint8_t LEN_EXTRA[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__constant__ uint16_t DIST_BASE[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
__constant__ uint8_t DIST_EXTRA[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
__constant__ uint8_t CL_ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// ---- the headers -----------------------------------------------------------------------------------------------------------------------
struct BlkInfo {  // what k_bgzf_head writes per block
    u64 *pay_off;
    u32 *pay_len, *isize;
};

__global__ __launch_bounds__(256) void k_bgzf_head(u32 n_blk, const u8 *__restrict__ bytes, u64 n_bytes, const u64 *__restrict__ blk_off, BlkInfo O,
                                                   u64 *__restrict__ status) {
    const u32 b = blockIdx.x * 256u + threadIdx.x;
    if (b >= n_blk) return;
    const u64 at = blk_off[b];
    hb::Block B{0, 0, 0, 0};
    const u32 code = hb::block(bytes, n_bytes, at, &B);
    if (code) {
        report(status, ((u64)b << 8) | code);
        B = hb::Block{0, 0, 0, 0};
    }
    O.pay_off[b] = code ? 0 : at + B.payload;
    O.pay_len[b] = B.pay_len;
    O.isize[b] = B.isize;
}

// ---- the compressed stream of one block, as the wave sees it -----------------------------------------------------------------------------
// All members but cw / cn hold the same value in every lane.  Words behind the payload's end read as zeros; the caller compares
// used_bits() with the payload's length after every symbol.
struct Bits {
    const u8 *P;  // the payload
    u32 n;        // its bytes
    u32 cw, cn;   // this lane's word of the current 256-byte chunk, and of the next
    u32 wi;       // the next word to enter bb
    u64 bb;       // the bit buffer, low bits first
    u32 bc;       // bits in it

    __device__ __forceinline__ u32 load_word(u32 w) const {  // word w of the payload, zeros behind its end
        const u32 at = w * 4u;  // (w < 2^15: wi stops growing once used_bits() passes 8 n)
        u32 v = 0;
        if (at < n && n - at >= 4u) __builtin_memcpy(&v, P + at, 4);
        else
            for (u32 j = 0; j < 4u; j++)
                if (at + j < n) v |= (u32)P[at + j] << (8u * j);
        return v;
    }
    __device__ __forceinline__ void refill() {  // afterwards bc > 32
        if (bc <= 32u) {
            const u32 w = __builtin_amdgcn_readlane(cw, __builtin_amdgcn_readfirstlane(wi & 63u));
            bb |= (u64)w << bc;
            bc += 32u;
            wi++;
            if ((wi & 63u) == 0) {
                cw = cn;
                cn = load_word(((wi >> 6) + 1u) * 64u + (threadIdx.x & 63u));
            }
        }
    }
    __device__ __forceinline__ void seek(u32 byte) {
        wi = byte >> 2;
        const u32 c = wi >> 6, lane = threadIdx.x & 63u;
        cw = load_word(c * 64u + lane);
        cn = load_word((c + 1u) * 64u + lane);
        bb = 0;
        bc = 0;
        refill();
        drop((byte & 3u) * 8u);
    }
    __device__ __forceinline__ u32 peek(u32 k) const { return (u32)bb & ((1u << k) - 1u); }
    __device__ __forceinline__ void drop(u32 k) { bb >>= k; bc -= k; }
    __device__ __forceinline__ u32 take(u32 k) { const u32 v = peek(k); drop(k); return v; }
    __device__ __forceinline__ u32 used_bits() const { return wi * 32u - bc; }
    __device__ __forceinline__ bool past() const { return used_bits() > n * 8u; }
};

// ---- the decode tables of one code, built by the wave from its code lengths (LDS) -------------------------------------------------------
struct Code {
    uint16_t *tab;     // 1 << bits entries: symbol << 4 | length, 0 = a longer code or none
    uint16_t *sorted;  // the symbols with a code, by length, then by symbol
    u32 *cnt;          // codes per length (16 words)
    uint16_t *first;   // the first code of every length | the offset of its symbols in `sorted` (2 x 16)
    u32 bits;
};

__device__ __forceinline__ void wave_sync() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); }

// 0: built; 1: over-subscribed; 2: incomplete (the caller decides: zlib takes an incomplete code of a single 1-bit length, or of no
// symbol at all, for literal/length and distance, never for the code lengths' own code).  *max_len = the longest code.
__device__ u32 build_code(const Code &C, const u8 *lens, u32 n, u32 *max_len) {
    const u32 lane = threadIdx.x & 63u;
    for (u32 i = lane; i < (1u << C.bits); i += 64u) C.tab[i] = 0;
    if (lane < 16u) C.cnt[lane] = 0;
    wave_sync();
    for (u32 s = lane; s < n; s += 64u) {
        const u32 l = lens[s];
        if (l) atomicAdd(&C.cnt[l], 1u);
    }
    wave_sync();
    int left = 1;
    u32 code = 0, off = 0, maxl = 0;
    bool over = false;
    for (u32 l = 1; l < 16u; l++) {  // (every lane: the same values)
        const u32 c = __builtin_amdgcn_readfirstlane(C.cnt[l]);
        left = (left << 1) - (int)c;
        over |= left < 0;
        if (left < 0) left = 0;
        if (lane == 0) { C.first[l] = (uint16_t)code; C.first[16u + l] = (uint16_t)off; }
        code = (code + c) << 1;
        off += c;
        if (c) maxl = l;
    }
    *max_len = maxl;
    if (over) return 1u;
    wave_sync();
    u32 base[16];
#pragma unroll
    for (u32 v = 0; v < 16u; v++) base[v] = 0;
    const u64 below = (1ull << lane) - 1ull;
    for (u32 s0 = 0; s0 < n; s0 += 64u) {
        const u32 s = s0 + lane, l = s < n ? lens[s] : 0u;
        u32 rank = 0;
#pragma unroll
        for (u32 v = 1; v < 16u; v++) {
            const u64 m = __ballot(l == v);
            if (l == v) rank = base[v] + (u32)__popcll(m & below);
            base[v] += (u32)__popcll(m);
        }
        if (l) {
            C.sorted[C.first[16u + l] + rank] = (uint16_t)s;  // (below the number of symbols with a code: <= n)
            if (l <= C.bits) {
                const u32 r = __brev((u32)C.first[l] + rank) >> (32u - l);  // the code as the stream has it: first bit lowest
                for (u32 j = r; j < (1u << C.bits); j += 1u << l) C.tab[j] = (uint16_t)(s << 4 | l);
            }
        }
    }
    wave_sync();
    return left > 0 ? 2u : 0u;
}

// one symbol: the first-level table, else the canonical search bit by bit.  Returns its length, 0 = no such code.
__device__ __forceinline__ u32 decode_sym(const Code &C, u32 window, u32 *sym) {
    const u32 e = __builtin_amdgcn_readfirstlane((u32)C.tab[window & ((1u << C.bits) - 1u)]);
    if (e & 15u) {
        *sym = e >> 4;
        return e & 15u;
    }
    int code = 0, first = 0, index = 0;
    for (u32 len = 1; len < 16u; len++) {
        code |= (int)(window & 1u);
        window >>= 1;
        const int count = (int)__builtin_amdgcn_readfirstlane(C.cnt[len]);
        if (code - count < first) {
            *sym = __builtin_amdgcn_readfirstlane((u32)C.sorted[index + (code - first)]);
            return len;
        }
        index += count;
        first += count;
        first <<= 1;
        code <<= 1;
    }
    return 0;
}

struct InflateArgs {
    const u8 *bytes;
    const u64 *pay_off;
    const u32 *pay_len, *isize;
    const u64 *out_off;
    u8 *out;
    u64 *status;
    u32 first_blk, n_blk;
};

__global__ __launch_bounds__(64) void k_bgzf_inflate(InflateArgs A) {
    __shared__ uint16_t s_lit[1u << LIT_BITS], s_dist[1u << DIST_BITS], s_lit_sorted[288], s_dist_sorted[32], s_first[64];
    __shared__ u32 s_cnt[32];
    __shared__ u8 s_lens[MAX_LENS];
    const u32 b = A.first_blk + blockIdx.x, lane = threadIdx.x;
    if (b >= A.n_blk) return;
    const u32 isize = A.isize[b];
    u8 *__restrict__ const O = A.out + A.out_off[b];  // the block's room: isize bytes
    Bits S;
    S.P = A.bytes + A.pay_off[b];
    S.n = A.pay_len[b];
    S.seek(0);
    const Code LIT{s_lit, s_lit_sorted, s_cnt, s_first, LIT_BITS}, DIST{s_dist, s_dist_sorted, s_cnt + 16, s_first + 32, DIST_BITS};
    const Code CL{s_lit, s_lit_sorted, s_cnt, s_first, CL_BITS};  // the code lengths' own code: gone before the literal code is built
    u32 pos = 0, flushed = 0, err = 0, last = 0;
    while (!last && !err) {  // one DEFLATE block per trip: at least three bits
        S.refill();
        last = S.take(1);
        const u32 type = S.take(2);
        if (type == 3u) { err = BZ_BTYPE; break; }
        if (type == 0u) {  // ---- stored: to the byte boundary, LEN, ~LEN, the bytes
            S.drop(S.bc & 7u);
            S.refill();
            const u32 len = S.take(16), nlen = S.take(16);  // (bc is a multiple of 8 above 32: 40 bits at least)
            if ((len ^ nlen) != 0xFFFFu) { err = BZ_STORED; break; }
            if (S.past()) { err = BZ_PAST; break; }
            const u32 at = S.used_bits() >> 3;
            if (len > S.n - at) { err = BZ_PAST; break; }
            if (len > isize - pos) { err = BZ_LONG; break; }
            for (u32 i = lane * 16u; i < len; i += 1024u) {
                if (len - i >= 16u) {
                    uint4 v;
                    __builtin_memcpy(&v, S.P + at + i, 16);
                    __builtin_memcpy(O + pos + i, &v, 16);
                } else
                    for (u32 j = i; j < len; j++) O[pos + j] = S.P[at + j];
            }
            pos += len;
            S.seek(at + len);
            continue;
        }
        // ---- the two codes
        u32 hlit = 288, hdist = 32;  // the fixed codes: complete, with the symbols 286, 287 and 30, 31 that no stream may use
        if (type == 1u) {
            for (u32 s = lane; s < 288u + 32u; s += 64u) s_lens[s] = s < 144u ? 8 : (s < 256u ? 9 : (s < 280u ? 7 : (s < 288u ? 8 : 5)));
        } else {
            S.refill();
            hlit = S.take(5) + 257u;
            hdist = S.take(5) + 1u;
            const u32 hclen = S.take(4) + 4u;
            if (hlit > 286u || hdist > 30u) { err = BZ_CODES; break; }
            if (lane < 19u) s_lens[lane] = 0;
            wave_sync();
            for (u32 i = 0; i < hclen; i++) {
                S.refill();
                const u32 v = S.take(3);
                if (lane == 0) s_lens[CL_ORDER[i]] = (u8)v;
            }
            u32 maxl;
            wave_sync();
            if (build_code(CL, s_lens, 19, &maxl)) { err = BZ_CODES; break; }  // over-subscribed or incomplete
            // the lengths of both codes, one run of hlit + hdist; kept in registers until the code-length code is used up
            const u32 total = hlit + hdist;
            u32 i = 0, prev = 0;
            u8 mine[MAX_LENS / 64];  // lengths i = 64 k + lane
#pragma unroll
            for (u32 k = 0; k < MAX_LENS / 64u; k++) mine[k] = 0;
            while (i < total) {  // every trip takes at least one bit
                S.refill();
                u32 sym;
                const u32 l = decode_sym(CL, S.peek(CL_BITS), &sym);
                if (l == 0) { err = BZ_CODES; break; }
                S.drop(l);
                u32 rep = 1, val = sym;
                if (sym == 16u) {
                    if (i == 0) { err = BZ_CODES; break; }
                    val = prev;
                    rep = 3u + S.take(2);
                } else if (sym == 17u) {
                    val = 0;
                    rep = 3u + S.take(3);
                } else if (sym == 18u) {
                    val = 0;
                    rep = 11u + S.take(7);
                }
                if (rep > total - i) { err = BZ_CODES; break; }
                if (S.past()) { err = BZ_PAST; break; }
#pragma unroll
                for (u32 k = 0; k < MAX_LENS / 64u; k++) {
                    const u32 at = 64u * k + lane;
                    if (at >= i && at < i + rep) mine[k] = (u8)val;
                }
                prev = val;
                i += rep;
            }
            if (err) break;
            wave_sync();
#pragma unroll
            for (u32 k = 0; k < MAX_LENS / 64u; k++)
                if (64u * k + lane < total) s_lens[64u * k + lane] = mine[k];
            wave_sync();
            if (__builtin_amdgcn_readfirstlane((u32)s_lens[256]) == 0) { err = BZ_CODES; break; }  // no end-of-block code
        }
        wave_sync();
        u32 max_lit, max_dist;
        const u32 rl = build_code(LIT, s_lens, hlit, &max_lit);
        if (rl == 1u || (rl == 2u && max_lit != 1u)) { err = BZ_CODES; break; }
        const u32 rd = build_code(DIST, s_lens + hlit, hdist, &max_dist);
        if (rd == 1u || (rd == 2u && max_dist > 1u)) { err = BZ_CODES; break; }
        // ---- the symbols: every trip takes at least one bit, and both positions are looked at before the next one
        for (;;) {
            S.refill();
            u32 sym;
            u32 l = decode_sym(LIT, S.peek(15), &sym);
            if (l == 0) { err = BZ_SYMBOL; break; }
            S.drop(l);
            if (S.past()) { err = BZ_PAST; break; }
            if (sym < 256u) {
                if (pos >= isize) { err = BZ_LONG; break; }
                if (lane == 0) O[pos] = (u8)sym;
                pos++;
                continue;
            }
            if (sym == 256u) break;
            if (sym > 285u) { err = BZ_SYMBOL; break; }
            const u32 len = (u32)LEN_BASE[sym - 257u] + S.take(LEN_EXTRA[sym - 257u]);
            S.refill();
            l = decode_sym(DIST, S.peek(15), &sym);
            if (l == 0 || sym > 29u) { err = BZ_SYMBOL; break; }
            S.drop(l);
            const u32 dist = (u32)DIST_BASE[sym] + S.take(DIST_EXTRA[sym]);
            if (S.past()) { err = BZ_PAST; break; }
            if (dist > pos) { err = BZ_DISTANCE; break; }
            if (len > isize - pos) { err = BZ_LONG; break; }
            const u32 src = pos - dist, fresh = min(len, dist);  // the source bytes: [src, src + fresh), all in front of pos
            if (src + fresh > flushed) {  // written since the last fence: the lanes' stores before the lanes' loads
                wave_sync();
                flushed = pos;
            }
            for (u32 i = lane; i < len; i += 64u) O[pos + i] = O[src + (dist >= len ? i : i % dist)];
            pos += len;
        }
    }
    if (!err && pos != isize) err = BZ_SHORT;
    if (err && lane == 0) report(A.status, ((u64)b << 8) | err);
}

__global__ __launch_bounds__(64) void k_bgzf_crc(u32 first_blk, u32 n_blk, const u8 *__restrict__ bytes, const u64 *__restrict__ pay_off,
                                                 const u32 *__restrict__ pay_len, const u32 *__restrict__ isize, const u64 *__restrict__ out_off,
                                                 const u8 *__restrict__ out, u64 *__restrict__ status) {
    __shared__ u32 s_tab[256];
    const u32 b = first_blk + blockIdx.x, lane = threadIdx.x;
    if (b >= n_blk) return;
    for (u32 i = lane; i < 256u; i += 64u) {
        u32 c = i;
        for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ CRC_POLY : c >> 1;
        s_tab[i] = c;
    }
    __syncthreads();
    const u32 n = isize[b], per = ((n + 63u) / 64u + 15u) & ~15u;  // a lane's bytes: 16 per load (the room's start has any alignment)
    const u32 lo = min(n, lane * per), hi = min(n, lo + per);
    const u8 *__restrict__ const O = out + out_off[b];
    u32 c = 0xFFFFFFFFu, i = lo;
    for (; hi - i >= 16u; i += 16u) {
        u32 w[4];
        __builtin_memcpy(w, O + i, 16);
#pragma unroll
        for (u32 j = 0; j < 16u; j++) c = s_tab[(c ^ (w[j >> 2] >> (8u * (j & 3u)))) & 0xFFu] ^ (c >> 8);
    }
    for (; i < hi; i++) c = s_tab[(c ^ O[i]) & 0xFFu] ^ (c >> 8);
    c = ~c;  // the CRC32 of this lane's bytes; of no bytes: 0
    u32 len = hi - lo;
    for (u32 step = 1; step < 64u; step <<= 1) {  // lane i takes in lane i + step: crc(A B) = crc(A) x^(8 |B|) + crc(B)
        const u32 c2 = __shfl_down(c, step, 64), len2 = __shfl_down(len, step, 64);
        if ((lane & (2u * step - 1u)) == 0) {
            c = multmodp(x8n_modp(len2), c) ^ c2;
            len += len2;
        }
    }
    if (lane == 0) {
        const u8 *f = bytes + pay_off[b] + pay_len[b];  // the footer: CRC32, ISIZE (inside the array: k_bgzf_head)
        const u32 want = (u32)f[0] | (u32)f[1] << 8 | (u32)f[2] << 16 | (u32)f[3] << 24;
        if (c != want) report(status, ((u64)b << 8) | BZ_CRC);
    }
}

const char *defect_text(u32 code) {
    switch (code) {
    case BZ_BTYPE: return "has a DEFLATE block of type 3";
    case BZ_STORED: return "has a stored block whose LEN is not the complement of its NLEN";
    case BZ_CODES: return "has a set of code lengths that is over-subscribed, incomplete, overruns HLIT + HDIST, repeats no length or has no end-of-block code";
    case BZ_SYMBOL: return "uses a code that stands for no literal, length or distance";
    case BZ_DISTANCE: return "has a match that starts in front of the block's first byte";
    case BZ_LONG: return "inflates to more than its ISIZE";
    case BZ_PAST: return "has a DEFLATE stream that runs past its payload";
    case BZ_SHORT: return "inflates to less than its ISIZE";
    case BZ_CRC: return "does not have the CRC32 of its footer";
    default: return hb::defect_text(code);
    }
}

}  // namespace

extern "C" int pp_bgzf_walk(const uint8_t *bytes, uint64_t n_bytes, uint64_t from, uint64_t *blk_off, uint64_t *out_off, uint64_t cap,
                            uint64_t *n_blk, uint64_t *end) {
    size_t mcap = 0;
    char *msg = pp_bam_msg_buf_(&mcap);
    msg[0] = 0;
    return hb::walk(bytes, n_bytes, from, (uint64_t *)blk_off, (uint64_t *)out_off, cap, (uint64_t *)n_blk, (uint64_t *)end, msg, mcap);
}

extern "C" void pp_bgzf_free(pp_bgzf *z) {
    if (z) pp_bam_offs_free(z->offs);
    delete z;
}

extern "C" void pp_bgzf_bytes(const pp_bgzf *z, const uint8_t **dev, uint64_t *n_bytes) {
    if (dev) *dev = z ? z->d_out : nullptr;
    if (n_bytes) *n_bytes = z ? z->n_out : 0;
}

extern "C" const uint64_t *pp_bgzf_rec_off(const pp_bgzf *z) { return z ? pp_bam_offs_dev(z->offs) : nullptr; }

extern "C" int pp_bgzf_kernel_ms(const pp_bgzf *z, float *ms) {
    return z ? z->t.total(z->ctx, "pp_bgzf_kernel_ms", "when the blocks were inflated", ms) : PP_ERR_ARG;
}

// (internal hook, not part of the header: tools/bgzf_timing.py) the same time by stage: header, scan and inflate | CRC | pp_bgzf_bam_walk's kernels
extern "C" int pp_bgzf_stage_ms_(const pp_bgzf *z, float *ms3) { return z ? z->t.stages(ms3) : PP_ERR_ARG; }

extern "C" int pp_bgzf_inflate(pp_ctx *ctx, const uint8_t *bytes, uint64_t n_bytes, const uint64_t *blk_off, uint64_t n_blk, int mem,
                               pp_bgzf **out, uint64_t *bad_block) {
    if (!ctx) return PP_ERR_ARG;
    if (int rdy = pp_ctx_wait(ctx)) return rdy;
    if (bad_block) *bad_block = ~0ull;
    if (!out) return ctx->fail(PP_ERR_ARG, "pp_bgzf_inflate: null argument");
    *out = nullptr;
    if (mem != PP_MEM_HOST && mem != PP_MEM_DEVICE)
        return ctx->fail(PP_ERR_ARG, "pp_bgzf_inflate: the bytes must be host memory or memory of the context's device");
    if (n_bytes && !bytes) return ctx->fail(PP_ERR_ARG, "pp_bgzf_inflate: null bytes with n_bytes > 0");
    if (mem == PP_MEM_DEVICE && !blk_off) return ctx->fail(PP_ERR_ARG, "pp_bgzf_inflate: device bytes need blk_off (the BSIZE chain is walked on the host: pp_bgzf_walk)");
    std::vector<uint64_t> walked;
    if (!blk_off) {  // host bytes: the chain from offset 0
        uint64_t n = 0, end = 0;
        char msg[256] = "";
        if (hb::walk(bytes, n_bytes, 0, nullptr, nullptr, 0, (uint64_t *)&n, (uint64_t *)&end, msg, sizeof msg)) {
            if (bad_block) *bad_block = n;
            return ctx->fail(PP_ERR_ARG, "pp_bgzf_inflate: %s", msg);
        }
        walked.resize((size_t)n + 1);
        if (n) (void)hb::walk(bytes, n_bytes, 0, (uint64_t *)walked.data(), nullptr, n, (uint64_t *)&n, (uint64_t *)&end, msg, sizeof msg);
        blk_off = walked.data();
        n_blk = n;
    }
    if (n_blk >= 0xFFFFFFFFull) return ctx->fail(PP_ERR_LIMIT, "more than 2^32-1 BGZF blocks in one call");
    PP_HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const u32 n = (u32)n_blk;

    std::unique_ptr<pp_bgzf> Z(new pp_bgzf(ctx));  // (no offsets yet: plain delete on an early return)
    CallScratch T;  // the compressed copy and the per-block arrays: released when the call returns
    StageTimer timer(ctx, ctx->profiling != 0);
    int rc;
    if (n == 0) {  // no blocks: an empty object, and with profiling no time
        if ((rc = Z->alloc(Z->d_out, 0))) return rc;
        PP_HIPCHK(ctx, hipStreamSynchronize(st));
        if ((rc = Z->t.take(timer))) return rc;
        *out = Z.release();
        return PP_OK;
    }
    const u8 *d_bytes = nullptr;
    const u64 *d_blk_off = nullptr;
    if ((rc = on_device(ctx, T, mem, (const u8 *)bytes, (size_t)n_bytes, &d_bytes)) || (rc = on_device(ctx, T, mem, (const u64 *)blk_off, (size_t)n, &d_blk_off)))
        return rc;
    void *d_pay_off, *d_pay_len, *d_isize, *d_out_off, *d_status;
    if ((rc = T.get(ctx, &d_pay_off, (size_t)n * 8)) || (rc = T.get(ctx, &d_pay_len, (size_t)n * 4)) || (rc = T.get(ctx, &d_isize, (size_t)n * 4)) ||
        (rc = T.get(ctx, &d_out_off, ((size_t)n + 1) * 8)) || (rc = T.get(ctx, &d_status, 16)))
        return rc;
    PP_HIPCHK(ctx, hipMemsetAsync(d_status, 0xFF, 16, st));
    pp::DevBuf b_sums, b_sums_off;
    struct Free {
        pp::DevBuf &a, &b;
        ~Free() { pp::dev_free(a); pp::dev_free(b); }
    } free_sums{b_sums, b_sums_off};

    // ---- the headers, the rooms ----
    if ((rc = timer.begin(0))) return rc;
    hipLaunchKernelGGL(k_bgzf_head, dim3((n + 255u) / 256u), dim3(256), 0, st, n, d_bytes, (u64)n_bytes, d_blk_off,
                       BlkInfo{(u64 *)d_pay_off, (u32 *)d_pay_len, (u32 *)d_isize}, (u64 *)d_status);
    if ((rc = scan_u32<u64>(ctx, b_sums, b_sums_off, (const u32 *)d_isize, (u64)n, (u64 *)d_out_off))) return rc;
    if ((rc = timer.end())) return rc;
    PP_HIPCHK(ctx, hipGetLastError());
    u64 head_status = ~0ull, total = 0;
    if ((rc = fetch(ctx, d_status, &head_status)) || (rc = fetch(ctx, (const u64 *)d_out_off + n, &total))) return rc;
    // a block with a header defect stops the run in front of it: a stream defect in an earlier block is the first one
    const u32 n_run = head_status != ~0ull ? (u32)(head_status >> 8) : n;
    if ((rc = Z->alloc(Z->d_out, (size_t)total))) return rc;
    Z->n_out = total;

    // ---- the streams, the checksums ----
    InflateArgs A{d_bytes, (const u64 *)d_pay_off, (const u32 *)d_pay_len, (const u32 *)d_isize, (const u64 *)d_out_off, (u8 *)Z->d_out, (u64 *)d_status, 0, n_run};
    constexpr u32 SLICE = 1u << 30;  // blocks per launch
    if ((rc = timer.begin(0))) return rc;
    for (u32 lo = 0; lo < n_run; lo += std::min(SLICE, n_run - lo)) {
        A.first_blk = lo;
        hipLaunchKernelGGL(k_bgzf_inflate, dim3(std::min(SLICE, n_run - lo)), dim3(64), 0, st, A);
    }
    if ((rc = timer.end()) || (rc = timer.begin(1))) return rc;
    for (u32 lo = 0; lo < n_run; lo += std::min(SLICE, n_run - lo))
        hipLaunchKernelGGL(k_bgzf_crc, dim3(std::min(SLICE, n_run - lo)), dim3(64), 0, st, lo, n_run, d_bytes, (const u64 *)d_pay_off, (const u32 *)d_pay_len,
                           (const u32 *)d_isize, (const u64 *)d_out_off, (const u8 *)Z->d_out, (u64 *)d_status);
    if ((rc = timer.end())) return rc;
    PP_HIPCHK(ctx, hipGetLastError());
    u64 status = ~0ull;
    if ((rc = fetch(ctx, d_status, &status))) return rc;  // (the stream is synchronised: host inputs may be released)
    if (status != ~0ull) {
        if (bad_block) *bad_block = status >> 8;
        return ctx->fail(PP_ERR_ARG, "pp_bgzf_inflate: block %llu %s", (unsigned long long)(status >> 8), defect_text((u32)(status & 0xFFu)));
    }
    if ((rc = Z->t.take(timer))) return rc;  // (stage 2 has no span here: zero)
    *out = Z.release();
    return PP_OK;
}

// The device walk (pp_bam_walk.hip) over the inflated bytes: they stay where they are, the object keeps the offsets.
extern "C" int pp_bgzf_bam_walk(pp_bgzf *z, uint64_t from, uint64_t *n_rec, uint64_t *end) {
    if (!z || !z->ctx) return PP_ERR_ARG;
    pp_ctx *ctx = z->ctx;
    if (n_rec) *n_rec = 0;
    if (end) *end = from;
    if (!n_rec || !end) return ctx->fail(PP_ERR_ARG, "pp_bgzf_bam_walk: null argument");
    pp_bam_offs_free(z->offs);
    z->offs = nullptr;
    const int rc = pp_bam_walk_device(ctx, (const uint8_t *)z->d_out, z->n_out, from, PP_MEM_DEVICE, &z->offs, n_rec, end);
    if (rc) {
        const char *msg = pp_bam_last_error();
        return rc == PP_ERR_ARG && msg[0] ? ctx->fail(rc, "pp_bgzf_bam_walk: %s", msg) : rc;  // (a chain that breaks: pp_bam_walk's words)
    }
    float ms = 0.f;
    if (z->t.timed) z->t.ms[2] = ctx->profiling && pp_bam_offs_kernel_ms(z->offs, &ms) == PP_OK ? ms : 0.f;
    return PP_OK;
}
