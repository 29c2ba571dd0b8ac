// pp_bam_out.hip -- pp_bam_tagged: the filter's verdicts written back as a BAM file, on the device.  The WRITE side of the record chain
// for a caller who holds BAM: from the uncompressed BAM bytes in device memory, the records' offsets and one verdict byte per aligned
// record it makes what `polypolish filter` makes of SAM text (filter_sam, src/filter.rs:296-343) -- every record again, ZP:Z:fail
// appended to the aligned ones that failed -- framed as level-0 BGZF, as bytes in device memory; pp_bam_out_write puts them on disk.
//
// pp_bam_tagged_head is the same call with a header of the caller's (HOST bytes, uploaded) as source 0 of the stream in the place of
// bytes[0, records_at): one host function behind both symbols, one more pointer in the framing kernel's arguments.
//
// The uncompressed output U' is bytes[0, records_at), then per record r in index order its 4 + block_size bytes; a failing record has
// block_size + 8 in its first word and the eight bytes Z P Z f a i l NUL behind its last.  The file is U' cut every 65,280 bytes,
// each piece one BGZF block around one stored DEFLATE block (pp_bgzf_host.h: len + 31 bytes, block b at b * 65,311), then the EOF block.
//   k_tag_scan    pass A, one lane per record: the record's range (pp_bam_host::step_kind: the walk's own verdict, nothing read
//                 through an offset before it is checked, no sum that could wrap), the flag at record offset 18, and the
//                 workgroups' numbers of aligned records.  A defect is status[0] = record << 8 | kind by atomicMin: the first
//                 record in index order wins; a block_size that + 8 does not fit its word the same way in status[1]
//   k_tag_len     the aligned records numbered by the workgroup scan of pp_dev.h over k_colscan's bases, the verdict at that rank,
//                 the output length block_size + 8 fail (the 4 bytes of the word are added per index: the sum of a workgroup stays
//                 inside the scan's 64 bits whatever the records hold); its sums, then start[R]: where source R starts in U', R = 0
//                 the header as a pseudo-record, R = r + 1 record r, start[n_rec + 1] = |U'|
//   k_tag_frame   pass B, the hot kernel: ONE WORKGROUP PER OUTPUT BLOCK.  The block's whole image -- header, stored-block prefix,
//                 payload, footer -- is put together in LDS at the 16-byte phase of its place in the file (b * 65,311 is odd):
//                 wave 0 finds the source that covers the block's first byte (a 64-ary search in start[], four rounds for 2^24
//                 records), the workgroup takes the starts inside the block into LDS (at most 1,814: a record is 36 bytes or more),
//                 then every lane owns 16-byte pieces of the image.  A piece that lies inside one source's verbatim bytes is one
//                 16-byte load at the source's alignment; a piece over a seam (a record's end, the appended bytes, the patched
//                 block_size word, the block's own header and footer) touches at most two sources and is put together from one
//                 load of at most 16 bytes per source that stays inside the array.  A lane's four pieces are loaded level by
//                 level (the records' offsets, then the bytes), so it waits for two round trips and not for two per piece.  The
//                 CRC32 runs over LDS: every lane the byte table over 68 bytes (17 words apart: no bank conflict),
//                 slices counted from the payload's END so that every right-hand side of the combination tree has a length known to
//                 the compiler (pp_crc.h), six steps in the wave and four over the sixteen waves.  The image then leaves with 16-byte
//                 aligned stores, its first and last bytes byte by byte.  Every input byte is read from memory once and every output
//                 byte written once.  Workgroup n_blocks writes the EOF block.
// No byte outside [0, n_bytes) is loaded: a wide load is issued only inside a record that pass A found inside the array, or inside
// the header (records_at <= n_bytes).
#include "pp_bam_host.h"
#include "pp_bam_index_host.h"
#include "pp_bgzf_host.h"
#include "pp_crc.h"
#include "pp_dev.h"
#include "pp_k_index.h"
#include "pp_rg_sort.h"

#include <fcntl.h>
#include <unistd.h>

struct pp_bam_out : DevOwner {
    using DevOwner::DevOwner;
    uint8_t *d_out = nullptr;  // DEVICE: the file
    uint64_t n_out = 0;
    uint64_t pass_count = 0, fail_count = 0, n_blocks = 0;
    StageMs<3> t;              // pass A | the scans | pass B
};

namespace {

namespace hb = pp_bgzf_host;

constexpr u32 TAG_BLOCK = 1024;           // records per workgroup of pass A, threads of pass B
constexpr u32 PAY = hb::STORE_PAYLOAD, HEAD = hb::STORE_HEAD, BLK = hb::STORE_BLOCK;
constexpr u32 IMG16 = (15u + BLK + 15u) / 16u;  // the image of a block at any 16-byte phase, in 16-byte pieces
constexpr u32 TRIPS = (IMG16 + TAG_BLOCK - 1u) / TAG_BLOCK;  // pieces per lane
constexpr u32 REL_CAP = 2048;             // starts inside one block kept in LDS (at most 65,280 / 36 + 1, and one behind)
constexpr u32 REL_FAR = 0x7FFFFFFFu;      // a start that far behind the block's first byte, or none
constexpr u32 SLICE = 68;                 // bytes per lane of the CRC: 17 words, so that the lanes' words fall into 32 banks
constexpr u64 TAG_BYTES = 0x006C6961665A505Aull;  // Z P Z f a i l NUL, low byte first
constexpr u32 TL_BLOCK_SIZE = 1;          // status[1]: block_size + 8 does not fit 32 bits

__device__ __forceinline__ u32 ld32(const u8 *__restrict__ p, u64 at) {  // four bytes at any alignment, inside a checked range
    u32 w;
    __builtin_memcpy(&w, p + at, 4);
    return w;
}

// ---- pass A ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TAG_BLOCK) void k_tag_scan(u32 n_rec, const u8 *__restrict__ B, u64 N, const u64 *__restrict__ rec_off,
                                                        u8 *__restrict__ aligned, u64 *__restrict__ blk_al, u64 *__restrict__ status) {
    __shared__ u64 s_w[TAG_BLOCK / 64];
    const u64 r = (u64)blockIdx.x * TAG_BLOCK + threadIdx.x;
    u32 al = 0;
    if (r < n_rec) {
        const u64 o = rec_off[r];
        const u64 left = o <= N ? N - o : 0;  // (an offset behind the array: the walk's "ends inside the block_size word")
        const u32 bs = left >= 4 ? ld32(B, o) : 0u;
        const u32 kind = pp_bam_host::step_kind(left, bs);
        if (kind) report(status, (r << 8) | kind);
        else {
            if (bs > 0xFFFFFFF7u) report(status + 1, (r << 8) | TL_BLOCK_SIZE);
            al = (B[o + 18u] & 4u) ? 0u : 1u;  // the flag's low byte: inside the 32 bytes of the fixed part
        }
        aligned[r] = (u8)al;
    }
    u64 total;
    (void)block_scan_excl64<TAG_BLOCK>(al, s_w, &total);
    if (threadIdx.x == 0) blk_al[blockIdx.x] = total;
}

// PLACE == false: the workgroups' output bytes (without the 4 of each block_size word) and failing records (blk2: two words per
// workgroup).  PLACE == true: blk2 holds their exclusive scan: start[R] of every source.
template <bool PLACE>
__global__ __launch_bounds__(TAG_BLOCK) void k_tag_len(u32 n_rec, const u8 *__restrict__ B, const u64 *__restrict__ rec_off, const u8 *__restrict__ aligned,
                                                       const u64 *__restrict__ al_base, const u8 *__restrict__ pass, u64 records_at,
                                                       u64 *__restrict__ blk2, u64 *__restrict__ start) {
    __shared__ u64 s_w[TAG_BLOCK / 64];
    const u64 r = (u64)blockIdx.x * TAG_BLOCK + threadIdx.x;
    const u32 al = r < n_rec ? aligned[r] : 0u;
    u64 t_al, t_len, t_fail;
    const u64 rank = al_base[blockIdx.x] + block_scan_excl64<TAG_BLOCK>(al, s_w, &t_al);
    const u32 fail = (al && pass[rank] == 0) ? 1u : 0u;
    const u32 len = r < n_rec ? ld32(B, rec_off[r]) + 8u * fail : 0u;  // (block_size <= 0xFFFFFFF7: pass A)
    const u64 ex_len = block_scan_excl64<TAG_BLOCK>(len, s_w, &t_len);
    (void)block_scan_excl64<TAG_BLOCK>(fail, s_w, &t_fail);
    u64 *const mine = blk2 + 2ull * blockIdx.x;
    if (!PLACE) {
        if (threadIdx.x == 0) { mine[0] = t_len; mine[1] = t_fail; }
        return;
    }
    if (r >= n_rec) return;
    const u64 at = records_at + 4ull * r + mine[0] + ex_len;
    if (r == 0) start[0] = 0;
    start[r + 1] = at;
    if (r + 1 == n_rec) start[r + 2] = at + 4ull + len;
}

// ---- pass B ----------------------------------------------------------------------------------------------------------------------
struct Piece16 {  // sixteen bytes of the image, low byte first
    u64 lo, hi;
    // `v` holds bytes for the positions at, at + 1, ... (its low byte first); those below `end` are taken
    __device__ __forceinline__ void put(u64 v_lo, u64 v_hi, u32 at, u32 end) {
        const u32 sh = 8u * at;  // < 128
        u64 a, b;
        if (sh == 0) { a = v_lo; b = v_hi; }
        else if (sh < 64u) { a = v_lo << sh; b = (v_hi << sh) | (v_lo >> (64u - sh)); }
        else { a = 0; b = v_lo << (sh - 64u); }
        if (end < 8u) { a &= (1ull << (8u * end)) - 1ull; b = 0; }
        else if (end < 16u) b &= (1ull << (8u * (end - 8u))) - 1ull;
        lo |= a;
        hi |= b;
    }
};

// sixteen bytes from `at`, of which `need` >= 1 are wanted and lie inside the array; the array's last bytes byte by byte
__device__ __forceinline__ void load16(const u8 *__restrict__ B, u64 N, u64 at, u32 need, u64 *lo, u64 *hi) {
    if (N - at >= 16u) {
        u64 v[2];
        __builtin_memcpy(v, B + at, 16);  // (any alignment: one global_load_dwordx4)
        *lo = v[0];
        *hi = v[1];
    } else {
        u64 a = 0, b = 0;
        for (u32 j = 0; j < need; j++) {
            if (j < 8u) a |= (u64)B[at + j] << (8u * j); else b |= (u64)B[at + j] << (8u * (j - 8u));
        }
        *lo = a;
        *hi = b;
    }
}

struct FrameArgs {
    const u8 *bytes;
    u64 n_bytes;
    const u8 *head;    // source 0, the header: `bytes` itself (pp_bam_tagged) or the caller's header (pp_bam_tagged_head) ...
    u64 n_head_cap;    // ... and the bytes that may be loaded from it
    const u64 *rec_off;
    const u64 *start;  // n_rec + 2 entries
    u32 n_rec;
    u64 total;         // |U'|
    u64 n_blocks;
    u8 *out;
};

__global__ __launch_bounds__(TAG_BLOCK, 8) void k_tag_frame(FrameArgs A) {
    __shared__ uint4 s_img[IMG16];
    __shared__ u32 s_rel[REL_CAP];
    __shared__ u32 s_tab[256];
    __shared__ u32 s_wave[TAG_BLOCK / 64];
    __shared__ u64 s_first[2];
    const u64 b = blockIdx.x;
    const u32 t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    u8 *const dst = A.out + b * (u64)BLK;
    if (b == A.n_blocks) {  // the EOF block, behind the last block's last byte
        if (t < hb::EOF_SIZE) A.out[A.total + (u64)hb::STORE_EXTRA * A.n_blocks + t] = hb::eof_byte(t);
        return;
    }
    const u8 *__restrict__ const B = A.bytes;
    const u64 *__restrict__ const start = A.start;
    const u64 lo = b * (u64)PAY;
    const u32 len = (u32)min((u64)PAY, A.total - lo);
    const u32 ph = (u32)((b * (u64)BLK) & 15u);  // image byte i is block byte i - ph
    u8 *const img8 = (u8 *)s_img;
    const u32 *const img32 = (const u32 *)s_img;

    // ---- the source that covers the block's first byte: the last R with start[R] <= lo (start[0] = 0, start[n_rec + 1] = |U'| > lo)
    crc_table_fill(s_tab, t, TAG_BLOCK);
    if (wave == 0) {
        u64 a = 0, z = (u64)A.n_rec + 2u;
        while (z - a > 1u) {  // (every round cuts the range to a 64th, rounded up)
            const u64 step = (z - a + 63u) / 64u, at = a + lane * step;
            const u64 m = __ballot(at < z && start[at] <= lo);  // a prefix of the lanes, lane 0 among them
            const u32 h = 63u - (u32)__clzll(m);
            a += h * step;
            z = min(z, a + step);
        }
        if (lane == 0) { s_first[0] = a; s_first[1] = lo - start[a]; }
    }
    __syncthreads();
    const u64 R0 = s_first[0], back = s_first[1];  // the block's first byte is byte `back` of source R0
    // ---- the starts behind it, relative to the block: s_rel[i] belongs to source R0 + 1 + i; one of the first 1,815 lies behind the block
    u32 n_rel = 0;
    for (u32 base = 0; base < REL_CAP; base += TAG_BLOCK) {
        const u64 R = R0 + 1u + base + t;
        s_rel[base + t] = R <= (u64)A.n_rec + 1u ? (u32)min(start[R] - lo, (u64)REL_FAR) : REL_FAR;
        n_rel = base + TAG_BLOCK;
        __syncthreads();
        if (s_rel[n_rel - 1u] >= len) break;  // (the same for every thread)
    }
    // the number of starts at or below payload offset q: q belongs to source R0 + that number
    auto source_of = [&](u32 q) {
        u32 at = 0, n = n_rel;
        while (n) {
            const u32 half = n >> 1;
            if (s_rel[at + half] <= q) { at += half + 1u; n -= half + 1u; }
            else n = half;
        }
        return at;
    };

    // a piece over a seam: the block's own head and foot, a record's end, the appended bytes, the patched word.  Its payload bytes lie
    // in at most two sources (a record is 36 bytes or more); what both need is loaded together: their starts and offsets, then their
    // block_size words and bytes.
    auto seam = [&](u32 k) {
        Piece16 Q{0, 0};
        const int j0 = (int)(16u * k) - (int)ph;  // the piece's first byte in the block
        u32 i = 0;
        for (; i < 16u && j0 + (int)i < (int)HEAD; i++)
            if (j0 + (int)i >= 0) Q.put(hb::store_head_byte((u32)(j0 + (int)i), len), 0, i, i + 1u);
        const int end_in = min((int)16, (int)(HEAD + len) - j0);  // the payload's bytes of this piece: [i, i_end); the foot stays zero
        const u32 i_end = end_in > 0 ? (u32)end_in : 0u;
        if (i >= i_end) return Q;
        const u32 q = (u32)(j0 + (int)i) - HEAD;
        const u64 Ra = R0 + source_of(q), last = (u64)A.n_rec + 1u;
        const u64 u0 = lo + q, u1 = u0 + (i_end - i);  // the bytes of U' this piece holds
        u64 Sx[3], ox[2] = {0, 0}, v_lo[2] = {0, 0}, v_hi[2] = {0, 0};
        u32 bsx[2] = {0, 0};
#pragma unroll
        for (u32 s = 0; s < 3u; s++) Sx[s] = start[min(Ra + s, last)];
        if (A.n_rec) {
#pragma unroll
            for (u32 s = 0; s < 2u; s++) ox[s] = A.rec_off[min(max(Ra + s, (u64)1) - 1u, (u64)A.n_rec - 1u)];
        }
#pragma unroll
        for (u32 s = 0; s < 2u; s++) {
            const u64 R = Ra + s, S = Sx[s], a = max(u0, S), z = min(u1, Sx[s + 1u]);
            if (R > A.n_rec || a >= z) continue;
            if (R == 0) load16(A.head, A.n_head_cap, a, (u32)(z - a), &v_lo[s], &v_hi[s]);  // the header: its bytes are where they were
            else {
                bsx[s] = ld32(B, ox[s]);
                const u64 from = ox[s] + (max(a, S + 4u) - S);  // (behind the record's bytes where the piece holds only appended ones)
                if (from < A.n_bytes) load16(B, A.n_bytes, from, (u32)min((u64)16, A.n_bytes - from), &v_lo[s], &v_hi[s]);
            }
        }
#pragma unroll
        for (u32 s = 0; s < 2u; s++) {
            const u64 R = Ra + s, S = Sx[s], E = Sx[s + 1u], a = max(u0, S), z = min(u1, E);
            if (R > A.n_rec || a >= z) continue;
            if (R == 0) {
                Q.put(v_lo[s], v_hi[s], i + (u32)(a - u0), i + (u32)(z - u0));
                continue;
            }
            const u64 bs = bsx[s], body = S + 4u, tail = body + bs;  // the word | the record's bytes | the appended bytes
            if (a < body) Q.put((u64)(bsx[s] + (E - S != 4ull + bs ? 8u : 0u)) >> (8u * (u32)(a - S)), 0, i + (u32)(a - u0), i + (u32)(min(z, body) - u0));
            const u64 va = max(a, body), vz = min(z, tail);
            if (va < vz) Q.put(v_lo[s], v_hi[s], i + (u32)(va - u0), i + (u32)(vz - u0));
            const u64 ta = max(a, tail);
            if (ta < z) Q.put(TAG_BYTES >> (8u * (u32)(ta - tail)), 0, i + (u32)(ta - u0), i + (u32)(z - u0));
        }
        return Q;
    };

    // ---- the image, 16 bytes per lane and trip.  The loads of all four trips are issued level by level -- the records' offsets, then
    // the bytes -- so that a lane waits for two round trips, not for two per trip.
    const u32 n_piece = (ph + len + hb::STORE_EXTRA + 15u) / 16u;
    u64 at[TRIPS], o[TRIPS];   // the piece's first byte in its source; the source record's index, then its offset (the header: 0)
    u32 fast = 0, in_rec = 0;  // per trip: one load does it; ... from a record
#pragma unroll
    for (u32 j = 0; j < TRIPS; j++) {
        const u32 k = t + j * TAG_BLOCK;
        const int q0 = (int)(16u * k) - (int)ph - (int)HEAD;  // the piece's first byte in the payload
        at[j] = 0;
        o[j] = 0;
        if (k < n_piece && q0 >= 0 && (u32)q0 + 16u <= len) {
            const u32 idx = source_of((u32)q0), e = s_rel[idx];
            const u64 d = idx ? (u64)((u32)q0 - s_rel[idx - 1u]) : (u64)(u32)q0 + back;  // the piece's first byte in its source
            if (R0 + idx == 0) {  // the header
                if ((u32)q0 + 16u <= e) { at[j] = d; fast |= 1u << j; }
            } else if (d >= 4u && (u32)q0 + 24u <= e) {  // behind the block_size word, in front of the last 8 bytes whatever they are
                at[j] = d;
                o[j] = R0 + idx - 1u;
                fast |= 1u << j;
                in_rec |= 1u << j;
            }
        }
    }
#pragma unroll
    for (u32 j = 0; j < TRIPS; j++)
        if ((in_rec >> j) & 1u) o[j] = A.rec_off[o[j]];
    Piece16 P[TRIPS];
#pragma unroll
    for (u32 j = 0; j < TRIPS; j++) {
        P[j] = Piece16{0, 0};
        if ((fast >> j) & 1u) {
            const bool rec = (in_rec >> j) & 1u;
            load16(rec ? B : A.head, rec ? A.n_bytes : A.n_head_cap, o[j] + at[j], 16, &P[j].lo, &P[j].hi);
        }
    }
#pragma unroll
    for (u32 j = 0; j < TRIPS; j++) {
        const u32 k = t + j * TAG_BLOCK;
        if (k >= n_piece) break;
        if (!((fast >> j) & 1u)) P[j] = seam(k);
        s_img[k] = make_uint4((u32)P[j].lo, (u32)(P[j].lo >> 32), (u32)P[j].hi, (u32)(P[j].hi >> 32));
    }
    __syncthreads();

    // ---- the CRC32 of the payload: thread T owns the 68 bytes that end 68 (1023 - T) bytes in front of the payload's end
    const int p0 = (int)(ph + HEAD), p1 = p0 + (int)len;
    const int hi_at = p1 - (int)(SLICE * (TAG_BLOCK - 1u - t)), lo_at = hi_at - (int)SLICE;
    u32 c = 0;  // the CRC32 of no bytes
    if (hi_at > p0) {
        c = 0xFFFFFFFFu;
        if (lo_at >= p0) {
            const u32 w0 = (u32)lo_at >> 2, sh = (u32)lo_at & 3u;  // (sh: the same for every thread)
            u32 prev = img32[w0];
#pragma unroll
            for (u32 j = 0; j < SLICE / 4u; j++) {
                const u32 next = img32[w0 + j + 1u];
                c = crc_word(s_tab, c, __builtin_amdgcn_alignbyte(next, prev, sh));
                prev = next;
            }
        } else {
            for (int i = p0; i < hi_at; i++) c = crc_byte(s_tab, c, img8[i]);
        }
        c = ~c;
    }
    constexpr X8N2K<SLICE, 10> MUL = X8N2K<SLICE, 10>();  // x^(8 * 68 * 2^k): a right-hand side of 2^k whole slices
#pragma unroll
    for (u32 k = 0; k < 6u; k++) {  // lane i takes in lane i + 2^k: crc(A B) = crc(A) x^(8 |B|) + crc(B)
        const u32 c2 = __shfl_down(c, 1u << k, 64);
        if ((lane & ((2u << k) - 1u)) == 0) c = multmodp(MUL.v[k], c) ^ c2;
    }
    if (lane == 0) s_wave[wave] = c;
    __syncthreads();
    if (wave == 0) {
        c = lane < TAG_BLOCK / 64u ? s_wave[lane] : 0u;
#pragma unroll
        for (u32 k = 0; k < 4u; k++) {
            const u32 c2 = __shfl_down(c, 1u << k, 64);
            if ((lane & ((2u << k) - 1u)) == 0) c = multmodp(MUL.v[6u + k], c) ^ c2;
        }
        const u32 crc = __shfl(c, 0, 64);
        if (lane < 8u) img8[p1 + (int)lane] = (u8)((lane < 4u ? crc : len) >> (8u * (lane & 3u)));  // CRC32, ISIZE
    }
    __syncthreads();

    // ---- out: 16-byte aligned stores, the first and the last piece byte by byte
    u8 *const out16 = dst - ph;
    const u32 img_end = ph + len + hb::STORE_EXTRA;
    for (u32 k = t; k < n_piece; k += TAG_BLOCK) {
        if ((k == 0 && ph) || 16u * k + 16u > img_end) {
            for (u32 i = max(16u * k, ph); i < min(16u * k + 16u, img_end); i++) out16[i] = img8[i];
        } else *(uint4 *)(out16 + 16u * k) = s_img[k];
    }
}

}  // namespace

extern "C" void pp_bam_out_free(pp_bam_out *o) { delete o; }

extern "C" void pp_bam_out_bytes(const pp_bam_out *o, const uint8_t **dev, uint64_t *n_bytes) {
    if (dev) *dev = o ? o->d_out : nullptr;
    if (n_bytes) *n_bytes = o ? o->n_out : 0;
}

extern "C" void pp_bam_out_counts(const pp_bam_out *o, uint64_t *pass_count, uint64_t *fail_count, uint64_t *n_blocks) {
    if (pass_count) *pass_count = o ? o->pass_count : 0;
    if (fail_count) *fail_count = o ? o->fail_count : 0;
    if (n_blocks) *n_blocks = o ? o->n_blocks : 0;
}

extern "C" int pp_bam_out_kernel_ms(const pp_bam_out *o, float *ms) {
    return o ? o->t.total(o->ctx, "pp_bam_out_kernel_ms", "when the records were tagged", ms) : PP_ERR_ARG;
}

// (internal hook, not part of the header: tools/bam_tag_timing.py) the same time by stage: pass A | the scans | pass B
extern "C" int pp_bam_out_stage_ms_(const pp_bam_out *o, float *ms3) { return o ? o->t.stages(ms3) : PP_ERR_ARG; }

// a file in device memory to `path`, in slices through a host buffer (pp_bam_out_write, pp_bgzf_out_write); a path that cannot be
// created or written: as pp_filter_write
int pp::write_device_file(pp_ctx *ctx, const char *who, const void *dev, uint64_t n, const char *path) {
    PP_HIPCHK(ctx, hipSetDevice(ctx->device));
    const int fd = open(path, O_WRONLY | O_CREAT | O_TRUNC, 0666);
    if (fd < 0) return ctx->fail(PP_ERR_QUIT, "unable to write alignments to \"%s\"", path);
    constexpr size_t PIECE = (size_t)64 << 20;
    std::vector<uint8_t> buf((size_t)std::min<uint64_t>(n, PIECE));
    int rc = PP_OK;
    for (uint64_t at = 0; at < n && !rc; at += PIECE) {
        const size_t k = (size_t)std::min<uint64_t>(PIECE, n - at);
        const hipError_t e = hipMemcpy(buf.data(), (const uint8_t *)dev + at, k, hipMemcpyDeviceToHost);
        if (e != hipSuccess) { rc = ctx->fail(PP_ERR_HIP, "%s: hipMemcpy failed: %s", who, hipGetErrorString(e)); break; }
        for (size_t done = 0; done < k;) {
            const ssize_t w = write(fd, buf.data() + done, k - done);
            if (w <= 0) { rc = ctx->fail(PP_ERR_QUIT, "unable to write alignments to \"%s\"", path); break; }
            done += (size_t)w;
        }
    }
    if (close(fd) != 0 && !rc) rc = ctx->fail(PP_ERR_QUIT, "unable to write alignments to \"%s\"", path);
    return rc;
}

extern "C" int pp_bam_out_write(const pp_bam_out *o, const char *path) {
    if (!o || !o->ctx) return PP_ERR_ARG;
    if (!path) return o->ctx->fail(PP_ERR_ARG, "pp_bam_out_write: null argument");
    return pp::write_device_file(o->ctx, "pp_bam_out_write", o->d_out, o->n_out, path);
}

namespace {

// pp_bam_tagged (the stream starts with bytes[0, records_at)) and pp_bam_tagged_head (with_head: it starts with the HOST bytes
// head[0, n_head)): `who` words the refusals, which are the same
int tagged(pp_ctx *ctx, const char *who, const uint8_t *bytes, uint64_t n_bytes, uint64_t records_at, const uint64_t *rec_off, uint64_t n_rec,
           int mem, const uint8_t *pass, uint64_t n_pass, const uint8_t *head, uint64_t n_head, bool with_head, pp_bam_out **out, uint64_t *bad_record) {
    if (!ctx) return PP_ERR_ARG;
    if (int rdy = pp_ctx_wait(ctx)) return rdy;
    if (bad_record) *bad_record = ~0ull;
    if (!out) return ctx->fail(PP_ERR_ARG, "%s: null argument", who);
    *out = nullptr;
    if (mem != PP_MEM_HOST && mem != PP_MEM_DEVICE)
        return ctx->fail(PP_ERR_ARG, "%s: the bytes must be host memory or memory of the context's device", who);
    if ((n_bytes && !bytes) || (n_rec && !rec_off)) return ctx->fail(PP_ERR_ARG, "%s: null bytes with n_bytes > 0, or null rec_off with n_rec > 0", who);
    if (with_head && n_head && !head) return ctx->fail(PP_ERR_ARG, "%s: null head with n_head > 0", who);
    if (records_at > n_bytes) return ctx->fail(PP_ERR_ARG, "%s: records_at %llu lies behind the %llu bytes", who, (unsigned long long)records_at, (unsigned long long)n_bytes);
    if (n_rec >= 0xFFFFFFFFull) return ctx->fail(PP_ERR_LIMIT, "more than 2^32-1 alignments in one batch");
    if (n_bytes >= (1ull << 40) || n_head >= (1ull << 40)) return ctx->fail(PP_ERR_LIMIT, "%s: 2^40 or more bytes in one call", who);
    PP_HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const u32 n = (u32)n_rec;

    std::unique_ptr<pp_bam_out> P(new pp_bam_out(ctx));
    CallScratch T;  // the copy of host bytes and the per-record arrays: released when the call returns
    StageTimer timer(ctx, ctx->profiling != 0);
    int rc;
    const u8 *d_bytes = nullptr;
    const u64 *d_rec_off = nullptr;
    if ((rc = on_device(ctx, T, mem, (const u8 *)bytes, (size_t)n_bytes, &d_bytes)) || (rc = on_device(ctx, T, mem, (const u64 *)rec_off, (size_t)n, &d_rec_off)))
        return rc;
    const u8 *d_head = d_bytes;               // source 0 of the stream: the bytes' own header ...
    u64 head_len = records_at, head_cap = n_bytes;
    if (with_head) {                          // ... or the caller's
        if ((rc = on_device(ctx, T, PP_MEM_HOST, (const u8 *)head, (size_t)n_head, &d_head))) return rc;
        head_len = head_cap = n_head;
    }
    const u32 nb = std::max(1u, (n + TAG_BLOCK - 1u) / TAG_BLOCK);
    void *d_aligned, *d_blk_al, *d_al_base, *d_blk2, *d_blk2off, *d_start, *d_status, *d_pass;
    if ((rc = T.get(ctx, &d_aligned, (size_t)n)) || (rc = T.get(ctx, &d_blk_al, (size_t)nb * 8)) || (rc = T.get(ctx, &d_al_base, ((size_t)nb + 1) * 8)) ||
        (rc = T.get(ctx, &d_blk2, (size_t)nb * 16)) || (rc = T.get(ctx, &d_blk2off, ((size_t)nb + 1) * 16)) || (rc = T.get(ctx, &d_start, ((size_t)n + 2) * 8)) ||
        (rc = T.get(ctx, &d_status, 16)))
        return rc;

    // ---- pass A: the ranges, the aligned records ----
    u64 n_al = 0, u_total = head_len, n_fail = 0;
    if (n) {
        PP_HIPCHK(ctx, hipMemsetAsync(d_status, 0xFF, 16, st));
        if ((rc = timer.begin(0))) return rc;
        hipLaunchKernelGGL(k_tag_scan, dim3(nb), dim3(TAG_BLOCK), 0, st, n, d_bytes, (u64)n_bytes, d_rec_off, (u8 *)d_aligned, (u64 *)d_blk_al, (u64 *)d_status);
        if ((rc = timer.end()) || (rc = timer.begin(1))) return rc;
        hipLaunchKernelGGL(k_colscan<1>, dim3(1), dim3(1024), 0, st, (const u64 *)d_blk_al, (u64)nb, (u64 *)d_al_base);
        if ((rc = timer.end())) return rc;
        PP_HIPCHK(ctx, hipGetLastError());
        u64 status[2] = {~0ull, ~0ull};
        if ((rc = fetch(ctx, d_status, status, 2)) || (rc = fetch(ctx, (const u64 *)d_al_base + nb, &n_al))) return rc;
        if (status[0] != ~0ull) {
            const u64 r = status[0] >> 8;
            const u32 kind = (u32)(status[0] & 0xFFu);
            if (bad_record) *bad_record = r;
            return ctx->fail(PP_ERR_ARG, "%s: record %llu %s", who, (unsigned long long)r,
                             kind == pp_bam_host::W_CUT ? "has an offset outside the bytes, or the bytes end inside its block_size"
                             : kind == pp_bam_host::W_SMALL ? "has a block_size below the 32 bytes of its fixed part" : "runs past the end of the bytes");
        }
        if (status[1] != ~0ull) {
            if (bad_record) *bad_record = status[1] >> 8;
            return ctx->fail(PP_ERR_LIMIT, "%s: record %llu has a block_size above 0xFFFFFFF7", who, (unsigned long long)(status[1] >> 8));
        }
    }
    if (n_al && !pass) return ctx->fail(PP_ERR_ARG, "%s: null pass with %llu aligned records", who, (unsigned long long)n_al);
    if (n_pass != n_al)
        return ctx->fail(PP_ERR_ARG, "%s: %llu verdicts for %llu aligned records", who, (unsigned long long)n_pass, (unsigned long long)n_al);

    // ---- the verdicts (host memory whatever `mem`), the lengths, the starts ----
    if ((rc = T.get(ctx, &d_pass, (size_t)n_al))) return rc;
    if (n_al) PP_HIPCHK(ctx, hipMemcpyAsync(d_pass, pass, (size_t)n_al, hipMemcpyHostToDevice, st));
    if (n) {
        if ((rc = timer.begin(1))) return rc;
        hipLaunchKernelGGL(k_tag_len<false>, dim3(nb), dim3(TAG_BLOCK), 0, st, n, d_bytes, d_rec_off, (const u8 *)d_aligned, (const u64 *)d_al_base,
                           (const u8 *)d_pass, head_len, (u64 *)d_blk2, (u64 *)nullptr);
        hipLaunchKernelGGL(k_colscan<2>, dim3(1), dim3(1024), 0, st, (const u64 *)d_blk2, (u64)nb, (u64 *)d_blk2off);
        hipLaunchKernelGGL(k_tag_len<true>, dim3(nb), dim3(TAG_BLOCK), 0, st, n, d_bytes, d_rec_off, (const u8 *)d_aligned, (const u64 *)d_al_base,
                           (const u8 *)d_pass, head_len, (u64 *)d_blk2off, (u64 *)d_start);
        if ((rc = timer.end())) return rc;
        PP_HIPCHK(ctx, hipGetLastError());
        u64 totals[2] = {0, 0};
        if ((rc = fetch(ctx, (const u64 *)d_blk2off + 2ull * nb, totals, 2))) return rc;
        u_total = head_len + 4ull * n + totals[0];
        n_fail = totals[1];
    } else {  // the header alone
        const u64 two[2] = {0, head_len};
        PP_HIPCHK(ctx, hipMemcpyAsync(d_start, two, sizeof two, hipMemcpyHostToDevice, st));
        PP_HIPCHK(ctx, hipStreamSynchronize(st));
    }

    // ---- pass B: the blocks ----
    const u64 n_blocks = (u_total + PAY - 1u) / PAY;
    P->n_out = u_total + (u64)hb::STORE_EXTRA * n_blocks + hb::EOF_SIZE;
    P->n_blocks = n_blocks;
    P->pass_count = n_al - n_fail;
    P->fail_count = n_fail;
    if ((rc = P->alloc(P->d_out, (size_t)P->n_out))) return rc;
    if ((rc = timer.begin(2))) return rc;
    hipLaunchKernelGGL(k_tag_frame, dim3((unsigned)(n_blocks + 1u)), dim3(TAG_BLOCK), 0, st,
                       FrameArgs{d_bytes, (u64)n_bytes, d_head, head_cap, d_rec_off, (const u64 *)d_start, n, u_total, n_blocks, (u8 *)P->d_out});
    if ((rc = timer.end())) return rc;
    PP_HIPCHK(ctx, hipGetLastError());
    PP_HIPCHK(ctx, hipStreamSynchronize(st));  // host inputs may be released, the scratch goes away
    if ((rc = P->t.take(timer))) return rc;
    *out = P.release();
    return PP_OK;
}

}  // namespace

extern "C" int pp_bam_tagged(pp_ctx *ctx, const uint8_t *bytes, uint64_t n_bytes, uint64_t records_at, const uint64_t *rec_off, uint64_t n_rec,
                             int mem, const uint8_t *pass, uint64_t n_pass, pp_bam_out **out, uint64_t *bad_record) {
    return tagged(ctx, "pp_bam_tagged", bytes, n_bytes, records_at, rec_off, n_rec, mem, pass, n_pass, nullptr, 0, false, out, bad_record);
}

extern "C" int pp_bam_tagged_head(pp_ctx *ctx, const uint8_t *bytes, uint64_t n_bytes, uint64_t records_at, const uint64_t *rec_off, uint64_t n_rec,
                                  int mem, const uint8_t *pass, uint64_t n_pass, const uint8_t *head, uint64_t n_head, pp_bam_out **out,
                                  uint64_t *bad_record) {
    return tagged(ctx, "pp_bam_tagged_head", bytes, n_bytes, records_at, rec_off, n_rec, mem, pass, n_pass, head, n_head, true, out, bad_record);
}

// ---- pp_bam_index: the .bai of the file pp_bam_tagged_head makes of the same arguments -----------------------------------------------
// The records' places in the stream are pass A and the scans above (start[]); a stream offset u is the virtual offset
// blk_off[u / 65,280] << 16 | u % 65,280.  Then one lane per record:
//   k_ix_rec     ref_id, pos, flag and the reference span of the CIGAR (M D N = X), read inside the record pass A found inside the
//                array; a CIGAR that leaves its record is refused before a run is read
//   k_ix_check   ref_id against n_ref, a placed record's pos, the order against the record in front, end against 2^29; the bin.  The
//                first offender in index order by atomicMin
// and the table stage that pp_tabix_index shares (pp_k_index.h: k_ix_run, k_ix_chunk, k_ix_ref, k_ix_lin, k_ix_fill, k_ix_gather):
//   k_rg_hist / k_rg_scatter (pp_rg_sort.h)  the chunk table brought into (ref_id, bin) order, stable: a bin's chunks in file order
// The host (pp_bam_index_host.h) writes the downloaded tables out.
namespace {

enum : u32 { IX_CIGAR = 8, IX_REF = 9, IX_PLACED = 10, IX_ORDER = 11, IX_END = 12 };

enum : int { IX_SCANS = 0, IX_RECORDS = 1, IX_CHUNKS = 2, IX_LINEAR = 3 };

__global__ __launch_bounds__(256) void k_ix_rec(u32 n, const u8 *__restrict__ B, const u64 *__restrict__ rec_off, IxRec *__restrict__ rec,
                                                uint16_t *__restrict__ flag, u64 *__restrict__ status) {
    const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
    if (r >= n) return;
    const u64 o = rec_off[r];  // (pass A: the 4 + block_size >= 36 bytes from o on lie inside the array)
    const u32 bs = ld32(B, o);
    const int32_t ref = (int32_t)ld32(B, o + 4u), pos = (int32_t)ld32(B, o + 8u);
    const u32 l_name = B[o + 12u], n_cig = (u32)B[o + 16u] | (u32)B[o + 17u] << 8, f = (u32)B[o + 18u] | (u32)B[o + 19u] << 8;
    u64 span = 0;
    if (32ull + l_name + 4ull * n_cig > bs) report(status, (r << 8) | IX_CIGAR);
    else
        for (u32 i = 0; i < n_cig; i++) {
            const u32 w = ld32(B, o + 36u + l_name + 4ull * i), op = w & 15u;
            if (op == 0u || op == 2u || op == 3u || op == 7u || op == 8u) span += w >> 4;
        }
    const u64 e = (u64)(pos > 0 ? pos : 0) + ((span && !(f & 4u)) ? span : 1ull);
    rec[r] = IxRec{ref, pos, (u32)min(e, (u64)0xFFFFFFFFu)};
    flag[r] = (uint16_t)f;
}

__device__ __forceinline__ u64 ix_key(const IxRec &R) { return (u64)(u32)R.ref << 32 | (u64)(R.ref < 0 ? 0u : (u32)R.pos); }

__global__ __launch_bounds__(256) void k_ix_check(u32 n, const IxRec *__restrict__ rec, u32 n_ref, u32 *__restrict__ bin, u64 *__restrict__ status) {
    const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
    if (r >= n) return;
    const IxRec R = rec[r];
    u32 kind = 0;
    if (R.ref < -1 || (R.ref >= 0 && (u32)R.ref >= n_ref)) kind = IX_REF;
    else if (R.ref >= 0 && R.pos < 0) kind = IX_PLACED;
    else if (r > 0 && ix_key(R) < ix_key(rec[r - 1u])) kind = IX_ORDER;
    else if (R.ref >= 0 && R.end > IX_MAX_END) kind = IX_END;
    if (kind) report(status, (r << 8) | kind);
    bin[r] = (!kind && R.ref >= 0) ? reg2bin((u32)R.pos, R.end) : 0u;
}

__global__ __launch_bounds__(256) void k_ix_blk(u64 n, const u64 *__restrict__ blk_off, u64 *__restrict__ status) {
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    if (i < n && blk_off[i] >= pp_bam_index_host::MAX_COFFSET) report(status, i);
}

}  // namespace

extern "C" int pp_bam_index(pp_ctx *ctx, const uint8_t *bytes, uint64_t n_bytes, uint64_t n_head, const uint64_t *rec_off, uint64_t n_rec, int mem,
                            const uint8_t *pass, uint64_t n_pass, uint32_t n_ref, const uint64_t *blk_off, uint64_t n_blk, int blk_mem, pp_bytes *bai,
                            uint64_t *bad_record) {
    if (!ctx) return PP_ERR_ARG;
    if (int rdy = pp_ctx_wait(ctx)) return rdy;
    if (bad_record) *bad_record = ~0ull;
    if (!bai) return ctx->fail(PP_ERR_ARG, "pp_bam_index: null argument");
    bai->data = nullptr;
    bai->len = 0;
    if ((mem != PP_MEM_HOST && mem != PP_MEM_DEVICE) || (blk_mem != PP_MEM_HOST && blk_mem != PP_MEM_DEVICE))
        return ctx->fail(PP_ERR_ARG, "pp_bam_index: the bytes and the block offsets must be host memory or memory of the context's device");
    if ((n_bytes && !bytes) || (n_rec && !rec_off) || !blk_off) return ctx->fail(PP_ERR_ARG, "pp_bam_index: null bytes, rec_off or blk_off");
    if (n_rec >= 0xFFFFFFFFull) return ctx->fail(PP_ERR_LIMIT, "more than 2^32-1 alignments in one batch");
    if (n_bytes >= (1ull << 40) || n_head >= (1ull << 40)) return ctx->fail(PP_ERR_LIMIT, "pp_bam_index: 2^40 or more bytes in one call");
    if (n_ref > IX_MAX_REF) return ctx->fail(PP_ERR_LIMIT, "pp_bam_index: more than 2^24 references");
    if (n_blk >= (1ull << 32)) return ctx->fail(PP_ERR_LIMIT, "pp_bam_index: 2^32 or more blocks");
    PP_HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const u32 n = (u32)n_rec;
    CallScratch T;
    CtxScratch S(ctx, ctx->g_rec, "pp_bam_index");  // (scan_u32's block sums)
    StageTimer timer(ctx, ctx->profiling != 0);     // scans | records | chunks | linear (pp_bam_index_stage_ms_)
    ctx->ix_timed = false;
    int rc;
    const u8 *d_bytes = nullptr;
    const u64 *d_rec_off = nullptr, *d_blk = nullptr;
    if ((rc = on_device(ctx, T, mem, (const u8 *)bytes, (size_t)n_bytes, &d_bytes)) || (rc = on_device(ctx, T, mem, (const u64 *)rec_off, (size_t)n, &d_rec_off)) ||
        (rc = on_device(ctx, T, blk_mem, (const u64 *)blk_off, (size_t)n_blk + 1, &d_blk)))
        return rc;
    const u32 nb = std::max(1u, (n + TAG_BLOCK - 1u) / TAG_BLOCK);
    const unsigned gb = std::max(1u, (unsigned)(((u64)n + 255u) / 256u));
    void *d_aligned, *d_blk_al, *d_al_base, *d_blk2, *d_blk2off, *d_start, *d_status, *d_pass, *d_rec, *d_flag, *d_bin, *d_st2;
    if ((rc = T.get(ctx, &d_aligned, (size_t)n)) || (rc = T.get(ctx, &d_blk_al, (size_t)nb * 8)) || (rc = T.get(ctx, &d_al_base, ((size_t)nb + 1) * 8)) ||
        (rc = T.get(ctx, &d_blk2, (size_t)nb * 16)) || (rc = T.get(ctx, &d_blk2off, ((size_t)nb + 1) * 16)) || (rc = T.get(ctx, &d_start, ((size_t)n + 2) * 8)) ||
        (rc = T.get(ctx, &d_status, 16)) || (rc = T.get(ctx, &d_rec, (size_t)n * sizeof(IxRec))) || (rc = T.get(ctx, &d_flag, (size_t)n * 2)) ||
        (rc = T.get(ctx, &d_bin, (size_t)n * 4)) || (rc = T.get(ctx, &d_st2, 32)))
        return rc;
    PP_HIPCHK(ctx, hipMemsetAsync(d_status, 0xFF, 16, st));
    PP_HIPCHK(ctx, hipMemsetAsync(d_st2, 0xFF, 32, st));

    // ---- pass A and the scans, as pp_bam_tagged_head makes them: the records' ranges, the aligned records, start[] ----
    u64 n_al = 0, u_total = n_head;
    if (n) {
        if ((rc = timer.begin(IX_SCANS))) return rc;
        hipLaunchKernelGGL(k_tag_scan, dim3(nb), dim3(TAG_BLOCK), 0, st, n, d_bytes, (u64)n_bytes, d_rec_off, (u8 *)d_aligned, (u64 *)d_blk_al, (u64 *)d_status);
        hipLaunchKernelGGL(k_colscan<1>, dim3(1), dim3(1024), 0, st, (const u64 *)d_blk_al, (u64)nb, (u64 *)d_al_base);
        if ((rc = timer.end())) return rc;
        PP_HIPCHK(ctx, hipGetLastError());
        u64 status[2] = {~0ull, ~0ull};
        if ((rc = fetch(ctx, d_status, status, 2)) || (rc = fetch(ctx, (const u64 *)d_al_base + nb, &n_al))) return rc;
        if (status[0] != ~0ull) {
            const u64 r = status[0] >> 8;
            const u32 kind = (u32)(status[0] & 0xFFu);
            if (bad_record) *bad_record = r;
            return ctx->fail(PP_ERR_ARG, "pp_bam_index: record %llu %s", (unsigned long long)r,
                             kind == pp_bam_host::W_CUT ? "has an offset outside the bytes, or the bytes end inside its block_size"
                             : kind == pp_bam_host::W_SMALL ? "has a block_size below the 32 bytes of its fixed part" : "runs past the end of the bytes");
        }
        if (status[1] != ~0ull) {
            if (bad_record) *bad_record = status[1] >> 8;
            return ctx->fail(PP_ERR_LIMIT, "pp_bam_index: record %llu has a block_size above 0xFFFFFFF7", (unsigned long long)(status[1] >> 8));
        }
        if ((rc = timer.begin(IX_RECORDS))) return rc;
        hipLaunchKernelGGL(k_ix_rec, dim3(gb), dim3(256), 0, st, n, d_bytes, d_rec_off, (IxRec *)d_rec, (uint16_t *)d_flag, (u64 *)d_st2);
        if ((rc = timer.end())) return rc;
        PP_HIPCHK(ctx, hipGetLastError());
        u64 cig = ~0ull;
        if ((rc = fetch(ctx, d_st2, &cig))) return rc;
        if (cig != ~0ull) {
            if (bad_record) *bad_record = cig >> 8;
            return ctx->fail(PP_ERR_ARG, "pp_bam_index: the CIGAR of record %llu runs past its block_size", (unsigned long long)(cig >> 8));
        }
    }
    if (n_al && !pass) return ctx->fail(PP_ERR_ARG, "pp_bam_index: null pass with %llu aligned records", (unsigned long long)n_al);
    if (n_pass != n_al)
        return ctx->fail(PP_ERR_ARG, "pp_bam_index: %llu verdicts for %llu aligned records", (unsigned long long)n_pass, (unsigned long long)n_al);
    {
        hipLaunchKernelGGL(k_ix_blk, dim3((unsigned)((n_blk + 256u) / 256u)), dim3(256), 0, st, (u64)n_blk + 1u, d_blk, (u64 *)d_st2 + 1);
        PP_HIPCHK(ctx, hipGetLastError());
        u64 far = ~0ull;
        if ((rc = fetch(ctx, (const u64 *)d_st2 + 1, &far))) return rc;
        if (far != ~0ull) return ctx->fail(PP_ERR_LIMIT, "pp_bam_index: block %llu starts at 2^48 or behind: a virtual offset cannot hold it", (unsigned long long)far);
    }
    if ((rc = T.get(ctx, &d_pass, (size_t)n_al))) return rc;
    if (n_al) PP_HIPCHK(ctx, hipMemcpyAsync(d_pass, pass, (size_t)n_al, hipMemcpyHostToDevice, st));
    if (n) {
        if ((rc = timer.begin(IX_SCANS))) return rc;
        hipLaunchKernelGGL(k_tag_len<false>, dim3(nb), dim3(TAG_BLOCK), 0, st, n, d_bytes, d_rec_off, (const u8 *)d_aligned, (const u64 *)d_al_base,
                           (const u8 *)d_pass, (u64)n_head, (u64 *)d_blk2, (u64 *)nullptr);
        hipLaunchKernelGGL(k_colscan<2>, dim3(1), dim3(1024), 0, st, (const u64 *)d_blk2, (u64)nb, (u64 *)d_blk2off);
        hipLaunchKernelGGL(k_tag_len<true>, dim3(nb), dim3(TAG_BLOCK), 0, st, n, d_bytes, d_rec_off, (const u8 *)d_aligned, (const u64 *)d_al_base,
                           (const u8 *)d_pass, (u64)n_head, (u64 *)d_blk2off, (u64 *)d_start);
        if ((rc = timer.end()) || (rc = timer.begin(IX_RECORDS))) return rc;
        hipLaunchKernelGGL(k_ix_check, dim3(gb), dim3(256), 0, st, n, (const IxRec *)d_rec, n_ref, (u32 *)d_bin, (u64 *)d_st2 + 2);
        if ((rc = timer.end())) return rc;
        PP_HIPCHK(ctx, hipGetLastError());
        u64 totals[2] = {0, 0}, bad = ~0ull;
        if ((rc = fetch(ctx, (const u64 *)d_blk2off + 2ull * nb, totals, 2)) || (rc = fetch(ctx, (const u64 *)d_st2 + 2, &bad))) return rc;
        u_total = n_head + 4ull * n + totals[0];
        if (bad != ~0ull) {
            const u32 kind = (u32)(bad & 0xFFu);
            if (bad_record) *bad_record = bad >> 8;
            if (kind == IX_END) return ctx->fail(PP_ERR_LIMIT, "pp_bam_index: record %llu ends behind 2^29: BAI holds positions below 2^29", (unsigned long long)(bad >> 8));
            return ctx->fail(PP_ERR_ARG, "pp_bam_index: record %llu %s", (unsigned long long)(bad >> 8),
                             kind == IX_REF ? "has a reference id outside [-1, n_ref)" : kind == IX_PLACED ? "is placed on a reference at a negative position"
                                                                                                        : "stands in front of the record before it: the records are not in coordinate order");
        }
    }
    if (n_blk != (u_total + PAY - 1u) / PAY)
        return ctx->fail(PP_ERR_ARG, "pp_bam_index: %llu block offsets and one for a stream of %llu bytes, which has %llu blocks", (unsigned long long)n_blk,
                         (unsigned long long)u_total, (unsigned long long)((u_total + PAY - 1u) / PAY));

    // ---- the tables ----
    namespace ih = pp_bam_index_host;
    std::vector<uint64_t> h_key, h_beg, h_end, h_lin, h_lin_off((size_t)n_ref + 1, 0), h_ref[4];
    std::vector<u32> h_intv(n_ref, 0);
    for (auto &v : h_ref) v.assign(n_ref, 0);
    uint64_t n_chunk = 0, no_coor = 0;
    if (n) {
        const IxWhere W{(const u64 *)d_start, d_blk};
        void *d_head, *d_cidx, *d_intv, *d_ref4, *d_nc;
        if ((rc = T.get(ctx, &d_head, (size_t)n * 4)) || (rc = T.get(ctx, &d_cidx, ((size_t)n + 1) * 4)) || (rc = T.get(ctx, &d_intv, (size_t)n_ref * 4)) ||
            (rc = T.get(ctx, &d_ref4, (size_t)n_ref * 32)) || (rc = T.get(ctx, &d_nc, 8)))
            return rc;
        u64 *const d_rb = (u64 *)d_ref4, *const d_re = d_rb + n_ref, *const d_map = d_re + n_ref, *const d_unm = d_map + n_ref;
        PP_HIPCHK(ctx, hipMemsetAsync(d_intv, 0, std::max<size_t>((size_t)n_ref * 4, 16), st));
        PP_HIPCHK(ctx, hipMemsetAsync(d_ref4, 0, std::max<size_t>((size_t)n_ref * 32, 16), st));
        PP_HIPCHK(ctx, hipMemsetAsync(d_nc, 0, 8, st));
        if ((rc = timer.begin(IX_CHUNKS))) return rc;
        hipLaunchKernelGGL(k_ix_run, dim3(gb), dim3(256), 0, st, n, (const IxRec *)d_rec, (const u32 *)d_bin, (u32 *)d_head);
        if ((rc = scan_u32<u32>(ctx, S.sums(), S.sums_off(), (const u32 *)d_head, (u64)n, (u32 *)d_cidx))) return rc;
        if ((rc = timer.end()) || (rc = timer.begin(IX_LINEAR))) return rc;
        hipLaunchKernelGGL(k_ix_ref, dim3(gb), dim3(256), 0, st, n, (const IxRec *)d_rec, (const uint16_t *)d_flag, W, (u32 *)d_intv, d_rb, d_re, d_map, d_unm, (u64 *)d_nc);
        if ((rc = timer.end())) return rc;
        PP_HIPCHK(ctx, hipGetLastError());
        u32 nc32 = 0;
        if ((rc = fetch(ctx, (const u32 *)d_cidx + n, &nc32)) || (rc = fetch(ctx, d_nc, &no_coor))) return rc;
        n_chunk = nc32;
        if (n_ref) {
            if ((rc = fetch(ctx, d_intv, h_intv.data(), n_ref))) return rc;
            for (int k = 0; k < 4; k++)
                if ((rc = fetch(ctx, d_rb + (size_t)k * n_ref, h_ref[k].data(), n_ref))) return rc;
        }
        for (u32 r = 0; r < n_ref; r++) h_lin_off[r + 1] = h_lin_off[r] + h_intv[r];
        const u64 n_win = h_lin_off[n_ref];
        if (n_win > IX_MAX_WINDOWS) return ctx->fail(PP_ERR_LIMIT, "pp_bam_index: %llu windows of 16,384 bases in the linear index, above 2^27", (unsigned long long)n_win);
        // the linear index
        if (n_win) {
            void *d_lin_off, *d_lin;
            if ((rc = T.get(ctx, &d_lin_off, ((size_t)n_ref + 1) * 8)) || (rc = T.get(ctx, &d_lin, (size_t)n_win * 8))) return rc;
            PP_HIPCHK(ctx, hipMemcpyAsync(d_lin_off, h_lin_off.data(), ((size_t)n_ref + 1) * 8, hipMemcpyHostToDevice, st));
            PP_HIPCHK(ctx, hipMemsetAsync(d_lin, 0xFF, (size_t)n_win * 8, st));
            if ((rc = timer.begin(IX_LINEAR))) return rc;
            hipLaunchKernelGGL(k_ix_lin, dim3(gb), dim3(256), 0, st, n, (const IxRec *)d_rec, W, (const u64 *)d_lin_off, (u64 *)d_lin);
            hipLaunchKernelGGL(k_ix_fill, dim3((n_ref + 255u) / 256u), dim3(256), 0, st, n_ref, (const u64 *)d_lin_off, (u64 *)d_lin);
            if ((rc = timer.end())) return rc;
            PP_HIPCHK(ctx, hipGetLastError());
            h_lin.resize((size_t)n_win);
            if ((rc = fetch(ctx, d_lin, h_lin.data(), (size_t)n_win))) return rc;
        }
        // the chunk table, then its order
        if (n_chunk) {
            const u32 m = (u32)n_chunk;
            const unsigned gm = (unsigned)(((u64)m + 255u) / 256u);
            const u32 m_tiles = (u32)(((u64)m + RG_TILE - 1u) / RG_TILE);
            const u64 m_cnt = 256ull * m_tiles;
            void *d_key[2], *d_beg, *d_end, *d_idx[2], *d_cnt, *d_off, *d_sb, *d_se;
            if ((rc = T.get(ctx, &d_key[0], (size_t)m * 8)) || (rc = T.get(ctx, &d_key[1], (size_t)m * 8)) || (rc = T.get(ctx, &d_beg, (size_t)m * 8)) ||
                (rc = T.get(ctx, &d_end, (size_t)m * 8)) || (rc = T.get(ctx, &d_idx[0], (size_t)m * 4)) || (rc = T.get(ctx, &d_idx[1], (size_t)m * 4)) ||
                (rc = T.get(ctx, &d_cnt, (size_t)m_cnt * 4)) || (rc = T.get(ctx, &d_off, (size_t)(m_cnt + 1) * 4)) || (rc = T.get(ctx, &d_sb, (size_t)m * 8)) ||
                (rc = T.get(ctx, &d_se, (size_t)m * 8)))
                return rc;
            if ((rc = timer.begin(IX_CHUNKS))) return rc;
            hipLaunchKernelGGL(k_ix_chunk, dim3(gb), dim3(256), 0, st, n, (const IxRec *)d_rec, (const u32 *)d_bin, (const u32 *)d_head, (const u32 *)d_cidx, W,
                               (u64 *)d_key[0], (u64 *)d_beg, (u64 *)d_end);
            u32 shifts[6], passes = 0;
            shifts[passes++] = 0;
            shifts[passes++] = 8;  // bins are below 2^16
            for (u32 top = n_ref - 1u, b = 0; top; top >>= 8, b++) shifts[passes++] = 32u + 8u * b;
            const u32 *idx_in = nullptr;
            for (u32 p = 0; p < passes; p++) {
                const u64 *const key_in = (const u64 *)d_key[p & 1u];
                u64 *const key_out = (u64 *)d_key[(p + 1u) & 1u];
                u32 *const idx_out = (u32 *)d_idx[p & 1u];
                hipLaunchKernelGGL(k_rg_hist<u64>, dim3(m_tiles), dim3(RG_BLOCK), 0, st, m, key_in, shifts[p], m_tiles, (u32 *)d_cnt);
                if ((rc = scan_u32<u32>(ctx, S.sums(), S.sums_off(), (const u32 *)d_cnt, m_cnt, (u32 *)d_off))) return rc;
                hipLaunchKernelGGL(k_rg_scatter<u64>, dim3(m_tiles), dim3(RG_BLOCK), 0, st, m, key_in, idx_in, shifts[p], m_tiles, (const u32 *)d_off, key_out, idx_out);
                idx_in = idx_out;
            }
            hipLaunchKernelGGL(k_ix_gather, dim3(gm), dim3(256), 0, st, m, idx_in, (const u64 *)d_beg, (const u64 *)d_end, (u64 *)d_sb, (u64 *)d_se);
            if ((rc = timer.end())) return rc;
            PP_HIPCHK(ctx, hipGetLastError());
            h_key.resize(m);
            h_beg.resize(m);
            h_end.resize(m);
            if ((rc = fetch(ctx, d_key[passes & 1u], h_key.data(), m)) || (rc = fetch(ctx, d_sb, h_beg.data(), m)) || (rc = fetch(ctx, d_se, h_end.data(), m))) return rc;
        }
    }
    PP_HIPCHK(ctx, hipStreamSynchronize(st));
    if (timer.on) {
        if ((rc = timer.sums(ctx->ix_ms, 4))) return rc;
        ctx->ix_timed = true;
    }
    ih::Tables Tb;
    Tb.n_ref = n_ref;
    Tb.n_chunk = n_chunk;
    Tb.chunk_key = h_key.data();
    Tb.chunk_beg = h_beg.data();
    Tb.chunk_end = h_end.data();
    Tb.n_intv = h_intv.data();
    Tb.lin_off = h_lin_off.data();
    Tb.lin = h_lin.data();
    Tb.ref_beg = h_ref[0].data();
    Tb.ref_end = h_ref[1].data();
    Tb.mapped = h_ref[2].data();
    Tb.unmapped = h_ref[3].data();
    Tb.n_no_coor = no_coor;
    std::vector<uint8_t> file;
    char msg[200];
    msg[0] = 0;
    if ((rc = ih::serialise(Tb, &file, msg, sizeof msg))) return ctx->fail(rc, "%s", msg);
    bai->data = (uint8_t *)malloc(file.size() + 1);
    if (!bai->data) return ctx->fail(PP_ERR_HIP, "pp_bam_index: out of host memory");
    memcpy(bai->data, file.data(), file.size());
    bai->len = file.size();
    return PP_OK;
}

// (internal hook, not part of the header: tools/bam_sort_timing.py) the HIP-event time of the context's last pp_bam_index by stage:
// scans | records | chunks | linear; PP_ERR_ARG where the context had no profiling on
extern "C" int pp_bam_index_stage_ms_(const pp_ctx *ctx, float *ms4) {
    if (!ctx || !ms4 || !ctx->ix_timed) return PP_ERR_ARG;
    std::copy(ctx->ix_ms, ctx->ix_ms + 4, ms4);
    return PP_OK;
}
