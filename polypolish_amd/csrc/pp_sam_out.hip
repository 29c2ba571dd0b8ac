// pp_sam_out.hip -- pp_sam_tagged: the filter's verdicts written back as SAM TEXT, on the device.  The write side of the record chain
// for a caller who holds text, the text twin of pp_bam_tagged (pp_bam_out.hip): from the text in device memory and one verdict byte
// per aligned record it makes, byte for byte, what pp_filter_write_text makes on the host (pp_filter_host.cpp, write_text_fd; the
// reference's filter_sam, src/filter.rs:309-349) -- every line again, "\tZP:Z:fail" behind the content of the aligned ones that
// failed, every line ended by "\n" -- as bytes in device memory; pp_sam_out_write puts them on disk, pp_bgzf_deflate compresses them.
//
// A line is cut at '\n'; one trailing '\r' is not content.  It is an ALIGNED RECORD when it is not empty, does not begin with '@',
// has a tab, and its second column parses as parse::<u32> with bit 2 clear: write_text_fd's is_aligned, not the eleven columns of
// pp_sam_records.  Nothing else is looked at, nothing can be refused, bytes >= 0x80 are bytes.
//
// The geometry (pp_sam_out_geometry_; the tests aim at these seams):
//   ST_LINES = 1,024    lines per workgroup of pass A
//   ST_TILE  = 16,384   output bytes per workgroup of pass B
//   ST_STORE = 16       bytes per store of pass B, aligned on the OUTPUT
//
//   k_in_nl_count, k_in_nl_write   (pp_textin.h) the newline index, as newline_index of pp_devtext.h (count per 64 KB block, scan, write) but on a
//                 text that is BORROWED: not padded, at any alignment, bytes >= 0x80 welcome.  A thread's 64 bytes are four 16-byte
//                 loads when they lie inside the text, single bytes at the text's end
//   k_st_lines    pass A, one lane per line: the '\r', the predicate (the head of the line up to its second tab, eight bytes per step
//                 where eight lie inside the text), kind[line] = aligned | cr << 1, and the workgroups' numbers of aligned records
//   k_st_off      the aligned rank by the workgroup scan of pp_dev.h over k_colscan's bases, the verdict at that rank, the line's
//                 output length content + 1 + 10 fail, a 64-bit workgroup scan of the lengths (a line may be longer than 4 GB); first
//                 the workgroups' sums of bytes and failures, then off[line], off[n_lines] = the output's size, fail into kind bit 2,
//                 and tile_first[tile] = the line that holds the first byte of pass B's tile: the line whose output covers a multiple
//                 of ST_TILE writes it (a line longer than a tile writes several), so pass B starts without a search
//   k_st_copy     pass B, the hot pass, output-centric: a workgroup owns ST_TILE output bytes.  tile_first gives the line of its first
//                 byte and the line of the first byte behind it; the starts of the lines in between -- in the output, relative to the
//                 tile, the verdict in bit 31, and in the text -- go to LDS (ST_CAP = 2,048 of them; a tile that holds more, almost
//                 nothing but line ends, bisects off[] in memory instead).  Every lane owns four 16-byte pieces of the tile, finds each
//                 piece's line by bisection in LDS and, where the piece lies inside one line's content -- almost all of a file of
//                 300-byte lines -- fetches it with ONE 16-byte load at the source's own alignment: source and destination differ by a
//                 shift that only changes at a failing line, a "\r\n" or a last line without newline.  A piece over a seam takes one
//                 load of at most 16 bytes per line it touches (inside the text: the text's last bytes byte by byte), shifted and
//                 masked into place, the tag and the newline from a constant, as many lines as the piece holds (sixteen "\n" at the
//                 most).  The four pieces go level by level -- lines, then bytes -- so a lane waits for a round trip per level.  A line
//                 longer than a tile simply spans workgroups, a tag cut by a tile or a piece spans two pieces.  Every piece leaves
//                 with one 16-byte aligned store; the output's allocation is rounded up to 16, the last piece's spare bytes are zeros.
// No byte outside [0, n_bytes) of the text is loaded, by a wide load either: every load is checked against the text's size or lies
// inside a line's content.  No kernel keeps a register in scratch memory (.private_segment_fixed_size: 0 for all of them).
#include "pp_textin.h"

#include <cstring>

struct pp_sam_out : DevOwner {
    using DevOwner::DevOwner;
    uint8_t *d_out = nullptr;  // DEVICE: the text
    uint64_t n_out = 0;
    uint64_t pass_count = 0, fail_count = 0, n_lines = 0;
    StageMs<4> t;              // newline index | pass A | the scans | pass B
};

namespace {

constexpr u32 NL_BLOCK = IN_NL_BLOCK;  // bytes of text per workgroup of the newline kernels (pp_textin.h)
constexpr u32 ST_LINES = 1024;    // lines per workgroup of pass A
constexpr u32 ST_TILE = 16384;    // output bytes per workgroup of pass B
constexpr u32 ST_STORE = 16;      // bytes per store of pass B
constexpr u32 ST_THREADS = 256;   // threads of pass B: four pieces each
constexpr u32 ST_TRIPS = ST_TILE / ST_STORE / ST_THREADS;
constexpr u32 ST_CAP = 2048;      // line starts of one tile kept in LDS (and one line end); a tile with more is searched in memory
constexpr u64 TAG_LO = 0x61663A5A3A505A09ull, TAG_HI = 0x0A6C69ull;  // \t Z P : Z : f a | i l \n, low byte first

// ---- pass A ------------------------------------------------------------------------------------------------------------------------
// str::parse::<u32>() of text[a, b) (parse_u of pp_devtext.h on a column of any length), then bit 2 clear
__device__ __forceinline__ bool flag_aligned(const u8 *__restrict__ T, u64 a, u64 b) {
    if (a == b) return false;
    if (T[a] == (u8)'+') { a++; if (a == b) return false; }
    u64 v = 0;
    for (; a < b; a++) {
        const u8 c = T[a];
        if (c < (u8)'0' || c > (u8)'9') return false;
        v = v * 10u + (u64)(c - (u8)'0');
        if (v > 0xFFFFFFFFull) return false;
    }
    return (v & 4u) == 0;
}

__global__ __launch_bounds__(ST_LINES) void k_st_lines(const u8 *__restrict__ T, u64 size, const u64 *__restrict__ nl, u64 n_nl, u64 n_lines,
                                                       u8 *__restrict__ kind, u64 *__restrict__ blk_al) {
    __shared__ u64 s_w[ST_LINES / 64];
    const u64 li = (u64)blockIdx.x * ST_LINES + threadIdx.x;
    u32 al = 0;
    if (li < n_lines) {
        const u64 ls = li ? nl[li - 1] + 1 : 0, le = li < n_nl ? nl[li] : size;
        u64 ce = le;  // the content's end
        if (ce > ls && T[ce - 1] == (u8)'\r') ce--;
        if (ce > ls && T[ls] != (u8)'@') {
            const u64 t1 = find_tab_in(T, size, ls, ce);
            if (t1 < ce) al = flag_aligned(T, t1 + 1, find_tab_in(T, size, t1 + 1, ce)) ? 1u : 0u;
        }
        kind[li] = (u8)(al | (ce != le ? 2u : 0u));
    }
    u64 total;
    (void)block_scan_excl64<ST_LINES>(al, s_w, &total);
    if (threadIdx.x == 0) blk_al[blockIdx.x] = total;
}

// PLACE == false: the workgroups' output bytes and failing records (blk2: two words per workgroup).  PLACE == true: blk2 holds their
// exclusive scan: off[line], off[n_lines], and the line's verdict into kind.
template <bool PLACE>
__global__ __launch_bounds__(ST_LINES) void k_st_off(u64 n_lines, u64 size, const u64 *__restrict__ nl, u64 n_nl, u8 *__restrict__ kind,
                                                     const u64 *__restrict__ al_base, const u8 *__restrict__ pass, u64 *__restrict__ blk2,
                                                     u64 *__restrict__ off, u32 *__restrict__ tile_first) {
    __shared__ u64 s_w[ST_LINES / 64];
    const u64 li = (u64)blockIdx.x * ST_LINES + threadIdx.x;
    const u32 k = li < n_lines ? kind[li] : 0u, al = k & 1u;
    u64 t_al, t_len, t_fail;
    const u64 rank = al_base[blockIdx.x] + block_scan_excl64<ST_LINES>(al, s_w, &t_al);
    const u32 fail = (al && pass[rank] == 0) ? 1u : 0u;
    u64 len = 0;
    if (li < n_lines) {
        const u64 ls = li ? nl[li - 1] + 1 : 0, le = li < n_nl ? nl[li] : size;
        len = le - ls - ((k >> 1) & 1u) + 1u + 10u * fail;
    }
    const u64 ex_len = block_scan_excl_u64<ST_LINES>(len, s_w, &t_len);
    (void)block_scan_excl64<ST_LINES>(fail, s_w, &t_fail);
    u64 *const mine = blk2 + 2ull * blockIdx.x;
    if (!PLACE) {
        if (threadIdx.x == 0) { mine[0] = t_len; mine[1] = t_fail; }
        return;
    }
    if (li >= n_lines) return;
    const u64 s = mine[0] + ex_len, e = s + len;
    off[li] = s;
    if (li + 1 == n_lines) off[n_lines] = e;
    kind[li] = (u8)((k & 3u) | (fail << 2));
    // the tiles of pass B whose first byte this line holds: one now and then, several for a line longer than a tile
    for (u64 tile = (s + ST_TILE - 1u) / ST_TILE; tile * ST_TILE < e; tile++) tile_first[tile] = (u32)li;
}

// ---- pass B ------------------------------------------------------------------------------------------------------------------------
struct CopyArgs {
    const u8 *text;
    u64 size;         // the text's bytes
    const u64 *nl;    // the newline index
    u64 n_nl;
    const u64 *off;   // n_lines + 1 entries: where a line starts in the output
    const u8 *kind;   // aligned | cr << 1 | fail << 2
    const u32 *tile_first;  // the line of every tile's first byte
    u64 n_lines;
    u64 total;        // the output's bytes
    u8 *out;          // ... in an allocation of a multiple of ST_STORE
};

struct Piece16 {  // sixteen bytes of the output, low byte first
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

// Sixteen output bytes from `o` that do not lie inside one line's content: the content's end, the tag, the newline, the lines behind,
// stretch by stretch -- one load of at most 16 bytes per line the piece touches, shifted and masked into place, the tag and the newline
// from the constant.  `l` is the line of the first byte, start / len its place in the output, ls its place in the text.
__device__ __forceinline__ uint4 seam_piece(const CopyArgs &A, u64 o, u64 l, u64 start, u64 len, u64 ls, u32 fail) {
    Piece16 Q{0, 0};
    const u32 want = (u32)min((u64)ST_STORE, A.total - o);  // (the output's last piece may be short: its spare bytes stay zero)
    u32 i = 0;
    while (true) {
        const u64 clen = len - 1u - 10u * fail;
        u64 rel = o + i - start;
        if (rel < clen) {  // content
            const u32 k = (u32)min(clen - rel, (u64)(want - i));
            u64 a, b;
            load16_in(A.text, A.size, ls + rel, k, &a, &b);
            Q.put(a, b, i, i + k);
            i += k;
            rel += k;
        }
        if (i < want) {  // the line's ending: byte rel - clen of "\tZP:Z:fail\n", or of "\n"
            const u32 from = (fail ? 0u : 10u) + (u32)(rel - clen), k = min((u32)(len - rel), want - i), sh = 8u * from;
            const u64 a = from == 0 ? TAG_LO : (from < 8u ? (TAG_LO >> sh) | (TAG_HI << (64u - sh)) : TAG_HI >> (sh - 64u));
            const u64 b = from == 0 ? TAG_HI : (from < 8u ? TAG_HI >> sh : 0ull);
            Q.put(a, b, i, i + k);
            i += k;
        }
        if (i >= want) break;
        l++;  // (the output goes on, so there is a next line)
        ls = A.nl[l - 1] + 1;
        start += len;
        len = A.off[l + 1] - start;
        fail = ((u32)A.kind[l] >> 2) & 1u;
    }
    return make_uint4((u32)Q.lo, (u32)(Q.lo >> 32), (u32)Q.hi, (u32)(Q.hi >> 32));
}

__global__ __launch_bounds__(ST_THREADS) void k_st_copy(CopyArgs A) {
    __shared__ u32 s_out[ST_CAP], s_src[ST_CAP];
    const u8 *__restrict__ const T = A.text;
    const u64 *__restrict__ const off = A.off;
    const u32 t = threadIdx.x;
    const u64 t0 = (u64)blockIdx.x * ST_TILE, t1 = min(A.total, t0 + (u64)ST_TILE);
    // ---- the tile's lines: l_lo holds its first byte, l_hi the first byte behind it (the last line, for the last tile)
    const u64 l_lo = A.tile_first[blockIdx.x], l_hi = blockIdx.x + 1u < gridDim.x ? (u64)A.tile_first[blockIdx.x + 1u] : A.n_lines - 1u;
    const u32 n_in = (u32)(l_hi - l_lo);  // the lines behind l_lo that may start inside the tile
    const bool in_lds = n_in < ST_CAP;
    const u64 start0 = off[l_lo], ls0 = l_lo ? A.nl[l_lo - 1] + 1 : 0, src1 = n_in ? A.nl[l_lo] + 1 : 0;  // (src1: where line l_lo + 1 starts in the text)
    const u32 fail0 = ((u32)A.kind[l_lo] >> 2) & 1u;
    if (in_lds) {
        // s_out[k]: where line l_lo + 1 + k starts, from the tile's first byte (1 .. ST_TILE; behind l_hi: where l_hi ends, cut to 31 bits),
        // its verdict in bit 31; s_src[k]: where it starts in the text, from src1.  One entry more than lines: the end of l_hi
        for (u32 k = t; k <= n_in; k += ST_THREADS) {
            const u64 L = l_lo + 1u + k;
            const u32 f = L < A.n_lines ? ((u32)A.kind[L] >> 2) & 1u : 0u;
            s_out[k] = (u32)min(off[L] - t0, (u64)0x7FFFFFFFu) | (f << 31);
            s_src[k] = L - 1u < A.n_nl ? (u32)(A.nl[L - 1u] + 1u - src1) : 0u;
        }
        __syncthreads();
    }
    u64 o[ST_TRIPS], l[ST_TRIPS], start[ST_TRIPS], len[ST_TRIPS], ls[ST_TRIPS];
    u32 fail[ST_TRIPS];
#pragma unroll
    for (u32 j = 0; j < ST_TRIPS; j++) o[j] = t0 + (u64)ST_STORE * (t + j * ST_THREADS);
    if (in_lds) {
#pragma unroll
        for (u32 j = 0; j < ST_TRIPS; j++) {
            const u32 q = (u32)(min(o[j], t1 - 1u) - t0);
            u32 at = 0, n = n_in;  // the number of lines behind l_lo that start at or below q
            while (n) {
                const u32 half = n >> 1;
                if ((s_out[at + half] & 0x7FFFFFFFu) <= q) { at += half + 1u; n -= half + 1u; }
                else n = half;
            }
            const u32 mine = at ? s_out[at - 1u] : 0u, next = s_out[at] & 0x7FFFFFFFu;
            l[j] = l_lo + at;
            start[j] = at ? t0 + (mine & 0x7FFFFFFFu) : start0;
            len[j] = t0 + next - start[j];
            ls[j] = at ? src1 + s_src[at - 1u] : ls0;
            fail[j] = at ? mine >> 31 : fail0;
        }
    } else {
        // more lines than the table holds (a tile of almost nothing but line ends): bisection in off[] itself, the pieces' steps together
#pragma unroll
        for (u32 j = 0; j < ST_TRIPS; j++) l[j] = l_lo;
        for (u64 n = l_hi - l_lo + 1u; n > 1u;) {  // the piece's first byte lies in a line of [l, l + n); a piece behind the tile ends at l_hi
            const u64 half = n >> 1;
#pragma unroll
            for (u32 j = 0; j < ST_TRIPS; j++)
                if (off[l[j] + half] <= o[j]) l[j] += half;
            n -= half;
        }
#pragma unroll
        for (u32 j = 0; j < ST_TRIPS; j++) {
            start[j] = off[l[j]];
            len[j] = off[l[j] + 1] - start[j];
            ls[j] = l[j] ? A.nl[l[j] - 1] + 1 : 0;
            fail[j] = ((u32)A.kind[l[j]] >> 2) & 1u;
        }
    }
    uint4 v[ST_TRIPS];
    u32 fast = 0;
#pragma unroll
    for (u32 j = 0; j < ST_TRIPS; j++) {
        const u64 clen = len[j] - 1u - 10u * fail[j], rel = o[j] - start[j];  // the content's length; the piece's first byte in the line's output
        v[j] = make_uint4(0, 0, 0, 0);
        if (o[j] < t1 && rel + ST_STORE <= clen) {  // inside the content: one load at the source's alignment
            __builtin_memcpy(&v[j], T + ls[j] + rel, 16);
            fast |= 1u << j;
        }
    }
#pragma unroll
    for (u32 j = 0; j < ST_TRIPS; j++) {
        if (o[j] >= t1) break;
        if (!((fast >> j) & 1u)) v[j] = seam_piece(A, o[j], l[j], start[j], len[j], ls[j], fail[j]);
        *(uint4 *)(A.out + o[j]) = v[j];
    }
}

int tagged(pp_ctx *ctx, const char *who, const uint8_t *text, uint64_t n_bytes, int mem, const uint8_t *pass, uint64_t n_pass, pp_sam_out **out) {
    PP_HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const u64 size = n_bytes;
    std::unique_ptr<pp_sam_out> P(new pp_sam_out(ctx));
    CallScratch T;  // the copy of host text, the index and the per-line arrays: released when the call returns
    StageTimer timer(ctx, ctx->profiling != 0 && size != 0);
    int rc;
    auto verdicts = [&](u64 n_al) {
        if (n_al && !pass) return ctx->fail(PP_ERR_ARG, "%s: null pass with %llu aligned records", who, (unsigned long long)n_al);
        if (n_pass != n_al)
            return ctx->fail(PP_ERR_ARG, "%s: %llu verdicts for %llu aligned records", who, (unsigned long long)n_pass, (unsigned long long)n_al);
        return (int)PP_OK;
    };
    if (size == 0) {  // no text: no bytes
        if ((rc = verdicts(0)) || (rc = P->alloc(P->d_out, ST_STORE))) return rc;
        PP_HIPCHK(ctx, hipStreamSynchronize(st));
        *out = P.release();
        return PP_OK;
    }
    const u8 *d_text = nullptr;
    if ((rc = on_device(ctx, T, mem, (const u8 *)text, (size_t)size, &d_text))) return rc;

    // ---- the newline index ----
    const u64 n_blk = (size + NL_BLOCK - 1) / NL_BLOCK;
    void *d_blk, *d_blkoff, *d_nl;
    if ((rc = T.get(ctx, &d_blk, (size_t)n_blk * 4)) || (rc = T.get(ctx, &d_blkoff, ((size_t)n_blk + 1) * 8))) return rc;
    if ((rc = timer.begin(0))) return rc;
    hipLaunchKernelGGL(k_in_nl_count<false>, dim3((unsigned)n_blk), dim3(1024), 0, st, d_text, size, (u32 *)d_blk);
    hipLaunchKernelGGL(k_tscan<u64>, dim3(1), dim3(1024), 0, st, (const u32 *)d_blk, n_blk, (u64 *)d_blkoff);
    if ((rc = timer.end())) return rc;
    PP_HIPCHK(ctx, hipGetLastError());
    u64 n_nl = 0;
    u8 last = 0;
    if ((rc = fetch(ctx, (const u64 *)d_blkoff + n_blk, &n_nl)) || (rc = fetch(ctx, d_text + size - 1, &last))) return rc;
    const u64 n_lines = n_nl + (last != (u8)'\n' ? 1 : 0);
    if (n_lines >= 0xFFFFFFFFull) return ctx->fail(PP_ERR_LIMIT, "%s: 2^32-1 or more lines in one text", who);
    if ((rc = T.get(ctx, &d_nl, (size_t)std::max<u64>(1, n_nl) * 8)) || (rc = timer.begin(0))) return rc;
    hipLaunchKernelGGL(k_in_nl_write, dim3((unsigned)n_blk), dim3(1024), 0, st, d_text, size, (const u64 *)d_blkoff, (u64 *)d_nl);
    if ((rc = timer.end())) return rc;

    // ---- pass A: the aligned records ----
    const u32 nb = (u32)((n_lines + ST_LINES - 1) / ST_LINES);
    const u64 max_tiles = (size + 11u * n_lines) / ST_TILE + 1u;  // (the output has at most 11 bytes more than the text per line)
    void *d_kind, *d_blk_al, *d_al_base, *d_blk2, *d_blk2off, *d_off, *d_tile, *d_pass;
    if ((rc = T.get(ctx, &d_kind, (size_t)n_lines)) || (rc = T.get(ctx, &d_blk_al, (size_t)nb * 8)) || (rc = T.get(ctx, &d_al_base, ((size_t)nb + 1) * 8)) ||
        (rc = T.get(ctx, &d_blk2, (size_t)nb * 16)) || (rc = T.get(ctx, &d_blk2off, ((size_t)nb + 1) * 16)) || (rc = T.get(ctx, &d_off, ((size_t)n_lines + 1) * 8)) ||
        (rc = T.get(ctx, &d_tile, (size_t)max_tiles * 4)))
        return rc;
    if ((rc = timer.begin(1))) return rc;
    hipLaunchKernelGGL(k_st_lines, dim3(nb), dim3(ST_LINES), 0, st, d_text, size, (const u64 *)d_nl, n_nl, n_lines, (u8 *)d_kind, (u64 *)d_blk_al);
    if ((rc = timer.end()) || (rc = timer.begin(2))) return rc;
    hipLaunchKernelGGL(k_colscan<1>, dim3(1), dim3(1024), 0, st, (const u64 *)d_blk_al, (u64)nb, (u64 *)d_al_base);
    if ((rc = timer.end())) return rc;
    PP_HIPCHK(ctx, hipGetLastError());
    u64 n_al = 0;
    if ((rc = fetch(ctx, (const u64 *)d_al_base + nb, &n_al)) || (rc = verdicts(n_al))) return rc;

    // ---- the verdicts (host memory whatever `mem`), the lengths, the offsets ----
    if ((rc = T.get(ctx, &d_pass, (size_t)n_al))) return rc;
    if (n_al) PP_HIPCHK(ctx, hipMemcpyAsync(d_pass, pass, (size_t)n_al, hipMemcpyHostToDevice, st));
    if ((rc = timer.begin(2))) return rc;
    hipLaunchKernelGGL(k_st_off<false>, dim3(nb), dim3(ST_LINES), 0, st, n_lines, size, (const u64 *)d_nl, n_nl, (u8 *)d_kind, (const u64 *)d_al_base,
                       (const u8 *)d_pass, (u64 *)d_blk2, (u64 *)nullptr, (u32 *)nullptr);
    hipLaunchKernelGGL(k_colscan<2>, dim3(1), dim3(1024), 0, st, (const u64 *)d_blk2, (u64)nb, (u64 *)d_blk2off);
    hipLaunchKernelGGL(k_st_off<true>, dim3(nb), dim3(ST_LINES), 0, st, n_lines, size, (const u64 *)d_nl, n_nl, (u8 *)d_kind, (const u64 *)d_al_base,
                       (const u8 *)d_pass, (u64 *)d_blk2off, (u64 *)d_off, (u32 *)d_tile);
    if ((rc = timer.end())) return rc;
    PP_HIPCHK(ctx, hipGetLastError());
    u64 totals[2] = {0, 0};
    if ((rc = fetch(ctx, (const u64 *)d_blk2off + 2ull * nb, totals, 2))) return rc;
    const u64 total = totals[0];

    // ---- pass B: the bytes ----
    P->n_out = total;
    P->n_lines = n_lines;
    P->pass_count = n_al - totals[1];
    P->fail_count = totals[1];
    if ((rc = P->alloc(P->d_out, (size_t)((total + ST_STORE - 1) / ST_STORE * ST_STORE)))) return rc;
    if ((rc = timer.begin(3))) return rc;
    hipLaunchKernelGGL(k_st_copy, dim3((unsigned)((total + ST_TILE - 1) / ST_TILE)), dim3(ST_THREADS), 0, st,
                       CopyArgs{d_text, size, (const u64 *)d_nl, n_nl, (const u64 *)d_off, (const u8 *)d_kind, (const u32 *)d_tile, n_lines, total, (u8 *)P->d_out});
    if ((rc = timer.end())) return rc;
    PP_HIPCHK(ctx, hipGetLastError());
    PP_HIPCHK(ctx, hipStreamSynchronize(st));  // the caller's text may be released, the scratch goes away
    if ((rc = P->t.take(timer))) return rc;
    *out = P.release();
    return PP_OK;
}

}  // namespace

extern "C" void pp_sam_out_free(pp_sam_out *o) { delete o; }

extern "C" void pp_sam_out_bytes(const pp_sam_out *o, const uint8_t **dev, uint64_t *n_bytes) {
    if (dev) *dev = o ? o->d_out : nullptr;
    if (n_bytes) *n_bytes = o ? o->n_out : 0;
}

extern "C" void pp_sam_out_counts(const pp_sam_out *o, uint64_t *pass_count, uint64_t *fail_count, uint64_t *n_lines) {
    if (pass_count) *pass_count = o ? o->pass_count : 0;
    if (fail_count) *fail_count = o ? o->fail_count : 0;
    if (n_lines) *n_lines = o ? o->n_lines : 0;
}

extern "C" int pp_sam_out_kernel_ms(const pp_sam_out *o, float *ms) {
    return o ? o->t.total(o->ctx, "pp_sam_out_kernel_ms", "when the text was tagged", ms) : PP_ERR_ARG;
}

// (internal hooks, not part of the header: tools/sam_tag_timing.py, the tests) the same time by stage: newline index | pass A | the
// scans | pass B; the geometry: lines per workgroup of pass A, output bytes per workgroup of pass B, bytes per store
extern "C" int pp_sam_out_stage_ms_(const pp_sam_out *o, float *ms4) { return o ? o->t.stages(ms4) : PP_ERR_ARG; }
extern "C" void pp_sam_out_geometry_(uint32_t *lines, uint32_t *tile, uint32_t *store) {
    if (lines) *lines = ST_LINES;
    if (tile) *tile = ST_TILE;
    if (store) *store = ST_STORE;
}

// (internal, pp_bam_sam.hip: the link that makes the same object from BAM) an object with room for `alloc` bytes of text in device
// memory, then what it holds; ms4: the stage times, or null where the context had no profiling on
extern "C" int pp_sam_out_new_(pp_ctx *ctx, uint64_t alloc, pp_sam_out **out, uint8_t **d_out) {
    std::unique_ptr<pp_sam_out> P(new pp_sam_out(ctx));
    if (int rc = P->alloc(P->d_out, (size_t)std::max<uint64_t>(alloc, ST_STORE))) return rc;
    *d_out = P->d_out;
    *out = P.release();
    return PP_OK;
}
extern "C" void pp_sam_out_set_(pp_sam_out *o, uint64_t n_out, uint64_t pass_count, uint64_t fail_count, uint64_t n_lines, const float *ms4) {
    o->n_out = n_out;
    o->pass_count = pass_count;
    o->fail_count = fail_count;
    o->n_lines = n_lines;
    o->t.timed = ms4 != nullptr;
    if (ms4) std::copy(ms4, ms4 + 4, o->t.ms);
}

extern "C" int pp_sam_out_write(const pp_sam_out *o, const char *path) {
    if (!o || !o->ctx) return PP_ERR_ARG;
    if (!path) return o->ctx->fail(PP_ERR_ARG, "pp_sam_out_write: null argument");
    return pp::write_device_file(o->ctx, "pp_sam_out_write", o->d_out, o->n_out, path);
}

extern "C" int pp_sam_tagged(pp_ctx *ctx, const uint8_t *text, uint64_t n_bytes, int mem, const uint8_t *pass, uint64_t n_pass, pp_sam_out **out) {
    if (!ctx) return PP_ERR_ARG;
    if (int rdy = pp_ctx_wait(ctx)) return rdy;
    if (!out) return ctx->fail(PP_ERR_ARG, "pp_sam_tagged: null argument");
    *out = nullptr;
    if (mem != PP_MEM_HOST && mem != PP_MEM_DEVICE)
        return ctx->fail(PP_ERR_ARG, "pp_sam_tagged: the text must be host memory or memory of the context's device");
    if (n_bytes && !text) return ctx->fail(PP_ERR_ARG, "pp_sam_tagged: null text with n_bytes > 0");
    if (n_bytes >= (1ull << 40)) return ctx->fail(PP_ERR_LIMIT, "pp_sam_tagged: 2^40 or more bytes in one call");
    return tagged(ctx, "pp_sam_tagged", text, n_bytes, mem, pass, n_pass, out);
}

extern "C" int pp_sam_tagged_records(pp_ctx *ctx, const pp_sam *s, const uint8_t *pass, uint64_t n_pass, pp_sam_out **out) {
    if (!ctx) return PP_ERR_ARG;
    if (int rdy = pp_ctx_wait(ctx)) return rdy;
    if (!out) return ctx->fail(PP_ERR_ARG, "pp_sam_tagged_records: null argument");
    *out = nullptr;
    if (!s) return ctx->fail(PP_ERR_ARG, "pp_sam_tagged_records: null argument");
    const uint8_t *text = nullptr;  // the object's own device copy of the text
    uint64_t n_bytes = 0;
    pp_sam_names(s, &text, &n_bytes, nullptr, nullptr);
    return tagged(ctx, "pp_sam_tagged_records", text, n_bytes, PP_MEM_DEVICE, pass, n_pass, out);
}
