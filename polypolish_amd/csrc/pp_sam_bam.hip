// pp_sam_bam.hip -- pp_sam_header and pp_sam_bam: SAM TEXT encoded as uncompressed BAM, on the device.  The link of the record chain
// that turns one format into the other: its output (the bytes, records_at, rec_off, all in device memory) is exactly what
// pp_bam_records, pp_bam_walk_device and pp_bam_tagged take with PP_MEM_DEVICE, so pp_bam_tagged -> pp_bam_out_deflate ->
// pp_bgzf_out_write finish a compressed BAM file from text.  The bytes are defined by include/polypolish_hip.h and restated by a plain
// model, tests/sam_bam_model.py.  The text is BORROWED (pp_textin.h): no byte outside [0, n_bytes) is loaded, by a wide load either.
//
// The geometry (pp_sam_bam_geometry_; the tests aim at these seams):
//   SB_LINES = 1,024    lines per workgroup of the placing kernel
//   SB_TILE  = 16,384   output bytes per workgroup of pass B
//   SB_STORE = 16       bytes per store of pass B, aligned on the OUTPUT
//
//   k_in_nl_count, k_in_nl_write   (pp_textin.h) the newline index; the count also notices a byte >= 0x80
//   k_sb_scan     pass A, one lane per line, the wave's 64 lines through LDS (stage_lines_in: the stage of pp_devtext.h in its three
//                 sizes, filled with loads that stay inside the text; a line that does not fit is read where it lies, byte by byte).
//                 The lane validates its line in the order the header gives, notes the columns' offsets, l_read_name, n_cigar_op,
//                 l_seq, the aux bytes (the aux walk with a counting emitter), the bin and the record's size, and reports a refusal as
//                 status = line << 16 | why << 8 | aux field by atomicMin: the first line in file order wins, whatever its kind
//   k_sb_off      record index and a 64-bit scan of 4 + block_size (sums per workgroup, k_colscan over them); PLACE: rec_off, the line
//                 of every record, the RNAME / RNEXT ranges for pp_names_ids, and tile_first[tile] = the record that holds the first
//                 byte of pass B's tile.  The pass without PLACE also refuses a line that begins with '@' behind the first record
//   pp_names_ids  the existing link, on a table seeded with the SN names in header order: id < n_ref is the refID
//   k_sb_refid    "*" -> -1, "=" -> the record's refID, a name no @SQ line has -> a refusal
//   k_sb_emit     pass B, the hot pass, output-centric: a workgroup owns SB_TILE output bytes as an image in LDS.  The image starts as
//                 zeros and the header's bytes; then, each in its own loop: (1) one lane per record writes what is serial by nature --
//                 the nine fixed words, the CIGAR words, the aux fields (the same walk with a writing emitter); (2) half a wave per
//                 record packs the name, the nibbles (16 text bytes from one load make 8 bytes) and QUAL (16 bytes less 33 in one
//                 step); (3) the image leaves through 16-byte stores aligned on the output.  A record longer than a tile spans
//                 workgroups: every write into the image is clipped to the tile.
// No kernel keeps a register in scratch memory.
#include "pp_devtext.h"
#include "pp_textin.h"
#include "pp_sam_host.h"

#include <cstring>
#include <string>

extern "C" char *pp_bam_msg_buf_(size_t *cap);  // pp_bam.hip: the per-thread message behind pp_bam_last_error()

struct pp_bam_enc : DevOwner {
    using DevOwner::DevOwner;
    uint8_t *d_out = nullptr;   // DEVICE: uncompressed BAM
    uint64_t n_out = 0, records_at = 0, n_rec = 0;
    u64 *rec_off = nullptr;     // DEVICE: n_rec + 1 entries
    StageMs<5> t;               // newline index | pass A | the names | the scans | pass B
};

namespace {

typedef int32_t i32;
typedef long long i64;

constexpr u32 SB_LINES = 1024;   // lines per workgroup of the placing kernel
constexpr u32 SB_TILE = 16384;   // output bytes per workgroup of pass B
constexpr u32 SB_STORE = 16;     // bytes per store of pass B
constexpr u32 SB_THREADS = 256;  // threads of pass B
enum : u32 { LK_SKIP = 0, LK_RECORD = 1, LK_AT = 2 };  // kind[line]; LK_AT: begins with '@' behind the header
// why a line is refused, in the order a line is looked at; QUIT or LIMIT by the table why_code below
enum : u32 { W_LONG = 1, W_COLS, W_QNAME, W_FLAG_NUM, W_FLAG, W_POS_NUM, W_POS, W_MAPQ_NUM, W_MAPQ, W_CIGAR, W_CIGAR_RUN, W_CIGAR_MANY,
             W_PNEXT_NUM, W_PNEXT, W_TLEN_NUM, W_TLEN, W_SEQ, W_QUAL, W_BIN, W_AUX, W_AUX_LIMIT, W_SIZE, W_RNAME, W_RNEXT, W_AT };

struct SbLine {  // one record line; offsets relative to the start of the line
    u32 len, name_len, rname_off, rname_len, cig_off, n_cig, rnext_off, rnext_len;
    u32 seq_off, l_seq, qual_off /* 0: "*" */, aux_off /* 0: no aux column */, aux_bytes, size /* 4 + block_size */;
    i32 pos, next_pos, tlen;
    u32 flag_mapq /* flag | mapq << 16 */, bin, pad;
};

__device__ const double POW10[23] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};

// ---- small parsers (L may be LDS or global memory) ----------------------------------------------------------------------------------
// [+]digits: 0 = ok, 1 = not a number, 2 = above max (max < 2^60)
__device__ __forceinline__ u32 num_u(const u8 *s, u32 n, u64 max, u64 &out) {
    u32 i = (n && s[0] == (u8)'+') ? 1u : 0u;
    if (i == n) return 1;
    u64 v = 0;
    bool big = false;
    for (; i < n; i++) {
        const u32 d = (u32)s[i] - (u32)'0';
        if (d > 9u) return 1;
        v = v * 10u + d;
        if (v > max) { big = true; v = max + 1u; }
    }
    out = v;
    return big ? 2u : 0u;
}
// [+-]digits in [lo, hi] (|lo|, hi < 2^60): 0 = ok, 1 = not a number, 2 = outside
__device__ __forceinline__ u32 num_s(const u8 *s, u32 n, i64 lo, i64 hi, i64 &out) {
    const bool neg = n && s[0] == (u8)'-';
    const u32 i = (n && (s[0] == (u8)'+' || neg)) ? 1u : 0u;
    if (i == n) return 1;
    u64 v = 0;
    for (u32 k = i; k < n; k++) {
        if ((u32)s[k] - (u32)'0' > 9u) return 1;
    }
    const u32 r = num_u(s + i, n - i, 1ull << 60, v);
    if (r) return r;
    const i64 x = neg ? -(i64)v : (i64)v;
    if (x < lo || x > hi) return 2;
    out = x;
    return 0;
}

// =ACMGRSVTWYHKDBN in either case -> 0 .. 15; 16 for any other byte
__device__ __forceinline__ u32 nib(u32 c) {
    if (c == (u32)'=') return 0;
    const u32 i = (c | 0x20u) - (u32)'a';
    if (c < (u32)'A' || i > 25u || !((0x16E34CFu >> i) & 1u)) return 16;
    return (u32)((i < 16u ? 0x00F30C00B400D2E1ull >> (4u * i) : 0x0A09708650ull >> (4u * (i - 16u))) & 15ull);
}

// the header's float rule on s[0, n): the float's bits, or false
__device__ __forceinline__ bool float_bits(const u8 *s, u32 n, u32 *bits) {
    u32 at = 0;
    const bool neg = n && s[0] == (u8)'-';
    if (n && (s[0] == (u8)'+' || neg)) at = 1;
    u64 w = 0;
    u32 nd = 0, frac = 0;  // nd: digits of w once its leading zeros are gone
    u32 st = at;
    for (; at < n && (u32)s[at] - (u32)'0' <= 9u; at++) {
        w = nd < 16u ? w * 10u + ((u32)s[at] - (u32)'0') : w;
        nd += (w || nd) ? 1u : 0u;
    }
    if (at == st) return false;
    if (at < n && s[at] == (u8)'.') {
        st = ++at;
        for (; at < n && (u32)s[at] - (u32)'0' <= 9u; at++) {
            w = nd < 16u ? w * 10u + ((u32)s[at] - (u32)'0') : w;
            nd += (w || nd) ? 1u : 0u;
        }
        if (at == st) return false;
        frac = at - st;
    }
    i64 ex = 0;
    if (at < n && (s[at] | 0x20u) == (u8)'e') {
        at++;
        const bool eneg = at < n && s[at] == (u8)'-';
        if (at < n && (s[at] == (u8)'+' || eneg)) at++;
        st = at;
        for (; at < n && (u32)s[at] - (u32)'0' <= 9u; at++) ex = ex < 100000 ? ex * 10 + (i64)((u32)s[at] - (u32)'0') : ex;
        if (at == st) return false;
        if (eneg) ex = -ex;
    }
    if (at != n) return false;
    if (w == 0) { *bits = neg ? 0x80000000u : 0u; return true; }
    const i64 e10 = ex - (i64)frac;
    if (nd > 15u || e10 > 22 || e10 < -22) return false;
    const double d = e10 >= 0 ? (double)w * POW10[e10] : (double)w / POW10[-e10];
    *bits = __float_as_uint((float)d) | (neg ? 0x80000000u : 0u);
    return true;
}

// ---- the aux walk: one field f[0, n) -> its BAM bytes through the emitter E (put(v, k): the k <= 8 low bytes of v) -------------------
struct AuxCount {
    u64 n = 0;
    __device__ __forceinline__ void put(u64, u32 k) { n += k; }
};
struct ImgPut {  // bytes into the tile's image at `pos` (relative to the tile, may lie outside it on either side): clipped
    u8 *img;
    i64 pos;
    __device__ __forceinline__ void put(u64 v, u32 k) {
        for (u32 j = 0; j < k; j++) {
            const i64 p = pos + j;
            if (p >= 0 && p < (i64)SB_TILE) img[p] = (u8)(v >> (8u * j));
        }
        pos += k;
    }
};

template <class E>
__device__ __forceinline__ u32 aux_int(E &e, u32 sub, i64 v) {  // one value of type `sub`
    const u32 k = (sub | 0x20u) == (u32)'c' ? 1u : ((sub | 0x20u) == (u32)'s' ? 2u : 4u);
    e.put((u64)v, k);
    return 0;
}

// 0, W_AUX or W_AUX_LIMIT
template <class E>
__device__ __forceinline__ u32 aux_field(E &e, const u8 *f, u32 n) {
    if (n < 5u || f[2] != (u8)':' || f[4] != (u8)':') return W_AUX;
    const u32 ty = f[3];
    const u8 *v = f + 5;
    const u32 vn = n - 5u;
    const u64 tag = (u64)f[0] | (u64)f[1] << 8;
    switch (ty) {
    case 'A':
        if (vn != 1u) return W_AUX;
        e.put(tag | (u64)'A' << 16 | (u64)v[0] << 24, 4);
        return 0;
    case 'i': {
        i64 x = 0;
        const u32 r = num_s(v, vn, -(1ll << 31), (1ll << 32) - 1, x);
        if (r) return r == 1u ? W_AUX : W_AUX_LIMIT;
        const u32 t = x >= 0 ? (x <= 255 ? 'C' : (x <= 65535 ? 'S' : 'I')) : (x >= -128 ? 'c' : (x >= -32768 ? 's' : 'i'));
        e.put(tag | (u64)t << 16, 3);
        return aux_int(e, t, x);
    }
    case 'Z':
    case 'H':
        if (ty == 'H') {
            if (vn & 1u) return W_AUX;
            for (u32 k = 0; k < vn; k++) {
                const u32 c = v[k], l = (c | 0x20u) - (u32)'a';
                if (!(c - (u32)'0' <= 9u || (l <= 5u && c >= (u32)'A'))) return W_AUX;
            }
        }
        e.put(tag | (u64)ty << 16, 3);
        for (u32 k = 0; k < vn; k++) e.put(v[k], 1);
        e.put(0, 1);
        return 0;
    case 'f': {
        u32 bits;
        if (!float_bits(v, vn, &bits)) return W_AUX_LIMIT;
        e.put(tag | (u64)'f' << 16 | (u64)bits << 24, 7);
        return 0;
    }
    case 'B': {
        if (vn == 0u) return W_AUX;
        const u32 sub = v[0];
        i64 lo, hi;
        switch (sub) {
        case 'c': lo = -128; hi = 127; break;
        case 'C': lo = 0; hi = 255; break;
        case 's': lo = -32768; hi = 32767; break;
        case 'S': lo = 0; hi = 65535; break;
        case 'i': lo = -(1ll << 31); hi = (1ll << 31) - 1; break;
        case 'I': lo = 0; hi = (1ll << 32) - 1; break;
        case 'f': lo = hi = 0; break;
        default: return W_AUX;
        }
        if (vn > 1u && v[1] != (u8)',') return W_AUX;
        u32 count = 0;  // the elements: one more than the commas behind the sub-type
        for (u32 k = 1; k < vn; k++) count += v[k] == (u8)',' ? 1u : 0u;
        e.put(tag | (u64)'B' << 16 | (u64)sub << 24 | (u64)count << 32, 8);
        u32 at = 2;
        for (u32 c = 0; c < count; c++) {
            u32 end = at;
            while (end < vn && v[end] != (u8)',') end++;
            if (end == at) return W_AUX;
            if (sub == (u32)'f') {
                u32 bits;
                if (!float_bits(v + at, end - at, &bits)) return W_AUX_LIMIT;
                e.put(bits, 4);
            } else {
                i64 x = 0;
                if (num_s(v + at, end - at, lo, hi, x)) return W_AUX;
                aux_int(e, sub, x);
            }
            at = end + 1u;
        }
        return 0;
    }
    default: return W_AUX;
    }
}

// the first '\t' in L[from, n), or n: eight bytes per step where the line lies in the stage (its copy runs past the line), else bytes
__device__ __forceinline__ u32 tab_from(const u8 *L, u32 from, u32 n, bool wide) {
    if (wide) return find_tab(L, from, n);
    while (from < n && L[from] != (u8)'\t') from++;
    return from;
}

// ---- pass A --------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ u32 reg2bin(i64 pos, i64 end) {
    end--;
    if (pos >> 14 == end >> 14) return (u32)(4681 + (pos >> 14));
    if (pos >> 17 == end >> 17) return (u32)(585 + (pos >> 17));
    if (pos >> 20 == end >> 20) return (u32)(73 + (pos >> 20));
    if (pos >> 23 == end >> 23) return (u32)(9 + (pos >> 23));
    if (pos >> 26 == end >> 26) return (u32)(1 + (pos >> 26));
    return 0;
}

// the checks of one record line in the header's order: 0 and *out, or why << 8 | aux field
__device__ __forceinline__ u32 sb_parse_line(const u8 *L, u32 n, bool wide, SbLine *out) {
    u32 cs[11], cl[11], nc = 0, q = 0;
#pragma unroll
    for (u32 c = 0; c < 11u; c++) {
        if (q <= n) {
            const u32 t = tab_from(L, q, n, wide);
            cs[c] = q;
            cl[c] = t - q;
            nc++;
            q = t + 1u;  // (n + 1 behind the last column)
        } else {
            cs[c] = cl[c] = 0;
        }
    }
    if (nc < 11u) return W_COLS << 8;
    if (cl[0] == 0u || cl[0] > 254u) return W_QNAME << 8;
    u64 flag, pos, mapq, pnext;
    u32 r;
    if ((r = num_u(L + cs[1], cl[1], 0xFFFFu, flag))) return (r == 1u ? W_FLAG_NUM : W_FLAG) << 8;
    if ((r = num_u(L + cs[3], cl[3], 1ull << 31, pos))) return (r == 1u ? W_POS_NUM : W_POS) << 8;
    if ((r = num_u(L + cs[4], cl[4], 255u, mapq))) return (r == 1u ? W_MAPQ_NUM : W_MAPQ) << 8;
    // the CIGAR: runs of digits and one of MIDNSHP=X
    u32 n_cig = 0;
    u64 ref = 0;
    {
        const u8 *cg = L + cs[5];
        const u32 cgl = cl[5];
        if (!(cgl == 1u && cg[0] == (u8)'*')) {
            u32 i = 0;
            while (i < cgl) {
                u32 j = i;
                while (j < cgl && (u32)cg[j] - (u32)'0' <= 9u) j++;
                const int op = j < cgl ? op_code(cg[j]) : -1;
                if (j == i || op < 0) return W_CIGAR << 8;
                u64 num = 0;
                (void)num_u(cg + i, j - i, (1ull << 28) - 1u, num);
                if (num == 0 || num >= (1ull << 28)) return W_CIGAR_RUN << 8;
                if (op == PP_OP_M || op == PP_OP_D || op == PP_OP_N || op == PP_OP_EQ || op == PP_OP_X) ref += num;
                n_cig++;  // (below 2^31: the line has fewer bytes)
                i = j + 1u;
            }
            if (n_cig > 65535u) return W_CIGAR_MANY << 8;
        }
    }
    if ((r = num_u(L + cs[7], cl[7], 1ull << 31, pnext))) return (r == 1u ? W_PNEXT_NUM : W_PNEXT) << 8;
    i64 tlen = 0;
    if ((r = num_s(L + cs[8], cl[8], -(1ll << 31), (1ll << 31) - 1, tlen))) return (r == 1u ? W_TLEN_NUM : W_TLEN) << 8;
    const u32 l_seq = (cl[9] == 1u && L[cs[9]] == (u8)'*') ? 0u : cl[9];
    for (u32 k = 0; k < l_seq; k++)
        if (nib(L[cs[9] + k]) > 15u) return W_SEQ << 8;
    const bool qual_star = cl[10] == 1u && L[cs[10]] == (u8)'*';
    if (!qual_star) {
        if (l_seq == 0u || cl[10] != l_seq) return W_QUAL << 8;
        for (u32 k = 0; k < l_seq; k++)
            if (L[cs[10] + k] < 33u) return W_QUAL << 8;
    }
    const i64 p0 = (i64)pos - 1;
    const i64 end = (!(flag & 4u) && ref > 0) ? p0 + (i64)ref : p0 + 1;
    if (end > (1ll << 29)) return W_BIN << 8;
    // the aux fields
    AuxCount cnt;
    u32 fld = 0;
    for (u32 a = q; a <= n; fld++) {
        const u32 t = tab_from(L, a, n, wide);
        if ((r = aux_field(cnt, L + a, t - a))) return r << 8 | min(fld, 255u);
        a = t + 1u;
    }
    const u64 size = 36ull + cl[0] + 1u + 4ull * n_cig + (l_seq + 1u) / 2u + l_seq + cnt.n;
    if (size - 4u > 0xFFFFFFF7ull) return W_SIZE << 8;
    SbLine o;
    o.len = n;
    o.name_len = cl[0];
    o.rname_off = cs[2]; o.rname_len = cl[2];
    o.cig_off = cs[5]; o.n_cig = n_cig;
    o.rnext_off = cs[6]; o.rnext_len = cl[6];
    o.seq_off = cs[9]; o.l_seq = l_seq;
    o.qual_off = qual_star ? 0u : cs[10];
    o.aux_off = q <= n ? q : 0u;
    o.aux_bytes = (u32)cnt.n;
    o.size = (u32)size;
    o.pos = (i32)p0; o.next_pos = (i32)((i64)pnext - 1); o.tlen = (i32)tlen;
    o.flag_mapq = (u32)flag | (u32)mapq << 16;
    o.bin = reg2bin(p0, end);
    o.pad = 0;
    *out = o;
    return 0;
}

// stage_wave_lines of pp_devtext.h for a borrowed text: the wave's stretch goes to LDS through loads that stay inside the text, zeros
// behind its end.  *wide: the line lies in the stage and may be read eight bytes at a time up to eight bytes past its end.
template <u32 TOK_STAGE>
__device__ __forceinline__ bool stage_lines_in(const u8 *__restrict__ text, u64 size, const u64 *__restrict__ nl_pos, u64 n_nl, u64 n_lines,
                                               u8 *stage, const u8 **L, u32 *n, u64 *li, bool *wide, u64 *line_len) {
    const u32 lane = threadIdx.x;
    const u64 l0 = (u64)blockIdx.x * 64u, l1 = min(n_lines, l0 + 64u);
    const u64 s0 = l0 ? nl_pos[l0 - 1] + 1 : 0;
    const u64 e1 = (l1 - 1 < n_nl) ? nl_pos[l1 - 1] : size;
    const u64 want = e1 - s0 + 16;
    const u32 span = (u32)min((u64)TOK_STAGE + 16u, (want + 15ull) & ~15ull);
    for (u32 c = lane * 16u; c < span; c += 1024u) {
        const u64 at = s0 + c;
        u64 lo = 0, hi = 0;
        if (at < size) load16_in(text, size, at, (u32)min((u64)16, size - at), &lo, &hi);
        *(uint4 *)(stage + c) = make_uint4((u32)lo, (u32)(lo >> 32), (u32)hi, (u32)(hi >> 32));
    }
    __syncthreads();
    *li = l0 + lane;
    if (*li >= n_lines) return false;
    const u64 ls = *li ? nl_pos[*li - 1] + 1 : 0, le = *li < n_nl ? nl_pos[*li] : size;
    *line_len = le - ls;
    const bool staged = le - s0 + 8 <= (u64)TOK_STAGE + 16u;
    const u8 *p = staged ? (const u8 *)stage + (ls - s0) : text + ls;
    u32 len = (u32)min(le - ls, (u64)0xFFFFFFFFu);
    if (len > 0 && p[len - 1] == (u8)'\r') len--;
    *L = p;
    *n = len;
    *wide = staged;
    return true;
}

// status[0]: the first refusal, line << 16 | why << 8 | aux field; status[1]: the first record line
template <u32 TOK_STAGE>
__global__ __launch_bounds__(64) void k_sb_scan(const u8 *__restrict__ text, u64 size, const u64 *__restrict__ nl_pos, u64 n_nl, u64 n_lines,
                                                u64 n_hdr, SbLine *__restrict__ rec, u8 *__restrict__ kind, u64 *__restrict__ status) {
    __shared__ __attribute__((aligned(16))) u8 stage[TOK_STAGE + 32];
    const u8 *L;
    u32 n;
    u64 li, line_len;
    bool wide;
    if (!stage_lines_in<TOK_STAGE>(text, size, nl_pos, n_nl, n_lines, stage, &L, &n, &li, &wide, &line_len)) return;
    u32 k = LK_SKIP;
    if (n != 0u && li >= n_hdr) {
        if (L[0] == (u8)'@') {
            k = LK_AT;
        } else {
            if (li < status[1]) atomicMin(&status[1], li);
            const u32 why = line_len >= (1ull << 31) ? (u32)W_LONG << 8 : sb_parse_line(L, n, wide, &rec[li]);
            if (why) report(status, (li << 16) | why);
            else k = LK_RECORD;
        }
    }
    kind[li] = (u8)k;
}

// PLACE == false: the workgroups' records and bytes (blk2: two words per workgroup), and the '@' lines behind the first record.
// PLACE == true: blk2 holds their exclusive scan: rec_off, the record's line, its two name ranges, the tiles it starts.
template <bool PLACE>
__global__ __launch_bounds__(SB_LINES) void k_sb_off(u64 n_lines, const u8 *__restrict__ kind, const SbLine *__restrict__ rec,
                                                     const u64 *__restrict__ nl_pos, u64 *__restrict__ blk2, u64 *__restrict__ status,
                                                     u64 records_at, u64 n_rec, u64 *__restrict__ rec_off, u32 *__restrict__ rec_line,
                                                     u64 *__restrict__ nm_off, u32 *__restrict__ nm_len, u32 *__restrict__ tile_first) {
    __shared__ u64 s_w[SB_LINES / 64];
    const u64 li = (u64)blockIdx.x * SB_LINES + threadIdx.x;
    const u32 k = li < n_lines ? kind[li] : (u32)LK_SKIP;
    const u32 is_rec = k == LK_RECORD ? 1u : 0u;
    const u64 size = is_rec ? rec[li].size : 0u;
    u64 t_rec, t_size;
    const u64 ex_rec = block_scan_excl64<SB_LINES>(is_rec, s_w, &t_rec);
    const u64 ex_size = block_scan_excl_u64<SB_LINES>(size, s_w, &t_size);
    u64 *const mine = blk2 + 2ull * blockIdx.x;
    if (!PLACE) {
        if (threadIdx.x == 0) { mine[0] = t_rec; mine[1] = t_size; }
        if (k == LK_AT && li > status[1]) report(status, (li << 16) | ((u32)W_AT << 8));
        return;
    }
    if (!is_rec) return;
    const SbLine a = rec[li];
    const u64 r = mine[0] + ex_rec, s = records_at + mine[1] + ex_size, e = s + size, ls = li ? nl_pos[li - 1] + 1 : 0;
    rec_off[r] = s;
    if (r + 1 == n_rec) rec_off[n_rec] = e;
    rec_line[r] = (u32)li;
    nm_off[r] = ls + a.rname_off;
    nm_len[r] = a.rname_len;
    nm_off[n_rec + r] = ls + a.rnext_off;
    nm_len[n_rec + r] = a.rnext_len;
    for (u64 tile = (s + SB_TILE - 1u) / SB_TILE; tile * SB_TILE < e; tile++) tile_first[tile] = (u32)r;
}

// the ids of pp_names_ids as refID / next_refID: "*" is -1, "=" (RNEXT) the record's refID, an id the header does not have a refusal
__global__ __launch_bounds__(256) void k_sb_refid(u64 n_rec, u32 n_ref, const u8 *__restrict__ text, const u64 *__restrict__ nm_off,
                                                  const u32 *__restrict__ nm_len, const u32 *__restrict__ id, const u32 *__restrict__ rec_line,
                                                  i32 *__restrict__ refid, u64 *__restrict__ status) {
    const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
    if (r >= n_rec) return;
    i32 v[2];
#pragma unroll
    for (u32 c = 0; c < 2u; c++) {
        const u64 i = c * n_rec + r;
        const u32 one = nm_len[i] == 1u ? (u32)text[nm_off[i]] : 0u;
        if (one == (u32)'*') v[c] = -1;
        else if (c == 1u && one == (u32)'=') v[c] = v[0];
        else if (id[i] < n_ref) v[c] = (i32)id[i];
        else {
            v[c] = -1;
            report(status, ((u64)rec_line[r] << 16) | ((c ? (u32)W_RNEXT : (u32)W_RNAME) << 8));
        }
    }
    refid[2 * r] = v[0];
    refid[2 * r + 1] = v[1];
}

// ---- pass B --------------------------------------------------------------------------------------------------------------------------
struct EmitArgs {
    const u8 *text;
    u64 size;
    const u64 *nl;
    const SbLine *lines;
    const u32 *rec_line;
    const u64 *rec_off;       // n_rec + 1 entries
    const i32 *refid;         // two per record
    const u32 *tile_first;    // the record of every tile's first byte (tiles that begin at or behind records_at)
    const u8 *hdr;            // the header's bytes, zeros up to a multiple of SB_STORE
    u64 records_at, n_rec, total;
    u8 *out;                  // ... in an allocation of a multiple of SB_STORE
};

// k <= 16 bytes (lo, hi: low byte first) into the image at p, clipped to the tile
__device__ __forceinline__ void img_put16(u8 *img, i64 p, u64 lo, u64 hi, u32 k) {
    if (p >= 0 && p + 16 <= (i64)SB_TILE) {
#pragma unroll
        for (u32 j = 0; j < 16u; j++)
            if (j < k) img[p + j] = (u8)((j < 8u ? lo >> (8u * j) : hi >> (8u * (j - 8u))));
        return;
    }
    for (u32 j = 0; j < k; j++) {
        const i64 at = p + j;
        if (at >= 0 && at < (i64)SB_TILE) img[at] = (u8)((j < 8u ? lo >> (8u * j) : hi >> (8u * (j - 8u))));
    }
}

// sixteen SEQ bytes (the first `need` are the read's) -> eight bytes of nibbles, high nibble first; a byte behind the read is 0
__device__ __forceinline__ u64 pack_nibbles(u64 lo, u64 hi, u32 need) {
    u64 o = 0;
#pragma unroll
    for (u32 j = 0; j < 16u; j++) {
        const u32 c = (u32)((j < 8u ? lo >> (8u * j) : hi >> (8u * (j - 8u))) & 0xFFu);
        const u64 v = j < need ? (u64)(nib(c) & 15u) : 0ull;
        o |= v << (8u * (j >> 1) + ((j & 1u) ? 0u : 4u));
    }
    return o;
}

__global__ __launch_bounds__(SB_THREADS) void k_sb_emit(EmitArgs A) {
    __shared__ __attribute__((aligned(16))) u8 img[SB_TILE];
    const u32 t = threadIdx.x;
    const u64 t0 = (u64)blockIdx.x * SB_TILE, t1 = min(A.total, t0 + (u64)SB_TILE);
    // ---- the image starts as the header's bytes and zeros
    const u64 hdr_pad = (A.records_at + SB_STORE - 1u) / SB_STORE * SB_STORE;
#pragma unroll
    for (u32 j = 0; j < SB_TILE / SB_STORE / SB_THREADS; j++) {
        const u32 c = SB_STORE * (t + j * SB_THREADS);
        uint4 v = make_uint4(0, 0, 0, 0);
        if (t0 + c < hdr_pad) v = *(const uint4 *)(A.hdr + t0 + c);
        *(uint4 *)(img + c) = v;
    }
    __syncthreads();
    if (A.n_rec && t1 > A.records_at) {
        const u64 r_lo = t0 <= A.records_at ? 0 : (u64)A.tile_first[blockIdx.x];
        const u64 r_hi = t0 + SB_TILE < A.total ? (u64)A.tile_first[blockIdx.x + 1u] : A.n_rec - 1u;
        // ---- (1) what is serial: the fixed words, the CIGAR words, the aux fields; one lane per record
        for (u64 r = r_lo + t; r <= r_hi; r += SB_THREADS) {
            const u64 li = A.rec_line[r], ls = li ? A.nl[li - 1] + 1 : 0;
            const SbLine a = A.lines[li];
            const i64 base = (i64)(A.rec_off[r] - t0);
            ImgPut W{img, base};
            if (base + 36 > 0 && base < (i64)SB_TILE) {
                W.put((u64)(a.size - 4u) | (u64)(u32)A.refid[2 * r] << 32, 8);
                W.put((u64)(u32)a.pos | (u64)((a.name_len + 1u) | (a.flag_mapq >> 16) << 8 | a.bin << 16) << 32, 8);
                W.put((u64)(a.n_cig | (a.flag_mapq & 0xFFFFu) << 16) | (u64)a.l_seq << 32, 8);
                W.put((u64)(u32)A.refid[2 * r + 1] | (u64)(u32)a.next_pos << 32, 8);
                W.put((u64)(u32)a.tlen, 4);
            }
            const i64 cig_at = base + 36 + a.name_len + 1u;
            if (a.n_cig && cig_at + 4ll * a.n_cig > 0 && cig_at < (i64)SB_TILE) {
                W.pos = cig_at;
                const u8 *cg = A.text + ls + a.cig_off;
                for (u32 w = 0, i = 0; w < a.n_cig; w++) {
                    u32 num = 0;
                    while ((u32)cg[i] - (u32)'0' <= 9u) num = num * 10u + ((u32)cg[i++] - (u32)'0');
                    W.put((u64)(num << 4 | (u32)op_code(cg[i++])), 4);
                }
            }
            const i64 aux_at = cig_at + 4ll * a.n_cig + (a.l_seq + 1u) / 2u + a.l_seq;
            if (a.aux_off && aux_at + (i64)a.aux_bytes > 0 && aux_at < (i64)SB_TILE) {
                W.pos = aux_at;
                const u8 *L = A.text + ls;
                for (u32 f = a.aux_off; f <= a.len;) {
                    const u32 e = tab_from(L, f, a.len, false);
                    (void)aux_field(W, L + f, e - f);
                    f = e + 1u;
                }
            }
        }
        // ---- (2) what is wide: the name, the nibbles, QUAL; half a wave per record, a lane per sixteen text bytes
        const u32 half = t >> 5, hl = t & 31u;
        for (u64 r = r_lo + half; r <= r_hi; r += SB_THREADS / 32u) {
            const u64 li = A.rec_line[r], ls = li ? A.nl[li - 1] + 1 : 0;
            const SbLine &a = A.lines[li];
            const u32 name_len = a.name_len, l_seq = a.l_seq, qual_off = a.qual_off;
            const i64 name_at = (i64)(A.rec_off[r] - t0) + 36, seq_at = name_at + name_len + 1u + 4ll * a.n_cig;
            const i64 qual_at = seq_at + (l_seq + 1u) / 2u;
            if (seq_at > 0 && name_at < (i64)SB_TILE) {
                for (u32 c = hl * 16u; c < name_len + 1u; c += 512u) {  // (the NUL: a zero behind the name's bytes)
                    u64 lo = 0, hi = 0;
                    const u32 k = min(16u, name_len + 1u - c), need = min(16u, name_len - min(name_len, c));
                    if (need) load16_in(A.text, A.size, ls + c, need, &lo, &hi);
                    if (need < 16u) {  // nothing behind the name's bytes
                        if (need < 8u) { lo &= (1ull << (8u * need)) - 1ull; hi = 0; }
                        else if (need < 16u) hi &= (1ull << (8u * (need - 8u))) - 1ull;
                    }
                    img_put16(img, name_at + c, lo, hi, k);
                }
            }
            if (l_seq && qual_at > 0 && seq_at < (i64)SB_TILE) {
                const u64 src = ls + a.seq_off;
                for (u32 c = hl * 16u; c < l_seq; c += 512u) {
                    u64 lo, hi;
                    const u32 need = min(16u, l_seq - c);
                    load16_in(A.text, A.size, src + c, need, &lo, &hi);
                    img_put16(img, seq_at + (c >> 1), pack_nibbles(lo, hi, need), 0, (need + 1u) >> 1);
                }
            }
            if (l_seq && qual_at + (i64)l_seq > 0 && qual_at < (i64)SB_TILE) {
                const u64 src = ls + qual_off;
                for (u32 c = hl * 16u; c < l_seq; c += 512u) {
                    u64 lo = ~0ull, hi = ~0ull;  // "*": 0xFF
                    const u32 need = min(16u, l_seq - c);
                    if (qual_off) {
                        load16_in(A.text, A.size, src + c, need, &lo, &hi);
                        lo -= 0x2121212121212121ull;  // (every wanted byte is 33 or more: no borrow reaches one)
                        hi -= 0x2121212121212121ull;
                    }
                    img_put16(img, qual_at + c, lo, hi, need);
                }
            }
        }
        __syncthreads();
    }
    // ---- (3) the image leaves through 16-byte stores aligned on the output
#pragma unroll
    for (u32 j = 0; j < SB_TILE / SB_STORE / SB_THREADS; j++) {
        const u32 c = SB_STORE * (t + j * SB_THREADS);
        if (t0 + c < t1) *(uint4 *)(A.out + t0 + c) = *(const uint4 *)(img + c);
    }
}

// ---- the host side ---------------------------------------------------------------------------------------------------------------------
struct Why { int code; const char *what; };
Why why_of(u32 w) {
    switch (w) {
    case W_LONG: return {PP_ERR_LIMIT, "a line of 2^31 or more bytes"};
    case W_COLS: return {PP_ERR_QUIT, "fewer than 11 columns"};
    case W_QNAME: return {PP_ERR_LIMIT, "a QNAME that is empty or longer than 254 bytes"};
    case W_FLAG_NUM: return {PP_ERR_QUIT, "a FLAG that is no number"};
    case W_FLAG: return {PP_ERR_LIMIT, "a FLAG above 65535"};
    case W_POS_NUM: return {PP_ERR_QUIT, "a POS that is no number"};
    case W_POS: return {PP_ERR_LIMIT, "a POS above 2147483648"};
    case W_MAPQ_NUM: return {PP_ERR_QUIT, "a MAPQ that is no number"};
    case W_MAPQ: return {PP_ERR_LIMIT, "a MAPQ above 255"};
    case W_CIGAR: return {PP_ERR_QUIT, "a CIGAR that is not runs of digits and one of MIDNSHP=X"};
    case W_CIGAR_RUN: return {PP_ERR_LIMIT, "a CIGAR run of length 0, or of 2^28 or more"};
    case W_CIGAR_MANY: return {PP_ERR_LIMIT, "a CIGAR of more than 65535 runs"};
    case W_PNEXT_NUM: return {PP_ERR_QUIT, "a PNEXT that is no number"};
    case W_PNEXT: return {PP_ERR_LIMIT, "a PNEXT above 2147483648"};
    case W_TLEN_NUM: return {PP_ERR_QUIT, "a TLEN that is no number"};
    case W_TLEN: return {PP_ERR_LIMIT, "a TLEN outside 32 bits"};
    case W_SEQ: return {PP_ERR_LIMIT, "a SEQ byte outside =ACMGRSVTWYHKDBN"};
    case W_QUAL: return {PP_ERR_QUIT, "a QUAL that does not fit its SEQ (another length, SEQ \"*\", or a byte below 33)"};
    case W_BIN: return {PP_ERR_LIMIT, "an alignment that ends above 2^29 (POS and CIGAR), where the bin has no number"};
    case W_AUX: return {PP_ERR_QUIT, "a malformed aux field"};
    case W_AUX_LIMIT: return {PP_ERR_LIMIT, "an aux value this encoder does not hold (an integer beyond 32 bits, a float beyond 15 digits or 10^+-22)"};
    case W_SIZE: return {PP_ERR_LIMIT, "a record beyond block_size"};
    case W_RNAME: return {PP_ERR_QUIT, "an RNAME that no @SQ line names"};
    case W_RNEXT: return {PP_ERR_QUIT, "an RNEXT that no @SQ line names"};
    default: return {PP_ERR_QUIT, "a line that begins with '@' behind the first record"};
    }
}

int encode(pp_ctx *ctx, const char *who, const uint8_t *text, uint64_t n_bytes, int mem, pp_bam_enc **out, uint64_t *bad_line) {
    PP_HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const u64 size = n_bytes;
    std::unique_ptr<pp_bam_enc> P(new pp_bam_enc(ctx));
    CallScratch T;
    StageTimer timer(ctx, ctx->profiling != 0 && size != 0);
    int rc;
    const u8 *d_text = nullptr;
    if (size && (rc = on_device(ctx, T, mem, (const u8 *)text, (size_t)size, &d_text))) return rc;

    // ---- the newline index ----
    u64 n_nl = 0, n_lines = 0;
    void *d_nl = nullptr;
    if (size) {
        const u64 n_blk = (size + IN_NL_BLOCK - 1) / IN_NL_BLOCK;
        void *d_blk, *d_blkoff;
        if ((rc = T.get(ctx, &d_blk, ((size_t)n_blk + 1) * 4)) || (rc = T.get(ctx, &d_blkoff, ((size_t)n_blk + 1) * 8))) return rc;
        PP_HIPCHK(ctx, hipMemsetAsync((u32 *)d_blk + n_blk, 0, 4, st));
        if ((rc = timer.begin(0))) return rc;
        hipLaunchKernelGGL(k_in_nl_count<true>, dim3((unsigned)n_blk), dim3(1024), 0, st, d_text, size, (u32 *)d_blk);
        hipLaunchKernelGGL(k_tscan<u64>, dim3(1), dim3(1024), 0, st, (const u32 *)d_blk, n_blk, (u64 *)d_blkoff);
        if ((rc = timer.end())) return rc;
        PP_HIPCHK(ctx, hipGetLastError());
        u32 not_ascii = 0;
        u8 last = 0;
        if ((rc = fetch(ctx, (const u64 *)d_blkoff + n_blk, &n_nl)) || (rc = fetch(ctx, (const u32 *)d_blk + n_blk, &not_ascii)) ||
            (rc = fetch(ctx, d_text + size - 1, &last)))
            return rc;
        if (not_ascii) return ctx->fail(PP_ERR_NOT_ASCII, "%s: the text holds bytes outside ASCII", who);
        n_lines = n_nl + (last != (u8)'\n' ? 1 : 0);
        if (n_lines >= 0xFFFFFFFFull) return ctx->fail(PP_ERR_LIMIT, "%s: 2^32-1 or more lines in one text", who);
        if ((rc = T.get(ctx, &d_nl, (size_t)std::max<u64>(1, n_nl) * 8)) || (rc = timer.begin(0))) return rc;
        hipLaunchKernelGGL(k_in_nl_write, dim3((unsigned)n_blk), dim3(1024), 0, st, d_text, size, (const u64 *)d_blkoff, (u64 *)d_nl);
        if ((rc = timer.end())) return rc;
    }

    // ---- the header: on the host, from the text or from as much of a device text as holds it ----
    std::vector<u8> head;  // the downloaded head of a device text
    const u8 *h_text = mem == PP_MEM_HOST ? (const u8 *)text : nullptr;
    std::vector<uint64_t> sn_off;
    std::vector<u32> sn_len, sn_ln;
    uint64_t header_end = 0, n_hdr = 0;
    u32 n_ref = 0;
    {
        size_t cap = 0;
        char *msg = pp_bam_msg_buf_(&cap);
        u64 got = mem == PP_MEM_HOST ? size : std::min<u64>(size, 1u << 16);
        uint64_t bad = ~0ull;
        while (true) {
            if (mem != PP_MEM_HOST) {
                head.resize((size_t)got);
                if (got && (rc = fetch(ctx, d_text, head.data(), (size_t)got))) return rc;
                h_text = head.data();
            }
            rc = pp_sam_host::header(h_text, got, 0, &n_ref, nullptr, nullptr, nullptr, &header_end, &n_hdr, &bad, msg, cap);
            if (rc == PP_ERR_ARG && n_ref) {
                sn_off.resize(n_ref); sn_len.resize(n_ref); sn_ln.resize(n_ref);
                rc = pp_sam_host::header(h_text, got, n_ref, &n_ref, sn_off.data(), sn_len.data(), sn_ln.data(), &header_end, &n_hdr, &bad, msg, cap);
            }
            if (got < size && (rc != PP_OK || header_end == got)) {  // the head may cut the header: more of it
                got = std::min<u64>(size, got * 8);
                continue;
            }
            break;
        }
        if (rc) {
            if (bad_line) *bad_line = bad;
            return ctx->fail(rc, "%s: \"text\": %s", who, msg);
        }
    }
    // the BAM header: magic, l_text, the header lines with "\n" ends, n_ref, the references
    std::vector<u8> hdr;
    auto put32 = [&](u32 v) { for (int i = 0; i < 4; i++) hdr.push_back((u8)(v >> (8 * i))); };
    hdr.insert(hdr.end(), {(u8)'B', (u8)'A', (u8)'M', 1, 0, 0, 0, 0});
    for (u64 at = 0; at < header_end;) {
        const void *nl = memchr(h_text + at, '\n', (size_t)(header_end - at));
        const u64 le = nl ? (u64)((const u8 *)nl - h_text) : header_end;
        const u64 ce = (le > at && h_text[le - 1] == (u8)'\r') ? le - 1 : le;
        hdr.insert(hdr.end(), h_text + at, h_text + ce);
        hdr.push_back((u8)'\n');
        at = le + 1;
    }
    if (hdr.size() - 8 > 0x7FFFFFFFull) return ctx->fail(PP_ERR_LIMIT, "%s: a header text of 2^31 or more bytes", who);
    const u32 l_text = (u32)(hdr.size() - 8);
    for (int i = 0; i < 4; i++) hdr[4 + i] = (u8)(l_text >> (8 * i));
    put32(n_ref);
    for (u32 i = 0; i < n_ref; i++) {
        put32(sn_len[i] + 1u);
        hdr.insert(hdr.end(), h_text + sn_off[i], h_text + sn_off[i] + sn_len[i]);
        hdr.push_back(0);
        put32(sn_ln[i]);
    }
    const u64 records_at = hdr.size();
    hdr.resize((size_t)((records_at + SB_STORE - 1) / SB_STORE * SB_STORE), 0);
    void *d_hdr;
    if ((rc = T.get(ctx, &d_hdr, hdr.size()))) return rc;
    PP_HIPCHK(ctx, hipMemcpyAsync(d_hdr, hdr.data(), hdr.size(), hipMemcpyHostToDevice, st));

    // ---- pass A, the sums ----
    const u32 nb = (u32)((n_lines + SB_LINES - 1) / SB_LINES);
    void *d_rec = nullptr, *d_kind = nullptr, *d_blk2 = nullptr, *d_blk2off = nullptr, *d_status = nullptr;
    u64 status[2] = {~0ull, ~0ull}, totals[2] = {0, 0};
    if (n_lines) {
        if ((rc = T.get(ctx, &d_rec, (size_t)n_lines * sizeof(SbLine))) || (rc = T.get(ctx, &d_kind, (size_t)n_lines)) ||
            (rc = T.get(ctx, &d_blk2, (size_t)nb * 16)) || (rc = T.get(ctx, &d_blk2off, ((size_t)nb + 1) * 16)) || (rc = T.get(ctx, &d_status, 16)))
            return rc;
        PP_HIPCHK(ctx, hipMemsetAsync(d_status, 0xFF, 16, st));
        if ((rc = timer.begin(1))) return rc;
        with_stage(tok_stage_for(size, n_lines), [&](auto stage) {
            hipLaunchKernelGGL(k_sb_scan<decltype(stage)::value>, dim3((unsigned)((n_lines + 63) / 64)), dim3(64), 0, st, d_text, size, (const u64 *)d_nl,
                               n_nl, n_lines, n_hdr, (SbLine *)d_rec, (u8 *)d_kind, (u64 *)d_status);
        });
        if ((rc = timer.end()) || (rc = timer.begin(3))) return rc;
        hipLaunchKernelGGL(k_sb_off<false>, dim3(nb), dim3(SB_LINES), 0, st, n_lines, (const u8 *)d_kind, (const SbLine *)d_rec, (const u64 *)d_nl,
                           (u64 *)d_blk2, (u64 *)d_status, records_at, (u64)0, (u64 *)nullptr, (u32 *)nullptr, (u64 *)nullptr, (u32 *)nullptr, (u32 *)nullptr);
        hipLaunchKernelGGL(k_colscan<2>, dim3(1), dim3(1024), 0, st, (const u64 *)d_blk2, (u64)nb, (u64 *)d_blk2off);
        if ((rc = timer.end())) return rc;
        PP_HIPCHK(ctx, hipGetLastError());
        if ((rc = fetch(ctx, (const u64 *)d_blk2off + 2ull * nb, totals, 2))) return rc;
    }
    const u64 n_rec = totals[0], total = records_at + totals[1];

    // ---- the records' places, the names, the refIDs ----
    void *d_line = nullptr, *d_nm_off = nullptr, *d_nm_len = nullptr, *d_id = nullptr, *d_refid = nullptr, *d_tile = nullptr;
    float names_ms = 0.f;
    if (n_rec) {
        if ((rc = P->alloc(P->rec_off, (size_t)n_rec + 1)) || (rc = T.get(ctx, &d_line, (size_t)n_rec * 4)) || (rc = T.get(ctx, &d_nm_off, (size_t)n_rec * 16)) ||
            (rc = T.get(ctx, &d_nm_len, (size_t)n_rec * 8)) || (rc = T.get(ctx, &d_id, (size_t)n_rec * 8)) || (rc = T.get(ctx, &d_refid, (size_t)n_rec * 8)) ||
            (rc = T.get(ctx, &d_tile, (size_t)(total / SB_TILE + 2) * 4)))
            return rc;
        if ((rc = timer.begin(3))) return rc;
        hipLaunchKernelGGL(k_sb_off<true>, dim3(nb), dim3(SB_LINES), 0, st, n_lines, (const u8 *)d_kind, (const SbLine *)d_rec, (const u64 *)d_nl,
                           (u64 *)d_blk2off, (u64 *)d_status, records_at, n_rec, P->rec_off, (u32 *)d_line, (u64 *)d_nm_off, (u32 *)d_nm_len, (u32 *)d_tile);
        if ((rc = timer.end())) return rc;
        PP_HIPCHK(ctx, hipGetLastError());
        pp_names *names = nullptr;
        if ((rc = pp_names_create(ctx, n_ref, &names))) return rc;
        std::unique_ptr<pp_names, void (*)(pp_names *)> names_owner(names, pp_names_free);
        if (n_ref) {
            std::vector<u32> seeded(n_ref);
            if ((rc = pp_names_ids(names, h_text, header_end, sn_off.data(), sn_len.data(), n_ref, PP_MEM_HOST, nullptr, seeded.data(), nullptr))) return rc;
        }
        for (u32 c = 0; c < 2u; c++) {
            if ((rc = pp_names_ids(names, d_text, size, (const uint64_t *)d_nm_off + c * n_rec, (const u32 *)d_nm_len + c * n_rec, n_rec, PP_MEM_DEVICE, nullptr,
                                   (u32 *)d_id + c * n_rec, nullptr)))
                return rc;
            float ms = 0.f;
            if (timer.on && (rc = pp_names_kernel_ms(names, &ms))) return rc;
            names_ms += ms;
        }
        if ((rc = timer.begin(3))) return rc;
        hipLaunchKernelGGL(k_sb_refid, dim3((unsigned)((n_rec + 255) / 256)), dim3(256), 0, st, n_rec, n_ref, d_text, (const u64 *)d_nm_off, (const u32 *)d_nm_len,
                           (const u32 *)d_id, (const u32 *)d_line, (i32 *)d_refid, (u64 *)d_status);
        if ((rc = timer.end())) return rc;
        PP_HIPCHK(ctx, hipGetLastError());
    }
    if (n_lines && (rc = fetch(ctx, d_status, status, 2))) return rc;
    if (status[0] != ~0ull) {  // the first refused line
        const u64 li = status[0] >> 16;
        const u32 why = (u32)(status[0] >> 8) & 0xFFu, fld = (u32)status[0] & 0xFFu;
        const Why w = why_of(why);
        if (bad_line) *bad_line = li;
        std::string tag;
        if (why == W_AUX || why == W_AUX_LIMIT) {  // the field's first two bytes: the tag
            u64 a = 0, b = size;
            if (li && (rc = fetch(ctx, (const u64 *)d_nl + (li - 1), &a))) return rc;
            if (li) a += 1;
            if (li < n_nl && (rc = fetch(ctx, (const u64 *)d_nl + li, &b))) return rc;
            std::vector<u8> line((size_t)(b - a));
            if (b > a) {
                if (mem == PP_MEM_HOST) memcpy(line.data(), text + a, (size_t)(b - a));
                else if ((rc = fetch(ctx, d_text + a, line.data(), (size_t)(b - a)))) return rc;
            }
            size_t at = 0;
            for (u32 tabs = 0; at < line.size() && tabs < 11u + fld; at++) tabs += line[at] == (u8)'\t' ? 1u : 0u;
            for (size_t k = at; k < line.size() && k < at + 2 && line[k] >= 0x20 && line[k] != (u8)':'; k++) tag.push_back((char)line[k]);
            if (fld == 255u) tag.clear();
        }
        if (!tag.empty())
            return ctx->fail(w.code, "%s: %s (aux field %s) in \"text\" (line %llu)", who, w.what, tag.c_str(), (unsigned long long)(li + 1));
        return ctx->fail(w.code, "%s: %s in \"text\" (line %llu)", who, w.what, (unsigned long long)(li + 1));
    }
    if (total >= (1ull << 40)) return ctx->fail(PP_ERR_LIMIT, "%s: an output of 2^40 or more bytes", who);

    // ---- pass B: the bytes ----
    P->n_out = total;
    P->records_at = records_at;
    P->n_rec = n_rec;
    if (!n_rec && (rc = P->alloc(P->rec_off, 1))) return rc;
    if ((rc = P->alloc(P->d_out, (size_t)((total + SB_STORE - 1) / SB_STORE * SB_STORE)))) return rc;
    if ((rc = timer.begin(4))) return rc;
    hipLaunchKernelGGL(k_sb_emit, dim3((unsigned)((total + SB_TILE - 1) / SB_TILE)), dim3(SB_THREADS), 0, st,
                       EmitArgs{d_text, size, (const u64 *)d_nl, (const SbLine *)d_rec, (const u32 *)d_line, P->rec_off, (const i32 *)d_refid, (const u32 *)d_tile,
                                (const u8 *)d_hdr, records_at, n_rec, total, P->d_out});
    if ((rc = timer.end())) return rc;
    PP_HIPCHK(ctx, hipGetLastError());
    PP_HIPCHK(ctx, hipStreamSynchronize(st));  // the caller's text may be released, the scratch goes away
    if ((rc = P->t.take(timer))) return rc;
    P->t.ms[2] = names_ms;
    *out = P.release();
    return PP_OK;
}

int checked(pp_ctx *ctx, const char *who, pp_bam_enc **out, uint64_t *bad_line) {
    if (bad_line) *bad_line = ~0ull;
    if (!out) return ctx->fail(PP_ERR_ARG, "%s: null argument", who);
    *out = nullptr;
    return PP_OK;
}

}  // namespace

extern "C" int pp_sam_header(const uint8_t *text, uint64_t n_bytes, uint32_t cap, uint32_t *n_ref, uint64_t *name_off, uint32_t *name_len,
                             uint32_t *ref_len, uint64_t *header_end) {
    size_t msg_cap = 0;
    char *msg = pp_bam_msg_buf_(&msg_cap);
    if (msg_cap) msg[0] = 0;
    return pp_sam_host::header(text, n_bytes, cap, n_ref, name_off, name_len, ref_len, header_end, nullptr, nullptr, msg, msg_cap);
}

extern "C" int pp_sam_bam(pp_ctx *ctx, const uint8_t *text, uint64_t n_bytes, int mem, pp_bam_enc **out, uint64_t *bad_line) {
    if (!ctx) return PP_ERR_ARG;
    if (int rdy = pp_ctx_wait(ctx)) return rdy;
    if (int rc = checked(ctx, "pp_sam_bam", out, bad_line)) return rc;
    if (mem != PP_MEM_HOST && mem != PP_MEM_DEVICE)
        return ctx->fail(PP_ERR_ARG, "pp_sam_bam: the text must be host memory or memory of the context's device");
    if (n_bytes && !text) return ctx->fail(PP_ERR_ARG, "pp_sam_bam: null text with n_bytes > 0");
    if (n_bytes >= (1ull << 40)) return ctx->fail(PP_ERR_LIMIT, "pp_sam_bam: 2^40 or more bytes in one call");
    return encode(ctx, "pp_sam_bam", text, n_bytes, mem, out, bad_line);
}

extern "C" int pp_sam_bam_records(pp_ctx *ctx, const pp_sam *s, pp_bam_enc **out, uint64_t *bad_line) {
    if (!ctx) return PP_ERR_ARG;
    if (int rdy = pp_ctx_wait(ctx)) return rdy;
    if (int rc = checked(ctx, "pp_sam_bam_records", out, bad_line)) return rc;
    if (!s) return ctx->fail(PP_ERR_ARG, "pp_sam_bam_records: null argument");
    const uint8_t *text = nullptr;  // the object's own device copy of the text
    uint64_t n_bytes = 0;
    pp_sam_names(s, &text, &n_bytes, nullptr, nullptr);
    return encode(ctx, "pp_sam_bam_records", text, n_bytes, PP_MEM_DEVICE, out, bad_line);
}

extern "C" void pp_bam_enc_free(pp_bam_enc *e) { delete e; }

extern "C" void pp_bam_enc_bytes(const pp_bam_enc *e, const uint8_t **dev, uint64_t *n_bytes, uint64_t *records_at) {
    if (dev) *dev = e ? e->d_out : nullptr;
    if (n_bytes) *n_bytes = e ? e->n_out : 0;
    if (records_at) *records_at = e ? e->records_at : 0;
}

extern "C" const uint64_t *pp_bam_enc_rec_off(const pp_bam_enc *e, uint64_t *n_rec) {
    if (n_rec) *n_rec = e ? e->n_rec : 0;
    return e ? (const uint64_t *)e->rec_off : nullptr;
}

extern "C" int pp_bam_enc_kernel_ms(const pp_bam_enc *e, float *ms) {
    return e ? e->t.total(e->ctx, "pp_bam_enc_kernel_ms", "when the text was encoded", ms) : PP_ERR_ARG;
}

// (internal hooks, not part of the header: tools/sam_bam_timing.py, the tests) the same time by stage: newline index | pass A | the
// names | the scans | pass B; the geometry: lines per workgroup of the placing kernel, output bytes per workgroup of pass B, bytes per store
extern "C" int pp_bam_enc_stage_ms_(const pp_bam_enc *e, float *ms5) { return e ? e->t.stages(ms5) : PP_ERR_ARG; }
extern "C" void pp_sam_bam_geometry_(uint32_t *lines, uint32_t *tile, uint32_t *store) {
    if (lines) *lines = SB_LINES;
    if (tile) *tile = SB_TILE;
    if (store) *store = SB_STORE;
}

extern "C" int pp_ctx_set_out_bam(pp_ctx *ctx, int on) {
    if (!ctx) return PP_ERR_ARG;
    ctx->out_bam = on != 0;
    return PP_OK;
}

// (internal, the filter drivers: pp_filter_host.cpp)
extern "C" int pp_ctx_out_bam_(const pp_ctx *ctx) { return ctx && ctx->out_bam ? 1 : 0; }

extern "C" int pp_ctx_set_sort_out(pp_ctx *ctx, int on, int index) {
    if (!ctx) return PP_ERR_ARG;
    if (index && !on) return ctx->fail(PP_ERR_ARG, "pp_ctx_set_sort_out: an index needs the sorted output (--out_bai needs --sort_out)");
    ctx->sort_out = on != 0;
    ctx->out_bai = index != 0;
    return PP_OK;
}

// (internal, the filter drivers: pp_filter_host.cpp)
extern "C" int pp_ctx_sort_out_(const pp_ctx *ctx, int *index) {
    if (index) *index = ctx && ctx->out_bai ? 1 : 0;
    return ctx && ctx->sort_out ? 1 : 0;
}
