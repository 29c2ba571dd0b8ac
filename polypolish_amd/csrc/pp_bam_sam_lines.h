// pp_bam_sam_lines.h -- what pp_bam_sam (pp_bam_sam.hip) does with ONE record, as plain C++ that compiles for the device and for the host:
// the check of a record (check_record), the walk that counts a line's bytes in pass A and writes them in pass B (emit_line with one of
// two emitters), and the wide parts of pass B for one lane of a record's group (wide_parts).  The kernels call these per lane;
// tools/bam_sam_host_check.cpp calls them in loops over tiles, records and lanes, so that a sanitizer sees every load and a plain
// model (tests/bam_sam_model.py) can be compared with the bytes without a device.  No byte outside [0, N) is loaded.
#pragma once
#include "pp_bam_host.h"
#include "pp_fmt_g.h"

#if defined(__HIPCC__)
#define PP_BS_HD __host__ __device__
#else
#define PP_BS_HD
#endif

namespace {

typedef unsigned long long u64;
typedef uint32_t u32;
typedef uint8_t u8;
typedef int32_t i32;
typedef long long i64;

constexpr u32 BS_RECS = 1024;    // records per workgroup of pass A and of the placing kernel
constexpr u32 BS_TILE = 16384;   // output bytes per workgroup of pass B
constexpr u32 BS_STORE = 16;     // bytes per store of pass B
constexpr u32 BS_LANE = 16;      // output bytes per lane and step of the wide parts
constexpr u32 BS_GROUP = 32;     // lanes per record of the wide parts
constexpr u32 BS_THREADS = 256;  // threads of pass B
constexpr u32 BS_STRIDE = BS_LANE * BS_GROUP;
// why a record is refused: the three of the walk (pp_bam_host::W_CUT, W_SMALL, W_PAST = 1, 2, 3), pp_bam_records' inner defects,
// then -- from Y_QNAME on -- what makes a valid record PP_ERR_LIMIT
enum : u32 { Y_BLOCK = 4, Y_NAME, Y_CIGAR_OP, Y_REF_ID, Y_AUX, Y_POS, Y_QNAME = 16, Y_REF_NAME, Y_QUAL, Y_TAG, Y_A, Y_Z, Y_H, Y_FLOAT };
constexpr u64 TAG_LO = 0x61663A5A3A505A09ull, TAG_HI = 0x6C69ull;  // \t Z P : Z : f a | i l, low byte first
constexpr u64 OPS8 = 0x3D5048534E44494Dull;                          // M I D N S H P =, low byte first (8: X)
constexpr u64 NIB_LO = 0x565352474D43413Dull, NIB_HI = 0x4E42444B48595754ull;  // = A C M G R S V | T W Y H K D B N

struct RefTab {       // the reference table of the header (device memory)
    const u8 *names;  // the names back to back
    const u64 *off;   // n_ref + 1 entries
    const u8 *ok;     // 1: the name can stand in a line
    u32 n_ref;
};

PP_BS_HD inline u32 ld32(const u8 *__restrict__ p, u64 at) {  // four bytes at any alignment, inside a checked range
    u32 w;
    __builtin_memcpy(&w, p + at, 4);
    return w;
}

// ---- the emitters: a line goes through put1 (one byte) and skip (bytes somebody else writes) -----------------------------------------
struct Count {
    u64 n = 0, seq_at = 0;  // the bytes so far; where SEQ starts in the line (mark)
    PP_BS_HD inline void put1(u32) { n++; }
    PP_BS_HD inline void mark() { seq_at = n; }
    PP_BS_HD inline void skip(u64 k) { n += k; }
    PP_BS_HD inline bool done() const { return false; }
};
struct Img {  // into the tile's image at `pos` (relative to the tile, may lie outside it on either side): clipped
    u8 *img;
    i64 pos;
    PP_BS_HD inline void put1(u32 c) {
        if (pos >= 0 && pos < (i64)BS_TILE) img[pos] = (u8)c;
        pos++;
    }
    PP_BS_HD inline void skip(u64 k) { pos += (i64)k; }
    PP_BS_HD inline void mark() {}
    PP_BS_HD inline bool done() const { return pos >= (i64)BS_TILE; }  // nothing behind this point lies in the tile
};

template <class E>
PP_BS_HD inline void put_u(E &e, u64 v) {  // plain decimal, v < 10^16
    u64 bcd = 0;
    u32 n = 0;
    do {
        bcd = bcd << 4 | (v % 10u);
        v /= 10u;
        n++;
    } while (v);
    for (; n; n--, bcd >>= 4) e.put1((u32)'0' + (u32)(bcd & 15u));
}
template <class E>
PP_BS_HD inline void put_s(E &e, i64 v) {
    if (v < 0) { e.put1('-'); v = -v; }
    put_u(e, (u64)v);
}
template <class E>
PP_BS_HD inline void put_bytes(E &e, const u8 *__restrict__ p, u64 n) {
    for (u64 i = 0; i < n && !e.done(); i++) e.put1(p[i]);
}
PP_BS_HD __attribute__((noinline)) pp_fmt::Text16 g_of(u32 bits) { return pp_fmt::fmt_g(bits); }
template <class E>
PP_BS_HD inline void put_g(E &e, u32 bits) {
    const pp_fmt::Text16 T = g_of(bits);
    for (u32 i = 0; i < T.n; i++) e.put1(T.at(i));
}
// one value of an integer type c C s S i I at p (inside the record)
template <class E>
PP_BS_HD inline void put_int(E &e, const u8 *__restrict__ p, u32 ty) {
    const u32 size = (ty | 0x20u) == (u32)'c' ? 1u : ((ty | 0x20u) == (u32)'s' ? 2u : 4u);
    u32 v = 0;
    for (u32 j = 0; j < size; j++) v |= (u32)p[j] << (8u * j);
    if (ty == (u32)'c') put_s(e, (i64)(int8_t)v);
    else if (ty == (u32)'s') put_s(e, (i64)(int16_t)v);
    else if (ty == (u32)'i') put_s(e, (i64)(i32)v);
    else put_u(e, v);
}
PP_BS_HD inline u32 elem_size(u32 sub) {  // of a B array; 0: no such sub-type
    return (sub == 'c' || sub == 'C') ? 1u : ((sub == 's' || sub == 'S') ? 2u : ((sub == 'i' || sub == 'I' || sub == 'f') ? 4u : 0u));
}

// The line of the record whose fixed part starts at c (block_size bs), FREE OF DEFECTS: everything but QNAME, SEQ and QUAL, which are
// skipped; e.mark() where SEQ starts.  With an emitter that is done() the walk ends early.
template <class E>
PP_BS_HD inline void emit_line(E &e, const u8 *__restrict__ B, u64 c, u32 bs, const RefTab &R, bool fail) {
    const i32 ref_id = (i32)ld32(B, c), pos = (i32)ld32(B, c + 4u), next_ref = (i32)ld32(B, c + 20u), next_pos = (i32)ld32(B, c + 24u);
    const i32 tlen = (i32)ld32(B, c + 28u);
    const u32 w8 = ld32(B, c + 8u), w12 = ld32(B, c + 12u), lrn = w8 & 0xFFu, mapq = (w8 >> 8) & 0xFFu, nc = w12 & 0xFFFFu, flag = w12 >> 16;
    const u32 ls = ld32(B, c + 16u);
    e.skip(lrn - 1u);
    e.put1('\t');
    put_u(e, flag);
    e.put1('\t');
    if (ref_id < 0) e.put1('*');
    else put_bytes(e, R.names + R.off[ref_id], R.off[ref_id + 1] - R.off[ref_id]);
    e.put1('\t');
    put_u(e, (u64)((i64)pos + 1));
    e.put1('\t');
    put_u(e, mapq);
    e.put1('\t');
    const u64 cig = c + 32u + lrn;
    if (nc == 0) e.put1('*');
    for (u32 j = 0; j < nc && !e.done(); j++) {
        const u32 w = ld32(B, cig + 4ull * j), op = w & 15u;
        put_u(e, w >> 4);
        e.put1(op < 8u ? (u32)(OPS8 >> (8u * op)) & 0xFFu : (u32)'X');
    }
    e.put1('\t');
    if (next_ref < 0) e.put1('*');
    else if (next_ref == ref_id) e.put1('=');
    else put_bytes(e, R.names + R.off[next_ref], R.off[next_ref + 1] - R.off[next_ref]);
    e.put1('\t');
    put_u(e, (u64)((i64)next_pos + 1));
    e.put1('\t');
    put_s(e, (i64)tlen);
    e.put1('\t');
    const u64 seq_src = cig + 4ull * nc, qual_src = seq_src + ((u64)ls + 1u) / 2u;
    e.mark();  // (SEQ starts here: pass A keeps the offset for pass B's wide parts)
    if (ls == 0) e.put1('*');
    else e.skip(ls);
    e.put1('\t');
    if (ls == 0 || B[qual_src] == 0xFFu) e.put1('*');
    else e.skip(ls);
    // ---- the aux fields
    u64 p = qual_src + ls;
    const u64 end = c + bs;
    while (p < end && !e.done()) {
        const u32 ty = B[p + 2u];
        e.put1('\t');
        e.put1(B[p]);
        e.put1(B[p + 1u]);
        e.put1(':');
        p += 3u;
        if (ty == 'A') {
            e.put1('A'); e.put1(':'); e.put1(B[p]);
            p += 1u;
        } else if (ty == 'Z' || ty == 'H') {
            e.put1(ty); e.put1(':');
            while (B[p] != 0) {
                e.put1(B[p]);
                p++;
            }
            p++;
        } else if (ty == 'f') {
            e.put1('f'); e.put1(':');
            put_g(e, ld32(B, p));
            p += 4u;
        } else if (ty == 'B') {
            const u32 sub = B[p], cnt = ld32(B, p + 1u), es = elem_size(sub);
            e.put1('B'); e.put1(':'); e.put1(sub);
            p += 5u;
            for (u32 k = 0; k < cnt && !e.done(); k++) {
                e.put1(',');
                if (sub == 'f') put_g(e, ld32(B, p + 4ull * k));
                else put_int(e, B + p + (u64)es * k, sub);
            }
            p += (u64)cnt * es;
        } else {  // c C s S i I
            e.put1('i'); e.put1(':');
            put_int(e, B + p, ty);
            p += (ty | 0x20u) == (u32)'c' ? 1u : ((ty | 0x20u) == (u32)'s' ? 2u : 4u);
        }
    }
    if (fail)
        for (u32 j = 0; j < 10u; j++) e.put1((u32)((j < 8u ? TAG_LO >> (8u * j) : TAG_HI >> (8u * (j - 8u))) & 0xFFu));
    e.put1('\n');
}

// ---- pass A --------------------------------------------------------------------------------------------------------------------------
PP_BS_HD inline bool tag_ok(u32 a, u32 b) {  // [A-Za-z][A-Za-z0-9]
    const bool a_ok = ((a | 0x20u) - (u32)'a') <= 25u;
    const bool b_ok = ((b | 0x20u) - (u32)'a') <= 25u || (b - (u32)'0') <= 9u;
    return a_ok && b_ok;
}
PP_BS_HD inline bool hex_ok(u32 c) { return (c - (u32)'0') <= 9u || ((c | 0x20u) - (u32)'a') <= 5u; }
PP_BS_HD inline bool finite_bits(u32 bits) { return (bits & 0x7F800000u) != 0x7F800000u; }

// what is wrong with the record at offset o: 0, or a Y_ / W_ word; a structural defect in front of a limit.  *aligned, *c, *bs of a
// record without a structural defect
PP_BS_HD inline u32 check_record(const u8 *__restrict__ B, u64 N, u64 o, const RefTab &R, u32 *aligned, u64 *c_out, u32 *bs_out) {
    const u64 left = o <= N ? N - o : 0;  // (an offset behind the array: the walk's "ends inside the block_size word")
    const u32 bs = left >= 4u ? ld32(B, o) : 0u;
    const u32 kind = pp_bam_host::step_kind(left, bs);
    if (kind) return kind;
    const u64 c = o + 4u;  // [c, c + bs) lies inside the array
    const i32 ref_id = (i32)ld32(B, c), pos = (i32)ld32(B, c + 4u), next_ref = (i32)ld32(B, c + 20u), next_pos = (i32)ld32(B, c + 24u);
    const u32 w8 = ld32(B, c + 8u), w12 = ld32(B, c + 12u), lrn = w8 & 0xFFu, nc = w12 & 0xFFFFu, ls = ld32(B, c + 16u);
    const u64 need = 32ull + lrn + 4ull * nc + ((u64)ls + 1u) / 2u + (u64)ls;
    if ((u64)bs < need) return Y_BLOCK;
    if (lrn == 0 || B[c + 32u + lrn - 1u] != 0) return Y_NAME;
    const u64 cig = c + 32u + lrn;
    for (u32 j = 0; j < nc; j++)
        if ((ld32(B, cig + 4ull * j) & 15u) > 8u) return Y_CIGAR_OP;
    if (ref_id < -1 || (ref_id >= 0 && (u32)ref_id >= R.n_ref) || next_ref < -1 || (next_ref >= 0 && (u32)next_ref >= R.n_ref)) return Y_REF_ID;
    u32 lim = 0;  // the first limit met
    u64 p = c + need;
    const u64 e = c + bs;
    while (p < e) {
        if (e - p < 3u) return Y_AUX;
        const u32 t0 = B[p], t1 = B[p + 1u], ty = B[p + 2u];
        p += 3u;
        if (!lim && !tag_ok(t0, t1)) lim = Y_TAG;
        u32 size = 0;
        if (ty == 'A' || ty == 'c' || ty == 'C') size = 1;
        else if (ty == 's' || ty == 'S') size = 2;
        else if (ty == 'i' || ty == 'I' || ty == 'f') size = 4;
        else if (ty == 'Z' || ty == 'H') {
            const u64 start = p;
            bool bad = false;
            while (p < e && B[p] != 0) {
                const u32 ch = B[p];
                bad = bad || (ty == 'Z' ? (ch < 0x20u || ch > 0x7Eu) : !hex_ok(ch));
                p++;
            }
            if (p == e) return Y_AUX;  // no NUL inside the record
            if (!lim && (bad || (ty == 'H' && ((p - start) & 1u)))) lim = ty == 'Z' ? (u32)Y_Z : (u32)Y_H;
            p++;
            continue;
        } else if (ty == 'B') {
            if (e - p < 5u) return Y_AUX;
            const u32 sub = B[p], cnt = ld32(B, p + 1u), es = elem_size(sub);
            p += 5u;
            if (es == 0 || (u64)cnt * es > e - p) return Y_AUX;
            if (sub == 'f' && !lim)
                for (u32 k = 0; k < cnt; k++)
                    if (!finite_bits(ld32(B, p + 4ull * k))) { lim = Y_FLOAT; break; }
            p += (u64)cnt * es;
            continue;
        } else return Y_AUX;  // a type nobody knows
        if (e - p < size) return Y_AUX;
        if (!lim && ty == 'A' && (B[p] < 0x21u || B[p] > 0x7Eu)) lim = Y_A;
        if (!lim && ty == 'f' && !finite_bits(ld32(B, p))) lim = Y_FLOAT;
        p += size;
    }
    if (pos < -1 || next_pos < -1) return Y_POS;
    *aligned = (w12 >> 16) & 4u ? 0u : 1u;
    *c_out = c;
    *bs_out = bs;
    // ---- a valid record: can it be a line?
    if (lrn == 1u || B[c + 32u] == (u8)'@') return Y_QNAME;
    for (u32 j = 0; j + 1u < lrn; j++)
        if (B[c + 32u + j] < 0x21u || B[c + 32u + j] > 0x7Eu) return Y_QNAME;
    if ((ref_id >= 0 && !R.ok[ref_id]) || (next_ref >= 0 && !R.ok[next_ref])) return Y_REF_NAME;
    const u64 qual = cig + 4ull * nc + ((u64)ls + 1u) / 2u;
    if (ls && B[qual] != 0xFFu)
        for (u32 j = 0; j < ls; j++)
            if (B[qual + j] > 93u) return Y_QUAL;
    return lim;
}


// ---- pass B: the wide parts ---------------------------------------------------------------------------------------------------------
// k <= 16 bytes (lo, hi: low byte first) into the image at p, clipped to the tile
PP_BS_HD inline void img_put16(u8 *img, i64 p, u64 lo, u64 hi, u32 k) {
    for (u32 j = 0; j < k; j++) {
        const i64 at = p + j;
        if (at >= 0 && at < (i64)BS_TILE) img[at] = (u8)((j < 8u ? lo >> (8u * j) : hi >> (8u * (j - 8u))));
    }
}
// the first chunk of a part that starts at `at` (relative to the tile) that may touch the tile, for the group's lane hl
PP_BS_HD inline u64 first_chunk(i64 at, u32 hl) {
    const u64 before = at < 0 ? (u64)(-at) : 0u;  // bytes of the part in front of the tile
    return before / BS_STRIDE * BS_STRIDE + (u64)hl * BS_LANE;
}

// sixteen bytes from `at`, of which `need` >= 1 are wanted and lie inside the array; the array's last bytes byte by byte
PP_BS_HD inline void ld16_in(const u8 *__restrict__ B, u64 N, u64 at, u32 need, u64 *lo, u64 *hi) {
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

// QNAME, SEQ and QUAL of the record whose fixed part starts at c, whose line starts at line_at (relative to the tile) and whose SEQ
// starts seq_at bytes into the line (pass A's mark), for lane hl of the record's group of BS_GROUP lanes: sixteen output bytes per
// lane and step, only the chunks that may touch the tile
PP_BS_HD inline void wide_parts(u8 *img, const u8 *__restrict__ B, u64 N, u64 c, i64 line_at, u64 seq_at, u32 hl) {
    const u32 w8 = ld32(B, c + 8u), w12 = ld32(B, c + 12u), lrn = w8 & 0xFFu, nc = w12 & 0xFFFFu, ls = ld32(B, c + 16u);
    if (line_at < (i64)BS_TILE && line_at + (i64)lrn > 0) {  // QNAME
        const u32 n = lrn - 1u;
        for (u32 ch = hl * BS_LANE; ch < n; ch += BS_STRIDE) {
            u64 lo, hi;
            const u32 need = (n - ch < 16u ? n - ch : 16u);
            ld16_in(B, N, c + 32u + ch, need, &lo, &hi);
            img_put16(img, line_at + ch, lo, hi, need);
        }
    }
    if (ls == 0) return;
    const u64 seq_src = c + 32u + lrn + 4ull * nc, qual_src = seq_src + ((u64)ls + 1u) / 2u;
    const i64 s_at = line_at + (i64)seq_at, q_at = s_at + (i64)ls + 1;
    if (s_at < (i64)BS_TILE && s_at + (i64)ls > 0) {  // SEQ: eight bytes of nibbles are sixteen letters
        for (u64 ch = first_chunk(s_at, hl); ch < ls && s_at + (i64)ch < (i64)BS_TILE; ch += BS_STRIDE) {
            const u32 need = (u32)((u64)ls - ch < 16u ? (u64)ls - ch : 16u);
            u64 v, spare;  // (eight bytes are wanted at the most: the load's upper half is not looked at)
            ld16_in(B, N, seq_src + (ch >> 1), (need + 1u) >> 1, &v, &spare);
            u64 lo = 0, hi = 0;
#pragma unroll
            for (u32 j = 0; j < 16u; j++) {
                const u32 nb = (u32)(v >> (8u * (j >> 1) + ((j & 1u) ? 0u : 4u))) & 15u;
                const u64 l = (nb < 8u ? NIB_LO >> (8u * nb) : NIB_HI >> (8u * (nb - 8u))) & 0xFFull;
                if (j < 8u) lo |= l << (8u * j); else hi |= l << (8u * (j - 8u));
            }
            img_put16(img, s_at + (i64)ch, lo, hi, need);
        }
    }
    if (q_at < (i64)BS_TILE && q_at + (i64)ls > 0 && B[qual_src] != 0xFFu) {  // QUAL: plus 33
        for (u64 ch = first_chunk(q_at, hl); ch < ls && q_at + (i64)ch < (i64)BS_TILE; ch += BS_STRIDE) {
            u64 lo, hi;
            const u32 need = (u32)((u64)ls - ch < 16u ? (u64)ls - ch : 16u);
            ld16_in(B, N, qual_src + ch, need, &lo, &hi);
            lo += 0x2121212121212121ull;  // (every wanted byte is 93 or less: no carry leaves one; a carry out of an
            hi += 0x2121212121212121ull;  //  unwanted byte goes upwards, where no wanted byte lies)
            img_put16(img, q_at + (i64)ch, lo, hi, need);
        }
    }
}

}  // namespace
