// pp_bgzf_host.h -- the header of one BGZF block and the host walk over a file's blocks behind pp_bgzf_walk (pp_bgzf.hip): plain C++
// with no HIP in it, so that a stand-alone program can run the walk under a sanitizer (tools/bgzf_host_check.cpp).  block() is also
// what the device runs per block before anything is read through a block's offset (k_bgzf_head): one definition for both sides.
// Nothing here reads a byte outside [0, n_bytes) or forms a sum that could wrap: every length is compared with what is LEFT.
// The WRITING twin: the constants and bytes of a block around one stored DEFLATE block, which pp_bam_tagged frames its output with
// on the device (pp_bam_out.hip takes the head's and the EOF block's bytes from here), and store_block(), the same block in plain C++.
// The COMPRESSING twin: the rules of pp_bgzf_deflate's blocks and what is serial per piece (df_plan: code lengths, header runs, costs,
// codes), run by one lane of the kernel (pp_bgzf_deflate.hip) and by deflate_block(), the whole piece in plain C++.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>

#if defined(__HIPCC__)
#define PP_BGZF_HD __host__ __device__
#else
#define PP_BGZF_HD
#endif

namespace pp_bgzf_host {

constexpr int OK = 0, ERR_ARG = 4;  // PP_OK, PP_ERR_ARG
constexpr uint32_t MAX_ISIZE = 65536;

// what is wrong with a block's header, in the order it is looked for
enum : uint32_t { H_OK = 0, H_RANGE = 1, H_MAGIC = 2, H_EXTRA = 3, H_NO_BC = 4, H_BSIZE = 5, H_PAST = 6, H_ISIZE = 7 };

struct Block {
    uint32_t total;    // BSIZE + 1: the whole block
    uint32_t payload;  // offset of the DEFLATE stream inside the block (12 + XLEN)
    uint32_t pay_len;  // its length: total - payload - 8
    uint32_t isize;    // the footer's ISIZE
};

PP_BGZF_HD inline uint32_t le16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
PP_BGZF_HD inline uint32_t le32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// the block at `at`: 1f 8b 08, FLG with FEXTRA, XLEN, the BC subfield (SLEN 2) among the extra subfields, BSIZE, the footer's ISIZE
PP_BGZF_HD inline uint32_t block(const uint8_t *bytes, uint64_t n_bytes, uint64_t at, Block *out) {
    if (at > n_bytes || n_bytes - at < 12) return H_RANGE;
    const uint8_t *h = bytes + at;
    const uint64_t left = n_bytes - at;
    if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || !(h[3] & 4)) return H_MAGIC;
    const uint32_t xlen = le16(h + 10);
    if ((uint64_t)xlen > left - 12) return H_EXTRA;
    uint32_t p = 0, bsize = 0;
    bool found = false;
    while (xlen - p >= 4) {  // SI1 SI2 SLEN data
        const uint32_t slen = le16(h + 12 + p + 2);
        if (slen > xlen - p - 4) return H_EXTRA;
        if (!found && h[12 + p] == 'B' && h[12 + p + 1] == 'C' && slen == 2) {
            bsize = le16(h + 12 + p + 4);
            found = true;
        }
        p += 4 + slen;
    }
    if (p != xlen) return H_EXTRA;
    if (!found) return H_NO_BC;
    const uint32_t total = bsize + 1;
    if (total < 12 + xlen + 8) return H_BSIZE;
    if ((uint64_t)total > left) return H_PAST;
    const uint32_t isize = le32(h + total - 4);
    if (isize > MAX_ISIZE) return H_ISIZE;
    out->total = total;
    out->payload = 12 + xlen;
    out->pay_len = total - 12 - xlen - 8;
    out->isize = isize;
    return H_OK;
}

// ---- writing: one BGZF block around one STORED DEFLATE block (level 0), what pp_bam_tagged frames its output with (pp_bam_out.hip) ----
// 1f 8b 08 04 | MTIME 0 | XFL 0 | OS ff | XLEN 6 | B C 2 0 BSIZE | 01 LEN ~LEN | the bytes | CRC32 | ISIZE: len + 31 bytes, BSIZE = len + 30
constexpr uint32_t STORE_PAYLOAD = 0xff00;  // htslib's payload size: the output is cut every 65,280 bytes
constexpr uint32_t STORE_HEAD = 23;         // the 18 bytes of the header and 01 LEN ~LEN
constexpr uint32_t STORE_EXTRA = 31;        // ... and CRC32, ISIZE behind the bytes
constexpr uint32_t STORE_BLOCK = STORE_PAYLOAD + STORE_EXTRA;  // block b of a file starts at b * 65,311
constexpr uint32_t EOF_SIZE = 28;

// byte j < 18 of a block's header, total = the whole block's bytes
PP_BGZF_HD inline uint8_t head_byte(uint32_t j, uint32_t total) {
    if (j < 8) return (uint8_t)(0x0000000004088b1full >> (8 * j));
    if (j < 16) return (uint8_t)(0x000243420006ff00ull >> (8 * (j - 8)));
    return (uint8_t)((total - 1) >> (8 * (j - 16)));
}
// byte j < STORE_HEAD of the block that stores `len` bytes
PP_BGZF_HD inline uint8_t store_head_byte(uint32_t j, uint32_t len) {
    if (j < 18) return head_byte(j, len + STORE_EXTRA);
    if (j == 18) return 1;  // BFINAL, BTYPE 0
    const uint32_t w = j < 21 ? len : ~len;
    return (uint8_t)(w >> (8 * ((j - 19) & 1)));
}
// byte j < EOF_SIZE of the empty block that ends a file: the header, an empty fixed-code block (03 00), CRC32 0, ISIZE 0
PP_BGZF_HD inline uint8_t eof_byte(uint32_t j) { return j < 18 ? head_byte(j, EOF_SIZE) : (j == 18 ? 3 : 0); }

inline uint32_t crc32_bitwise(const uint8_t *data, uint32_t len) {
    uint32_t c = 0xFFFFFFFFu;
    for (uint32_t i = 0; i < len; i++) {
        c ^= data[i];
        for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
    }
    return ~c;
}

// the block that stores data[0, len), len <= STORE_PAYLOAD, into out[0, len + STORE_EXTRA); returns its size
inline uint32_t store_block(const uint8_t *data, uint32_t len, uint8_t *out) {
    for (uint32_t j = 0; j < STORE_HEAD; j++) out[j] = store_head_byte(j, len);
    if (len) memcpy(out + STORE_HEAD, data, len);
    const uint32_t foot[2] = {crc32_bitwise(data, len), len};
    for (uint32_t j = 0; j < 8; j++) out[STORE_HEAD + len + j] = (uint8_t)(foot[j >> 2] >> (8 * (j & 3)));
    return len + STORE_EXTRA;
}

// ---- writing, compressed: one BGZF block around ONE DEFLATE block (BFINAL = 1) per piece of at most STORE_PAYLOAD bytes, what
// pp_bgzf_deflate makes on the device (pp_bgzf_deflate.hip).  tests/bgzf_deflate_model.py is the definition; every rule is a function
// of the piece's bytes alone.  What is SERIAL per piece lives here, shared by the kernel (one lane runs it over LDS) and the host twin
// deflate_block(): the length-limited code lengths, the run-length coding of the header, the cost of the three forms and the choice.
//   candidates  positions in strips of DF_STRIP; a table of 2^DF_HB entries, empty at the piece's start; position i with i + 4 <= n reads
//               T[h(i)] as the strips in front left it, then T[h(i)] = max(T[h(i)], i) for the whole strip: a candidate is never in i's strip
//   match       the common prefix at the candidate, capped at min(258, n - i); it counts from 4 bytes on and up to a distance of 32,768
//   parse       greedy from 0, no lazy evaluation
//   lengths     used symbols sorted by (count, symbol), two-queue Huffman merge (a tie takes the leaf), depths folded into the limit and
//               one leaf moved down with a sibling from the limit until the Kraft sum is one, lengths handed out again in sorted order
//   header      HLIT, HDIST trimmed; the lengths of both codes as ONE sequence, coded greedily with 16 / 17 / 18; HCLEN trimmed
//   choice      the exact bit costs of stored, fixed, dynamic; the smallest wins, a tie goes to the earlier: never above len + 31 bytes
constexpr uint32_t DF_STRIP = 256, DF_HB = 13, DF_MIN_MATCH = 4, DF_MAX_MATCH = 258, DF_MAX_DIST = 32768;
constexpr uint32_t DF_NLIT = 286, DF_NDIST = 30, DF_NSYM = DF_NLIT + DF_NDIST, DF_NCL = 19;
constexpr uint32_t DF_STORED = 0, DF_FIXED = 1, DF_DYNAMIC = 2;
constexpr uint32_t DF_MATCH = 1u << 31;  // a token: a literal's byte, or DF_MATCH | (length - 3) << 16 | (distance - 1)

PP_BGZF_HD inline uint32_t df_hash(uint32_t w) { return (w * 2654435761u) >> (32u - DF_HB); }
PP_BGZF_HD inline uint32_t df_log2(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }  // v > 0
// the length symbol (without the 257) of a match of `len` bytes, and the distance symbol of `dist`; their extra bits are the low ones
PP_BGZF_HD inline uint32_t df_len_sym(uint32_t len) {
    const uint32_t l = len - 3u;
    if (l < 8u) return l;
    if (l == 255u) return 28u;
    const uint32_t nb = df_log2(l) - 2u;
    return 4u * nb + 4u + ((l >> nb) & 3u);
}
PP_BGZF_HD inline uint32_t df_dist_sym(uint32_t dist) {
    const uint32_t d = dist - 1u;
    if (d < 4u) return d;
    const uint32_t nb = df_log2(d) - 1u;
    return 2u * nb + 2u + ((d >> nb) & 1u);
}
PP_BGZF_HD inline uint32_t df_len_xbits(uint32_t c) { return (c < 8u || c == 28u) ? 0u : (c >> 2) - 1u; }
PP_BGZF_HD inline uint32_t df_dist_xbits(uint32_t c) { return c < 4u ? 0u : (c >> 1) - 1u; }
PP_BGZF_HD inline uint32_t df_fixed_len(uint32_t s) { return s < 144u ? 8u : (s < 256u ? 9u : (s < 280u ? 7u : 8u)); }
PP_BGZF_HD inline uint32_t df_fixed_code(uint32_t s) { return s < 144u ? 0x30u + s : (s < 256u ? 0x190u + (s - 144u) : (s < 280u ? s - 256u : 0xC0u + (s - 280u))); }
PP_BGZF_HD inline uint32_t df_rev(uint32_t code, uint32_t len) {  // a Huffman code goes out high bit first
    uint32_t r = 0;
    for (uint32_t i = 0; i < len; i++) r |= ((code >> i) & 1u) << (len - 1u - i);
    return r;
}
PP_BGZF_HD inline uint32_t df_cl_order(uint32_t i) {
    constexpr uint8_t ord[DF_NCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    return ord[i];
}
PP_BGZF_HD inline uint32_t df_cl_xbits(uint32_t s) { return s < 16u ? 0u : (s == 16u ? 2u : (s == 17u ? 3u : 7u)); }

struct DfPlan {  // one piece's symbol counts in, its codes and form out; on the device it lives in LDS
    uint32_t hist[DF_NSYM];   // in: literal/length symbols (256 counted once), then the distance symbols
    uint16_t order[DF_NSYM];  // in: the used symbols by (count, symbol): [0, m_lit) and, numbered from 0, [DF_NLIT, DF_NLIT + m_dist)
    uint32_t m_lit, m_dist;
    uint8_t len[DF_NSYM];     // the dynamic code's lengths
    uint16_t code[DF_NSYM];   // the chosen form's codes, bit-reversed, and their lengths
    uint8_t clen[DF_NSYM];
    uint16_t rle[DF_NSYM];    // the header's sequence: symbol | extra bits' value << 8
    uint32_t n_rle, hlit, hdist, hclen;
    uint32_t cl_hist[DF_NCL];
    uint16_t cl_order[DF_NCL], cl_code[DF_NCL];
    uint8_t cl_len[DF_NCL];
    uint32_t type, bits;      // the form and the bits of its stream, block header and end-of-block code included
    uint32_t w[2 * DF_NLIT], bl[16], next[16];  // work
    uint16_t parent[2 * DF_NLIT];
};

// the used symbols of count[0, n) by (count, symbol) into order[]; returns their number (the kernel ranks them in parallel instead)
PP_BGZF_HD inline uint32_t df_sort(const uint32_t *count, uint32_t n, uint16_t *order) {
    uint32_t m = 0;
    for (uint32_t s = 0; s < n; s++) {
        if (!count[s]) continue;
        uint32_t r = 0;
        for (uint32_t t = 0; t < n; t++) r += count[t] && (count[t] < count[s] || (count[t] == count[s] && t < s));
        order[r] = (uint16_t)s;
        m++;
    }
    return m;
}

// code lengths of at most `limit` bits for the m used symbols in order[]; len[] of the others stays as it is (zero).  Trips: the merge
// m - 1 steps, the repair fewer than m (every folded leaf adds less than one unit to the Kraft sum).
PP_BGZF_HD inline void df_lengths(const uint32_t *count, const uint16_t *order, uint32_t m, uint32_t limit, uint8_t *len, DfPlan *P) {
    if (m == 0) return;
    if (m == 1) { len[order[0]] = 1; return; }
    uint32_t *w = P->w, *bl = P->bl;
    uint16_t *parent = P->parent;
    for (uint32_t j = 0; j < m; j++) w[j] = count[order[j]];
    uint32_t a = 0, b = m;  // the next leaf, the next merged node: both queues are in rising order
    for (uint32_t k = m; k < 2u * m - 1u; k++) {
        uint32_t s = 0;
        for (int pick = 0; pick < 2; pick++) {
            const bool leaf = a < m && (b >= k || w[a] <= w[b]);
            const uint32_t idx = leaf ? a++ : b++;
            s += w[idx];
            parent[idx] = (uint16_t)k;
        }
        w[k] = s;
    }
    w[2u * m - 2u] = 0;  // depths from the root down: a node's parent has a higher index
    for (uint32_t k = 2u * m - 2u; k-- > 0;) w[k] = w[parent[k]] + 1u;
    for (uint32_t l = 0; l < 16u; l++) bl[l] = 0;
    for (uint32_t j = 0; j < m; j++) bl[w[j] < limit ? w[j] : limit]++;
    uint32_t kraft = 0;
    for (uint32_t l = 1; l <= limit; l++) kraft += bl[l] << (limit - l);
    for (uint32_t over = kraft - (1u << limit); over > 0; over--) {  // each step takes exactly one unit off the sum
        uint32_t bits = limit - 1u;
        while (bits > 1u && bl[bits] == 0) bits--;
        bl[bits]--;
        bl[bits + 1u] += 2u;
        bl[limit]--;
    }
    uint32_t j = 0;
    for (uint32_t l = limit; l >= 1u; l--)
        for (uint32_t c = 0; c < bl[l]; c++) len[order[j++]] = (uint8_t)l;
}

// the canonical codes of len[0, n), bit-reversed
PP_BGZF_HD inline void df_codes(const uint8_t *len, uint32_t n, uint16_t *code, DfPlan *P) {
    uint32_t *bl = P->bl, *next = P->next;
    for (uint32_t l = 0; l < 16u; l++) bl[l] = 0;
    for (uint32_t s = 0; s < n; s++) bl[len[s]]++;
    bl[0] = 0;
    uint32_t c = 0;
    for (uint32_t l = 1; l < 16u; l++) next[l] = c = (c + bl[l - 1u]) << 1;
    for (uint32_t s = 0; s < n; s++)
        if (len[s]) code[s] = (uint16_t)df_rev(next[len[s]]++, len[s]);
}

// from hist, order, m_lit, m_dist: everything else of the plan, for a piece of n bytes
PP_BGZF_HD inline void df_plan(DfPlan *P, uint32_t n) {
    for (uint32_t s = 0; s < DF_NSYM; s++) P->len[s] = 0;
    df_lengths(P->hist, P->order, P->m_lit, 15u, P->len, P);
    df_lengths(P->hist + DF_NLIT, P->order + DF_NLIT, P->m_dist, 15u, P->len + DF_NLIT, P);
    uint32_t hlit = DF_NLIT, hdist = DF_NDIST;
    while (hlit > 257u && P->len[hlit - 1u] == 0) hlit--;
    while (hdist > 1u && P->len[DF_NLIT + hdist - 1u] == 0) hdist--;
    // the lengths of both codes as one sequence, greedily: a run of zeros of 11 .. 138 is 18, of 3 .. 10 is 17; a length that repeats
    // the one in front of it 3 .. 6 times is 16; anything else is itself
    const uint32_t total = hlit + hdist;
    uint32_t n_rle = 0;
    for (uint32_t l = 0; l < DF_NCL; l++) { P->cl_hist[l] = 0; P->cl_len[l] = 0; }
    for (uint32_t p = 0; p < total;) {
        const uint32_t v = P->len[p < hlit ? p : DF_NLIT + (p - hlit)], cap = v ? 6u : 138u;
        uint32_t r = 1;
        while (r < cap && p + r < total && P->len[p + r < hlit ? p + r : DF_NLIT + (p + r - hlit)] == v) r++;
        uint32_t sym = v, extra = 0, step = 1;
        if (v == 0 && r >= 11u) { sym = 18; extra = r - 11u; step = r; }
        else if (v == 0 && r >= 3u) { sym = 17; extra = r - 3u; step = r; }
        else if (v != 0 && r >= 3u && p > 0 && P->len[p - 1u < hlit ? p - 1u : DF_NLIT + (p - 1u - hlit)] == v) { sym = 16; extra = r - 3u; step = r; }
        P->rle[n_rle++] = (uint16_t)(sym | extra << 8);
        P->cl_hist[sym]++;
        p += step;
    }
    const uint32_t m_cl = df_sort(P->cl_hist, DF_NCL, P->cl_order);
    df_lengths(P->cl_hist, P->cl_order, m_cl, 7u, P->cl_len, P);
    uint32_t hclen = DF_NCL;
    while (hclen > 4u && P->cl_len[df_cl_order(hclen - 1u)] == 0) hclen--;
    // the three costs in bits
    uint32_t extra_bits = 0, fixed = 3, dyn = 3 + 14 + 3 * hclen;
    for (uint32_t s = 0; s < DF_NLIT; s++) {
        if (s > 256u) extra_bits += P->hist[s] * df_len_xbits(s - 257u);
        fixed += P->hist[s] * df_fixed_len(s);
        dyn += P->hist[s] * P->len[s];
    }
    for (uint32_t d = 0; d < DF_NDIST; d++) {
        extra_bits += P->hist[DF_NLIT + d] * df_dist_xbits(d);
        fixed += P->hist[DF_NLIT + d] * 5u;
        dyn += P->hist[DF_NLIT + d] * P->len[DF_NLIT + d];
    }
    for (uint32_t l = 0; l < DF_NCL; l++) dyn += P->cl_hist[l] * (P->cl_len[l] + df_cl_xbits(l));
    fixed += extra_bits;
    dyn += extra_bits;
    const uint32_t stored = 8u * (5u + n);
    P->n_rle = n_rle; P->hlit = hlit; P->hdist = hdist; P->hclen = hclen;
    if (stored <= fixed && stored <= dyn) { P->type = DF_STORED; P->bits = stored; return; }
    if (fixed <= dyn) {
        P->type = DF_FIXED; P->bits = fixed;
        for (uint32_t s = 0; s < DF_NLIT; s++) { P->clen[s] = (uint8_t)df_fixed_len(s); P->code[s] = (uint16_t)df_rev(df_fixed_code(s), df_fixed_len(s)); }
        for (uint32_t d = 0; d < DF_NDIST; d++) { P->clen[DF_NLIT + d] = 5; P->code[DF_NLIT + d] = (uint16_t)df_rev(d, 5u); }
        return;
    }
    P->type = DF_DYNAMIC; P->bits = dyn;
    for (uint32_t s = 0; s < DF_NSYM; s++) P->clen[s] = P->len[s];
    df_codes(P->len, DF_NLIT, P->code, P);
    df_codes(P->len + DF_NLIT, DF_NDIST, P->code + DF_NLIT, P);
    df_codes(P->cl_len, DF_NCL, P->cl_code, P);
}

// the bits of one token under the plan's chosen codes (low bit first), at most 48; *nbits their number
PP_BGZF_HD inline uint64_t df_token_bits(const DfPlan *P, uint32_t tok, uint32_t *nbits) {
    if (!(tok & DF_MATCH)) { *nbits = P->clen[tok]; return P->code[tok]; }
    const uint32_t l = (tok >> 16) & 0xFFu, d = tok & 0xFFFFu, ls = df_len_sym(l + 3u), ds = df_dist_sym(d + 1u);
    const uint32_t lx = df_len_xbits(ls), dx = df_dist_xbits(ds);
    uint64_t v = P->code[257u + ls];
    uint32_t at = P->clen[257u + ls];
    v |= (uint64_t)(lx ? l & ((1u << lx) - 1u) : 0u) << at;  // (258 has its own symbol and no extra bits)
    at += lx;
    v |= (uint64_t)P->code[DF_NLIT + ds] << at;
    at += P->clen[DF_NLIT + ds];
    v |= (uint64_t)(d & ((1u << dx) - 1u)) << at;
    *nbits = at + dx;
    return v;
}

// the dynamic block's header behind BFINAL and BTYPE, one item at a time: item 0 = HLIT HDIST HCLEN, 1 .. hclen the code-length
// code's lengths, then the n_rle symbols of the sequence with their extra bits
PP_BGZF_HD inline uint32_t df_header_items(const DfPlan *P) { return 1u + P->hclen + P->n_rle; }
PP_BGZF_HD inline uint32_t df_header_item(const DfPlan *P, uint32_t i, uint32_t *nbits) {
    if (i == 0) { *nbits = 14; return (P->hlit - 257u) | (P->hdist - 1u) << 5 | (P->hclen - 4u) << 10; }
    if (i <= P->hclen) { *nbits = 3; return P->cl_len[df_cl_order(i - 1u)]; }
    const uint32_t e = P->rle[i - 1u - P->hclen], sym = e & 0xFFu, cl = P->cl_len[sym];
    *nbits = cl + df_cl_xbits(sym);
    return P->cl_code[sym] | (e >> 8) << cl;
}

// the host twin of the device's work on one piece: data[0, len), len <= STORE_PAYLOAD, into out[0, len + STORE_EXTRA); returns the
// block's size, *type (may be NULL) the form chosen
inline uint32_t deflate_block(const uint8_t *data, uint32_t len, uint8_t *out, uint32_t *type = nullptr) {
    DfPlan *P = new DfPlan();
    uint32_t *tok = new uint32_t[len ? len : 1], *T = new uint32_t[1u << DF_HB](), n_tok = 0;
    uint16_t *m_len = new uint16_t[DF_STRIP], *m_dist = new uint16_t[DF_STRIP];
    uint32_t next_free = 0;
    for (uint32_t s0 = 0; s0 < len; s0 += DF_STRIP) {
        const uint32_t s1 = s0 + DF_STRIP < len ? s0 + DF_STRIP : len;
        for (uint32_t i = s0; i < s1; i++) {  // every position reads the table as the strips in front left it
            m_len[i - s0] = 0;
            if (len - i < 4u) continue;
            const uint32_t cand = T[df_hash(le32(data + i))];
            if (!cand || i - (cand - 1u) > DF_MAX_DIST) continue;
            const uint32_t c = cand - 1u, cap = len - i < DF_MAX_MATCH ? len - i : DF_MAX_MATCH;
            uint32_t l = 0;
            while (l < cap && data[c + l] == data[i + l]) l++;
            if (l >= DF_MIN_MATCH) { m_len[i - s0] = (uint16_t)l; m_dist[i - s0] = (uint16_t)(i - c - 1u); }
        }
        for (uint32_t i = s0; i < s1 && len - i >= 4u; i++) {
            uint32_t *t = &T[df_hash(le32(data + i))];
            if (*t < i + 1u) *t = i + 1u;
        }
        while (next_free < s1) {  // the parse of this strip, from the carried next free position
            const uint32_t i = next_free;
            if (m_len[i - s0]) {
                tok[n_tok++] = DF_MATCH | (uint32_t)(m_len[i - s0] - 3u) << 16 | m_dist[i - s0];
                P->hist[257u + df_len_sym(m_len[i - s0])]++;
                P->hist[DF_NLIT + df_dist_sym(m_dist[i - s0] + 1u)]++;
                next_free += m_len[i - s0];
            } else {
                tok[n_tok++] = data[i];
                P->hist[data[i]]++;
                next_free++;
            }
        }
    }
    P->hist[256] = 1;
    P->m_lit = df_sort(P->hist, DF_NLIT, P->order);
    P->m_dist = df_sort(P->hist + DF_NLIT, DF_NDIST, P->order + DF_NLIT);
    df_plan(P, len);
    const uint32_t stream = (P->bits + 7u) / 8u, total = 18u + stream + 8u;
    for (uint32_t j = 0; j < 18u; j++) out[j] = head_byte(j, total);
    uint8_t *z = out + 18;
    if (P->type == DF_STORED) {
        for (uint32_t j = 0; j < 5u; j++) z[j] = store_head_byte(18u + j, len);
        if (len) memcpy(z + 5, data, len);
    } else {
        memset(z, 0, stream);
        uint32_t at = 0;
        auto put = [&](uint64_t v, uint32_t nbits) {
            for (uint32_t i = 0; i < nbits; i++, at++) z[at >> 3] |= (uint8_t)(((v >> i) & 1u) << (at & 7u));
        };
        put(1u | P->type << 1, 3);
        uint32_t nb;
        if (P->type == DF_DYNAMIC)
            for (uint32_t i = 0; i < df_header_items(P); i++) { const uint32_t v = df_header_item(P, i, &nb); put(v, nb); }
        for (uint32_t k = 0; k < n_tok; k++) { const uint64_t v = df_token_bits(P, tok[k], &nb); put(v, nb); }
        put(P->code[256], P->clen[256]);
    }
    const uint32_t foot[2] = {crc32_bitwise(data, len), len};
    for (uint32_t j = 0; j < 8u; j++) z[stream + j] = (uint8_t)(foot[j >> 2] >> (8u * (j & 3u)));
    if (type) *type = P->type;
    delete P;
    delete[] tok;
    delete[] T;
    delete[] m_len;
    delete[] m_dist;
    return total;
}

inline const char *defect_text(uint32_t code) {
    switch (code) {
    case H_RANGE: return "does not lie inside the bytes (12 bytes of header)";
    case H_MAGIC: return "does not start with 1f 8b 08 and a FLG with FEXTRA";
    case H_EXTRA: return "has extra subfields that do not fit its XLEN, or an XLEN that runs past the bytes";
    case H_NO_BC: return "has no BC subfield of SLEN 2";
    case H_BSIZE: return "has a BSIZE below its header and footer";
    case H_PAST: return "runs past the end of the bytes";
    default: return "has an ISIZE above 65536";
    }
}

inline int fail(char *msg, size_t msg_cap, const char *fmt, unsigned long long a = 0, unsigned long long b = 0, const char *s = "") {
    if (msg && msg_cap) snprintf(msg, msg_cap, fmt, a, b, s);
    return ERR_ARG;
}

// the BSIZE chain from `from`: stops at n_bytes, or after `cap` blocks when there is an array to fill.  blk_off has cap entries,
// out_off (may be NULL) cap + 1: out_off[b] = the ISIZEs in front of block b, and one more entry behind the last block written.
inline int walk(const uint8_t *bytes, uint64_t n_bytes, uint64_t from, uint64_t *blk_off, uint64_t *out_off, uint64_t cap, uint64_t *n_blk,
                uint64_t *end, char *msg, size_t msg_cap) {
    if (n_blk) *n_blk = 0;
    if (end) *end = from;
    if (!n_blk || !end || (n_bytes && !bytes)) return fail(msg, msg_cap, "pp_bgzf_walk: null argument");
    if (from > n_bytes) return fail(msg, msg_cap, "pp_bgzf_walk: the start %llu lies behind the %llu bytes", from, n_bytes);
    const bool fill = blk_off && cap;
    uint64_t at = from, n = 0, sum = 0;
    int rc = OK;
    while (at < n_bytes && !(fill && n == cap)) {
        Block b;
        const uint32_t code = block(bytes, n_bytes, at, &b);
        if (code) {
            rc = fail(msg, msg_cap, "pp_bgzf_walk: block %llu (offset %llu) %s", n, at, defect_text(code));
            break;
        }
        if (fill) {
            blk_off[n] = at;
            if (out_off) out_off[n] = sum;
        }
        sum += b.isize;
        n++;
        at += b.total;
    }
    if (fill && out_off) out_off[n] = sum;
    *n_blk = n;
    *end = at;
    return rc;
}

}  // namespace pp_bgzf_host
