// pp_bam_index_host.h -- the host side of pp_bam_index (pp_bam_out.hip): the tables the device made, written out as a .bai.  Plain C++
// with no HIP in it, so that a stand-alone program can run it under a sanitizer (tools/bam_sort_host_check.cpp).
//
// The file: "BAI\1", n_ref, then per reference n_bin, per bin {bin, n_chunk, n_chunk x {beg, end}}, n_intv, n_intv x ioffset; then
// n_no_coor.  The chunk table comes in (reference, bin) order with a bin's chunks in file order, so the bins of a reference stand in
// ascending number and the pseudo-bin 37450 -- {first record's start, last record's end}, {mapped, unmapped} -- is its last.  A
// reference without records has n_bin = 0 and n_intv = 0.  Nothing is read outside the arrays as their counts give them, and a table
// that is out of order or names a reference the file does not have is refused, not followed.
#pragma once
#include <cstdint>
#include <cstdio>
#include <vector>

namespace pp_bam_index_host {

constexpr int OK = 0, ERR_ARG = 4, ERR_LIMIT = 5;  // PP_OK, PP_ERR_ARG, PP_ERR_LIMIT
constexpr uint32_t PSEUDO_BIN = 37450;
constexpr uint64_t MAX_COFFSET = 1ull << 48;       // a virtual offset has 48 bits for the block's place in the file

struct Tables {
    uint32_t n_ref = 0;
    uint64_t n_chunk = 0;
    const uint64_t *chunk_key = nullptr;  // n_chunk: ref << 32 | bin, non-decreasing
    const uint64_t *chunk_beg = nullptr, *chunk_end = nullptr;
    const uint32_t *n_intv = nullptr;     // n_ref
    const uint64_t *lin_off = nullptr;    // n_ref + 1: where a reference's windows start in lin
    const uint64_t *lin = nullptr;        // lin_off[n_ref]
    const uint64_t *ref_beg = nullptr, *ref_end = nullptr, *mapped = nullptr, *unmapped = nullptr;  // n_ref; mapped + unmapped == 0: no records
    uint64_t n_no_coor = 0;
};

inline void put32(std::vector<uint8_t> &o, uint32_t v) { for (int i = 0; i < 4; i++) o.push_back((uint8_t)(v >> (8 * i))); }
inline void put64(std::vector<uint8_t> &o, uint64_t v) { for (int i = 0; i < 8; i++) o.push_back((uint8_t)(v >> (8 * i))); }

inline int refuse(char *msg, size_t cap, const char *what, unsigned long long a) {
    if (msg && cap) snprintf(msg, cap, "pp_bam_index: %s (%llu)", what, a);
    return ERR_ARG;
}

inline int serialise(const Tables &T, std::vector<uint8_t> *out, char *msg, size_t cap) {
    if (!out) return refuse(msg, cap, "null argument", 0);
    out->clear();
    if (T.n_ref > 0x7FFFFFFFu) return refuse(msg, cap, "a negative number of references", T.n_ref);
    if ((T.n_chunk && (!T.chunk_key || !T.chunk_beg || !T.chunk_end)) ||
        (T.n_ref && (!T.n_intv || !T.lin_off || !T.ref_beg || !T.ref_end || !T.mapped || !T.unmapped)))
        return refuse(msg, cap, "null table", 0);
    std::vector<uint8_t> &o = *out;
    const uint8_t magic[4] = {'B', 'A', 'I', 1};
    o.insert(o.end(), magic, magic + 4);
    put32(o, T.n_ref);
    uint64_t c = 0;
    for (uint32_t r = 0; r < T.n_ref; r++) {
        const bool any = T.mapped[r] + T.unmapped[r] != 0;
        const uint64_t c0 = c;
        uint64_t n_bin = 0;
        while (c < T.n_chunk && (T.chunk_key[c] >> 32) == r) {  // count the bins
            if (c > c0 && T.chunk_key[c] < T.chunk_key[c - 1]) return refuse(msg, cap, "the chunk table is out of order at chunk", c);
            if ((uint32_t)T.chunk_key[c] >= PSEUDO_BIN) return refuse(msg, cap, "a bin number outside the scheme at chunk", c);
            if (c == c0 || T.chunk_key[c] != T.chunk_key[c - 1]) n_bin++;
            c++;
        }
        if (c > c0 && !any) return refuse(msg, cap, "chunks of a reference without records", r);
        if (n_bin + 1 > 0x7FFFFFFFull) return refuse(msg, cap, "too many bins in reference", r);
        put32(o, (uint32_t)(n_bin + (any ? 1 : 0)));
        for (uint64_t i = c0; i < c;) {
            uint64_t j = i;
            while (j < c && T.chunk_key[j] == T.chunk_key[i]) j++;
            if (j - i > 0x7FFFFFFFull) return refuse(msg, cap, "too many chunks in one bin of reference", r);
            put32(o, (uint32_t)T.chunk_key[i]);
            put32(o, (uint32_t)(j - i));
            for (; i < j; i++) {
                put64(o, T.chunk_beg[i]);
                put64(o, T.chunk_end[i]);
            }
        }
        if (any) {
            put32(o, PSEUDO_BIN);
            put32(o, 2);
            put64(o, T.ref_beg[r]);
            put64(o, T.ref_end[r]);
            put64(o, T.mapped[r]);
            put64(o, T.unmapped[r]);
        }
        const uint32_t n_intv = T.n_intv[r];
        if (n_intv > 0x7FFFFFFFu || T.lin_off[r + 1] < T.lin_off[r] || T.lin_off[r + 1] - T.lin_off[r] != n_intv || (n_intv && !T.lin))
            return refuse(msg, cap, "the windows of a reference do not fit their table, reference", r);
        put32(o, n_intv);
        for (uint32_t w = 0; w < n_intv; w++) put64(o, T.lin[T.lin_off[r] + w]);
    }
    if (c != T.n_chunk) return refuse(msg, cap, "a chunk of a reference the file does not have, or out of order, chunk", c);
    put64(o, T.n_no_coor);
    return OK;
}

}  // namespace pp_bam_index_host
