// pp_tabix_host.h -- the host side of pp_tabix_index (pp_tabix.hip): the name list checked, and the tables the device made written out
// as the tabix specification lays a .tbi out.  Plain C++ with no HIP in it, so that a stand-alone program can run it under a sanitizer
// (tools/tabix_host_check.cpp).
//
// The bytes: "TBI\1", the int32 fields n_ref, format, col_seq, col_beg, col_end, meta, skip, l_nm, the names each closed by a NUL, and
// from there on what a .bai holds behind its n_ref (pp_bam_index_host.h's serialise writes it): per name n_bin, the bins
// {bin, n_chunk, chunks}, the pseudo-bin 37450 {first line's start, last line's end}, {lines, 0}, n_intv, ioff[]; then the uint64
// n_no_coor.  Nothing is read outside the arrays as their counts give them.
#pragma once
#include "pp_bam_index_host.h"

#include <algorithm>
#include <cstring>

namespace pp_tabix_host {

namespace ih = pp_bam_index_host;

constexpr int OK = ih::OK, ERR_ARG = ih::ERR_ARG, ERR_LIMIT = ih::ERR_LIMIT;
constexpr uint64_t MAX_NAMES = 1ull << 24, MAX_L_NM = 1ull << 31;  // l_nm is an int32

struct Head {
    int32_t format = 0, col_seq = 0, col_beg = 0, col_end = 0, meta = '#', skip = 0;
};

// Name h is names[name_off[h], name_off[h + 1]).  The first name, in order, that stood in the list before: its index, or n_names where
// the names are distinct.  (Sorted indices, equal names side by side in index order: the second of each group came back.)
inline uint64_t first_repeat(const uint8_t *names, const uint64_t *name_off, uint64_t n_names) {
    if (!n_names || !name_off) return n_names;
    std::vector<uint64_t> ix((size_t)n_names);
    for (uint64_t i = 0; i < n_names; i++) ix[(size_t)i] = i;
    const auto cmp = [&](uint64_t a, uint64_t b) {  // -1, 0, 1 by the bytes, the shorter of two with a common front first
        const uint64_t la = name_off[a + 1] - name_off[a], lb = name_off[b + 1] - name_off[b], m = std::min(la, lb);
        const int c = m ? memcmp(names + name_off[a], names + name_off[b], (size_t)m) : 0;
        return c ? (c < 0 ? -1 : 1) : (la < lb ? -1 : la > lb ? 1 : 0);
    };
    std::sort(ix.begin(), ix.end(), [&](uint64_t a, uint64_t b) {
        const int c = cmp(a, b);
        return c ? c < 0 : a < b;
    });
    uint64_t first = n_names;
    for (size_t i = 1; i < ix.size(); i++)
        if (cmp(ix[i - 1], ix[i]) == 0 && (i < 2 || cmp(ix[i - 2], ix[i]) != 0)) first = std::min(first, ix[i]);
    return first;
}

inline int refuse(char *msg, size_t cap, int code, const char *what, unsigned long long a) {
    if (msg && cap) snprintf(msg, cap, "pp_tabix_index: %s (%llu)", what, a);
    return code;
}

// T.n_ref names; T.mapped[r] = the lines of name r, T.unmapped[r] = 0
inline int serialise(const ih::Tables &T, const Head &H, const uint8_t *names, const uint64_t *name_off, std::vector<uint8_t> *out, char *msg,
                     size_t cap) {
    if (!out) return refuse(msg, cap, ERR_ARG, "null argument", 0);
    out->clear();
    if (T.n_ref > MAX_NAMES) return refuse(msg, cap, ERR_LIMIT, "more than 2^24 names", T.n_ref);
    if (T.n_ref && !name_off) return refuse(msg, cap, ERR_ARG, "null name table", 0);
    uint64_t l_nm = 0;
    for (uint32_t r = 0; r < T.n_ref; r++) {
        if (name_off[r + 1] <= name_off[r]) return refuse(msg, cap, ERR_ARG, "an empty name, or name offsets that decrease, name", r);
        l_nm += name_off[r + 1] - name_off[r] + 1;
        if (l_nm >= MAX_L_NM) return refuse(msg, cap, ERR_LIMIT, "the names and their NULs take 2^31 bytes or more, at name", r);
    }
    if (l_nm && !names) return refuse(msg, cap, ERR_ARG, "null names", 0);
    std::vector<uint8_t> body;
    if (int rc = ih::serialise(T, &body, msg, cap)) return rc;
    std::vector<uint8_t> &o = *out;
    o.reserve(36 + (size_t)l_nm + body.size());
    const uint8_t magic[4] = {'T', 'B', 'I', 1};
    o.insert(o.end(), magic, magic + 4);
    ih::put32(o, T.n_ref);
    ih::put32(o, (uint32_t)H.format);
    ih::put32(o, (uint32_t)H.col_seq);
    ih::put32(o, (uint32_t)H.col_beg);
    ih::put32(o, (uint32_t)H.col_end);
    ih::put32(o, (uint32_t)H.meta);
    ih::put32(o, (uint32_t)H.skip);
    ih::put32(o, (uint32_t)l_nm);
    for (uint32_t r = 0; r < T.n_ref; r++) {
        o.insert(o.end(), names + name_off[r], names + name_off[r + 1]);
        o.push_back(0);
    }
    o.insert(o.end(), body.begin() + 8, body.end());  // (behind "BAI\1" and n_ref)
    return OK;
}

}  // namespace pp_tabix_host
