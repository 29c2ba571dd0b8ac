// pp_bam_sort_host.h -- the host side of pp_bam_sort (pp_bam_sort.hip): the BAM header of a coordinate-sorted file.  Plain C++ with no
// HIP in it, so that a stand-alone program can run it under a sanitizer (tools/bam_sort_host_check.cpp).  No byte outside
// [0, records_at) is read: the header is walked by pp_bam_host::header first, and the text is looked at only inside its l_text bytes.
//
// head_sorted: bytes[0, records_at) -- magic, l_text, text, n_ref, the reference table -- with the text's FIRST line made to say
// SO:coordinate.  The text is what stands in front of its trailing NULs; the NULs are kept, byte for byte, behind the new text.
//   the first line is an @HD line ("@HD" alone or followed by a tab) with an SO: field   the first such field becomes SO:coordinate
//   ... without an SO: field                                                             "\tSO:coordinate" is appended to the line
//   anything else, no text included                                                      "@HD\tVN:1.6\tSO:coordinate\n" goes in front
// A line ends in front of its '\n' (or the text's end), and in front of a '\r' that stands there.  l_text is adjusted; the reference
// table is copied.
#pragma once
#include "pp_bam_host.h"

#include <vector>

namespace pp_bam_sort_host {

constexpr int OK = 0, ERR_ARG = 4, ERR_LIMIT = 5;  // PP_OK, PP_ERR_ARG, PP_ERR_LIMIT

inline void put(std::vector<uint8_t> &o, const char *s) { o.insert(o.end(), (const uint8_t *)s, (const uint8_t *)s + strlen(s)); }

// -> OK and *out = the rewritten header, *n_ref = its references; what pp_bam_header refuses: its code and its message; a header that
// ends elsewhere than at records_at: ERR_ARG; a text that would pass 2^31 - 1 bytes: ERR_LIMIT
inline int head_sorted(const uint8_t *bytes, uint64_t records_at, std::vector<uint8_t> *out, uint32_t *n_ref, char *msg, size_t msg_cap) {
    uint32_t n = 0;
    uint64_t at = 0;
    if (n_ref) *n_ref = 0;
    if (!out || !n_ref) return pp_bam_host::fail(msg, msg_cap, "pp_bam_sort: null argument");
    out->clear();
    const int rc = pp_bam_host::header(bytes, records_at, 0, &n, nullptr, nullptr, nullptr, &at, msg, msg_cap);
    if (rc != OK && at == 0) return rc;  // (at != 0: the walk reached the header's end and only had no room for the names)
    if (at != records_at) return pp_bam_host::fail(msg, msg_cap, "pp_bam_sort: the BAM header ends at %llu, not at records_at %llu", at, records_at);
    const uint64_t l_text = pp_bam_host::le32(bytes + 4);
    const uint8_t *const text = bytes + 8;
    uint64_t n_text = l_text;  // without the trailing NULs
    while (n_text && text[n_text - 1] == 0) n_text--;
    uint64_t eol = 0;  // the first line: [0, eol), its end mark(s) behind it
    while (eol < n_text && text[eol] != '\n') eol++;
    if (eol && text[eol - 1] == '\r') eol--;
    const bool hd = eol >= 3 && memcmp(text, "@HD", 3) == 0 && (eol == 3 || text[3] == '\t');
    std::vector<uint8_t> t;
    if (!hd) {
        put(t, "@HD\tVN:1.6\tSO:coordinate\n");
        t.insert(t.end(), text, text + n_text);
    } else {
        uint64_t so = eol, so_end = eol;  // the first field that starts with SO:
        for (uint64_t f = 3; f < eol;) {  // text[f] is the tab in front of a field
            uint64_t e = f + 1;
            while (e < eol && text[e] != '\t') e++;
            if (e - (f + 1) >= 3 && memcmp(text + f + 1, "SO:", 3) == 0) {
                so = f + 1;
                so_end = e;
                break;
            }
            f = e;
        }
        if (so < eol) {
            t.insert(t.end(), text, text + so);
            put(t, "SO:coordinate");
            t.insert(t.end(), text + so_end, text + n_text);
        } else {
            t.insert(t.end(), text, text + eol);
            put(t, "\tSO:coordinate");
            t.insert(t.end(), text + eol, text + n_text);
        }
    }
    const uint64_t l_new = (uint64_t)t.size() + (l_text - n_text);
    if (l_new > 0x7FFFFFFFull) {
        if (msg && msg_cap) snprintf(msg, msg_cap, "pp_bam_sort: the header text would have %llu bytes, above 2^31 - 1", (unsigned long long)l_new);
        return ERR_LIMIT;
    }
    out->reserve((size_t)(records_at - l_text + l_new));
    out->insert(out->end(), bytes, bytes + 4);
    for (int i = 0; i < 4; i++) out->push_back((uint8_t)(l_new >> (8 * i)));
    out->insert(out->end(), t.begin(), t.end());
    out->insert(out->end(), text + n_text, bytes + records_at);  // the NULs, n_ref, the reference table
    *n_ref = n;
    return OK;
}

}  // namespace pp_bam_sort_host
