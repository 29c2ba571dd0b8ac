// pp_sam_host.h -- the host walk over the header of a SAM text behind pp_sam_header (pp_sam_bam.hip): plain C++ with no HIP in it, as
// pp_bam_host.h, so that a stand-alone program can run it under a sanitizer.  It never reads a byte outside [0, n_bytes): a line ends
// at the first '\n' inside the bytes or at n_bytes, and every field is searched inside its line.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string_view>
#include <unordered_set>

namespace pp_sam_host {

constexpr int OK = 0, ERR_QUIT = 1, ERR_ARG = 4;  // PP_OK, PP_ERR_QUIT, PP_ERR_ARG

inline int fail(int code, char *msg, size_t msg_cap, const char *fmt, unsigned long long a = 0, unsigned long long b = 0) {
    if (msg && msg_cap) snprintf(msg, msg_cap, fmt, a, b);
    return code;
}

// the value of the first field of line [s, e) that begins with the three bytes `key` (behind the first column): its range, or false
inline bool field(const uint8_t *t, uint64_t s, uint64_t e, const char *key, uint64_t *vs, uint64_t *ve) {
    uint64_t at = s;
    bool first = true;
    while (at <= e) {
        const void *tab = at < e ? memchr(t + at, '\t', (size_t)(e - at)) : nullptr;
        const uint64_t fe = tab ? (uint64_t)((const uint8_t *)tab - t) : e;
        if (!first && fe - at >= 3 && memcmp(t + at, key, 3) == 0) {
            *vs = at + 3;
            *ve = fe;
            return true;
        }
        first = false;
        at = fe + 1;
    }
    return false;
}

// The leading run of lines that begin with '@'.  *header_end = the offset of the first line that is no header line, *n_lines the
// number of header lines; per @SQ line (first column exactly "@SQ") the SN: value's range and LN:.  On ERR_QUIT *bad_line = the
// 0-based line.
inline int header(const uint8_t *text, uint64_t n_bytes, uint32_t cap, uint32_t *n_ref, uint64_t *name_off, uint32_t *name_len,
                  uint32_t *ref_len, uint64_t *header_end, uint64_t *n_lines, uint64_t *bad_line, char *msg, size_t msg_cap) {
    if (n_ref) *n_ref = 0;
    if (header_end) *header_end = 0;
    if (n_lines) *n_lines = 0;
    if (bad_line) *bad_line = ~0ull;
    if (!n_ref || !header_end || (n_bytes && !text) || (cap && (!name_off || !name_len || !ref_len)))
        return fail(ERR_ARG, msg, msg_cap, "pp_sam_header: null argument");
    std::unordered_set<std::string_view> seen;
    uint64_t at = 0, line = 0;
    uint32_t n = 0;
    while (at < n_bytes && text[at] == (uint8_t)'@') {
        const void *nl = memchr(text + at, '\n', (size_t)(n_bytes - at));
        const uint64_t le = nl ? (uint64_t)((const uint8_t *)nl - text) : n_bytes;
        uint64_t ce = le;
        if (ce > at && text[ce - 1] == (uint8_t)'\r') ce--;
        const bool sq = ce - at >= 3 && memcmp(text + at, "@SQ", 3) == 0 && (ce - at == 3 || text[at + 3] == (uint8_t)'\t');
        if (sq) {
            uint64_t vs = 0, ve = 0;
            if (bad_line) *bad_line = line;
            if (!field(text, at, ce, "SN:", &vs, &ve) || ve == vs)
                return fail(ERR_QUIT, msg, msg_cap, "pp_sam_header: the @SQ line %llu has no SN: name", line + 1);
            const uint64_t ns = vs, ne = ve;
            uint64_t ln = 0;
            bool ok = field(text, at, ce, "LN:", &vs, &ve) && ve > vs;
            for (uint64_t i = vs; ok && i < ve; i++) {
                if (text[i] < (uint8_t)'0' || text[i] > (uint8_t)'9') ok = false;
                else if ((ln = ln * 10 + (uint64_t)(text[i] - (uint8_t)'0')) > 0x7FFFFFFFull) ok = false;
            }
            if (!ok || ln == 0)
                return fail(ERR_QUIT, msg, msg_cap, "pp_sam_header: the @SQ line %llu has no LN: length in 1 .. 2147483647", line + 1);
            if (ne - ns > 0x7FFFFFFEull) return fail(ERR_QUIT, msg, msg_cap, "pp_sam_header: the @SQ line %llu has a name beyond l_name", line + 1);
            if (!seen.insert(std::string_view((const char *)text + ns, (size_t)(ne - ns))).second)
                return fail(ERR_QUIT, msg, msg_cap, "pp_sam_header: the @SQ line %llu names a reference a second time", line + 1);
            if (bad_line) *bad_line = ~0ull;
            if (n == 0x7FFFFFFFu) return fail(ERR_QUIT, msg, msg_cap, "pp_sam_header: more than 2147483647 @SQ lines (line %llu)", line + 1);
            if (n < cap) {
                name_off[n] = ns;
                name_len[n] = (uint32_t)(ne - ns);
                ref_len[n] = (uint32_t)ln;
            }
            n++;
        }
        line++;
        at = le < n_bytes ? le + 1 : n_bytes;
    }
    *n_ref = n;
    *header_end = at;
    if (n_lines) *n_lines = line;
    if (n > cap) return fail(ERR_ARG, msg, msg_cap, "pp_sam_header: %llu references, room for %llu", n, cap);
    return OK;
}

}  // namespace pp_sam_host
