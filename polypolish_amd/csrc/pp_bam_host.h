// pp_bam_host.h -- the two host walks over uncompressed BAM bytes behind pp_bam_header / pp_bam_walk (pp_bam.hip): plain C++ with no
// HIP in it, so that a stand-alone program can run them under a sanitizer (tools/bam_host_check.cpp).  Neither reads a byte outside
// [0, n_bytes), and neither forms a sum that could wrap: every length is compared with what is LEFT of the array.
// step() -- one record of the block_size chain -- is also what the kernels of the device walk run (pp_bam_walk.hip), and
// walk_message() words a break for both walks: one definition for both sides, so that both refuse the same bytes in the same words.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>

#if defined(__HIPCC__)
#define PP_BAM_HD __host__ __device__
#else
#define PP_BAM_HD
#endif

namespace pp_bam_host {

constexpr int OK = 0, ERR_ARG = 4;  // PP_OK, PP_ERR_ARG

PP_BAM_HD inline uint32_t le32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// what one step of the chain finds, in the order it is looked for; W_START is the walk's own (a start behind the bytes)
enum : uint32_t { W_OK = 0, W_CUT = 1, W_SMALL = 2, W_PAST = 3, W_START = 4 };

// the verdict over a record of which `left` bytes exist, bs = its block_size word (looked at only where left >= 4)
PP_BAM_HD inline uint32_t step_kind(uint64_t left, uint32_t bs) {
    if (left < 4) return W_CUT;
    if (bs < 32) return W_SMALL;
    if ((uint64_t)bs > left - 4) return W_PAST;
    return W_OK;
}

// one record at `at` <= n_bytes: W_OK and *next = the offset behind it (> at, <= n_bytes), or what is wrong with it; *bs = its
// block_size word where the bytes hold one
PP_BAM_HD inline uint32_t step(const uint8_t *bytes, uint64_t n_bytes, uint64_t at, uint64_t *next, uint32_t *bs) {
    const uint64_t left = n_bytes - at;
    *bs = left >= 4 ? le32(bytes + at) : 0u;
    const uint32_t kind = step_kind(left, *bs);
    if (kind == W_OK) *next = at + 4 + (uint64_t)*bs;
    return kind;
}

// the message of a walk that stopped: record n at offset `at` with block_size bs (W_START: at = the start, n_bytes = the bytes)
inline void walk_message(char *msg, size_t msg_cap, uint32_t kind, uint64_t n, uint64_t at, uint32_t bs, uint64_t n_bytes) {
    if (!msg || !msg_cap) return;
    const unsigned long long N = n, A = at;
    switch (kind) {
    case W_CUT: snprintf(msg, msg_cap, "pp_bam_walk: the bytes end inside the block_size of record %llu (offset %llu)", N, A); break;
    case W_SMALL: snprintf(msg, msg_cap, "pp_bam_walk: record %llu has a block_size of %llu, below the 32 bytes of its fixed part", N, (unsigned long long)bs); break;
    case W_PAST: snprintf(msg, msg_cap, "pp_bam_walk: record %llu (offset %llu) runs past the end of the bytes", N, A); break;
    case W_START: snprintf(msg, msg_cap, "pp_bam_walk: the start %llu lies behind the %llu bytes", A, (unsigned long long)n_bytes); break;
    default: msg[0] = 0;
    }
}

inline int fail(char *msg, size_t msg_cap, const char *fmt, unsigned long long a = 0, unsigned long long b = 0) {
    if (msg && msg_cap) snprintf(msg, msg_cap, fmt, a, b);
    return ERR_ARG;
}

// magic, l_text, text, n_ref, then l_name, name, l_ref per reference
inline int header(const uint8_t *bytes, uint64_t n_bytes, uint32_t cap, uint32_t *n_ref, uint64_t *name_off, uint32_t *name_len,
                  uint32_t *ref_len, uint64_t *records_at, char *msg, size_t msg_cap) {
    if (n_ref) *n_ref = 0;
    if (records_at) *records_at = 0;
    if (!n_ref || !records_at || (n_bytes && !bytes) || (cap && (!name_off || !name_len || !ref_len)))
        return fail(msg, msg_cap, "pp_bam_header: null argument");
    if (n_bytes < 12) return fail(msg, msg_cap, "pp_bam_header: %llu bytes hold no BAM header", n_bytes);
    if (memcmp(bytes, "BAM\1", 4) != 0) return fail(msg, msg_cap, "pp_bam_header: the bytes do not start with the magic BAM\\1");
    const uint32_t l_text = le32(bytes + 4);
    uint64_t at = 8;
    if (l_text > 0x7FFFFFFFu || (uint64_t)l_text > n_bytes - at || n_bytes - at - l_text < 4)
        return fail(msg, msg_cap, "pp_bam_header: the header text of %llu bytes does not fit the %llu bytes", l_text, n_bytes);
    at += l_text;
    const uint32_t n = le32(bytes + at);
    at += 4;
    if (n > 0x7FFFFFFFu) return fail(msg, msg_cap, "pp_bam_header: a negative number of references");
    for (uint32_t i = 0; i < n; i++) {
        if (n_bytes - at < 4) return fail(msg, msg_cap, "pp_bam_header: the bytes end inside reference %llu of %llu", i, n);
        const uint32_t l_name = le32(bytes + at);
        at += 4;
        if (l_name == 0 || l_name > 0x7FFFFFFFu || (uint64_t)l_name > n_bytes - at || n_bytes - at - l_name < 4)
            return fail(msg, msg_cap, "pp_bam_header: the name of reference %llu (l_name %llu) does not fit the bytes", i, l_name);
        if (bytes[at + l_name - 1] != 0) return fail(msg, msg_cap, "pp_bam_header: the name of reference %llu does not end with a NUL", i);
        if (i < cap) {
            name_off[i] = at;
            name_len[i] = l_name - 1;
            ref_len[i] = le32(bytes + at + l_name);
        }
        at += (uint64_t)l_name + 4;
    }
    *n_ref = n;
    *records_at = at;
    if (n > cap) return fail(msg, msg_cap, "pp_bam_header: %llu references, room for %llu", n, cap);
    return OK;
}

// the block_size chain from `from`: stops at n_bytes, or after `cap` records when there is an array to fill
inline int walk(const uint8_t *bytes, uint64_t n_bytes, uint64_t from, uint64_t *rec_off, uint64_t cap, uint64_t *n_rec, uint64_t *end,
                char *msg, size_t msg_cap) {
    if (n_rec) *n_rec = 0;
    if (end) *end = from;
    if (!n_rec || !end || (n_bytes && !bytes)) return fail(msg, msg_cap, "pp_bam_walk: null argument");
    if (from > n_bytes) {
        walk_message(msg, msg_cap, W_START, 0, from, 0, n_bytes);
        return ERR_ARG;
    }
    const bool fill = rec_off && cap;
    uint64_t at = from, n = 0;
    while (at < n_bytes && !(fill && n == cap)) {
        uint64_t next = at;
        uint32_t bs = 0;
        const uint32_t kind = step(bytes, n_bytes, at, &next, &bs);
        if (kind != W_OK) {
            walk_message(msg, msg_cap, kind, n, at, bs, n_bytes);
            *n_rec = n;
            *end = at;
            return ERR_ARG;
        }
        if (fill) rec_off[n] = at;
        n++;
        at = next;
    }
    *n_rec = n;
    *end = at;
    return OK;
}

}  // namespace pp_bam_host
