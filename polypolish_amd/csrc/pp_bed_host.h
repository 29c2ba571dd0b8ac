// pp_bed_host.h -- the host part of pp_status_bed, pp_polish_bed and pp_polish_masked (pp_k_bed.h, pp_polish_text.hip): plain C++ with no
// HIP in it, as pp_vcf_host.h, so that a stand-alone program can run it under a sanitizer (tools/bed_host_check.cpp).  It holds the
// argument checks, the name table the kernels read, the parse of a status list (the commands' --bed_status) and the arithmetic of one
// BED line -- its length and its k-th byte -- as constexpr functions: the text kernel calls the very same ones, so the digit widths
// the GPU tests cannot reach (offsets of 10 decimal digits) are checked on the CPU.  tests/bed_model.py defines the bytes.
// plan() reads contig_off[0, n], names[0, n) and every name up to its NUL, and nothing else.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace pp_bed_host {

constexpr int OK = 0, ERR_ARG = 4, ERR_LIMIT = 5;  // PP_OK, PP_ERR_ARG, PP_ERR_LIMIT
constexpr uint64_t TEXT_LIMIT = 1ull << 40;        // a text of this many bytes or more is refused
constexpr uint32_t N_STATUS = 6;                   // PP_ST_KEPT .. PP_ST_TOO_CLOSE
constexpr uint32_t MASK_ALL = (1u << N_STATUS) - 1u;
constexpr uint32_t MASK_UNDECIDED = (1u << 2) | (1u << 3) | (1u << 4) | (1u << 5);  // PP_BED_UNDECIDED

// ---- one line: name \t start \t end \t word \n -------------------------------------------------------------------------------
// the reference's own word for a status (src/pileup.rs:156-163)
constexpr const char *word(uint32_t st) {
    switch (st) {
    case 0: return "kept";
    case 1: return "changed";
    case 2: return "low_depth";
    case 3: return "none";
    case 4: return "multiple";
    default: return "too_close";
    }
}
constexpr uint32_t word_len(uint32_t st) { return st == 0 || st == 3 ? 4u : (st == 1 ? 7u : (st == 4 ? 8u : 9u)); }
constexpr uint32_t ndig(uint64_t v) {
    uint32_t n = 1;
    for (; v >= 10u; v /= 10u) n++;
    return n;
}
constexpr uint64_t line_len(uint64_t name_len, uint64_t a, uint64_t b, uint32_t st) { return name_len + ndig(a) + ndig(b) + word_len(st) + 4u; }
// the decimal digit of v that has `behind` digits behind it
constexpr uint32_t digit(uint64_t v, uint32_t behind) {
    for (; behind > 0u; behind--) v /= 10u;
    return (uint32_t)'0' + (uint32_t)(v % 10u);
}
// byte k of the line (k < line_len): na = ndig(a), nb = ndig(b)
constexpr uint32_t line_byte(const uint8_t *name, uint64_t name_len, uint64_t a, uint32_t na, uint64_t b, uint32_t nb, uint32_t st, uint64_t k) {
    if (k < name_len) return name[k];
    k -= name_len;
    if (k == 0u) return (uint32_t)'\t';
    k -= 1u;
    if (k < na) return digit(a, na - 1u - (uint32_t)k);
    k -= na;
    if (k == 0u) return (uint32_t)'\t';
    k -= 1u;
    if (k < nb) return digit(b, nb - 1u - (uint32_t)k);
    k -= nb;
    if (k == 0u) return (uint32_t)'\t';
    k -= 1u;
    return k < word_len(st) ? (uint32_t)(uint8_t)word(st)[k] : (uint32_t)'\n';
}

// ---- the status list of --bed_status: comma-separated words, each one of the six ------------------------------------------------
// OK and *mask, or ERR_ARG with what is wrong in msg: an empty list, an empty item, an unknown word.  Reads list[0, len) only.
inline int parse_status_list(const char *list, size_t len, uint32_t *mask, char *msg, size_t cap) {
    *mask = 0;
    if (msg && cap) msg[0] = 0;
    if (!list || len == 0) {
        if (msg && cap) snprintf(msg, cap, "an empty status list");
        return ERR_ARG;
    }
    size_t at = 0;
    for (;;) {
        size_t end = at;
        while (end < len && list[end] != ',') end++;
        uint32_t st = N_STATUS;
        for (uint32_t s = 0; s < N_STATUS; s++)
            if (end - at == word_len(s) && memcmp(list + at, word(s), end - at) == 0) st = s;
        if (st == N_STATUS) {
            if (msg && cap) snprintf(msg, cap, "'%.*s' is not one of kept, changed, low_depth, none, multiple, too_close", (int)(end - at > 64 ? 64 : end - at), list + at);
            *mask = 0;
            return ERR_ARG;
        }
        *mask |= 1u << st;
        if (end == len) return OK;
        at = end + 1;  // (a comma at the end leaves an empty item: refused above on the next turn)
    }
}

// ---- the calls' arguments ------------------------------------------------------------------------------------------------------
struct JobState {  // of the context a pp_polish_* call is made on
    bool finished;   // a pp_polish_finish succeeded and no pp_polish_begin followed (a job that ended in an error leaves none)
    bool debug;      // ... with pp_polish_set_debug(ctx, 1): the job kept its per-position status
    bool emit_set;   // pp_polish_set_emit ranges: a rank's share has no defined runs at its edges
};

struct Plan {
    std::string names;               // the contig names, one behind the other ...
    std::vector<uint64_t> name_off;  // ... n + 1 offsets into them
    uint64_t G = 0;                  // contig_off[n]
};

inline int fail(int code, char *msg, size_t cap, const char *who, const char *what) {
    if (msg && cap) snprintf(msg, cap, "%s: %s", who, what);
    return code;
}

inline int check_mask(const char *who, uint32_t mask, char *msg, size_t cap) {
    if (mask == 0u) return fail(ERR_ARG, msg, cap, who, "a status mask of 0 selects nothing");
    if (mask & ~MASK_ALL) return fail(ERR_ARG, msg, cap, who, "a status mask with a bit above 5 (1 << PP_ST_TOO_CLOSE is the highest)");
    return OK;
}

// the state of the job, for the calls that read the job's own arrays
inline int check_job(const char *who, const JobState &S, char *msg, size_t cap) {
    if (!S.finished) return fail(ERR_ARG, msg, cap, who, "no finished polish job on this context (a job that ended in an error leaves none)");
    if (!S.debug) return fail(ERR_ARG, msg, cap, who, "the job kept no per-position status: pp_polish_set_debug(ctx, 1) before pp_polish_finish");
    if (S.emit_set) return fail(ERR_ARG, msg, cap, who, "the context has pp_polish_set_emit ranges: a rank's share has no defined runs at its edges");
    return OK;
}

// Judged in this order: null arguments, the memory kind (mem_ok: HOST or DEVICE), the mask, the offsets (they begin at 0, never
// decrease and end below 2^32), a null name, a name that holds a tab or a newline.  have_status: the status pointer is not null
// (with no position at all nobody reads it, but a null one is refused all the same).
inline int plan(const char *who, bool have_out, bool have_status, bool mem_ok, uint32_t n, const uint64_t *contig_off, const char *const *names,
                uint32_t mask, Plan &P, char *msg, size_t cap) {
    P = Plan();
    if (!have_out || !have_status || !names || !contig_off) return fail(ERR_ARG, msg, cap, who, "null argument");
    if (!mem_ok) return fail(ERR_ARG, msg, cap, who, "the status bytes are PP_MEM_HOST or PP_MEM_DEVICE");
    if (int rc = check_mask(who, mask, msg, cap)) return rc;
    if (contig_off[0] != 0u) return fail(ERR_ARG, msg, cap, who, "contig_off[0] is not 0");
    for (uint32_t c = 0; c < n; c++)
        if (contig_off[c + 1] < contig_off[c]) return fail(ERR_ARG, msg, cap, who, "contig offsets that decrease");
    if (contig_off[n] >= (1ull << 32)) return fail(ERR_ARG, msg, cap, who, "2^32 positions or more");
    P.G = contig_off[n];
    P.name_off.assign((size_t)n + 1, 0);
    for (uint32_t c = 0; c < n; c++) {
        if (!names[c]) return fail(ERR_ARG, msg, cap, who, "a contig name is NULL");
        const size_t len = strlen(names[c]);
        if (memchr(names[c], '\t', len) || memchr(names[c], '\n', len)) return fail(ERR_ARG, msg, cap, who, "a contig name that holds a tab or a newline");
        P.name_off[c + 1] = P.name_off[c] + len;
    }
    P.names.reserve((size_t)P.name_off[n]);
    for (uint32_t c = 0; c < n; c++) P.names += names[c];
    return OK;
}

// the text's size is known once the device has scanned the lines' lengths: judged before the text is allocated
inline int text_size(const char *who, uint64_t n_bytes, char *msg, size_t cap) {
    return n_bytes >= TEXT_LIMIT ? fail(ERR_LIMIT, msg, cap, who, "a text of 2^40 bytes or more") : OK;
}

}  // namespace pp_bed_host
