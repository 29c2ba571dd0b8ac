// pp_fasta_out_host.h -- the host part of pp_fasta_text (pp_fasta_out.hip) and of pp_bgzf_out_gzi (pp_bgzf_deflate.hip): what is
// proportional to the number of contigs (or of BGZF blocks), plain C++ with no HIP in it, as pp_fasta_host.h, so that a stand-alone
// program can run it under a sanitizer (tools/fasta_out_host_check.cpp).  plan() checks the caller's arguments and builds the table
// the kernel reads; fai() and gzi() write the two indexes from the same tables.  tests/fasta_text_model.py defines the bytes.
// It reads contig_off[0, n], header_off[0, n] and the header bytes [header_off[0], header_off[n]) -- those only once every size is
// known to be below the limit -- and no base.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace pp_fasta_out_host {

constexpr int OK = 0, ERR_ARG = 4, ERR_LIMIT = 5;  // PP_OK, PP_ERR_ARG, PP_ERR_LIMIT
constexpr uint64_t TEXT_LIMIT = 1ull << 40;        // a text of this many bytes or more is refused
constexpr uint64_t WIDTH_MAX = 0x7FFFFFFFull;
constexpr uint64_t GZI_PIECE = 65280;              // the uncompressed bytes of every BGZF block but the last (pp_bgzf_deflate)

struct Row {  // one contig as the kernel sees it; row n_contigs closes the table: hdr_at = the text's length
    uint64_t hdr_at;    // text offset of its '>'
    uint64_t body_at;   // text offset of its first body byte (behind the header's "\n")
    uint64_t base_off;  // of its first base in `bases`
    uint64_t len;       // its bases
    uint64_t hsrc;      // of its header's first byte in the uploaded header bytes
};

struct Plan {
    std::vector<Row> rows;  // n_contigs + 1
    uint64_t n_text = 0;    // bytes of text
    uint64_t n_hdr = 0;     // header bytes to upload: headers[header_off[0], header_off[n])
    uint64_t n_bases = 0;   // contig_off[n] - contig_off[0]
};

inline int fail(int code, char *msg, size_t cap, const char *what) {
    if (msg && cap) snprintf(msg, cap, "pp_fasta_text: %s", what);
    return code;
}

// the bytes of a body of L bases at width W (0: one line), L < 2^40
inline uint64_t body_bytes(uint64_t L, uint64_t W) { return W == 0 ? L + 1 : L + (L + W - 1) / W; }

// The arguments of pp_fasta_text, judged in this order: null arguments and the memory form (ERR_ARG), the width (ERR_LIMIT), offsets
// that decrease (ERR_ARG), the sizes (ERR_LIMIT), and only then -- every range is now known to be small -- null arrays with bytes
// to read and a header that holds "\n" (ERR_ARG).  mem_ok: the caller's mem is host or device memory.
inline int plan(bool have_bases, bool mem_ok, uint32_t n, const uint64_t *contig_off, const uint8_t *headers, const uint64_t *header_off,
                uint64_t width, Plan &P, char *msg, size_t cap) {
    P = Plan();
    if (!contig_off || !header_off) return fail(ERR_ARG, msg, cap, "null argument");
    if (!mem_ok) return fail(ERR_ARG, msg, cap, "the bases must be host memory or memory of the context's device");
    if (width > WIDTH_MAX) return fail(ERR_LIMIT, msg, cap, "a line width above 2^31-1");
    for (uint32_t c = 0; c < n; c++)
        if (contig_off[c + 1] < contig_off[c] || header_off[c + 1] < header_off[c]) return fail(ERR_ARG, msg, cap, "offsets that decrease");
    uint64_t at = 0;
    for (uint32_t c = 0; c < n; c++) {
        const uint64_t L = contig_off[c + 1] - contig_off[c], H = header_off[c + 1] - header_off[c];
        if (L >= TEXT_LIMIT || H >= TEXT_LIMIT) return fail(ERR_LIMIT, msg, cap, "a text of 2^40 bytes or more");
        at += 2 + H + body_bytes(L, width);  // (each term below 2^41, the sum checked every round: no wrap)
        if (at >= TEXT_LIMIT) return fail(ERR_LIMIT, msg, cap, "a text of 2^40 bytes or more");
    }
    P.n_text = at;
    P.n_bases = n ? contig_off[n] - contig_off[0] : 0;
    P.n_hdr = n ? header_off[n] - header_off[0] : 0;
    if (P.n_bases && !have_bases) return fail(ERR_ARG, msg, cap, "null bases with bytes to copy");
    if (P.n_hdr && !headers) return fail(ERR_ARG, msg, cap, "null headers with header bytes");
    if (P.n_hdr && memchr(headers + header_off[0], '\n', (size_t)P.n_hdr)) return fail(ERR_ARG, msg, cap, "a header that holds a newline");
    P.rows.resize((size_t)n + 1);
    at = 0;
    for (uint32_t c = 0; c < n; c++) {
        const uint64_t L = contig_off[c + 1] - contig_off[c], H = header_off[c + 1] - header_off[c];
        P.rows[c] = Row{at, at + 2 + H, contig_off[c] - contig_off[0], L, header_off[c] - header_off[0]};
        at += 2 + H + body_bytes(L, width);
    }
    P.rows[n] = Row{at, at, P.n_bases, 0, P.n_hdr};
    return OK;
}

// the .fai text of a plan: name \t L \t offset \t linebases \t linewidth \n, the name ending at the header's first space or tab
inline void fai(const Plan &P, const uint8_t *headers, const uint64_t *header_off, uint64_t width, std::string &out) {
    out.clear();
    char num[96];
    for (size_t c = 0; c + 1 < P.rows.size(); c++) {
        const uint8_t *h = headers ? headers + header_off[c] : nullptr;
        size_t k = 0;
        const size_t H = (size_t)(header_off[c + 1] - header_off[c]);
        while (k < H && h[k] != ' ' && h[k] != '\t') k++;
        if (k) out.append((const char *)h, k);
        const uint64_t L = P.rows[c].len, lb = width == 0 || L < width ? L : width;
        snprintf(num, sizeof num, "\t%llu\t%llu\t%llu\t%llu\n", (unsigned long long)L, (unsigned long long)P.rows[c].body_at,
                 (unsigned long long)lb, (unsigned long long)(L ? lb + 1 : 0));
        out += num;
    }
}

// the .gzi bytes of a file of n_blk blocks in front of its EOF block (blk_off: n_blk + 1 offsets, the EOF block's last): little-endian,
// a count, then per block except the first its offset in the file and the uncompressed bytes in front of it
inline void gzi(const uint64_t *blk_off, uint64_t n_blk, std::string &out) {
    const uint64_t n = n_blk ? n_blk - 1 : 0;
    out.clear();
    out.reserve((size_t)(8 + 16 * n));
    auto put = [&out](uint64_t v) {
        for (int i = 0; i < 8; i++) out.push_back((char)(v >> (8 * i)));
    };
    put(n);
    for (uint64_t b = 1; b <= n; b++) {
        put(blk_off[b]);
        put(b * GZI_PIECE);
    }
}

}  // namespace pp_fasta_out_host
