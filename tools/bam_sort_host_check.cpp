// bam_sort_host_check.cpp -- a stand-alone program over the host side of pp_bam_sort (polypolish_amd/csrc/pp_bam_sort_host.h), made
// to be built with a sanitizer and run on a machine without a GPU, as tools/bam_host_check.cpp is for the BAM helpers:
//   clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ipolypolish_amd/csrc tools/bam_sort_host_check.cpp -o bam_sort_host_check
//   ./bam_sort_host_check
// Every prefix of each built-in header goes to head_sorted() in a heap block of EXACTLY its length (a read past the cut is a read
// past the allocation), then every prefix with one byte replaced by a tab, a newline, a NUL, 'S' or 0xFF.  The program checks that a
// refusal has its words and leaves no bytes, and that an answer is a BAM header again: it ends where it is long, has the references
// of the input byte for byte behind a text that keeps the input's trailing NULs, says SO:coordinate in its first line, and stays as
// it is when it goes in again; the sanitizer checks every load.
// The second part hands pp_bam_index_host.h's serialiser hand-built tables -- every array a heap block of EXACTLY its count, offsets
// near 2^48 << 16 -- and parses its bytes back; then every table with one chunk key altered, which must be refused or still parse.
#include "pp_bam_index_host.h"
#include "pp_bam_sort_host.h"

#include <cstdlib>
#include <string>

namespace hs = pp_bam_sort_host;

static std::string le32s(uint32_t v) {
    std::string s(4, '\0');
    for (int i = 0; i < 4; i++) s[i] = (char)(v >> (8 * i));
    return s;
}

static std::string header_of(const std::string &text) {
    std::string h = "BAM\1" + le32s((uint32_t)text.size()) + text + le32s(2);
    h += le32s(6) + std::string("ctg_a\0", 6) + le32s(5000);
    h += le32s(2) + std::string("b\0", 2) + le32s(70000);
    return h;
}

static uint64_t g_taken = 0;  // the calls that gave a header

static int check(const uint8_t *p, uint64_t n) {
    std::vector<uint8_t> out, again;
    uint32_t n_ref = 77, n_ref2 = 0;
    char msg[256];
    msg[0] = 0;
    const int rc = hs::head_sorted(p, n, &out, &n_ref, msg, sizeof msg);
    if (rc != hs::OK) {
        if (!msg[0] || !out.empty() || n_ref != 0) return fprintf(stderr, "a refusal without its words, or with bytes, at %llu bytes\n", (unsigned long long)n), 1;
        return 0;
    }
    // the answer is a header ...
    uint32_t n2 = 0;
    uint64_t at = 0;
    const int rc2 = pp_bam_host::header(out.data(), out.size(), 0, &n2, nullptr, nullptr, nullptr, &at, msg, sizeof msg);
    if ((rc2 != hs::OK && at == 0) || at != out.size() || n2 != n_ref) return fprintf(stderr, "the answer is no header at %llu bytes\n", (unsigned long long)n), 1;
    // ... with the input's NULs and table behind its text ...
    const uint64_t l_in = pp_bam_host::le32(p + 4), l_out = pp_bam_host::le32(out.data() + 4);
    uint64_t t_in = l_in, t_out = l_out;
    while (t_in && p[8 + t_in - 1] == 0) t_in--;
    while (t_out && out[8 + t_out - 1] == 0) t_out--;
    if (l_in - t_in != l_out - t_out || n - (8 + l_in) != out.size() - (8 + l_out) || memcmp(p + 8 + l_in, out.data() + 8 + l_out, (size_t)(n - 8 - l_in)) != 0)
        return fprintf(stderr, "the NULs or the reference table changed at %llu bytes\n", (unsigned long long)n), 1;
    // ... whose first line is an @HD line that says SO:coordinate ...
    const std::string text((const char *)out.data() + 8, (size_t)t_out);
    const std::string line = text.substr(0, text.find('\n'));
    if (line.compare(0, 3, "@HD") != 0 || (line.size() > 3 && line[3] != '\t') || line.find("\tSO:coordinate") == std::string::npos)
        return fprintf(stderr, "the first line does not say SO:coordinate at %llu bytes\n", (unsigned long long)n), 1;
    // ... and that stays as it is
    if (hs::head_sorted(out.data(), out.size(), &again, &n_ref2, msg, sizeof msg) != hs::OK || again != out || n_ref2 != n_ref)
        return fprintf(stderr, "the answer changes when it goes in again at %llu bytes\n", (unsigned long long)n), 1;
    g_taken++;
    return 0;
}

// ---- the .bai serialiser --------------------------------------------------------------------------------------------------------------
namespace ih = pp_bam_index_host;

template <class T>
static T *block_of(const std::vector<T> &v) {  // a heap block of exactly v's bytes (one byte where there are none)
    T *p = (T *)malloc(v.empty() ? 1 : v.size() * sizeof(T));
    if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

static uint64_t rd(const std::vector<uint8_t> &b, size_t &at, int n) {
    uint64_t v = 0;
    if (at + (size_t)n > b.size()) { at = (size_t)-1 / 2; return 0; }
    for (int i = 0; i < n; i++) v |= (uint64_t)b[at + i] << (8 * i);
    at += (size_t)n;
    return v;
}

// the bytes parse as a BAI of n_ref references and end where they are long; -> the number of chunks read, or -1
static long parse_bai(const std::vector<uint8_t> &b, uint32_t n_ref, uint64_t n_no_coor) {
    size_t at = 0;
    long chunks = 0;
    if (rd(b, at, 4) != 0x01494142u || rd(b, at, 4) != n_ref) return -1;
    for (uint32_t r = 0; r < n_ref; r++) {
        const uint64_t n_bin = rd(b, at, 4);
        uint64_t last = 0;
        for (uint64_t i = 0; i < n_bin && at <= b.size(); i++) {
            const uint64_t bin = rd(b, at, 4), n_chunk = rd(b, at, 4);
            if (i && bin <= last) return -1;  // ascending
            last = bin;
            if (bin == ih::PSEUDO_BIN && (n_chunk != 2 || i + 1 != n_bin)) return -1;
            for (uint64_t c = 0; c < n_chunk && at <= b.size(); c++, chunks++) { rd(b, at, 8); rd(b, at, 8); }
        }
        const uint64_t n_intv = rd(b, at, 4);
        for (uint64_t w = 0; w < n_intv && at <= b.size(); w++) rd(b, at, 8);
    }
    if (rd(b, at, 8) != n_no_coor || at != b.size()) return -1;
    return chunks;
}

static int check_serialiser() {
    const uint64_t FAR = ((1ull << 48) - 1) << 16 | 0xFEFF;  // the last block a virtual offset can name, its last byte
    // reference 0: bins 0, 585 (two chunks), 37448; reference 1: none; reference 2: one bin; windows 3 | 0 | 1
    const std::vector<uint64_t> key = {0ull, 585ull, 585ull, 37448ull, 2ull << 32 | 4681ull};
    const std::vector<uint64_t> beg = {100, 5000, FAR - 70000, 1ull << 63, FAR - 9}, end = {200, 6000, FAR - 100, (1ull << 63) + 5, FAR};
    const std::vector<uint32_t> n_intv = {3, 0, 1};
    const std::vector<uint64_t> lin_off = {0, 3, 3, 4}, lin = {100, 100, FAR - 70000, FAR - 9};
    const std::vector<uint64_t> rb = {100, 0, FAR - 9}, re = {(1ull << 63) + 5, 0, FAR}, mp = {3, 0, 1}, um = {1, 0, 0};
    uint64_t calls = 0;
    for (int alter = -1; alter < (int)key.size() * 3; alter++) {
        std::vector<uint64_t> k = key;
        if (alter >= 0) {
            uint64_t &x = k[(size_t)alter / 3];
            x = alter % 3 == 0 ? x + (1ull << 32) : alter % 3 == 1 ? (x & ~0xFFFFFFFFull) | 40000ull : 0xFFFFFFFFFFFFFFFFull;
        }
        ih::Tables T;
        T.n_ref = 3;
        T.n_chunk = k.size();
        uint64_t *pk = block_of(k), *pb = block_of(beg), *pe = block_of(end), *plo = block_of(lin_off), *pl = block_of(lin);
        uint64_t *prb = block_of(rb), *pre = block_of(re), *pmp = block_of(mp), *pum = block_of(um);
        uint32_t *pi = block_of(n_intv);
        T.chunk_key = pk; T.chunk_beg = pb; T.chunk_end = pe; T.n_intv = pi; T.lin_off = plo; T.lin = pl;
        T.ref_beg = prb; T.ref_end = pre; T.mapped = pmp; T.unmapped = pum;
        T.n_no_coor = 0xFFFFFFFFFFFFFFFEull;
        std::vector<uint8_t> out;
        char msg[200];
        msg[0] = 0;
        const int rc = ih::serialise(T, &out, msg, sizeof msg);
        calls++;
        if (alter < 0) {
            // 8 + ref 0: 4 + 3 bins (8 each) + 4 chunks (16 each) + pseudo 40 + 4 + 24 | ref 1: 8 | ref 2: 4 + 8 + 16 + 40 + 4 + 8 | 8
            if (rc != ih::OK || parse_bai(out, 3, T.n_no_coor) != 5 + 4 || out.size() != 8 + (4 + 24 + 64 + 40 + 4 + 24) + 8 + (4 + 8 + 16 + 40 + 4 + 8) + 8)
                return fprintf(stderr, "the hand-built tables: rc %d, %zu bytes\n", rc, out.size()), 1;
            size_t at = out.size() - 8 - 8 - 4 - 16 - 8;  // behind it: n_no_coor, one window, n_intv, {mapped, unmapped}: the end of reference 2's span
            if (rd(out, at, 8) != FAR) return fprintf(stderr, "an offset near 2^48 << 16 did not survive\n"), 1;
        } else if (rc == ih::OK ? parse_bai(out, 3, T.n_no_coor) < 0 : (!msg[0] || rc != ih::ERR_ARG))
            return fprintf(stderr, "altered key %d: rc %d, neither refused with words nor a file that parses\n", alter, rc), 1;
        for (void *q : {(void *)pk, (void *)pb, (void *)pe, (void *)plo, (void *)pl, (void *)prb, (void *)pre, (void *)pmp, (void *)pum, (void *)pi}) free(q);
    }
    // no references, no chunks; null tables with counts
    ih::Tables E;
    std::vector<uint8_t> out;
    char msg[200];
    if (ih::serialise(E, &out, msg, sizeof msg) != ih::OK || out.size() != 16 || parse_bai(out, 0, 0) != 0) return fprintf(stderr, "the empty index\n"), 1;
    E.n_ref = 2;
    if (ih::serialise(E, &out, msg, sizeof msg) != ih::ERR_ARG || ih::serialise(E, nullptr, msg, sizeof msg) != ih::ERR_ARG) return fprintf(stderr, "null tables were taken\n"), 1;
    printf("bam_sort_host_check: %llu tables serialised, every file parses or is refused\n", (unsigned long long)(calls + 3));
    return 0;
}

int main() {
    const std::string texts[] = {"@HD\tVN:1.6\tSO:unsorted\tGO:query\n@SQ\tSN:ctg_a\tLN:5000\n", "@HD\tVN:1.6\r\n@CO\tSO:x\r\n", "@HD", "@HD\tSO:", "@SQ\tSN:ctg_a\tLN:5000\n",
                                 "", std::string("@HD\tVN:1.6\n\0\0\0", 14), std::string("\0\0", 2), "@HD\tVN:1.6\tSO:coordinate\n"};
    uint64_t calls = 0, taken = 0;
    for (const std::string &text : texts) {
        const std::string h = header_of(text);
        const uint64_t n = h.size();
        for (uint64_t cut = 0; cut <= n; cut++) {
            uint8_t *p = (uint8_t *)malloc(cut ? cut : 1);
            memcpy(p, h.data(), cut);
            const uint64_t before = g_taken;
            if (check(cut ? p : nullptr, cut)) return 1;
            calls++;
            if (cut == n) taken += g_taken - before;
            for (uint64_t at = 0; at < cut; at++)
                for (const int c : {(int)'\t', (int)'\n', 0, (int)'S', 0xFF}) {
                    const uint8_t was = p[at];
                    p[at] = (uint8_t)c;
                    if (check(p, cut)) return 1;
                    p[at] = was;
                    calls++;
                }
            free(p);
        }
    }
    if (taken != sizeof texts / sizeof texts[0]) return fprintf(stderr, "a whole header was refused\n"), 1;
    printf("bam_sort_host_check: %llu calls, every answer a header that says SO:coordinate\n", (unsigned long long)calls);
    return check_serialiser();
}
