// fasta_out_host_check.cpp -- a stand-alone program over the host part of pp_fasta_text and pp_bgzf_out_gzi
// (polypolish_amd/csrc/pp_fasta_out_host.h), made to be built with a sanitizer and run on a machine without a GPU, as
// tools/fasta_host_check.cpp is for pp_fasta_records:
//   clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ipolypolish_amd/csrc tools/fasta_out_host_check.cpp -o fasta_out_host_check
//   ./fasta_out_host_check
// For every prefix of a small contig set (contigs of no bytes, headers of no bytes, names cut at a space and at a tab among them)
// and every small width the offsets and the header bytes lie in heap blocks of EXACTLY the lengths given (a read past one is a read
// past the allocation); plan() and fai() run as pp_fasta_text runs them, gzi() as pp_bgzf_out_gzi does.  The program checks the
// table, the text's length and the .fai rows against a plain walk that writes the text byte by byte; the refusals, in their order,
// with offsets near 2^40 and 2^64 and a width of 2^31 (offsets only: the arrays behind them are one byte long); the sanitizer checks
// every load.
#include "pp_fasta_out_host.h"

#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace fo = pp_fasta_out_host;

static int failures = 0;
#define CHECK(cond)                                                           \
    do {                                                                      \
        if (!(cond)) {                                                        \
            fprintf(stderr, "line %d: %s\n", __LINE__, #cond);                \
            failures++;                                                       \
        }                                                                     \
    } while (0)

template <class T>
static std::unique_ptr<T[]> exact(const std::vector<T> &v) {  // a heap block of exactly v's length (none for an empty one)
    if (v.empty()) return nullptr;
    std::unique_ptr<T[]> p(new T[v.size()]);
    memcpy(p.get(), v.data(), v.size() * sizeof(T));
    return p;
}

struct Contig { std::string header; uint64_t len; };

// the text, written byte by byte; where each contig's '>' and first base lie
static std::string by_bytes(const std::vector<Contig> &cs, uint64_t W, std::vector<uint64_t> &hdr_at, std::vector<uint64_t> &body_at) {
    std::string t;
    for (const Contig &c : cs) {
        hdr_at.push_back(t.size());
        t += '>';
        t += c.header;
        t += '\n';
        body_at.push_back(t.size());
        for (uint64_t i = 0; i < c.len; i++) {
            t += "ACGT"[i & 3];
            if (W && (i + 1) % W == 0 && i + 1 < c.len) t += '\n';
        }
        if (W == 0 || c.len) t += '\n';
    }
    return t;
}

static void one_set(const std::vector<Contig> &cs, uint64_t W) {
    std::vector<uint64_t> coff{7}, hoff{3};  // (offsets need not begin at 0)
    std::vector<uint8_t> hbytes(3, (uint8_t)'\n');  // (what lies in front of the headers is not looked at)
    for (const Contig &c : cs) {
        coff.push_back(coff.back() + c.len);
        hbytes.insert(hbytes.end(), c.header.begin(), c.header.end());
        hoff.push_back(hbytes.size());
    }
    const auto co = exact(coff), ho = exact(hoff);
    const auto hb = exact(hbytes);
    fo::Plan P;
    char msg[256];
    const int rc = fo::plan(true, true, (uint32_t)cs.size(), co.get(), hb.get(), ho.get(), W, P, msg, sizeof msg);
    CHECK(rc == fo::OK);
    if (rc) return;
    std::vector<uint64_t> hdr_at, body_at;
    const std::string t = by_bytes(cs, W, hdr_at, body_at);
    CHECK(P.n_text == t.size() && P.rows.size() == cs.size() + 1 && P.rows.back().hdr_at == t.size());
    std::string want_fai;
    for (size_t c = 0; c < cs.size(); c++) {
        const fo::Row &R = P.rows[c];
        CHECK(R.hdr_at == hdr_at[c] && R.body_at == body_at[c] && R.len == cs[c].len && R.base_off == coff[c] - coff[0] && R.hsrc == hoff[c] - hoff[0]);
        CHECK(P.rows[c + 1].hdr_at - R.body_at == fo::body_bytes(cs[c].len, W));
        const std::string &h = cs[c].header;
        const std::string name = h.substr(0, std::min(h.find(' '), h.find('\t')));
        const uint64_t L = cs[c].len, lb = W == 0 ? L : std::min(L, W);
        want_fai += name + "\t" + std::to_string(L) + "\t" + std::to_string(body_at[c]) + "\t" + std::to_string(lb) + "\t" + std::to_string(L ? lb + 1 : 0) + "\n";
        for (uint64_t p = 0; p < L; p++) CHECK(t[body_at[c] + p / lb * (lb + 1) + p % lb] == "ACGT"[p & 3]);
    }
    std::string got_fai;
    fo::fai(P, hb.get(), ho.get(), W, got_fai);
    CHECK(got_fai == want_fai);
}

static int refusal(bool have_bases, bool mem_ok, const std::vector<uint64_t> &coff, const std::vector<uint8_t> &hbytes, const std::vector<uint64_t> &hoff,
                   uint64_t W, bool null_coff = false, bool null_hoff = false) {
    const auto co = exact(coff), ho = exact(hoff);
    const auto hb = exact(hbytes);
    fo::Plan P;
    char msg[256] = "";
    const int rc = fo::plan(have_bases, mem_ok, (uint32_t)coff.size() - 1, null_coff ? nullptr : co.get(), hb.get(), null_hoff ? nullptr : ho.get(), W, P, msg, sizeof msg);
    CHECK((rc == fo::OK) == (msg[0] == 0));
    return rc;
}

int main() {
    const std::vector<Contig> all = {{"a", 1}, {"", 0}, {"name with words", 5}, {"tab\tbed x", 16}, {"e", 0}, {"seventeen", 17}, {" lead", 33}, {"z z", 2}};
    for (size_t n = 0; n <= all.size(); n++)
        for (uint64_t W = 0; W <= 18; W++) one_set(std::vector<Contig>(all.begin(), all.begin() + n), W);
    one_set(all, 0x7FFFFFFFull);

    const uint64_t T40 = 1ull << 40, MAX = ~0ull;
    const std::vector<uint8_t> h1{'h'}, hnl{'a', '\n', 'b'};
    // null arguments, the memory form
    CHECK(refusal(true, true, {0, 1}, h1, {0, 1}, 0, true) == fo::ERR_ARG);
    CHECK(refusal(true, true, {0, 1}, h1, {0, 1}, 0, false, true) == fo::ERR_ARG);
    CHECK(refusal(true, false, {0, 1}, h1, {0, 1}, 0) == fo::ERR_ARG);
    // the width: 2^31 - 1 is the last one taken
    CHECK(refusal(true, true, {0, 1}, h1, {0, 1}, 0x7FFFFFFFull) == fo::OK);
    CHECK(refusal(true, true, {0, 1}, h1, {0, 1}, 0x80000000ull) == fo::ERR_LIMIT);
    CHECK(refusal(true, false, {0, 1}, h1, {0, 1}, 0x80000000ull) == fo::ERR_ARG);  // (the memory form is judged first)
    // offsets that decrease
    CHECK(refusal(true, true, {1, 0}, h1, {0, 1}, 0) == fo::ERR_ARG);
    CHECK(refusal(true, true, {0, 1, 1}, h1, {0, 1, 0}, 0) == fo::ERR_ARG);
    CHECK(refusal(true, true, {MAX, 0}, h1, {0, 1}, 0) == fo::ERR_ARG);
    // the sizes, with offsets only: none of these reads a header byte or a base
    CHECK(refusal(true, true, {0, T40}, h1, {0, 1}, 0) == fo::ERR_LIMIT);
    CHECK(refusal(true, true, {0, T40 - 4}, h1, {0, 1}, 0) == fo::ERR_LIMIT);  // '>' h \n, the bases, \n: 2^40 bytes
    CHECK(refusal(true, true, {0, T40 - 5}, h1, {0, 1}, 0) == fo::OK);         // ... and one fewer
    CHECK(refusal(true, true, {0, T40 - 5}, h1, {0, 1}, 60) == fo::ERR_LIMIT);  // (the line ends of the wrap take it over)
    CHECK(refusal(true, true, {0, MAX}, h1, {0, 1}, 1) == fo::ERR_LIMIT);
    CHECK(refusal(true, true, {MAX - 1, MAX}, h1, {0, 1}, 1) == fo::OK);
    CHECK(refusal(true, true, {0, T40 / 2, T40}, h1, {0, 0, 1}, 0) == fo::ERR_LIMIT);  // no contig alone, all of them together
    CHECK(refusal(true, true, {0, 1}, h1, {0, T40}, 0) == fo::ERR_LIMIT);              // a header of 2^40 bytes is not looked at
    CHECK(refusal(true, true, {0, 1}, h1, {0, MAX}, 0) == fo::ERR_LIMIT);
    // null arrays with bytes to read, a header that holds a newline
    CHECK(refusal(false, true, {0, 1}, h1, {0, 1}, 0) == fo::ERR_ARG);
    CHECK(refusal(false, true, {5, 5}, h1, {0, 1}, 0) == fo::OK);
    CHECK(refusal(true, true, {0, 1}, {}, {0, 1}, 0) == fo::ERR_ARG);
    CHECK(refusal(true, true, {0, 1}, {}, {4, 4}, 0) == fo::OK);
    CHECK(refusal(true, true, {0, 1}, hnl, {0, 3}, 0) == fo::ERR_ARG);
    CHECK(refusal(true, true, {0, 1, 2}, hnl, {0, 1, 1}, 0) == fo::OK);  // (the newline lies behind the headers)
    CHECK(refusal(true, true, {0, 1}, hnl, {2, 3}, 0) == fo::OK);        // (... in front of them)

    // the .gzi: a count, then a pair per block except the first; none for the EOF block
    std::string g;
    const std::vector<uint64_t> off{0, 100, 250, 300};  // three blocks, the EOF block at 300
    const auto bo = exact(off);
    fo::gzi(bo.get(), 3, g);
    CHECK(g.size() == 8 + 2 * 16);
    auto u64_at = [&g](size_t i) { uint64_t v = 0; for (int k = 7; k >= 0; k--) v = v << 8 | (uint8_t)g[i + (size_t)k]; return v; };
    CHECK(u64_at(0) == 2 && u64_at(8) == 100 && u64_at(16) == 65280 && u64_at(24) == 250 && u64_at(32) == 130560);
    for (uint64_t n = 0; n < 2; n++) {
        const std::vector<uint64_t> o(n + 1, 0);
        const auto b = exact(o);
        fo::gzi(b.get(), n, g);
        CHECK(g == std::string(8, '\0'));
    }
    if (failures) {
        fprintf(stderr, "fasta_out_host_check: %d failed\n", failures);
        return 1;
    }
    printf("fasta_out_host_check: OK\n");
    return 0;
}
