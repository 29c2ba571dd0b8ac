// depth_host_check.cpp -- a stand-alone program over the host part of pp_depth_bedgraph and pp_polish_depth
// (polypolish_amd/csrc/pp_depth_host.h), made to be built with a sanitizer and run on a machine without a GPU, as tools/bed_host_check.cpp
// is for the BED:
//   clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ipolypolish_amd/csrc tools/depth_host_check.cpp -o depth_host_check
//   ./depth_host_check
// For every prefix of a contig set (names of 1 byte and of several KiB, a contig of no positions) the offsets, the table of name pointers
// and every name lie in heap blocks of EXACTLY the lengths given; plan() runs as the calls run it, in the runs form and with bins, and
// the bins' table is held against a plain count.  The arithmetic of one line -- line_len and line_byte, the very functions the kernels
// call -- is held against snprintf in both forms: starts and ends at every digit seam up to 10 decimal digits, tenths and hundredths at
// every digit count up to their maxima (10 * 2^32 tenths, 100 * 2^32 hundredths).  mean_hundredths is held against __int128 arithmetic at
// n = 1, 2, 3, 2^24 and at ties on odd and even quotients.  The refusals, in their order; the sanitizer checks every load.
#include "pp_depth_host.h"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace dh = pp_depth_host;

static int failures = 0;
#define CHECK(cond)                                                           \
    do {                                                                      \
        if (!(cond)) {                                                        \
            fprintf(stderr, "line %d: %s\n", __LINE__, #cond);                \
            failures++;                                                       \
        }                                                                     \
    } while (0)

struct Contig { std::string name; uint64_t len; };

// the names and their table in heap blocks of exactly their lengths
struct Exact {
    std::vector<std::unique_ptr<char[]>> names;
    std::unique_ptr<const char *[]> table;
    std::unique_ptr<uint64_t[]> off;
    explicit Exact(const std::vector<Contig> &cs, int null_at = -1) {
        off.reset(new uint64_t[cs.size() + 1]);
        off[0] = 0;
        if (!cs.empty()) table.reset(new const char *[cs.size()]);
        for (size_t c = 0; c < cs.size(); c++) {
            off[c + 1] = off[c] + cs[c].len;
            names.emplace_back(new char[cs[c].name.size() + 1]);
            memcpy(names.back().get(), cs[c].name.c_str(), cs[c].name.size() + 1);
            table[c] = (int)c == null_at ? nullptr : names.back().get();
        }
    }
};

static const char *const NONE[1] = {nullptr};  // (no contig: a table nobody reads)

static void one_set(const std::vector<Contig> &cs, uint32_t bin) {
    const Exact E(cs);
    dh::Plan P;
    char msg[256] = "";
    const int rc = dh::plan("pp_depth_bedgraph", true, true, true, true, (uint32_t)cs.size(), E.off.get(), cs.empty() ? NONE : E.table.get(), bin, P, msg, sizeof msg);
    CHECK(rc == dh::OK && msg[0] == 0);
    if (rc) return;
    std::string names;
    uint64_t G = 0;
    for (const Contig &c : cs) {
        names += c.name;
        G += c.len;
    }
    CHECK(P.names.G == G && P.names.names == names && P.names.name_off.size() == cs.size() + 1 && P.names.name_off[0] == 0);
    for (size_t c = 0; c < cs.size(); c++)
        CHECK(P.names.name_off[c + 1] - P.names.name_off[c] == cs[c].name.size() &&
              P.names.names.compare((size_t)P.names.name_off[c], cs[c].name.size(), cs[c].name) == 0);
    if (!bin) {
        CHECK(P.bin_base.empty());
        return;
    }
    CHECK(P.bin_base.size() == cs.size() + 1 && P.bin_base[0] == 0);
    for (size_t c = 0; c < cs.size(); c++) {  // a plain count of the contig's bins
        uint64_t n = cs[c].len / bin;
        if (cs[c].len % bin) n++;
        CHECK(P.bin_base[c + 1] - P.bin_base[c] == n);
        CHECK((n == 0) == (cs[c].len == 0));
    }
}

struct Args {
    bool have_out = true, have_depth = true, mem_ok = true, aligned = true, null_names = false, null_off = false;
    uint32_t bin = 0;
    int null_at = -1;
};
static int refusal(const std::vector<Contig> &cs, const Args &A, const uint64_t *off_given = nullptr, const char *word = nullptr) {
    const Exact E(cs, A.null_at);
    dh::Plan P;
    char msg[256] = "";
    const int rc = dh::plan("pp_depth_bedgraph", A.have_out, A.have_depth, A.mem_ok, A.aligned, (uint32_t)cs.size(),
                            A.null_off ? nullptr : (off_given ? off_given : E.off.get()), A.null_names ? nullptr : (cs.empty() ? NONE : E.table.get()), A.bin, P,
                            msg, sizeof msg);
    CHECK((rc == dh::OK) == (msg[0] == 0));
    CHECK(rc == dh::OK || strncmp(msg, "pp_depth_bedgraph: ", 19) == 0);
    if (word) CHECK(strstr(msg, word) != nullptr);
    return rc;
}

// line_len and line_byte against snprintf: v with `frac` decimals
static void one_line(const std::string &name, uint64_t a, uint64_t b, uint64_t v, uint32_t frac) {
    std::unique_ptr<uint8_t[]> nm(new uint8_t[name.size() ? name.size() : 1]);  // exactly the name's bytes, no NUL
    memcpy(nm.get(), name.data(), name.size());
    char tail[128];
    if (frac == 1u)
        snprintf(tail, sizeof tail, "\t%llu\t%llu\t%llu.%llu\n", (unsigned long long)a, (unsigned long long)b, (unsigned long long)(v / 10), (unsigned long long)(v % 10));
    else
        snprintf(tail, sizeof tail, "\t%llu\t%llu\t%llu.%02llu\n", (unsigned long long)a, (unsigned long long)b, (unsigned long long)(v / 100), (unsigned long long)(v % 100));
    const std::string want = name + tail;
    const uint64_t len = dh::line_len(name.size(), a, b, v, frac);
    CHECK(len == want.size());
    if (len != want.size()) return;
    const uint32_t na = dh::ndig(a), nb = dh::ndig(b), nv = dh::value_len(v, frac);
    std::string got;
    for (uint64_t k = 0; k < len; k++) got += (char)dh::line_byte(nm.get(), name.size(), a, na, b, nb, v, nv, frac, k);
    CHECK(got == want);
}

// mean_hundredths against 128-bit arithmetic: 10 S / n rounded, ties to even
static void one_mean(uint64_t S, uint64_t n) {
    const unsigned __int128 num = (unsigned __int128)S * 10u;
    const unsigned __int128 q = num / n, r = num % n;
    const unsigned __int128 want = q + ((2u * r > n || (2u * r == n && (q & 1u))) ? 1u : 0u);
    CHECK((unsigned __int128)dh::mean_hundredths(S, n) == want);
}

int main() {
    const uint64_t NEAR = (1ull << 29);
    const std::vector<Contig> all = {{"a", 1},
                                     {std::string(5000, 'k'), NEAR},
                                     {"name with words;=<>", 0},
                                     {"z", NEAR + 4095},
                                     {std::string(9001, 'q'), NEAR - 1},
                                     {"0", 17},
                                     {std::string(255, 'm'), 1},
                                     {"last one", NEAR + 1}};
    for (uint32_t bin : {0u, 1u, 2u, 17u, 4096u, 1u << 24})
        for (size_t n = 0; n <= all.size(); n++) one_set(std::vector<Contig>(all.begin(), all.begin() + (long)n), bin);

    const std::vector<Contig> two = {{"a", 5}, {"b", 7}};
    Args A;
    CHECK(refusal(two, A) == dh::OK);
    // null arguments
    A = Args(); A.have_out = false;   CHECK(refusal(two, A, nullptr, "null argument") == dh::ERR_ARG);
    A = Args(); A.have_depth = false; CHECK(refusal(two, A, nullptr, "null argument") == dh::ERR_ARG);
    A = Args(); A.null_names = true;  CHECK(refusal(two, A, nullptr, "null argument") == dh::ERR_ARG);
    A = Args(); A.null_off = true;    CHECK(refusal(two, A, nullptr, "null argument") == dh::ERR_ARG);
    // the memory kind, then the bin, then the alignment: judged before any offset or name is looked at
    A = Args(); A.mem_ok = false; A.bin = (1u << 24) + 1u; CHECK(refusal(two, A, nullptr, "PP_MEM_HOST") == dh::ERR_ARG);
    A = Args(); A.bin = (1u << 24) + 1u; A.aligned = false; A.null_at = 0; CHECK(refusal(two, A, nullptr, "2^24") == dh::ERR_ARG);
    A = Args(); A.bin = 0xFFFFFFFFu; CHECK(refusal(two, A, nullptr, "2^24") == dh::ERR_ARG);
    A = Args(); A.aligned = false; A.null_at = 0; CHECK(refusal(two, A, nullptr, "aligned to 8 bytes") == dh::ERR_ARG);
    for (uint32_t w : {0u, 1u, 2u, 1000u, (1u << 24) - 1u, 1u << 24}) { A = Args(); A.bin = w; CHECK(refusal(two, A) == dh::OK); }
    // the offsets: from 0 on, never decreasing, below 2^32
    {
        std::unique_ptr<uint64_t[]> off(new uint64_t[3]);
        A = Args();
        off[0] = 0; off[1] = 5; off[2] = 4;            CHECK(refusal(two, A, off.get(), "decrease") == dh::ERR_ARG);
        off[0] = 1; off[1] = 5; off[2] = 9;            CHECK(refusal(two, A, off.get(), "contig_off[0]") == dh::ERR_ARG);
        off[0] = 0; off[1] = 5; off[2] = 1ull << 32;   CHECK(refusal(two, A, off.get(), "2^32") == dh::ERR_ARG);
        off[0] = 0; off[1] = 5; off[2] = (1ull << 32) - 1; CHECK(refusal(two, A, off.get()) == dh::OK);
        A.bin = 1;                                     CHECK(refusal(two, A, off.get()) == dh::OK);
        A.bin = 0;
        off[0] = 0; off[1] = 0; off[2] = 0;            CHECK(refusal(two, A, off.get()) == dh::OK);
        A.null_at = 1; off[2] = 1ull << 33;            CHECK(refusal(two, A, off.get(), "2^32") == dh::ERR_ARG);  // (before the names)
    }
    // a null name, a name that holds a tab or a newline -- at its start, inside, at its end
    A = Args(); A.null_at = 1; CHECK(refusal(two, A, nullptr, "name is NULL") == dh::ERR_ARG);
    A = Args();
    for (const char *bad : {"\t", "\n", "a\tb", "ab\n", "\nab", "x\ty\nz"}) {
        CHECK(refusal({{"fine", 3}, {bad, 4}}, A, nullptr, "tab or a newline") == dh::ERR_ARG);
        CHECK(refusal({{bad, 3}}, A, nullptr, "tab or a newline") == dh::ERR_ARG);
    }
    CHECK(refusal({{"a b;c=<d>,\r", 3}}, A) == dh::OK);  // (anything else is written as it is)
    CHECK(refusal({{"", 3}}, A) == dh::OK);              // (an empty name is a name)
    CHECK(refusal({}, A) == dh::OK);

    // one line in both forms: starts and ends at every digit seam up to 10 decimal digits, values at every digit count up to their maxima
    {
        std::vector<uint64_t> seams = {0, 1};
        for (uint64_t q = 10; q <= 1000000000ull; q *= 10) { seams.push_back(q - 1); seams.push_back(q); }
        seams.push_back((1ull << 32) - 2);
        seams.push_back((1ull << 32) - 1);
        std::vector<uint64_t> values = {0, 1, 5, 9};
        for (uint64_t q = 10; q <= 100000000000ull; q *= 10) { values.push_back(q - 1); values.push_back(q); values.push_back(q + 7); }
        values.push_back(dh::TENTHS_MAX - 1);
        values.push_back(dh::TENTHS_MAX);          // the largest tenths: 42949672960, "4294967296.0"
        values.push_back(10u * dh::TENTHS_MAX - 1);
        values.push_back(10u * dh::TENTHS_MAX);    // the largest hundredths: "4294967296.00"
        const std::string names[4] = {"", "c", "contig_1 with=<words>;", std::string(300, 'n')};
        size_t k = 0;
        for (size_t i = 0; i < seams.size(); i++)
            for (size_t j = i; j < seams.size(); j++, k++) {
                const uint64_t v = values[k % values.size()];
                one_line(names[(i + j) % 4], seams[i], seams[j] + (i == j ? 1 : 0), v, 1);
                one_line(names[(i + j + 1) % 4], seams[i], seams[j] + (i == j ? 1 : 0), v, 2);
            }
        for (uint64_t v : values) {
            one_line("c", 0, 1, v, 1);
            one_line("c", 0, 1, v, 2);
        }
        CHECK(dh::value_len(0, 1) == 3 && dh::value_len(99, 1) == 3 && dh::value_len(100, 1) == 4 && dh::value_len(dh::TENTHS_MAX, 1) == 12);
        CHECK(dh::value_len(0, 2) == 4 && dh::value_len(999, 2) == 4 && dh::value_len(1000, 2) == 5 && dh::value_len(10u * dh::TENTHS_MAX, 2) == 13);
    }

    // the mean's rounding against 128-bit arithmetic
    {
        const uint64_t N24 = 1ull << 24;
        const std::vector<uint64_t> lengths = {1, 2, 3, 4, 7, 1000, N24 - 1, N24};
        const std::vector<uint64_t> flat = {1, 9, 10, 999, 1000, 123456789, dh::TENTHS_MAX - 1, dh::TENTHS_MAX};
        for (uint64_t n : lengths) {
            for (uint64_t S = 0; S < 64; S++) one_mean(S, n);
            for (uint64_t t : flat) {
                one_mean(t * n, n);          // a flat bin: the mean is the value with a 0 appended
                CHECK(dh::mean_hundredths(t * n, n) == 10u * t);
                if (t * n >= 1) one_mean(t * n - 1, n);
                one_mean(t * (n / 2 + 1), n);
            }
        }
        // ties: 10 S / n = q + 1/2 exactly -- n = 4, S odd: 10 S / 4 = 2.5 S
        CHECK(dh::mean_hundredths(1, 4) == 2);   // 2.5: q = 2 is even, stays
        CHECK(dh::mean_hundredths(3, 4) == 8);   // 7.5: q = 7 is odd, goes up
        CHECK(dh::mean_hundredths(5, 4) == 12);  // 12.5
        CHECK(dh::mean_hundredths(7, 4) == 18);  // 17.5
        // ... and at n = 2^24: S = 2^23 k / 10 is a tie when 10 S = 2^24 q + 2^23, e.g. S = 2^22 * (2 q + 1) / 5 with (2 q + 1) a multiple of 5
        for (uint64_t q : {2ull, 7ull, 12ull, 17ull, 1000002ull, 1000007ull}) {
            const uint64_t S = (1ull << 22) * (2 * q + 1) / 5;
            CHECK(10 * S == N24 * q + (N24 >> 1));
            CHECK(dh::mean_hundredths(S, N24) == q + (q & 1u));
            one_mean(S, N24);
            one_mean(S - 1, N24);
            one_mean(S + 1, N24);
        }
        CHECK(dh::mean_hundredths(1, 3) == 3 && dh::mean_hundredths(2, 3) == 7 && dh::mean_hundredths(1, 2) == 5 && dh::mean_hundredths(7, 1) == 70);
        one_mean(dh::TENTHS_MAX * N24, N24);  // the largest sum: below 2^60
        CHECK(dh::TENTHS_MAX * N24 < (1ull << 60));
    }

    // the bits that are refused on the device: anything at or above the bits of 2^32, as an unsigned number
    {
        auto bits = [](double x) { uint64_t b; memcpy(&b, &x, 8); return b; };
        CHECK(bits(4294967296.0) == dh::DEPTH_BAD_BITS);
        for (double ok : {0.0, 0.1, 1.0, 4294967295.0, 4294967295.9999995}) CHECK(bits(ok) < dh::DEPTH_BAD_BITS);
        for (double bad : {-0.0, -1.0, 4294967296.0, 1e300, (double)INFINITY, (double)NAN, -(double)NAN}) CHECK(bits(bad) >= dh::DEPTH_BAD_BITS);
    }
    if (failures) {
        fprintf(stderr, "depth_host_check: %d failed\n", failures);
        return 1;
    }
    printf("depth_host_check: OK\n");
    return 0;
}
