// bed_host_check.cpp -- a stand-alone program over the host part of pp_status_bed, pp_polish_bed and pp_polish_masked
// (polypolish_amd/csrc/pp_bed_host.h), made to be built with a sanitizer and run on a machine without a GPU, as tools/vcf_host_check.cpp
// is for pp_polish_vcf:
//   clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ipolypolish_amd/csrc tools/bed_host_check.cpp -o bed_host_check
//   ./bed_host_check
// For every prefix of a contig set (names of 1 byte and of several KiB, a contig of no positions) the offsets, the table of name pointers
// and every name lie in heap blocks of EXACTLY the lengths given (a name's block ends with its NUL: a read past one is a read past the
// allocation); plan() runs as the calls run it.  Every prefix of a status list, in a heap block of exactly its length without a NUL,
// goes through parse_status_list.  The arithmetic of one line -- line_len and line_byte, the very functions the text kernel calls -- is
// held against snprintf with starts and ends at every digit seam up to 10 decimal digits (offsets near 2^32, which no GPU test can
// reach).  The refusals, in their order; the sanitizer checks every load.
#include "pp_bed_host.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace bh = pp_bed_host;

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

static void one_set(const std::vector<Contig> &cs) {
    const Exact E(cs);
    bh::Plan P;
    char msg[256] = "";
    const int rc = bh::plan("pp_status_bed", true, true, true, (uint32_t)cs.size(), E.off.get(), cs.empty() ? NONE : E.table.get(), bh::MASK_UNDECIDED, P, msg, sizeof msg);
    CHECK(rc == bh::OK && msg[0] == 0);
    if (rc) return;
    std::string names;
    uint64_t G = 0;
    for (const Contig &c : cs) {
        names += c.name;
        G += c.len;
    }
    CHECK(P.G == G && P.names == names && P.name_off.size() == cs.size() + 1 && P.name_off[0] == 0);
    for (size_t c = 0; c < cs.size(); c++)
        CHECK(P.name_off[c + 1] - P.name_off[c] == cs[c].name.size() && P.names.compare((size_t)P.name_off[c], cs[c].name.size(), cs[c].name) == 0);
}

struct Args {
    bool have_out = true, have_status = true, mem_ok = true, null_names = false, null_off = false;
    uint32_t mask = bh::MASK_UNDECIDED;
    int null_at = -1;
};
static int refusal(const std::vector<Contig> &cs, const Args &A, const uint64_t *off_given = nullptr, const char *word = nullptr) {
    const Exact E(cs, A.null_at);
    bh::Plan P;
    char msg[256] = "";
    const int rc = bh::plan("pp_status_bed", A.have_out, A.have_status, A.mem_ok, (uint32_t)cs.size(), A.null_off ? nullptr : (off_given ? off_given : E.off.get()),
                            A.null_names ? nullptr : (cs.empty() ? NONE : E.table.get()), A.mask, P, msg, sizeof msg);
    CHECK((rc == bh::OK) == (msg[0] == 0));
    CHECK(rc == bh::OK || strncmp(msg, "pp_status_bed: ", 15) == 0);
    if (word) CHECK(strstr(msg, word) != nullptr);
    return rc;
}

// line_len and line_byte against snprintf
static void one_line(const std::string &name, uint64_t a, uint64_t b, uint32_t st) {
    static const char *const words[6] = {"kept", "changed", "low_depth", "none", "multiple", "too_close"};
    std::unique_ptr<uint8_t[]> nm(new uint8_t[name.size() ? name.size() : 1]);  // exactly the name's bytes, no NUL
    memcpy(nm.get(), name.data(), name.size());
    char tail[96];
    snprintf(tail, sizeof tail, "\t%llu\t%llu\t%s\n", (unsigned long long)a, (unsigned long long)b, words[st]);
    const std::string want = name + tail;
    const uint64_t len = bh::line_len(name.size(), a, b, st);
    CHECK(len == want.size());
    if (len != want.size()) return;
    const uint32_t na = bh::ndig(a), nb = bh::ndig(b);
    std::string got;
    for (uint64_t k = 0; k < len; k++) got += (char)bh::line_byte(nm.get(), name.size(), a, na, b, nb, st, k);
    CHECK(got == want);
    CHECK(strcmp(bh::word(st), words[st]) == 0 && bh::word_len(st) == strlen(words[st]));
}

static int parsed(const std::string &list, uint32_t *mask) {
    std::unique_ptr<char[]> block(new char[list.size() ? list.size() : 1]);  // exactly the list's bytes, no NUL
    memcpy(block.get(), list.data(), list.size());
    char msg[192] = "x";
    const int rc = bh::parse_status_list(list.empty() ? nullptr : block.get(), list.size(), mask, msg, sizeof msg);
    CHECK((rc == bh::OK) == (msg[0] == 0));
    CHECK(rc == bh::OK || *mask == 0);
    return rc;
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
    for (size_t n = 0; n <= all.size(); n++) one_set(std::vector<Contig>(all.begin(), all.begin() + (long)n));

    const std::vector<Contig> two = {{"a", 5}, {"b", 7}};
    Args A;
    CHECK(refusal(two, A) == bh::OK);
    // null arguments
    A = Args(); A.have_out = false;    CHECK(refusal(two, A, nullptr, "null argument") == bh::ERR_ARG);
    A = Args(); A.have_status = false; CHECK(refusal(two, A, nullptr, "null argument") == bh::ERR_ARG);
    A = Args(); A.null_names = true;   CHECK(refusal(two, A, nullptr, "null argument") == bh::ERR_ARG);
    A = Args(); A.null_off = true;     CHECK(refusal(two, A, nullptr, "null argument") == bh::ERR_ARG);
    // the memory kind, then the mask: judged before any offset or name is looked at
    A = Args(); A.mem_ok = false; A.mask = 0; CHECK(refusal(two, A, nullptr, "PP_MEM_HOST") == bh::ERR_ARG);
    A = Args(); A.mask = 0; A.null_at = 0;    CHECK(refusal(two, A, nullptr, "mask of 0") == bh::ERR_ARG);
    for (uint32_t m : {64u, 65u, 0x80000000u, 0xFFFFFFFFu}) { A = Args(); A.mask = m; CHECK(refusal(two, A, nullptr, "bit above 5") == bh::ERR_ARG); }
    for (uint32_t m = 1; m < 64; m++) { A = Args(); A.mask = m; CHECK(refusal(two, A) == bh::OK); }
    // the offsets: from 0 on, never decreasing, below 2^32
    {
        std::unique_ptr<uint64_t[]> off(new uint64_t[3]);
        A = Args();
        off[0] = 0; off[1] = 5; off[2] = 4;            CHECK(refusal(two, A, off.get(), "decrease") == bh::ERR_ARG);
        off[0] = 1; off[1] = 5; off[2] = 9;            CHECK(refusal(two, A, off.get(), "contig_off[0]") == bh::ERR_ARG);
        off[0] = 0; off[1] = 5; off[2] = 1ull << 32;   CHECK(refusal(two, A, off.get(), "2^32") == bh::ERR_ARG);
        off[0] = 0; off[1] = 5; off[2] = (1ull << 32) - 1; CHECK(refusal(two, A, off.get()) == bh::OK);
        off[0] = 0; off[1] = 0; off[2] = 0;            CHECK(refusal(two, A, off.get()) == bh::OK);
        A.null_at = 1; off[2] = 1ull << 33;            CHECK(refusal(two, A, off.get(), "2^32") == bh::ERR_ARG);  // (before the names)
    }
    // a null name, a name that holds a tab or a newline -- at its start, inside, at its end
    A = Args(); A.null_at = 1; CHECK(refusal(two, A, nullptr, "name is NULL") == bh::ERR_ARG);
    A = Args();
    for (const char *bad : {"\t", "\n", "a\tb", "ab\n", "\nab", "x\ty\nz"}) {
        CHECK(refusal({{"fine", 3}, {bad, 4}}, A, nullptr, "tab or a newline") == bh::ERR_ARG);
        CHECK(refusal({{bad, 3}}, A, nullptr, "tab or a newline") == bh::ERR_ARG);
    }
    CHECK(refusal({{"a b;c=<d>,\r", 3}}, A) == bh::OK);  // (anything else is written as it is)
    CHECK(refusal({{"", 3}}, A) == bh::OK);              // (an empty name is a name)
    CHECK(refusal({}, A) == bh::OK);

    // the state of the job, in its order: no job, no records, emit ranges
    {
        char msg[256] = "";
        CHECK(bh::check_job("pp_polish_bed", bh::JobState{true, true, false}, msg, sizeof msg) == bh::OK && msg[0] == 0);
        CHECK(bh::check_job("pp_polish_bed", bh::JobState{false, false, true}, msg, sizeof msg) == bh::ERR_ARG && strstr(msg, "no finished polish job"));
        CHECK(bh::check_job("pp_polish_masked", bh::JobState{true, false, true}, msg, sizeof msg) == bh::ERR_ARG && strstr(msg, "pp_polish_set_debug(ctx, 1)") &&
              strncmp(msg, "pp_polish_masked: ", 18) == 0);
        CHECK(bh::check_job("pp_polish_bed", bh::JobState{true, true, true}, msg, sizeof msg) == bh::ERR_ARG && strstr(msg, "pp_polish_set_emit"));
    }

    // every prefix of a status list
    {
        const std::string list = "low_depth,none,multiple,too_close,kept,changed,none";
        const char *const words[6] = {"kept", "changed", "low_depth", "none", "multiple", "too_close"};
        for (size_t n = 0; n <= list.size(); n++) {
            const std::string pre = list.substr(0, n);
            uint32_t want = 0, got = 77;
            bool ok = n > 0;
            for (size_t at = 0; ok;) {  // a plain reading of the prefix
                const size_t end = std::min(pre.find(',', at), pre.size());
                const std::string w = pre.substr(at, end - at);
                int st = -1;
                for (int s = 0; s < 6; s++)
                    if (w == words[s]) st = s;
                if (st < 0) { ok = false; break; }
                want |= 1u << st;
                if (end == pre.size()) break;
                at = end + 1;
            }
            const int rc = parsed(pre, &got);
            CHECK((rc == bh::OK) == ok);
            CHECK(got == (ok ? want : 0u));
        }
        uint32_t m = 0;
        CHECK(parsed("low_depth,none,multiple,too_close", &m) == bh::OK && m == bh::MASK_UNDECIDED);
        CHECK(parsed("kept,changed,low_depth,none,multiple,too_close", &m) == bh::OK && m == bh::MASK_ALL);
        for (const char *bad : {",", "kept,", ",kept", "kept,,none", "Kept", "kept ", " kept", "low-depth", "all", "kep", "keptt", "too_close,x"})
            CHECK(parsed(bad, &m) == bh::ERR_ARG && m == 0);
    }

    // one line at every digit seam of start and end, up to 10 decimal digits
    {
        std::vector<uint64_t> seams = {0, 1};
        for (uint64_t q = 10; q <= 1000000000ull; q *= 10) { seams.push_back(q - 1); seams.push_back(q); }
        seams.push_back((1ull << 32) - 2);
        seams.push_back((1ull << 32) - 1);
        const std::string names[4] = {"", "c", "contig_1 with=<words>;", std::string(300, 'n')};
        uint32_t st = 0;
        for (size_t i = 0; i < seams.size(); i++)
            for (size_t j = i; j < seams.size(); j++)
                one_line(names[(i + j) % 4], seams[i], seams[j] + (i == j ? 1 : 0), st++ % 6);
        CHECK(bh::ndig(0) == 1 && bh::ndig(9) == 1 && bh::ndig(10) == 2 && bh::ndig(4294967295ull) == 10 && bh::ndig(9999999999ull) == 10 && bh::ndig(10000000000ull) == 11);
    }

    // the text's size: 2^40 bytes and more are refused
    {
        char msg[128] = "";
        const uint64_t T40 = 1ull << 40;
        CHECK(bh::text_size("pp_status_bed", 0, msg, sizeof msg) == bh::OK && bh::text_size("pp_status_bed", T40 - 1, msg, sizeof msg) == bh::OK && msg[0] == 0);
        CHECK(bh::text_size("pp_status_bed", T40, msg, sizeof msg) == bh::ERR_LIMIT && strstr(msg, "2^40") != nullptr);
        CHECK(bh::text_size("pp_polish_bed", ~0ull, msg, sizeof msg) == bh::ERR_LIMIT && strncmp(msg, "pp_polish_bed: ", 15) == 0);
    }
    if (failures) {
        fprintf(stderr, "bed_host_check: %d failed\n", failures);
        return 1;
    }
    printf("bed_host_check: OK\n");
    return 0;
}
