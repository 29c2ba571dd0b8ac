// vcf_host_check.cpp -- a stand-alone program over the host part of pp_polish_vcf (polypolish_amd/csrc/pp_vcf_host.h), made to be built
// with a sanitizer and run on a machine without a GPU, as tools/fasta_out_host_check.cpp is for pp_fasta_text:
//   clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ipolypolish_amd/csrc tools/vcf_host_check.cpp -o vcf_host_check
//   ./vcf_host_check
// For every prefix of a contig set (names of 1 byte and of several KiB, lengths near 2^32 - 4096, a contig of no bases) the offsets,
// the table of name pointers and every name lie in heap blocks of EXACTLY the lengths given (a name's block ends with its NUL: a read
// past one is a read past the allocation); plan() runs as pp_polish_vcf runs it.  The program checks the header against a plain
// writer and the name table against the names; the refusals, in their order; the sanitizer checks every load.
#include "pp_vcf_host.h"

#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace vh = pp_vcf_host;

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

static const vh::JobState FINISHED{true, false};
static const char *VERSION = "polypolish-check 1.0 (a version with words)";

static void one_set(const std::vector<Contig> &cs) {
    const Exact E(cs);
    static const char *const none[1] = {nullptr};
    vh::Plan P;
    char msg[256] = "";
    const int rc = vh::plan(true, FINISHED, (uint32_t)cs.size(), E.off.get(), cs.empty() ? none : E.table.get(), VERSION, P, msg, sizeof msg);
    CHECK(rc == vh::OK && msg[0] == 0);
    if (rc) return;
    std::string want = std::string("##fileformat=VCFv4.2\n##source=") + VERSION + "\n", names;
    for (const Contig &c : cs) {
        want += "##contig=<ID=" + c.name + ",length=" + std::to_string(c.len) + ">\n";
        names += c.name;
    }
    want += "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n";
    CHECK(P.header == want);
    CHECK(P.names == names && P.name_off.size() == cs.size() + 1 && P.name_off[0] == 0);
    for (size_t c = 0; c < cs.size(); c++)
        CHECK(P.name_off[c + 1] - P.name_off[c] == cs[c].name.size() && P.names.compare((size_t)P.name_off[c], cs[c].name.size(), cs[c].name) == 0);
}

static int refusal(bool have_out, vh::JobState S, const std::vector<Contig> &cs, bool null_names = false, bool null_off = false,
                   const char *version = VERSION, int null_at = -1) {
    const Exact E(cs, null_at);
    static const char *const none[1] = {nullptr};  // (no contig: a table nobody reads)
    vh::Plan P;
    char msg[256] = "";
    const int rc = vh::plan(have_out, S, (uint32_t)cs.size(), null_off ? nullptr : E.off.get(), null_names ? nullptr : (cs.empty() ? none : E.table.get()), version, P,
                            msg, sizeof msg);
    CHECK((rc == vh::OK) == (msg[0] == 0));
    CHECK(rc == vh::OK || strncmp(msg, "pp_polish_vcf: ", 15) == 0);
    return rc;
}

int main() {
    const uint64_t NEAR = (1ull << 32) - 4096;
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
    // null arguments
    CHECK(refusal(false, FINISHED, two) == vh::ERR_ARG);
    CHECK(refusal(true, FINISHED, two, true) == vh::ERR_ARG);
    CHECK(refusal(true, FINISHED, two, false, true) == vh::ERR_ARG);
    CHECK(refusal(true, FINISHED, two, false, false, nullptr) == vh::ERR_ARG);
    // the job's state: judged before any name is looked at
    CHECK(refusal(true, vh::JobState{false, false}, two) == vh::ERR_ARG);
    CHECK(refusal(true, vh::JobState{false, false}, two, false, false, VERSION, 0) == vh::ERR_ARG);
    CHECK(refusal(true, vh::JobState{true, true}, two) == vh::ERR_ARG);
    CHECK(refusal(true, vh::JobState{false, true}, two) == vh::ERR_ARG);
    // a null name, a name that holds a tab or a newline -- at its start, inside, at its end
    CHECK(refusal(true, FINISHED, two, false, false, VERSION, 1) == vh::ERR_ARG);
    for (const char *bad : {"\t", "\n", "a\tb", "ab\n", "\nab", "x\ty\nz"}) {
        CHECK(refusal(true, FINISHED, {{"fine", 3}, {bad, 4}}) == vh::ERR_ARG);
        CHECK(refusal(true, FINISHED, {{bad, 3}}) == vh::ERR_ARG);
    }
    CHECK(refusal(true, FINISHED, {{"a b;c=<d>,\r", 3}}) == vh::OK);  // (anything else is written as it is)
    CHECK(refusal(true, FINISHED, {}) == vh::OK);
    // the text's size once the records' bytes are known: 2^40 bytes and more are refused
    uint64_t n_text = 0;
    char msg[128] = "";
    const uint64_t T40 = 1ull << 40;
    CHECK(vh::text_size(100, 0, &n_text, msg, sizeof msg) == vh::OK && n_text == 100);
    CHECK(vh::text_size(100, T40 - 101, &n_text, msg, sizeof msg) == vh::OK && n_text == T40 - 1);
    CHECK(vh::text_size(100, T40 - 100, &n_text, msg, sizeof msg) == vh::ERR_LIMIT);
    CHECK(vh::text_size(0, T40, &n_text, msg, sizeof msg) == vh::ERR_LIMIT);
    CHECK(vh::text_size(100, ~0ull - 50, &n_text, msg, sizeof msg) == vh::ERR_LIMIT);  // (no sum that wraps)
    CHECK(strstr(msg, "2^40") != nullptr);
    if (failures) {
        fprintf(stderr, "vcf_host_check: %d failed\n", failures);
        return 1;
    }
    printf("vcf_host_check: OK\n");
    return 0;
}
