// sam_host_check.cpp -- a stand-alone program over the host walk behind pp_sam_header (polypolish_amd/csrc/pp_sam_host.h), made to be
// built with a sanitizer and run on a machine without a GPU, as tools/bam_host_check.cpp is for the BAM helpers:
//   clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ipolypolish_amd/csrc tools/sam_host_check.cpp -o sam_host_check
//   ./sam_host_check            (a built-in header)      ./sam_host_check some.sam
// Every prefix of the text goes to header() in a heap block of EXACTLY its length (a read past the cut is a read past the
// allocation), with cap 0 and with cap = n_ref, then every prefix with one byte replaced by a tab, a newline, a colon or a NUL.  The
// program checks that an answer lies inside the prefix -- header_end <= n, every name range inside [0, header_end) -- that the two
// calls agree, and that a refusal names a line of the prefix; the sanitizer checks every load.
#include "pp_sam_host.h"

#include <cstdlib>
#include <string>
#include <vector>

static int check(const uint8_t *p, uint64_t n) {
    uint32_t n_ref = 0, again = 0;
    uint64_t end = ~0ull, lines = 0, bad = 0;
    char msg[256];
    const int rc = pp_sam_host::header(p, n, 0, &n_ref, nullptr, nullptr, nullptr, &end, &lines, &bad, msg, sizeof msg);
    if (rc == pp_sam_host::ERR_QUIT) {
        if (bad == ~0ull || !msg[0]) return fprintf(stderr, "a refusal without its line at %llu bytes\n", (unsigned long long)n), 1;
        return 0;
    }
    if (rc != (n_ref ? pp_sam_host::ERR_ARG : pp_sam_host::OK) || end > n) return fprintf(stderr, "rc %d, end %llu of %llu bytes\n", rc, (unsigned long long)end, (unsigned long long)n), 1;
    std::vector<uint64_t> off(n_ref + 1);
    std::vector<uint32_t> len(n_ref + 1), ln(n_ref + 1);
    uint64_t end2 = ~0ull;
    if (pp_sam_host::header(p, n, n_ref, &again, off.data(), len.data(), ln.data(), &end2, &lines, &bad, msg, sizeof msg) != pp_sam_host::OK || again != n_ref || end2 != end)
        return fprintf(stderr, "the second call disagrees at %llu bytes\n", (unsigned long long)n), 1;
    for (uint32_t i = 0; i < n_ref; i++)
        if (len[i] == 0 || off[i] > end || len[i] > end - off[i] || ln[i] == 0 || ln[i] > 0x7FFFFFFFu)
            return fprintf(stderr, "reference %u outside the header at %llu bytes\n", i, (unsigned long long)n), 1;
    return 0;
}

int main(int argc, char **argv) {
    std::string text = "@HD\tVN:1.6\r\n@SQ\tSN:one\tLN:12\tM5:x\n@CO\tSN:no\n@SQ\tLN:2147483647\tSN:two\r\n@SQX\tSN:three\n@SQ\tSN:3\tLN:7\nr\t4\t*\n@SQ\tSN:late\n";
    if (argc > 1) {
        FILE *f = fopen(argv[1], "rb");
        if (!f) return fprintf(stderr, "cannot open %s\n", argv[1]), 2;
        text.clear();
        char buf[65536];
        for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0 && text.size() < (1u << 16);) text.append(buf, k);
        fclose(f);
    }
    const uint64_t n = text.size();
    uint64_t calls = 0;
    for (uint64_t cut = 0; cut <= n; cut++) {
        uint8_t *p = (uint8_t *)malloc(cut ? cut : 1);
        memcpy(p, text.data(), cut);
        if (check(cut ? p : nullptr, cut)) return 1;
        calls++;
        for (uint64_t at = 0; at < cut; at += (cut > 512 ? 7 : 1))
            for (const char c : {'\t', '\n', ':', '\0'}) {
                const uint8_t was = p[at];
                p[at] = (uint8_t)c;
                if (check(p, cut)) return 1;
                p[at] = was;
                calls++;
            }
        free(p);
    }
    printf("sam_host_check: %llu calls over %llu bytes, every answer inside its prefix\n", (unsigned long long)calls, (unsigned long long)n);
    return 0;
}
