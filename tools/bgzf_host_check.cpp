// bgzf_host_check.cpp -- a stand-alone program over the host walk behind pp_bgzf_walk (polypolish_amd/csrc/pp_bgzf_host.h), made to be
// built with a sanitizer and run on a machine without a GPU:
//   clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ipolypolish_amd/csrc tools/bgzf_host_check.cpp -o bgzf_host_check
//   python -c "import sys; sys.path.insert(0, 'tests'); import test_bgzf_model_cpu as t; open('three.bgzf', 'wb').write(t.three_blocks()[0])"
//   ./bgzf_host_check three.bgzf
// Every prefix of the file goes to the walk in a heap block of EXACTLY its length (so that a read past the cut is a read past the
// allocation), then every prefix with one byte of its last 48 turned over; the program checks what tests/test_bgzf_model_cpu.py
// checks -- a cut is refused or stops the walk at the cut, no block runs past it -- and the sanitizer checks every load.
#include "pp_bgzf_host.h"

#include <cstdlib>
#include <vector>

static int check(const uint8_t *p, uint64_t n, uint64_t *walked_ok) {
    char msg[256];
    uint64_t n_blk = 0, end = 0;
    std::vector<uint64_t> off(16), out(17);
    const int wr = pp_bgzf_host::walk(p, n, 0, off.data(), out.data(), off.size(), &n_blk, &end, msg, sizeof msg);
    if (n_blk > off.size() || end > n) return fprintf(stderr, "walk: %llu blocks, end %llu of %llu bytes\n", (unsigned long long)n_blk, (unsigned long long)end, (unsigned long long)n), 1;
    for (uint64_t b = 0; b < n_blk; b++) {
        pp_bgzf_host::Block B;
        if (pp_bgzf_host::block(p, n, off[b], &B) || B.total > n - off[b] || out[b + 1] - out[b] != B.isize)
            return fprintf(stderr, "block %llu runs past the cut at %llu\n", (unsigned long long)b, (unsigned long long)n), 1;
    }
    if (!wr && n_blk < off.size() && end != n) return fprintf(stderr, "a clean walk stopped at %llu of %llu bytes\n", (unsigned long long)end, (unsigned long long)n), 1;
    if (!wr) ++*walked_ok;
    uint64_t counted = 0, end2 = 0;
    const int cr = pp_bgzf_host::walk(p, n, 0, nullptr, nullptr, 0, &counted, &end2, msg, sizeof msg);
    if (n_blk < off.size() && (cr != wr || counted != n_blk || end2 != end)) return fprintf(stderr, "counting and filling disagree at %llu bytes\n", (unsigned long long)n), 1;
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 2) return fprintf(stderr, "usage: %s FILE (a few BGZF blocks)\n", argv[0]), 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return perror(argv[1]), 2;
    std::vector<uint8_t> all;
    uint8_t buf[4096];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) all.insert(all.end(), buf, buf + k);
    fclose(f);
    uint64_t runs = 0, ok = 0;
    for (uint64_t cut = 0; cut <= all.size(); cut++) {
        uint8_t *p = (uint8_t *)malloc(cut ? cut : 1);  // exactly the prefix: the byte behind it is not ours
        for (uint64_t i = 0; i < cut; i++) p[i] = all[i];
        if (check(p, cut, &ok)) return 1;
        runs++;
        if (cut) {  // ... and with a byte of its last 48 turned over (XLEN, SLEN, BSIZE, ISIZE)
            for (uint64_t back = 1; back <= 48 && back <= cut; back++) {
                p[cut - back] ^= 0xFF;
                if (check(p, cut, &ok)) return 1;
                p[cut - back] ^= 0xFF;
                runs++;
            }
        }
        free(p);
    }
    printf("bgzf_host_check: %llu runs over the prefixes of %zu bytes, %llu of them walked to a clean end\n", (unsigned long long)runs, all.size(),
           (unsigned long long)ok);
    return ok ? 0 : 1;
}
