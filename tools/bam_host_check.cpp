// bam_host_check.cpp -- a stand-alone program over the two host walks behind pp_bam_header / pp_bam_walk (polypolish_amd/csrc/
// pp_bam_host.h), made to be built with a sanitizer and run on a machine without a GPU:
//   clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ipolypolish_amd/csrc tools/bam_host_check.cpp -o bam_host_check
//   python -c "import sys; sys.path.insert(0, 'tests'); import test_bam_model_cpu as t; h, b, _, _ = t.small_file(); open('small.bam.raw', 'wb').write(h + b)"
//   ./bam_host_check small.bam.raw
// Every prefix of the file goes to both functions in a heap block of EXACTLY its length (so that a read past the cut is a read
// past the allocation), then every prefix with one byte flipped; the program checks what tests/test_bam_model_cpu.py checks -- a
// cut is refused or stops the walk at the cut, no record runs past it -- and the sanitizer checks every load.  step(), the one
// record of the chain that the device walk's kernels run as well (pp_bam_walk.hip), is called at EVERY offset of every prefix, on
// the chain or not, and every verdict is worded by walk_message() into a buffer of exactly the message's size.
#include "pp_bam_host.h"

#include <cstdlib>
#include <vector>

// step() at every offset of the prefix: a good record ends inside the prefix, a refused one names why, the message fits
static int check_steps(const uint8_t *p, uint64_t n) {
    for (uint64_t at = 0; at <= n; at++) {
        uint64_t next = ~0ull;
        uint32_t bs = ~0u;
        const uint32_t kind = pp_bam_host::step(p, n, at, &next, &bs);
        if (kind == pp_bam_host::W_OK ? (next < at + 36 || next > n || bs != next - at - 4) : (next != ~0ull || kind > pp_bam_host::W_PAST))
            return fprintf(stderr, "step at %llu of %llu bytes: kind %u, next %llu\n", (unsigned long long)at, (unsigned long long)n, kind, (unsigned long long)next), 1;
        if (kind != pp_bam_host::step_kind(n - at, bs)) return fprintf(stderr, "step and step_kind disagree at %llu\n", (unsigned long long)at), 1;
        if ((kind == pp_bam_host::W_CUT) != (n - at < 4)) return fprintf(stderr, "a cut block_size at %llu of %llu bytes\n", (unsigned long long)at, (unsigned long long)n), 1;
        char probe[256];
        pp_bam_host::walk_message(probe, sizeof probe, kind, at, at, bs, n);
        const size_t len = strlen(probe);
        char *exact = (char *)malloc(len + 1);  // exactly the message: one byte more is not ours
        pp_bam_host::walk_message(exact, len + 1, kind, at, at, bs, n);
        const bool same = strcmp(exact, probe) == 0 && (kind == pp_bam_host::W_OK) == (len == 0);
        free(exact);
        if (!same) return fprintf(stderr, "walk_message of kind %u\n", kind), 1;
    }
    return 0;
}

static int check(const uint8_t *p, uint64_t n, uint64_t *walked_ok) {
    if (check_steps(p, n)) return 1;
    uint32_t n_ref = 0;
    uint64_t at = 0, name_off[4];
    uint32_t name_len[4], ref_len[4];
    char msg[256];
    const int rc = pp_bam_host::header(p, n, 4, &n_ref, name_off, name_len, ref_len, &at, msg, sizeof msg);
    if (rc && n_ref <= 4) return 0;  // refused (n_ref > 4: only the arrays were short, the header itself stands)
    for (uint32_t i = 0; i < n_ref && i < 4; i++)
        if (name_off[i] > n || name_len[i] >= n - name_off[i]) return fprintf(stderr, "name %u runs past %llu bytes\n", i, (unsigned long long)n), 1;
    if (at > n) return fprintf(stderr, "records_at %llu past %llu bytes\n", (unsigned long long)at, (unsigned long long)n), 1;
    uint64_t n_rec = 0, end = 0;
    std::vector<uint64_t> off(64);
    const int wr = pp_bam_host::walk(p, n, at, off.data(), off.size(), &n_rec, &end, msg, sizeof msg);
    if (n_rec > off.size() || end > n) return fprintf(stderr, "walk: %llu records, end %llu of %llu bytes\n", (unsigned long long)n_rec, (unsigned long long)end, (unsigned long long)n), 1;
    for (uint64_t r = 0; r < n_rec; r++) {
        if (n - off[r] < 4 || (uint64_t)pp_bam_host::le32(p + off[r]) > n - off[r] - 4)
            return fprintf(stderr, "record %llu runs past the cut at %llu\n", (unsigned long long)r, (unsigned long long)n), 1;
    }
    if (!wr && n_rec < off.size() && end != n) return fprintf(stderr, "a clean walk stopped at %llu of %llu bytes\n", (unsigned long long)end, (unsigned long long)n), 1;
    if (!wr) ++*walked_ok;
    uint64_t counted = 0;
    const int cr = pp_bam_host::walk(p, n, at, nullptr, 0, &counted, &end, msg, sizeof msg);
    if (cr != wr && n_rec < off.size()) return fprintf(stderr, "counting and filling disagree at %llu bytes\n", (unsigned long long)n), 1;
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 2) return fprintf(stderr, "usage: %s FILE (header and records of an uncompressed BAM)\n", argv[0]), 2;
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
        if (cut) {  // ... and with a byte of its last 48 turned over (lengths, block sizes, NULs)
            for (uint64_t back = 1; back <= 48 && back <= cut; back += 5) {
                p[cut - back] ^= 0xFF;
                if (check(p, cut, &ok)) return 1;
                p[cut - back] ^= 0xFF;
                runs++;
            }
        }
        free(p);
    }
    printf("bam_host_check: %llu runs over the prefixes of %zu bytes, %llu of them walked to a clean end\n", (unsigned long long)runs, all.size(),
           (unsigned long long)ok);
    return ok ? 0 : 1;
}
