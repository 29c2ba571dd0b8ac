// bam_sam_host_check.cpp -- a stand-alone program over the host parts of pp_bam_sam (polypolish_amd/csrc/pp_bam_sam_host.h: the SAM
// header text of a BAM header, the @SQ synthesis; pp_fmt_g.h: "%g" of a float32 in integer arithmetic), made to be built with a
// sanitizer and run on a machine without a GPU, as tools/sam_host_check.cpp is for pp_sam_header:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ipolypolish_amd/csrc tools/bam_sam_host_check.cpp -o bam_sam_host_check
//   ./bam_sam_host_check [N]        N: random float32 bit patterns against printf (default 2,000,000; "all": every finite float32)
// (1) fmt_g against snprintf("%g", (double)f): the issue's table, every exponent with the mantissas 0, 1, 0x400000, 0x7FFFFF and
// their neighbours, then N random bit patterns.  (2) header_text on a built-in BAM header: every prefix in a heap block of EXACTLY its
// length (a read past the cut is a read past the allocation), then every prefix with one byte replaced; an accepted header must end at
// the cut, and its names must lie inside it.
//   ./bam_sam_host_check --decode BAM RECORDS_AT REC_OFF [PASS] > text
// (3) the kernels' own per-record code (pp_bam_sam_lines.h) in loops over tiles, records and lanes, as pass A and pass B run it:
// BAM = uncompressed BAM bytes, REC_OFF = the records' offsets as raw uint64, PASS = one verdict byte per aligned record.  Every
// input goes into a heap block of exactly its length.  A refusal prints "refused <why> <record>" and ends with status 3.
#include "pp_bam_sam_host.h"
#include "pp_bam_sam_lines.h"

#include <cstdlib>
#include <cstring>
#include <random>
#include <string>

static int check_g(uint32_t bits) {
    if ((bits & 0x7F800000u) == 0x7F800000u) return 0;  // inf, nan: the caller's
    float f;
    memcpy(&f, &bits, 4);
    char want[64];
    snprintf(want, sizeof want, "%g", (double)f);
    const pp_fmt::Text16 T = pp_fmt::fmt_g(bits);
    char got[17] = "";
    for (uint32_t i = 0; i < T.n && i < 16; i++) got[i] = (char)T.at(i);
    got[T.n < 16 ? T.n : 16] = 0;
    if (T.n > 16 || strcmp(got, want) != 0) return fprintf(stderr, "fmt_g(0x%08x) = \"%s\", printf says \"%s\"\n", bits, got, want), 1;
    return 0;
}

static void put32(std::string &s, uint32_t v) {
    for (int i = 0; i < 4; i++) s.push_back((char)(v >> (8 * i)));
}

static int check_header(const uint8_t *p, uint64_t n) {
    pp_bam_sam_host::Header H;
    char msg[256] = "";
    const int rc = pp_bam_sam_host::header_text(p, n, &H, msg, sizeof msg);
    if (rc == pp_bam_sam_host::OK) {
        if (H.name_off.size() != H.ok.size() + 1 || H.name_off.back() != H.names.size() || H.names.size() > n)
            return fprintf(stderr, "names outside the header at %llu bytes\n", (unsigned long long)n), 1;
        if (!H.text.empty() && H.text.back() != '\n') return fprintf(stderr, "a header text without its newline at %llu bytes\n", (unsigned long long)n), 1;
    } else if (rc != pp_bam_sam_host::ERR_ARG && rc != pp_bam_sam_host::ERR_LIMIT)
        return fprintf(stderr, "rc %d at %llu bytes\n", rc, (unsigned long long)n), 1;
    return 0;
}

static bool slurp(const char *path, uint8_t **p, uint64_t *n) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    std::string d;
    char buf[65536];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) d.append(buf, k);
    fclose(f);
    *n = d.size();
    *p = (uint8_t *)malloc(d.size() ? d.size() : 1);
    memcpy(*p, d.data(), d.size());
    return true;
}

static int decode(int argc, char **argv) {
    uint8_t *B = nullptr, *offs = nullptr, *pass = nullptr;
    uint64_t N = 0, n_off = 0, n_pass = 0;
    struct Free {
        uint8_t **a, **b, **c;
        ~Free() { free(*a); free(*b); free(*c); }
    } free_inputs{&B, &offs, &pass};
    if (argc < 5 || !slurp(argv[2], &B, &N) || !slurp(argv[4], &offs, &n_off) || (argc > 5 && !slurp(argv[5], &pass, &n_pass)))
        return fprintf(stderr, "usage: --decode BAM RECORDS_AT REC_OFF [PASS]\n"), 2;
    const uint64_t records_at = strtoull(argv[3], nullptr, 10), n_rec = n_off / 8;
    std::vector<u64> rec_off(n_rec);
    if (n_rec) memcpy(rec_off.data(), offs, n_rec * 8);
    pp_bam_sam_host::Header H;
    char msg[256] = "";
    if (records_at > N) return fprintf(stderr, "refused header -1\n"), 3;
    if (int rc = pp_bam_sam_host::header_text(B, records_at, &H, msg, sizeof msg)) return fprintf(stderr, "refused header%d -1 %s\n", rc, msg), 3;
    const RefTab R{H.names.data(), (const u64 *)H.name_off.data(), H.ok.data(), (u32)H.ok.size()};
    // pass A
    std::vector<u64> len(n_rec), seq_at(n_rec), off(n_rec + 1);
    std::vector<u8> kind(n_rec);
    u64 n_al = 0;
    for (u64 r = 0; r < n_rec; r++) {
        u32 al = 0, bs = 0;
        u64 c = 0;
        if (const u32 why = check_record(B, N, rec_off[r], R, &al, &c, &bs)) return fprintf(stderr, "refused %u %llu\n", why, r), 3;
        Count cnt;
        emit_line(cnt, B, c, bs, R, false);
        len[r] = cnt.n;
        seq_at[r] = cnt.seq_at;
        kind[r] = (u8)al;
        n_al += al;
    }
    if (pass && n_pass != n_al) return fprintf(stderr, "refused verdicts -1\n"), 3;
    // the offsets, the tiles
    const u64 hdr_len = H.text.size();
    u64 at = hdr_len, rank = 0;
    for (u64 r = 0; r < n_rec; r++) {
        const u32 fail = ((kind[r] & 1u) && pass && pass[rank] == 0) ? 1u : 0u;
        rank += kind[r] & 1u;
        kind[r] = (u8)(kind[r] | fail << 1);
        off[r] = at;
        at += len[r] + 10u * fail;
    }
    const u64 total = off[n_rec] = at;
    std::vector<u32> tile_first(total / BS_TILE + 2, 0xFFFFFFFFu);
    for (u64 r = 0; r < n_rec; r++)
        for (u64 tile = (off[r] + BS_TILE - 1u) / BS_TILE; tile * BS_TILE < off[r + 1]; tile++) tile_first[tile] = (u32)r;
    // pass B
    std::vector<u8> out(total);
    for (u64 blk = 0; blk * BS_TILE < total; blk++) {
        u8 *img = (u8 *)calloc(BS_TILE, 1);
        const u64 t0 = blk * BS_TILE, t1 = std::min(total, t0 + (u64)BS_TILE);
        for (u64 i = t0; i < std::min(t1, hdr_len); i++) img[i - t0] = (u8)H.text[i];
        if (n_rec && t1 > hdr_len) {
            const u64 r_lo = t0 <= hdr_len ? 0 : tile_first[blk], r_hi = t0 + BS_TILE < total ? tile_first[blk + 1] : n_rec - 1;
            if (r_lo >= n_rec || r_hi >= n_rec) {
                free(img);
                return fprintf(stderr, "tile %llu has no first record\n", blk), 1;
            }
            for (u64 r = r_lo; r <= r_hi; r++) {
                const u64 c = rec_off[r] + 4u;
                Img W{img, (i64)(off[r] - t0)};
                emit_line(W, B, c, ld32(B, c - 4u), R, (kind[r] >> 1) & 1u);
                for (u32 hl = 0; hl < BS_GROUP; hl++) wide_parts(img, B, N, c, (i64)(off[r] - t0), seq_at[r], hl);
            }
        }
        memcpy(out.data() + t0, img, t1 - t0);
        free(img);
    }
    fwrite(out.data(), 1, out.size(), stdout);
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && strcmp(argv[1], "--decode") == 0) return decode(argc, argv);
    // ---- (1) "%g"
    const struct { float f; const char *s; } table[] = {{1000005.0f, "1e+06"}, {1000015.0f, "1.00002e+06"}, {999999.5f, "1e+06"}, {1e-45f, "1.4013e-45"},
                                                         {3.4028235e38f, "3.40282e+38"}, {100000.0f, "100000"}, {1.234565e-05f, "1.23457e-05"}, {0.1f, "0.1"}};
    for (const auto &t : table) {
        uint32_t bits;
        memcpy(&bits, &t.f, 4);
        const pp_fmt::Text16 T = pp_fmt::fmt_g(bits);
        std::string got;
        for (uint32_t i = 0; i < T.n; i++) got.push_back((char)T.at(i));
        if (got != t.s) return fprintf(stderr, "fmt_g(%a) = \"%s\", the table says \"%s\"\n", (double)t.f, got.c_str(), t.s), 1;
    }
    uint64_t n_g = 0;
    for (uint32_t e = 0; e < 255; e++)
        for (uint32_t m : {0u, 1u, 2u, 0x3FFFFFu, 0x400000u, 0x400001u, 0x7FFFFEu, 0x7FFFFFu})
            for (uint32_t s = 0; s < 2; s++, n_g++)
                if (check_g(s << 31 | e << 23 | m)) return 1;
    if (argc > 1 && strcmp(argv[1], "all") == 0) {
        for (uint64_t b = 0; b < (1ull << 32); b++, n_g++)
            if (check_g((uint32_t)b)) return 1;
    } else {
        const uint64_t n = argc > 1 ? strtoull(argv[1], nullptr, 10) : 2000000ull;
        std::mt19937 rng(12345);
        for (uint64_t i = 0; i < n; i++, n_g++)
            if (check_g((uint32_t)rng())) return 1;
    }
    // ---- (2) the header
    uint64_t calls = 0;
    for (int with_sq = 0; with_sq < 2; with_sq++) {
        const std::string text = with_sq ? std::string("@HD\tVN:1.6\n@SQ\tSN:one\tLN:12\n@CO\tx") + std::string(3, '\0') : std::string("@HD\tVN:1.6\n@SQX\tSN:no");
        std::string bam("BAM\1", 4);
        put32(bam, (uint32_t)text.size());
        bam += text;
        put32(bam, 3);
        for (const char *name : {"one", "t w", "*"}) {
            put32(bam, (uint32_t)strlen(name) + 1);
            bam.append(name, strlen(name) + 1);
            put32(bam, name[0] == '*' ? 0u : 12u);
        }
        const uint64_t n = bam.size();
        for (uint64_t cut = 0; cut <= n; cut++) {
            uint8_t *p = (uint8_t *)malloc(cut ? cut : 1);
            memcpy(p, bam.data(), cut);
            if (check_header(cut ? p : nullptr, cut)) return 1;
            calls++;
            for (uint64_t at = 0; at < cut; at++)
                for (const int c : {0, 1, 10, 9, 0xFF}) {
                    const uint8_t was = p[at];
                    p[at] = (uint8_t)c;
                    if (check_header(p, cut)) return 1;
                    p[at] = was;
                    calls++;
                }
            free(p);
        }
    }
    printf("bam_sam_host_check: %llu floats as printf prints them, %llu header calls inside their bytes\n", (unsigned long long)n_g, (unsigned long long)calls);
    return 0;
}
