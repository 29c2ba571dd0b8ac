// bgzf_host_check.cpp -- a stand-alone program over the host walk behind pp_bgzf_walk (polypolish_amd/csrc/pp_bgzf_host.h), made to be
// built with a sanitizer and run on a machine without a GPU:
//   clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ipolypolish_amd/csrc tools/bgzf_host_check.cpp -o bgzf_host_check -lz
//   python -c "import sys; sys.path.insert(0, 'tests'); import test_bgzf_model_cpu as t; open('three.bgzf', 'wb').write(t.three_blocks()[0])"
//   ./bgzf_host_check three.bgzf
// Every prefix of the file goes to the walk in a heap block of EXACTLY its length (so that a read past the cut is a read past the
// allocation), then every prefix with one byte of its last 48 turned over; the program checks what tests/test_bgzf_model_cpu.py
// checks -- a cut is refused or stops the walk at the cut, no block runs past it -- and the sanitizer checks every load.
// First of all store_block(), the writing twin, runs at 0, 1, 65,279 and 65,280 bytes and each result goes through block() and the walk.
// Then deflate_block(), the host twin of pp_bgzf_deflate's work on one piece (the code lengths, the header's run-length coding, the three
// costs: the very functions the kernel runs), at 0, 1, 3, 4, 5, 65,279 and 65,280 bytes of zeros, noise and skewed counts; every result is
// read back with zlib's inflate (link with -lz) and held against the input, its CRC32 and the bound of len + 31 bytes.
#include "pp_bgzf_host.h"

#include <cstdlib>
#include <vector>
#include <zlib.h>

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

// store_block() at the lengths where the framing can go wrong: input and output in heap blocks of EXACTLY their lengths, the result
// read back by the header's own step of the walk (block()), its stored-block prefix, payload, CRC32 (a second, table-free form) and ISIZE
static int check_store(uint32_t len) {
    namespace hb = pp_bgzf_host;
    uint8_t *in = (uint8_t *)malloc(len ? len : 1), *out = (uint8_t *)malloc(len + hb::STORE_EXTRA);
    for (uint32_t i = 0; i < len; i++) in[i] = (uint8_t)(i * 2654435761u >> 13);
    const uint32_t n = hb::store_block(in, len, out);
    hb::Block B;
    int bad = 0;
    if (n != len + hb::STORE_EXTRA || hb::block(out, n, 0, &B) || B.total != n || B.payload != 18 || B.pay_len != len + 5 || B.isize != len) bad = 1;
    if (!bad && (out[18] != 1 || hb::le16(out + 19) != len || hb::le16(out + 21) != (~len & 0xFFFFu) || memcmp(out + hb::STORE_HEAD, in, len) != 0)) bad = 2;
    uint32_t c = 0xFFFFFFFFu;  // the CRC32 once more, by the shifted polynomial per bit of the message
    for (uint32_t i = 0; i < len * 8u; i++) c = ((c ^ (in[i >> 3] >> (i & 7u))) & 1u) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
    if (!bad && hb::le32(out + hb::STORE_HEAD + len) != ~c) bad = 3;
    uint64_t n_blk = 0, end = 0;
    char msg[256];
    if (!bad && (hb::walk(out, n, 0, nullptr, nullptr, 0, &n_blk, &end, msg, sizeof msg) || n_blk != 1 || end != n)) bad = 4;
    free(in);
    free(out);
    if (bad) fprintf(stderr, "store_block(%u bytes): check %d failed\n", len, bad);
    return bad;
}

static int check_eof() {
    namespace hb = pp_bgzf_host;
    uint8_t *e = (uint8_t *)malloc(hb::EOF_SIZE);
    for (uint32_t j = 0; j < hb::EOF_SIZE; j++) e[j] = hb::eof_byte(j);
    hb::Block B;
    const int bad = hb::block(e, hb::EOF_SIZE, 0, &B) || B.total != hb::EOF_SIZE || B.pay_len != 2 || B.isize != 0 || e[18] != 3 || e[19] != 0;
    free(e);
    if (bad) fprintf(stderr, "the EOF block is not one\n");
    return bad;
}

// deflate_block() on `len` bytes of kind 0 = zeros, 1 = noise, 2 = skewed counts (byte value k about 1.6 times as often as k + 1: a
// Huffman tree deeper than 15 levels at the full length, so the repair runs): input, output and what zlib inflates in heap blocks of
// EXACTLY their lengths
static int check_deflate(uint32_t len, int kind, uint32_t *forms) {
    namespace hb = pp_bgzf_host;
    uint8_t *in = (uint8_t *)malloc(len ? len : 1), *out = (uint8_t *)malloc(len + hb::STORE_EXTRA), *back = (uint8_t *)malloc(len ? len : 1);
    uint32_t x = 12345u + len;
    for (uint32_t i = 0; i < len; i++) {
        x = x * 1664525u + 1013904223u;
        uint32_t v = 0;
        if (kind == 1) v = x >> 24;
        if (kind == 2) for (uint32_t u = x >> 8; v < 40u && (u & 0xFFFFFFu) % 1000u < 618u; u = u * 2654435761u + 1u) v++;
        in[i] = (uint8_t)v;
    }
    uint32_t type = 9;
    const uint32_t n = hb::deflate_block(in, len, out, &type);
    hb::Block B;
    int bad = 0;
    if (n > len + hb::STORE_EXTRA || type > hb::DF_DYNAMIC || hb::block(out, n, 0, &B) || B.total != n || B.payload != 18 || B.isize != len) bad = 1;
    if (!bad) {
        z_stream zs;
        memset(&zs, 0, sizeof zs);
        if (inflateInit2(&zs, -15) != Z_OK) bad = 2;
        else {
            zs.next_in = out + 18;
            zs.avail_in = B.pay_len;
            zs.next_out = back;
            zs.avail_out = len;
            if (inflate(&zs, Z_FINISH) != Z_STREAM_END || zs.total_out != len || zs.avail_in != 0 || memcmp(back, in, len) != 0) bad = 3;
            inflateEnd(&zs);
        }
    }
    if (!bad && hb::le32(out + n - 8) != (uint32_t)crc32(crc32(0L, Z_NULL, 0), in, len)) bad = 4;
    if (!bad) forms[type]++;
    free(in);
    free(out);
    free(back);
    if (bad) fprintf(stderr, "deflate_block(%u bytes, kind %d): check %d failed\n", len, kind, bad);
    return bad;
}

int main(int argc, char **argv) {
    if (argc != 2) return fprintf(stderr, "usage: %s FILE (a few BGZF blocks)\n", argv[0]), 2;
    for (uint32_t len : {0u, 1u, pp_bgzf_host::STORE_PAYLOAD - 1u, pp_bgzf_host::STORE_PAYLOAD})
        if (check_store(len)) return 1;
    if (check_eof()) return 1;
    printf("bgzf_host_check: store_block at 0, 1, 65279 and 65280 bytes reads back through block() and the walk\n");
    uint32_t forms[3] = {0, 0, 0};
    for (int kind = 0; kind < 3; kind++)
        for (uint32_t len : {0u, 1u, 3u, 4u, 5u, pp_bgzf_host::STORE_PAYLOAD - 1u, pp_bgzf_host::STORE_PAYLOAD})
            if (check_deflate(len, kind, forms)) return 1;
    printf("bgzf_host_check: deflate_block at 0, 1, 3, 4, 5, 65279 and 65280 bytes of zeros, noise and skewed counts inflates back with zlib "
           "(%u stored, %u fixed, %u dynamic)\n", forms[0], forms[1], forms[2]);
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
