// text_chain_host_check.cpp -- a stand-alone program over the host code the commands' --text_chain adds in front of the device: the walk
// behind pp_aln_file_kind_text (polypolish_amd/csrc/pp_aln_kind_host.h) and the host side of opening a bgzipped text, the block chain
// pp_bgzf_inflate walks for a caller who brings no offsets (pp_bgzf_host.h).  Made to be built with a sanitizer and run on a machine
// without a GPU, as tools/sam_host_check.cpp and tools/bgzf_host_check.cpp are:
//   clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ipolypolish_amd/csrc tools/text_chain_host_check.cpp -o text_chain_host_check -lz
//   ./text_chain_host_check
// A small SAM text is bgzipped here -- a compressed block, a stored one, an empty block in the middle, a block with a subfield in front
// of BC, the EOF block; cuts inside a line and inside a "\r\n" -- and EVERY prefix of the file goes to both forms of the kind walk and
// to the block walk in a heap block of EXACTLY its length: a load behind the cut is a load behind the allocation.  The program checks
//   * both forms agree, except that the text form says SAM_BGZF where the other refuses NOT_BAM;
//   * a file cut inside its first gzip header is CUT; from the first whole block on it is SAM_BGZF; in between -- a whole header, the
//     block cut -- it is SAM_BGZF as soon as a byte of content is out and BAM by its head before that (the inflate names the truncation);
//   * the blocks the walk finds lie inside the prefix, and inflated with zlib they are a prefix of the text;
// then the same with a BAM magic as content (BAM by both forms), plain gzip (NOT_BGZF by both) and the text itself (SAM by both).
#include "pp_aln_kind_host.h"
#include "pp_bgzf_host.h"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

namespace ah = pp_aln_host;
namespace hb = pp_bgzf_host;

static std::vector<uint8_t> g_file;

static void add_block(const std::string &piece, bool stored, bool extra_front) {
    std::vector<uint8_t> out(piece.size() + hb::STORE_EXTRA + 64);
    const uint8_t *in = (const uint8_t *)piece.data();
    uint32_t n = stored ? hb::store_block(in, (uint32_t)piece.size(), out.data()) : hb::deflate_block(in, (uint32_t)piece.size(), out.data());
    out.resize(n);
    if (extra_front) {  // XY 3 abc in front of BC: XLEN and BSIZE grow by seven
        const uint8_t sub[7] = {'X', 'Y', 3, 0, 'a', 'b', 'c'};
        out.insert(out.begin() + 12, sub, sub + 7);
        const uint32_t xlen = hb::le16(out.data() + 10) + 7, bsize = hb::le16(out.data() + 12 + 7 + 4) + 7;
        out[10] = (uint8_t)xlen;
        out[11] = (uint8_t)(xlen >> 8);
        out[12 + 7 + 4] = (uint8_t)bsize;
        out[12 + 7 + 5] = (uint8_t)(bsize >> 8);
    }
    g_file.insert(g_file.end(), out.begin(), out.end());
}

static void add_eof() {
    for (uint32_t j = 0; j < hb::EOF_SIZE; j++) g_file.push_back(hb::eof_byte(j));
}

// both forms of the kind walk on a heap block of exactly n bytes -> the text form's answer and kind
static int kinds(const std::vector<uint8_t> &all, uint64_t n, int *kind_text, int *answer_plain, int *kind_plain) {
    uint8_t *p = (uint8_t *)malloc(n ? n : 1);
    memcpy(p, all.data(), n);
    ah::Bytes src{p, n};
    const int a = ah::kind_of(src, kind_text, true);
    *answer_plain = ah::kind_of(src, kind_plain, false);
    free(p);
    return a;
}

// the text form says SAM_BGZF exactly where the other refuses NOT_BAM; everywhere else the two answer alike
static bool agree(int at, int kt, int ap, int kp) {
    if (at == ah::OK && kt == ah::SAM_BGZF) return ap == ah::NOT_BAM;
    return ap == at && (at != ah::OK || kp == kt);
}

// the block walk on a heap block of exactly n bytes; what it finds inflates to a prefix of `text`
static int walk_and_inflate(const std::vector<uint8_t> &all, uint64_t n, const std::string &text, uint64_t *whole_blocks) {
    uint8_t *p = (uint8_t *)malloc(n ? n : 1);
    memcpy(p, all.data(), n);
    char msg[256] = "";
    uint64_t n_blk = 0, end = 0;
    std::vector<uint64_t> off(64), out(65);
    const int rc = hb::walk(p, n, 0, off.data(), out.data(), off.size(), &n_blk, &end, msg, sizeof msg);
    int bad = 0;
    if (n_blk > off.size() || end > n || (rc == hb::OK && end != n) || (rc != hb::OK && !msg[0])) bad = 1;
    std::string back;
    for (uint64_t b = 0; !bad && b < n_blk; b++) {
        hb::Block B;
        if (hb::block(p, n, off[b], &B) || B.total > n - off[b]) { bad = 2; break; }
        std::vector<uint8_t> piece(B.isize ? B.isize : 1);
        z_stream zs;
        memset(&zs, 0, sizeof zs);
        if (inflateInit2(&zs, -15) != Z_OK) { bad = 3; break; }
        zs.next_in = p + off[b] + B.payload;
        zs.avail_in = B.pay_len;
        zs.next_out = piece.data();
        zs.avail_out = B.isize;
        const int r = inflate(&zs, Z_FINISH);
        if (r != Z_STREAM_END || zs.total_out != B.isize) bad = 4;
        inflateEnd(&zs);
        back.append((const char *)piece.data(), B.isize);
        if (back.size() != out[b + 1]) bad = 5;
    }
    if (!bad && text.compare(0, back.size(), back) != 0) bad = 6;
    free(p);
    if (bad) fprintf(stderr, "the block walk at %llu bytes: check %d failed (%s)\n", (unsigned long long)n, bad, msg);
    *whole_blocks = n_blk;
    return bad;
}

int main() {
    std::string text = "@HD\tVN:1.6\r\n@SQ\tSN:ctg\tLN:100\r\n";
    for (int i = 0; i < 40; i++)
        text += "r" + std::to_string(i) + "\t" + (i % 3 ? "0" : "16") + "\tctg\t" + std::to_string(1 + i) + "\t60\t8M\t*\t0\t0\tACGTACGT\tIIIIIIII\tNM:i:" +
                std::to_string(i % 2) + (i % 2 ? "\r\n" : "\n");
    const size_t crlf = text.find("\r\n", 300);
    const size_t cuts[] = {0, 7, 150, crlf + 1, 700, text.size()};  // inside a line; between "\r" and "\n"
    for (int k = 0; k < 5; k++) {
        add_block(text.substr(cuts[k], cuts[k + 1] - cuts[k]), k == 1, k == 3);
        if (k == 2) add_eof();  // an empty block in the middle
    }
    add_eof();
    const uint32_t first_header = 18;
    hb::Block first;
    if (hb::block(g_file.data(), g_file.size(), 0, &first)) return fprintf(stderr, "the first block is not one\n"), 1;
    uint64_t calls = 0, with_blocks = 0;
    for (uint64_t n = 0; n <= g_file.size(); n++) {
        int kt = -1, kp = -1, ap = -1;
        const int at = kinds(g_file, n, &kt, &ap, &kp);
        const int want = n < 2 ? ah::OK : (n < first_header ? ah::CUT : ah::OK);
        const bool kind_ok = n < 2 ? kt == ah::SAM : (n >= first.total ? kt == ah::SAM_BGZF : (kt == ah::SAM_BGZF || kt == ah::BAM));
        if (at != want || (at == ah::OK && !kind_ok))
            return fprintf(stderr, "the text form at %llu bytes: answer %d kind %d\n", (unsigned long long)n, at, kt), 1;
        if (!agree(at, kt, ap, kp))
            return fprintf(stderr, "the two forms disagree at %llu bytes: %d/%d and %d/%d\n", (unsigned long long)n, at, kt, ap, kp), 1;
        uint64_t blocks = 0;
        if (walk_and_inflate(g_file, n, text, &blocks)) return 1;
        with_blocks += blocks != 0;
        calls += 3;
    }
    // the same head with BAM\1 as content, plain gzip, the text itself: every prefix again
    std::vector<uint8_t> bam;
    {
        std::vector<uint8_t> keep;
        keep.swap(g_file);
        add_block(std::string("BA"), false, true);
        add_block(std::string("M\1rest"), true, false);
        add_eof();
        bam.swap(g_file);
        g_file.swap(keep);
    }
    for (uint64_t n = 0; n <= bam.size(); n++) {
        int kt = -1, kp = -1, ap = -1;
        const int at = kinds(bam, n, &kt, &ap, &kp);
        // BAM once four bytes are out -- and before, while the cut keeps what is out from saying otherwise; "BA" and the end of the
        // file behind it is no BAM
        const bool head = n < 25;  // 12 + XLEN 13: the first block's header with its subfield in front of BC
        if (!agree(at, kt, ap, kp) || (head ? at != (n < 2 ? ah::OK : ah::CUT) : at != ah::OK) || (n == bam.size() && kt != ah::BAM))
            return fprintf(stderr, "the BAM head at %llu bytes: %d/%d and %d/%d\n", (unsigned long long)n, at, kt, ap, kp), 1;
        calls += 2;
    }
    std::vector<uint8_t> gz = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xff, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (uint64_t n = 0; n <= gz.size(); n++) {
        int kt = -1, kp = -1, ap = -1;
        const int at = kinds(gz, n, &kt, &ap, &kp), want = n < 2 ? ah::OK : (n < 10 ? ah::CUT : ah::NOT_BGZF);
        if (at != want || ap != want) return fprintf(stderr, "plain gzip at %llu bytes: %d and %d\n", (unsigned long long)n, at, ap), 1;
        calls += 2;
    }
    std::vector<uint8_t> plain(text.begin(), text.end());
    for (uint64_t n = 0; n <= plain.size(); n += 3) {
        int kt = -1, kp = -1, ap = -1;
        if (kinds(plain, n, &kt, &ap, &kp) != ah::OK || ap != ah::OK || kt != ah::SAM || kp != ah::SAM)
            return fprintf(stderr, "the text at %llu bytes is not text\n", (unsigned long long)n), 1;
        calls += 2;
    }
    printf("text_chain_host_check: %llu calls over the prefixes of a %zu-byte bgzipped SAM (%llu of them with whole blocks), a BAM head, plain gzip "
           "and the text: every answer as expected, every block inside its prefix\n", (unsigned long long)calls, g_file.size(), (unsigned long long)with_blocks);
    return 0;
}
