// fasta_host_check.cpp -- a stand-alone program over the host part of pp_fasta_records (polypolish_amd/csrc/pp_fasta_host.h), made to be
// built with a sanitizer and run on a machine without a GPU, as tools/sam_host_check.cpp is for pp_sam_header's walk:
//   clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ipolypolish_amd/csrc tools/fasta_host_check.cpp -lpthread -o fasta_host_check
//   ./fasta_host_check            (a built-in text)      ./fasta_host_check some.fasta
// For every prefix of the text a plain loop stands in for the device: the header lines' ranges, the bases in front of each, the first
// offending sequence byte.  The header lines are packed into a heap block of EXACTLY their length and the offending line into one of
// exactly its length (a read past either is a read past the allocation); then the host part runs as pp_fasta_records runs it:
// first_bad_header, sequence_line on the offending line, contigs.  The program checks the answers against a second plain walk over
// the prefix (the loader's own order: line by line); the sanitizer checks every load.
#include "pp_fasta_host.h"

#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace fh = pp_fasta_host;

struct Answer {
    int code = 0;
    std::string words;  // of a refusal
    std::vector<std::string> names, descs;
    std::vector<uint64_t> off;
    bool operator==(const Answer &o) const {  // (a refusal: its code and words; else the contigs)
        return code == o.code && words == o.words && (code != 0 || (names == o.names && descs == o.descs && off == o.off));
    }
};

// the lines of [0, n) as the loader's LineReader cuts them
template <class F>
static void each_line(const char *t, size_t n, F f) {
    size_t at = 0;
    while (at < n) {
        const void *nl = memchr(t + at, '\n', n - at);
        size_t l = nl ? (size_t)((const char *)nl - (t + at)) : n - at;
        const size_t next = at + l + (nl ? 1 : 0);
        if (l > 0 && t[at + l - 1] == '\r') l--;
        if (!f(at, l)) return;
        at = next;
    }
}

// load_fasta of pp_ingest.cpp, line by line, with the names and offsets only
static Answer by_lines(const char *t, size_t n) {
    Answer A;
    std::string name, desc;
    uint64_t bases = 0;
    bool have = false;
    auto refuse = [&](int code, const char *w) { A.code = code; A.words = w; return false; };
    A.off.push_back(0);
    auto push = [&] { A.names.push_back(name); A.descs.push_back(desc); A.off.push_back(bases); };
    each_line(t, n, [&](size_t at, size_t l) {
        const char *line = t + at;
        if (l == 0) return true;
        if (line[0] == '>') {
            if (!pph::valid_utf8(line, l)) return refuse(fh::ERR_QUIT, "unable to load \"p\"");
            if (have) push();
            fh::split_header(line, l, name, desc);
            have = !name.empty();
            return true;
        }
        char msg[256] = "";
        if (int code = fh::sequence_line("p", line, l, have, msg, sizeof msg)) return refuse(code, msg);
        bases += l;
        return true;
    });
    if (A.code) return A;
    if (have) push();
    if (A.names.empty()) return refuse(fh::ERR_QUIT, "\"p\" contains no sequences"), A;
    for (size_t i = 0; i < A.names.size(); i++)
        if (A.off[i + 1] == A.off[i]) return refuse(fh::ERR_QUIT, "\"p\" has an empty sequence"), A;
    for (size_t i = 0; i < A.names.size(); i++)
        for (size_t j = i + 1; j < A.names.size(); j++)
            if (A.names[i] == A.names[j]) return refuse(fh::ERR_QUIT, "\"p\" has a duplicated name"), A;
    return A;
}

// the device's part by a plain loop, then the host part on heap blocks of exactly the lengths it is given
static Answer as_the_call(const char *t, size_t n) {
    std::vector<fh::Header> hdr;
    uint64_t bases = 0, bad_at = ~0ull, bad_start = 0, bad_len = 0, pk_total = 0;
    bool have = false, bad_have = false;
    each_line(t, n, [&](size_t at, size_t l) {
        if (l == 0) return true;
        if (t[at] == '>') {
            hdr.push_back(fh::Header{at, l, bases});
            pk_total += l;
            // (the device's hdr_named: a line end, the text's end or a White_Space character behind '>')
            have = l > 1 && pph::rust_ws_len(t + at + 1, l - 1) == 0;
            return true;
        }
        bool ascii = true;
        for (size_t i = 0; i < l; i++) ascii = ascii && ((unsigned char)t[at + i] & 0x80u) == 0;
        if ((!have || !ascii) && bad_at == ~0ull) {
            bad_at = at; bad_start = at; bad_len = l; bad_have = have;
            return false;  // (what lies behind the first offending byte does not matter: the device reports the minimum)
        }
        bases += l;
        return true;
    });
    // headers behind the offending byte are still found by the device: take them all, as it does
    if (bad_at != ~0ull) {
        each_line(t, n, [&](size_t at, size_t l) {
            if (at <= bad_at) return true;
            if (l && t[at] == '>') { hdr.push_back(fh::Header{at, l, bases}); pk_total += l; }
            return true;
        });
    }
    char *packed = (char *)malloc(pk_total ? pk_total : 1);
    uint64_t w = 0;
    for (const fh::Header &h : hdr) { memcpy(packed + w, t + h.off, h.len); w += h.len; }
    Answer A;
    char msg[256] = "";
    const size_t ib = fh::first_bad_header(pk_total ? packed : nullptr, hdr.data(), hdr.size(), bad_at);
    if (ib < hdr.size()) {
        A.code = fh::ERR_QUIT; A.words = "unable to load \"p\"";
    } else if (bad_at != ~0ull) {
        char *line = (char *)malloc(bad_len ? bad_len : 1);
        memcpy(line, t + bad_start, bad_len);
        A.code = fh::sequence_line("p", line, bad_len, bad_have, msg, sizeof msg);
        A.words = msg;
        free(line);
        if (A.code == fh::OK) { A.code = -1; A.words = "the host takes a line the device refused"; }
    } else {
        fh::Contigs c;
        A.code = fh::contigs("p", pk_total ? packed : nullptr, hdr.data(), hdr.size(), bases, c, msg, sizeof msg);
        A.words = msg;
        if (A.code == fh::OK) { A.names = c.names; A.descs = c.descs; A.off = c.off; }
    }
    free(packed);
    return A;
}

int main(int argc, char **argv) {
    std::string text =
        ">one first  contig\r\nACGTacgt\r\nNNNN\n\n>\xC2\xA0unnamed\n>two\xE2\x80\x83wide blank\nAC\rGT\n>\n> d\n>three\tx\nTT\r\r\n"
        ">one again\nAC\n>bad\xE2\x80\nAC\nA\xC3\xA9\nA\xFF\n>\nAC\n>last\nACGT\r";
    if (argc > 1) {
        FILE *f = fopen(argv[1], "rb");
        if (!f) return fprintf(stderr, "cannot open %s\n", argv[1]), 2;
        text.clear();
        char buf[65536];
        for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0 && text.size() < (1u << 16);) text.append(buf, k);
        fclose(f);
    }
    const size_t n = text.size();
    unsigned long long calls = 0, refused = 0;
    for (size_t cut = 0; cut <= n; cut++) {
        char *p = (char *)malloc(cut ? cut : 1);
        memcpy(p, text.data(), cut);
        for (int alter = 0; alter < 4; alter++) {  // the prefix as it is, then with its last byte a '>', a '\r', a 0xC2
            if (alter && cut == 0) break;
            const char was = cut ? p[cut - 1] : 0;
            if (alter) p[cut - 1] = ">\r\xC2"[alter - 1];
            const Answer a = by_lines(p, cut), b = as_the_call(p, cut);
            if (!(a == b))
                return fprintf(stderr, "the two walks disagree at %zu bytes (form %d): %d \"%s\" against %d \"%s\"\n", cut, alter, a.code, a.words.c_str(), b.code,
                               b.words.c_str()), 1;
            refused += a.code != 0;
            calls++;
            if (alter) p[cut - 1] = was;
        }
        free(p);
    }
    printf("fasta_host_check: %llu calls over %zu bytes, %llu refusals, the host part agrees with the loader's walk on every prefix\n", calls, n, refused);
    return 0;
}
