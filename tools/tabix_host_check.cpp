// tabix_host_check.cpp -- a stand-alone program over the host side of pp_tabix_index (polypolish_amd/csrc/pp_tabix_host.h), made to be
// built with a sanitizer and run on a machine without a GPU, as tools/bam_sort_host_check.cpp is for the .bai:
//   clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ipolypolish_amd/csrc tools/tabix_host_check.cpp -o tabix_host_check
//   ./tabix_host_check
// A table set of six names -- chunks in three bins each, offsets near 2^48 << 16, windows -- is cut to every prefix of its names; each
// prefix goes to first_repeat() and serialise() with every array in a heap block of EXACTLY its count (a read past the count is a read
// past the allocation).  The program parses the bytes back field by field, checks that a name that comes back is found at its index
// whatever stands around it, that a table out of order, an empty name and an l_nm at its limit are refused with words and without
// bytes; the sanitizer checks every load.
#include "pp_tabix_host.h"

#include <cstdlib>
#include <string>

namespace th = pp_tabix_host;
namespace ih = pp_bam_index_host;

template <class T>
struct Exact {  // a heap block of exactly n elements (none: a null pointer)
    T *p = nullptr;
    explicit Exact(const std::vector<T> &v) {
        if (!v.empty()) {
            p = (T *)malloc(v.size() * sizeof(T));
            memcpy(p, v.data(), v.size() * sizeof(T));
        }
    }
    Exact(const Exact &) = delete;
    ~Exact() { free(p); }
};

static uint64_t rd(const std::vector<uint8_t> &b, size_t at, int n) {
    uint64_t v = 0;
    for (int i = 0; i < n; i++) v |= (uint64_t)b[at + i] << (8 * i);
    return v;
}

static int fail(const char *what, unsigned long long a) { return fprintf(stderr, "tabix_host_check: %s (%llu)\n", what, a), 1; }

struct Set {
    std::vector<std::string> names;
    std::vector<uint64_t> key, beg, end, lin_off, lin, ref_beg, ref_end, mapped, unmapped;
    std::vector<uint32_t> n_intv;
};

static Set build(const std::vector<std::string> &names) {
    Set S;
    S.names = names;
    const uint64_t far = ((1ull << 48) - 1) << 16;
    S.lin_off.push_back(0);
    for (uint32_t r = 0; r < names.size(); r++) {
        const uint32_t bins[3] = {r % 2 ? 0u : 1u, 585u + r, 4681u + 7 * r};
        for (int b = 0; b < 3; b++)
            for (uint32_t c = 0; c <= (uint32_t)b; c++) {
                S.key.push_back((uint64_t)r << 32 | bins[b]);
                S.beg.push_back(far - 1000 * (r + 1) + 10 * c);
                S.end.push_back(far - 1000 * (r + 1) + 10 * c + 9 + (c == (uint32_t)b ? 0xFFFFu - 9 : 0));
            }
        S.n_intv.push_back(r == 3 ? 0 : r + 1);
        for (uint32_t w = 0; w < S.n_intv.back(); w++) S.lin.push_back(far - w);
        S.lin_off.push_back(S.lin.size());
        S.ref_beg.push_back(far - 1000 * (r + 1));
        S.ref_end.push_back(far | 0xFFFF);
        S.mapped.push_back(r == 2 ? 0xFFFFFFFFFFull : r + 1);
        S.unmapped.push_back(0);
    }
    return S;
}

// serialise the first n names of S out of exact heap blocks; parse the bytes back
static int round_trip(const Set &S, uint32_t n, const th::Head &H) {
    uint64_t n_chunk = 0;
    while (n_chunk < S.key.size() && (S.key[n_chunk] >> 32) < n) n_chunk++;
    std::vector<uint8_t> names;
    std::vector<uint64_t> off(1, 0);
    for (uint32_t r = 0; r < n; r++) {
        names.insert(names.end(), S.names[r].begin(), S.names[r].end());
        off.push_back(names.size());
    }
    auto cut = [](const std::vector<uint64_t> &v, size_t k) { return std::vector<uint64_t>(v.begin(), v.begin() + k); };
    const Exact<uint8_t> x_names(names);
    const Exact<uint64_t> x_off(off), x_key(cut(S.key, n_chunk)), x_beg(cut(S.beg, n_chunk)), x_end(cut(S.end, n_chunk)), x_lin_off(cut(S.lin_off, n + 1)),
        x_lin(cut(S.lin, S.lin_off[n])), x_rb(cut(S.ref_beg, n)), x_re(cut(S.ref_end, n)), x_map(cut(S.mapped, n)), x_unm(cut(S.unmapped, n));
    const Exact<uint32_t> x_intv(std::vector<uint32_t>(S.n_intv.begin(), S.n_intv.begin() + n));
    ih::Tables T;
    T.n_ref = n;
    T.n_chunk = n_chunk;
    T.chunk_key = x_key.p;
    T.chunk_beg = x_beg.p;
    T.chunk_end = x_end.p;
    T.n_intv = x_intv.p;
    T.lin_off = x_lin_off.p;
    T.lin = x_lin.p;
    T.ref_beg = x_rb.p;
    T.ref_end = x_re.p;
    T.mapped = x_map.p;
    T.unmapped = x_unm.p;
    if (th::first_repeat(x_names.p, x_off.p, n) != n) return fail("distinct names were taken for a repeat at prefix", n);
    std::vector<uint8_t> out;
    char msg[200];
    msg[0] = 0;
    if (int rc = th::serialise(T, H, x_names.p, x_off.p, &out, msg, sizeof msg)) return fail(msg, (unsigned long long)rc);
    // ... and back
    if (out.size() < 44 || memcmp(out.data(), "TBI\1", 4) != 0) return fail("no magic at prefix", n);
    const int32_t want[8] = {(int32_t)n, H.format, H.col_seq, H.col_beg, H.col_end, 35, 0, (int32_t)(names.size() + n)};
    for (int i = 0; i < 8; i++)
        if ((int32_t)rd(out, 4 + 4 * i, 4) != want[i]) return fail("a header field differs, field", i);
    size_t at = 36;
    for (uint32_t r = 0; r < n; r++) {
        if (out.size() < at + S.names[r].size() + 1 || memcmp(out.data() + at, S.names[r].data(), S.names[r].size()) != 0 || out[at + S.names[r].size()] != 0)
            return fail("a name differs, name", r);
        at += S.names[r].size() + 1;
    }
    uint64_t c = 0;
    for (uint32_t r = 0; r < n; r++) {
        const uint32_t n_bin = (uint32_t)rd(out, at, 4);
        at += 4;
        if (n_bin != 4) return fail("three bins and the pseudo-bin expected, name", r);
        for (uint32_t b = 0; b < n_bin; b++) {
            const uint32_t bin = (uint32_t)rd(out, at, 4), n_c = (uint32_t)rd(out, at + 4, 4);
            at += 8;
            if (b == 3) {
                if (bin != ih::PSEUDO_BIN || n_c != 2 || rd(out, at, 8) != S.ref_beg[r] || rd(out, at + 8, 8) != S.ref_end[r] || rd(out, at + 16, 8) != S.mapped[r] ||
                    rd(out, at + 24, 8) != 0)
                    return fail("the pseudo-bin differs, name", r);
                at += 32;
                continue;
            }
            if (n_c != b + 1 || bin != (uint32_t)S.key[c]) return fail("a bin differs, name", r);
            for (uint32_t k = 0; k < n_c; k++, c++, at += 16)
                if (rd(out, at, 8) != S.beg[c] || rd(out, at + 8, 8) != S.end[c]) return fail("a chunk differs, chunk", c);
        }
        const uint32_t n_intv = (uint32_t)rd(out, at, 4);
        at += 4;
        if (n_intv != S.n_intv[r]) return fail("n_intv differs, name", r);
        for (uint32_t w = 0; w < n_intv; w++, at += 8)
            if (rd(out, at, 8) != S.lin[S.lin_off[r] + w]) return fail("a window differs, name", r);
    }
    if (at + 8 != out.size() || rd(out, at, 8) != 0) return fail("the file does not end behind n_no_coor = 0, prefix", n);
    return 0;
}

static int refusals(const Set &S) {
    const uint32_t n = (uint32_t)S.names.size();
    std::vector<uint8_t> names, out(3, 7);
    std::vector<uint64_t> off(1, 0);
    for (const std::string &s : S.names) {
        names.insert(names.end(), s.begin(), s.end());
        off.push_back(names.size());
    }
    ih::Tables T;
    T.n_ref = n;
    T.n_chunk = S.key.size();
    std::vector<uint64_t> key = S.key;
    T.chunk_key = key.data();
    T.chunk_beg = S.beg.data();
    T.chunk_end = S.end.data();
    T.n_intv = S.n_intv.data();
    T.lin_off = S.lin_off.data();
    T.lin = S.lin.data();
    T.ref_beg = S.ref_beg.data();
    T.ref_end = S.ref_end.data();
    T.mapped = S.mapped.data();
    T.unmapped = S.unmapped.data();
    th::Head H;
    char msg[200];
    // one chunk key altered: refused with words and no bytes, or still a file
    for (size_t i = 0; i < key.size(); i++)
        for (uint64_t k : {(uint64_t)(key[i] ^ 1u), (uint64_t)(key[i] + (1ull << 32)), (uint64_t)(key[i] | 0xFFFFu), (uint64_t)n << 32, (uint64_t)0}) {
            const uint64_t keep = key[i];
            key[i] = k;
            msg[0] = 0;
            const int rc = th::serialise(T, H, names.data(), off.data(), &out, msg, sizeof msg);
            if (rc != th::OK && (!msg[0] || !out.empty())) return fail("a refusal without its words, or with bytes, at chunk", i);
            if (rc == th::OK && (out.size() < 44 || memcmp(out.data(), "TBI\1", 4) != 0)) return fail("an answer that is no file, at chunk", i);
            key[i] = keep;
        }
    // an empty name, name offsets that decrease, null tables
    std::vector<uint64_t> bad = off;
    bad[2] = bad[1];
    if (th::serialise(T, H, names.data(), bad.data(), &out, msg, sizeof msg) != th::ERR_ARG || !out.empty()) return fail("an empty name was taken", 0);
    bad[2] = bad[1] - 1;
    if (th::serialise(T, H, names.data(), bad.data(), &out, msg, sizeof msg) != th::ERR_ARG) return fail("decreasing name offsets were taken", 0);
    if (th::serialise(T, H, nullptr, off.data(), &out, msg, sizeof msg) != th::ERR_ARG || th::serialise(T, H, names.data(), nullptr, &out, msg, sizeof msg) != th::ERR_ARG ||
        th::serialise(T, H, names.data(), off.data(), nullptr, msg, sizeof msg) != th::ERR_ARG)
        return fail("a null argument was taken", 0);
    // l_nm at its limit: the offsets say so, no byte of such a name is read before the refusal
    std::vector<uint64_t> big = off;
    for (size_t i = 1; i < big.size(); i++) big[i] = off[i] + ((1ull << 31) - names.size() - n);      // l_nm == 2^31 exactly
    if (th::serialise(T, H, names.data(), big.data(), &out, msg, sizeof msg) != th::ERR_LIMIT || !out.empty() || !msg[0]) return fail("l_nm of 2^31 was taken", 0);
    ih::Tables M = T;
    M.n_ref = (uint32_t)th::MAX_NAMES + 1;
    if (th::serialise(M, H, names.data(), off.data(), &out, msg, sizeof msg) != th::ERR_LIMIT) return fail("2^24 + 1 names were taken", 0);
    return 0;
}

static int repeats() {
    // a name list with one name put back at every place behind its first: found at that index, whatever stands around it
    const std::vector<std::string> base = {"chr1", "chr10", "chr", "c", "chr1x", "x", "chr2", std::string(300, 'n'), std::string(300, 'n') + "1"};
    for (size_t first = 0; first < base.size(); first++)
        for (size_t back = first + 1; back <= base.size(); back++) {
            std::vector<std::string> v = base;
            v.insert(v.begin() + back, base[first]);
            if (back + 2 <= v.size()) v.push_back(v[1]);  // a later repeat, behind `back`: it must not win
            std::vector<uint8_t> names;
            std::vector<uint64_t> off(1, 0);
            for (const std::string &s : v) {
                names.insert(names.end(), s.begin(), s.end());
                off.push_back(names.size());
            }
            const Exact<uint8_t> x_names(names);
            const Exact<uint64_t> x_off(off);
            const uint64_t want = back, got = th::first_repeat(x_names.p, x_off.p, v.size());
            if (got != want) return fail("the name that came back was found elsewhere than at", back);
            for (uint64_t k = 0; k <= back; k++)
                if (th::first_repeat(x_names.p, x_off.p, k) != k) return fail("a prefix of distinct names has a repeat, prefix", k);
        }
    if (th::first_repeat(nullptr, nullptr, 0) != 0) return fail("no names, and a repeat", 0);
    return 0;
}

int main() {
    const Set S = build({"ctg_a", "b", std::string(70000, 'L'), "chr1", "chr10", "chr1 "});
    th::Head vcf, bed;
    vcf.format = 2, vcf.col_seq = 1, vcf.col_beg = 2, vcf.col_end = 0;
    bed.format = 0x10000, bed.col_seq = 1, bed.col_beg = 2, bed.col_end = 3;
    for (uint32_t n = 0; n <= S.names.size(); n++)
        if (round_trip(S, n, vcf) || round_trip(S, n, bed)) return 1;
    if (refusals(S) || repeats()) return 1;
    printf("tabix_host_check: %zu prefixes of a table set in both presets, the refusals and the name list's repeats: OK\n", S.names.size() + 1);
    return 0;
}
