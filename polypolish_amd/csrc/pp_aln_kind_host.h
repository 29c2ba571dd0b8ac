// pp_aln_kind_host.h -- what an alignment file holds, told by its head: the walk behind pp_aln_file_kind and pp_aln_file_kind_text
// (pp_bam_files.cpp), over a source of bytes instead of a file descriptor so that tools/text_chain_host_check.cpp can run it under a
// sanitizer on heap blocks of exactly a file's length.  Host code, zlib for the first inflated bytes, nothing of the library.
#pragma once
#include <zlib.h>

#include <algorithm>
#include <cstdint>
#include <cstring>

namespace pp_aln_host {

enum Kind { SAM = 0, BAM = 1, BAM_RAW = 2, SAM_BGZF = 3 };              // = PP_ALN_* (include/polypolish_hip.h)
enum Answer { OK = 0, UNABLE = 1, NOT_BGZF = 2, NOT_BAM = 3, CUT = 4 };  // the refusals, as pp_aln_file_kind words them
constexpr size_t WINDOW = 65536;                                         // a BGZF block is at most 64 KiB

inline uint32_t le16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }

// src.at(off, &n): up to WINDOW bytes of the file from `off` -- a pointer to n valid bytes (n == 0 at or behind the end), or nullptr
// when the file cannot be read.  with_text: BGZF whose inflated head is not BAM\1 is SAM_BGZF, not the refusal NOT_BAM.
template <class Src>
int kind_of(Src &src, int *kind, bool with_text) {
    *kind = SAM;
    size_t n = 0;
    const uint8_t *h = src.at(0, &n);
    if (!h) return UNABLE;
    if (n >= 4 && memcmp(h, "BAM\1", 4) == 0) {
        *kind = BAM_RAW;
        return OK;
    }
    if (n < 2 || h[0] != 0x1f || h[1] != 0x8b) return OK;
    // a gzip member: BGZF, if it has the BC subfield; the first four inflated bytes say whether it is BAM.  (The header is read here
    // and not by pp_bgzf_host::block: that one wants the whole block inside the bytes, and a file cut inside its first block is still
    // told by its head -- the inflate then names the truncation.)
    uint8_t got[4] = {0, 0, 0, 0};
    unsigned n_got = 0;
    bool defect = false;  // something pp_bgzf_inflate will name: the block is not looked into here
    uint64_t at = 0;
    for (int b = 0; n_got < 4 && b < 64; b++) {
        if (b) {
            h = src.at(at, &n);
            if (!h) return UNABLE;
            if (n == 0) break;
        }
        const bool first = b == 0;
        if (n < 10) { if (first) return CUT; defect = true; break; }
        if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || !(h[3] & 4)) { if (first) return NOT_BGZF; defect = true; break; }
        if (n < 12) { if (first) return CUT; defect = true; break; }
        const uint32_t xlen = le16(h + 10);
        if ((uint64_t)n - 12 < xlen) { if (first) return CUT; defect = true; break; }
        uint32_t p = 0, bsize = 0;
        bool found = false, malformed = false;
        while (xlen - p >= 4) {  // SI1 SI2 SLEN data, as pp_bgzf_walk goes through them
            const uint32_t slen = le16(h + 12 + p + 2);
            if (slen > xlen - p - 4) { malformed = true; break; }
            if (!found && h[12 + p] == 'B' && h[12 + p + 1] == 'C' && slen == 2) {
                bsize = le16(h + 12 + p + 4);
                found = true;
            }
            p += 4 + slen;
        }
        if (malformed || p != xlen || !found) { if (first) return NOT_BGZF; defect = true; break; }
        const uint32_t total = bsize + 1, head = 12 + xlen;
        if (total < head + 8) { defect = true; break; }
        const uint32_t avail = (uint32_t)std::min<uint64_t>((uint64_t)n, total - 8) - head;  // payload bytes at hand (head <= n)
        z_stream zs;
        memset(&zs, 0, sizeof zs);
        if (inflateInit2(&zs, -15) != Z_OK) return UNABLE;
        zs.next_in = (Bytef *)(h + head);
        zs.avail_in = avail;
        zs.next_out = got + n_got;
        zs.avail_out = 4 - n_got;
        const int r = inflate(&zs, Z_SYNC_FLUSH);
        n_got = 4 - zs.avail_out;
        inflateEnd(&zs);
        if (r != Z_OK && r != Z_STREAM_END && r != Z_BUF_ERROR) { defect = true; break; }
        if ((uint64_t)n < total) { defect = true; break; }  // the file ends inside this block
        at += total;
    }
    if (memcmp(got, "BAM\1", n_got) != 0 || (n_got < 4 && !defect)) {  // (or fewer than four bytes of content)
        if (!with_text) return NOT_BAM;
        *kind = SAM_BGZF;
        return OK;
    }
    *kind = BAM;
    return OK;
}

// a source over bytes in memory: the window is the bytes themselves, so a load behind them is a load behind their allocation
struct Bytes {
    const uint8_t *p;
    uint64_t n;
    const uint8_t *at(uint64_t off, size_t *got) const {
        static const uint8_t none = 0;
        *got = off < n ? (size_t)std::min<uint64_t>(WINDOW, n - off) : 0;
        return *got ? p + off : &none;
    }
};

}  // namespace pp_aln_host
