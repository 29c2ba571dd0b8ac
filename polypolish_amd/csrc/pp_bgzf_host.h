// pp_bgzf_host.h -- the header of one BGZF block and the host walk over a file's blocks behind pp_bgzf_walk (pp_bgzf.hip): plain C++
// with no HIP in it, so that a stand-alone program can run the walk under a sanitizer (tools/bgzf_host_check.cpp).  block() is also
// what the device runs per block before anything is read through a block's offset (k_bgzf_head): one definition for both sides.
// Nothing here reads a byte outside [0, n_bytes) or forms a sum that could wrap: every length is compared with what is LEFT.
// The WRITING twin: the constants and bytes of a block around one stored DEFLATE block, which pp_bam_tagged frames its output with
// on the device (pp_bam_out.hip takes the head's and the EOF block's bytes from here), and store_block(), the same block in plain C++.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>

#if defined(__HIPCC__)
#define PP_BGZF_HD __host__ __device__
#else
#define PP_BGZF_HD
#endif

namespace pp_bgzf_host {

constexpr int OK = 0, ERR_ARG = 4;  // PP_OK, PP_ERR_ARG
constexpr uint32_t MAX_ISIZE = 65536;

// what is wrong with a block's header, in the order it is looked for
enum : uint32_t { H_OK = 0, H_RANGE = 1, H_MAGIC = 2, H_EXTRA = 3, H_NO_BC = 4, H_BSIZE = 5, H_PAST = 6, H_ISIZE = 7 };

struct Block {
    uint32_t total;    // BSIZE + 1: the whole block
    uint32_t payload;  // offset of the DEFLATE stream inside the block (12 + XLEN)
    uint32_t pay_len;  // its length: total - payload - 8
    uint32_t isize;    // the footer's ISIZE
};

PP_BGZF_HD inline uint32_t le16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
PP_BGZF_HD inline uint32_t le32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// the block at `at`: 1f 8b 08, FLG with FEXTRA, XLEN, the BC subfield (SLEN 2) among the extra subfields, BSIZE, the footer's ISIZE
PP_BGZF_HD inline uint32_t block(const uint8_t *bytes, uint64_t n_bytes, uint64_t at, Block *out) {
    if (at > n_bytes || n_bytes - at < 12) return H_RANGE;
    const uint8_t *h = bytes + at;
    const uint64_t left = n_bytes - at;
    if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || !(h[3] & 4)) return H_MAGIC;
    const uint32_t xlen = le16(h + 10);
    if ((uint64_t)xlen > left - 12) return H_EXTRA;
    uint32_t p = 0, bsize = 0;
    bool found = false;
    while (xlen - p >= 4) {  // SI1 SI2 SLEN data
        const uint32_t slen = le16(h + 12 + p + 2);
        if (slen > xlen - p - 4) return H_EXTRA;
        if (!found && h[12 + p] == 'B' && h[12 + p + 1] == 'C' && slen == 2) {
            bsize = le16(h + 12 + p + 4);
            found = true;
        }
        p += 4 + slen;
    }
    if (p != xlen) return H_EXTRA;
    if (!found) return H_NO_BC;
    const uint32_t total = bsize + 1;
    if (total < 12 + xlen + 8) return H_BSIZE;
    if ((uint64_t)total > left) return H_PAST;
    const uint32_t isize = le32(h + total - 4);
    if (isize > MAX_ISIZE) return H_ISIZE;
    out->total = total;
    out->payload = 12 + xlen;
    out->pay_len = total - 12 - xlen - 8;
    out->isize = isize;
    return H_OK;
}

// ---- writing: one BGZF block around one STORED DEFLATE block (level 0), what pp_bam_tagged frames its output with (pp_bam_out.hip) ----
// 1f 8b 08 04 | MTIME 0 | XFL 0 | OS ff | XLEN 6 | B C 2 0 BSIZE | 01 LEN ~LEN | the bytes | CRC32 | ISIZE: len + 31 bytes, BSIZE = len + 30
constexpr uint32_t STORE_PAYLOAD = 0xff00;  // htslib's payload size: the output is cut every 65,280 bytes
constexpr uint32_t STORE_HEAD = 23;         // the 18 bytes of the header and 01 LEN ~LEN
constexpr uint32_t STORE_EXTRA = 31;        // ... and CRC32, ISIZE behind the bytes
constexpr uint32_t STORE_BLOCK = STORE_PAYLOAD + STORE_EXTRA;  // block b of a file starts at b * 65,311
constexpr uint32_t EOF_SIZE = 28;

// byte j < 18 of a block's header, total = the whole block's bytes
PP_BGZF_HD inline uint8_t head_byte(uint32_t j, uint32_t total) {
    if (j < 8) return (uint8_t)(0x0000000004088b1full >> (8 * j));
    if (j < 16) return (uint8_t)(0x000243420006ff00ull >> (8 * (j - 8)));
    return (uint8_t)((total - 1) >> (8 * (j - 16)));
}
// byte j < STORE_HEAD of the block that stores `len` bytes
PP_BGZF_HD inline uint8_t store_head_byte(uint32_t j, uint32_t len) {
    if (j < 18) return head_byte(j, len + STORE_EXTRA);
    if (j == 18) return 1;  // BFINAL, BTYPE 0
    const uint32_t w = j < 21 ? len : ~len;
    return (uint8_t)(w >> (8 * ((j - 19) & 1)));
}
// byte j < EOF_SIZE of the empty block that ends a file: the header, an empty fixed-code block (03 00), CRC32 0, ISIZE 0
PP_BGZF_HD inline uint8_t eof_byte(uint32_t j) { return j < 18 ? head_byte(j, EOF_SIZE) : (j == 18 ? 3 : 0); }

inline uint32_t crc32_bitwise(const uint8_t *data, uint32_t len) {
    uint32_t c = 0xFFFFFFFFu;
    for (uint32_t i = 0; i < len; i++) {
        c ^= data[i];
        for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
    }
    return ~c;
}

// the block that stores data[0, len), len <= STORE_PAYLOAD, into out[0, len + STORE_EXTRA); returns its size
inline uint32_t store_block(const uint8_t *data, uint32_t len, uint8_t *out) {
    for (uint32_t j = 0; j < STORE_HEAD; j++) out[j] = store_head_byte(j, len);
    if (len) memcpy(out + STORE_HEAD, data, len);
    const uint32_t foot[2] = {crc32_bitwise(data, len), len};
    for (uint32_t j = 0; j < 8; j++) out[STORE_HEAD + len + j] = (uint8_t)(foot[j >> 2] >> (8 * (j & 3)));
    return len + STORE_EXTRA;
}

inline const char *defect_text(uint32_t code) {
    switch (code) {
    case H_RANGE: return "does not lie inside the bytes (12 bytes of header)";
    case H_MAGIC: return "does not start with 1f 8b 08 and a FLG with FEXTRA";
    case H_EXTRA: return "has extra subfields that do not fit its XLEN, or an XLEN that runs past the bytes";
    case H_NO_BC: return "has no BC subfield of SLEN 2";
    case H_BSIZE: return "has a BSIZE below its header and footer";
    case H_PAST: return "runs past the end of the bytes";
    default: return "has an ISIZE above 65536";
    }
}

inline int fail(char *msg, size_t msg_cap, const char *fmt, unsigned long long a = 0, unsigned long long b = 0, const char *s = "") {
    if (msg && msg_cap) snprintf(msg, msg_cap, fmt, a, b, s);
    return ERR_ARG;
}

// the BSIZE chain from `from`: stops at n_bytes, or after `cap` blocks when there is an array to fill.  blk_off has cap entries,
// out_off (may be NULL) cap + 1: out_off[b] = the ISIZEs in front of block b, and one more entry behind the last block written.
inline int walk(const uint8_t *bytes, uint64_t n_bytes, uint64_t from, uint64_t *blk_off, uint64_t *out_off, uint64_t cap, uint64_t *n_blk,
                uint64_t *end, char *msg, size_t msg_cap) {
    if (n_blk) *n_blk = 0;
    if (end) *end = from;
    if (!n_blk || !end || (n_bytes && !bytes)) return fail(msg, msg_cap, "pp_bgzf_walk: null argument");
    if (from > n_bytes) return fail(msg, msg_cap, "pp_bgzf_walk: the start %llu lies behind the %llu bytes", from, n_bytes);
    const bool fill = blk_off && cap;
    uint64_t at = from, n = 0, sum = 0;
    int rc = OK;
    while (at < n_bytes && !(fill && n == cap)) {
        Block b;
        const uint32_t code = block(bytes, n_bytes, at, &b);
        if (code) {
            rc = fail(msg, msg_cap, "pp_bgzf_walk: block %llu (offset %llu) %s", n, at, defect_text(code));
            break;
        }
        if (fill) {
            blk_off[n] = at;
            if (out_off) out_off[n] = sum;
        }
        sum += b.isize;
        n++;
        at += b.total;
    }
    if (fill && out_off) out_off[n] = sum;
    *n_blk = n;
    *end = at;
    return rc;
}

}  // namespace pp_bgzf_host
