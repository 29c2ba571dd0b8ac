// pp_crc.h -- CRC32 (reflected, P = 0xEDB88320) on the device and the combination of the CRCs of adjacent byte ranges, after zlib's
// crc32_combine: crc(A B) = crc(A) x^(8 |B|) + crc(B) mod P.  Shared by the BGZF reader (pp_bgzf.hip: k_bgzf_crc checks a block's
// footer, one wave per block) and the BGZF writer (pp_bam_out.hip: k_tag_frame makes the footer, one workgroup per block).  Both run
// the byte-table CRC per lane over the lane's own bytes (table in LDS, crc_table_fill) and combine the lanes' values pairwise.
#pragma once
#include "pp_dev.h"

namespace {

constexpr u32 CRC_POLY = 0xEDB88320u;
__host__ __device__ constexpr u32 multmodp(u32 a, u32 b) {  // a(x) * b(x) mod P; bit 31 is x^0
    u32 m = 1u << 31, p = 0;
    for (int i = 0; i < 32; i++) {
        if (a & m) {
            p ^= b;
            if ((a & (m - 1)) == 0) break;
        }
        m >>= 1;
        b = (b & 1u) ? (b >> 1) ^ CRC_POLY : b >> 1;
    }
    return p;
}
struct X2N {
    u32 v[32];  // x^(2^k) mod P
    constexpr X2N() : v{} {
        u32 p = 1u << 30;  // x^1
        v[0] = p;
        for (int n = 1; n < 32; n++) v[n] = p = multmodp(p, p);
    }
};
__constant__ X2N X2N_TAB = X2N();
__device__ u32 x8n_modp(u32 n) {  // x^(8 n) mod P
    u32 p = 1u << 31, k = 3;
    while (n) {
        if (n & 1u) p = multmodp(X2N_TAB.v[k & 31u], p);
        n >>= 1;
        k++;
    }
    return p;
}

// x^(8 n 2^k) mod P for k = 0 .. K-1, made by the compiler: the multipliers of a combination tree over ranges of n bytes each
template <u32 N_BYTES, u32 K>
struct X8N2K {
    u32 v[K];
    constexpr X8N2K() : v{} {
        u32 p = 1u << 31, sq = X2N().v[3], n = N_BYTES;  // x^0, x^8
        while (n) {
            if (n & 1u) p = multmodp(sq, p);
            sq = multmodp(sq, sq);
            n >>= 1;
        }
        v[0] = p;
        for (u32 k = 1; k < K; k++) v[k] = p = multmodp(p, p);
    }
};

// the byte table into 256 words of LDS, by the first 256 threads of `n_threads` (a barrier follows at the caller's)
__device__ __forceinline__ void crc_table_fill(u32 *s_tab, u32 thread, u32 n_threads) {
    for (u32 i = thread; i < 256u; i += n_threads) {
        u32 c = i;
        for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ CRC_POLY : c >> 1;
        s_tab[i] = c;
    }
}
__device__ __forceinline__ u32 crc_byte(const u32 *s_tab, u32 c, u32 byte) { return s_tab[(c ^ byte) & 0xFFu] ^ (c >> 8); }
// the four bytes of a word, low byte first
__device__ __forceinline__ u32 crc_word(const u32 *s_tab, u32 c, u32 w) {
#pragma unroll
    for (u32 j = 0; j < 4u; j++) c = crc_byte(s_tab, c, w >> (8u * j));
    return c;
}

}  // namespace
