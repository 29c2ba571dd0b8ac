// pp_cut16.h -- 16 bytes of a source at any alignment for the kernels that cut their OUTPUT into aligned 16-byte stores: k_fasta_text
// (pp_fasta_out.hip) and k_vcf_text (pp_k_vcf.h, pp_polish_text.hip).  The run is taken from the one or two 16-byte pieces of ADDRESS
// that hold it, each with one wide load where the piece lies wholly inside the array, byte by byte behind the test otherwise:
// no byte outside [lo, hi) is loaded.  Device code only.
#pragma once
#include "pp_dev.h"

namespace {

// the 16 bytes at the 16-byte multiple of address q: one wide load where they all lie in [lo, hi), else those that do, one by one
__device__ __forceinline__ uint4 piece16(const u8 *q, const u8 *lo, const u8 *hi) {
    if ((uintptr_t)q >= (uintptr_t)lo && (uintptr_t)q + 16u <= (uintptr_t)hi) return *(const uint4 *)q;
    u32 w[4] = {0, 0, 0, 0};
#pragma unroll
    for (u32 j = 0; j < 16; j++) {
        const uintptr_t a = (uintptr_t)q + j;
        if (a >= (uintptr_t)lo && a < (uintptr_t)hi) w[j >> 2] |= (u32) * (const u8 *)a << (8 * (j & 3));
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// bytes [a, a + 16) of the 32 bytes (p0, p1), a in 0..15
__device__ __forceinline__ uint4 bytes_from(const uint4 p0, const uint4 p1, u32 a) {
    u32 x0, x1, x2, x3, x4;
    switch (a >> 2) {
    case 0: x0 = p0.x; x1 = p0.y; x2 = p0.z; x3 = p0.w; x4 = p1.x; break;
    case 1: x0 = p0.y; x1 = p0.z; x2 = p0.w; x3 = p1.x; x4 = p1.y; break;
    case 2: x0 = p0.z; x1 = p0.w; x2 = p1.x; x3 = p1.y; x4 = p1.z; break;
    default: x0 = p0.w; x1 = p1.x; x2 = p1.y; x3 = p1.z; x4 = p1.w; break;
    }
    const u32 s = a & 3u;
    return make_uint4(__builtin_amdgcn_alignbyte(x1, x0, s), __builtin_amdgcn_alignbyte(x2, x1, s), __builtin_amdgcn_alignbyte(x3, x2, s),
                      __builtin_amdgcn_alignbyte(x4, x3, s));
}

// 16 bytes from src (any alignment), all of them inside [lo, hi)
__device__ __forceinline__ uint4 copy16(const u8 *src, const u8 *lo, const u8 *hi) {
    const u32 a = (u32)((uintptr_t)src & 15u);
    const uint4 p0 = piece16(src - a, lo, hi);
    const uint4 p1 = a ? piece16(src - a + 16, lo, hi) : make_uint4(0, 0, 0, 0);
    return bytes_from(p0, p1, a);
}

}  // namespace
