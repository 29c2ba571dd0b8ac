// pp_textin.h -- device-side utilities for a text that is BORROWED: not padded, at any alignment, possibly ending where its allocation
// ends (pp_sam_out.hip: pp_sam_tagged; pp_sam_bam.hip: pp_sam_bam; pp_tabix.hip: pp_tabix_index).  pp_devtext.h's kernels read a padded copy; everything here checks
// every load against the text's size, a wide load too: no byte outside [0, size) is loaded.  Anonymous namespace, as pp_dev.h.
#pragma once
#include "pp_dev.h"

namespace {

constexpr u32 IN_NL_BLOCK = 1024 * 64;  // bytes of text per workgroup of the newline kernels (64 per thread), as pp_devtext.h's

__device__ __forceinline__ u32 nl_mask(u32 w) {  // bit 7 of every byte that is '\n'
    const u32 x = w ^ 0x0A0A0A0Au;
    return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;
}

// ---- the newline index of a borrowed text ------------------------------------------------------------------------------------------
// the 64 bytes from `base` as sixteen words; those behind the text's end are zeros
__device__ __forceinline__ void load64_in(const u8 *__restrict__ T, u64 size, u64 base, u32 w[16]) {
    if (base < size && size - base >= 64u) {
        uint4 q[4];
        __builtin_memcpy(q, T + base, 64);  // (any alignment: four global_load_dwordx4)
#pragma unroll
        for (int v = 0; v < 4; v++) { w[4 * v] = q[v].x; w[4 * v + 1] = q[v].y; w[4 * v + 2] = q[v].z; w[4 * v + 3] = q[v].w; }
        return;
    }
    const u32 left = base < size ? (u32)(size - base) : 0u;
#pragma unroll
    for (u32 i = 0; i < 16u; i++) {
        u32 x = 0;
#pragma unroll
        for (u32 b = 0; b < 4u; b++)
            if (4u * i + b < left) x |= (u32)T[base + 4u * i + b] << (8u * b);
        w[i] = x;
    }
}

// ASCII: blk_cnt[gridDim.x] (zeroed by the caller) is set when a byte >= 0x80 shows up anywhere
template <bool ASCII>
__global__ __launch_bounds__(1024) void k_in_nl_count(const u8 *__restrict__ text, u64 size, u32 *__restrict__ blk_cnt) {
    __shared__ u32 s_sum;
    if (threadIdx.x == 0) s_sum = 0;
    __syncthreads();
    u32 w[16], v = 0;
    load64_in(text, size, (u64)blockIdx.x * IN_NL_BLOCK + (u64)threadIdx.x * 64u, w);
    if (ASCII) {
        u32 high = 0;
#pragma unroll
        for (u32 i = 0; i < 16u; i++) high |= w[i];
        if (__ballot((high & 0x80808080u) != 0) && (threadIdx.x & 63u) == 0) atomicOr(&blk_cnt[gridDim.x], 1u);
    }
#pragma unroll
    for (u32 i = 0; i < 16u; i++) v += (u32)__popc(nl_mask(w[i]));
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63u) == 0 && v) atomicAdd(&s_sum, v);
    __syncthreads();
    if (threadIdx.x == 0) blk_cnt[blockIdx.x] = s_sum;
}

__global__ __launch_bounds__(1024) void k_in_nl_write(const u8 *__restrict__ text, u64 size, const u64 *__restrict__ blk_off,
                                                      u64 *__restrict__ nl_pos) {
    __shared__ u32 s_w[16];
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const u64 base = (u64)blockIdx.x * IN_NL_BLOCK + (u64)threadIdx.x * 64u;
    u32 w[16], n = 0;
    load64_in(text, size, base, w);
#pragma unroll
    for (u32 i = 0; i < 16u; i++) n += (u32)__popc(nl_mask(w[i]));
    const u32 inc = pp::wave_scan_incl(n);
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    u32 before = inc - n;
    for (u32 i = 0; i < wave; i++) before += s_w[i];
    if (!n) return;
    u64 out = blk_off[blockIdx.x] + before;
#pragma unroll
    for (u32 i = 0; i < 16u; i++) {
        u32 m = nl_mask(w[i]);
        while (m) {
            const u32 b = ((u32)__ffs((int)m) - 1u) >> 3;
            m &= m - 1u;
            nl_pos[out++] = base + 4u * i + b;
        }
    }
}

// the first '\t' in text[from, end), or end: eight bytes per step where eight lie inside the text (end <= size)
__device__ __forceinline__ u64 find_tab_in(const u8 *__restrict__ T, u64 size, u64 from, u64 end) {
    u64 i = from;
    while (i < end) {
        if (size - i >= 8u) {
            u64 w;
            __builtin_memcpy(&w, T + i, 8);
            const u64 x = w ^ 0x0909090909090909ull;
            const u64 m = (x - 0x0101010101010101ull) & ~x & 0x8080808080808080ull;  // bit 7 of the zero bytes (first one exact)
            if (m) return min(end, i + ((u32)__ffsll((long long)m) - 1u) / 8u);
            i += 8;
        } else {
            if (T[i] == (u8)'\t') return i;
            i++;
        }
    }
    return end;
}

// sixteen bytes of the text from `at`, of which `need` >= 1 are wanted and lie inside it; the text's last bytes byte by byte
__device__ __forceinline__ void load16_in(const u8 *__restrict__ T, u64 size, u64 at, u32 need, u64 *lo, u64 *hi) {
    if (size - at >= 16u) {
        u64 v[2];
        __builtin_memcpy(v, T + at, 16);  // (any alignment: one global_load_dwordx4)
        *lo = v[0];
        *hi = v[1];
    } else {
        u64 a = 0, b = 0;
        for (u32 j = 0; j < need; j++) {
            if (j < 8u) a |= (u64)T[at + j] << (8u * j); else b |= (u64)T[at + j] << (8u * (j - 8u));
        }
        *lo = a;
        *hi = b;
    }
}

// a workgroup's exclusive prefix of 64-bit values (a line may be longer than 4 GB), *total its sum
template <u32 BLOCK>
__device__ __forceinline__ u64 block_scan_excl_u64(u64 v, u64 *s_w, u64 *total) {
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    u64 inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const u64 t = __shfl_up(inc, o, 64);
        if ((int)lane >= o) inc += t;
    }
    if (lane == 63u) s_w[wave] = inc;
    __syncthreads();
    u64 before = 0, sum = 0;
#pragma unroll
    for (u32 i = 0; i < BLOCK / 64u; i++) {
        const u64 w = s_w[i];
        before += i < wave ? w : 0ull;
        sum += w;
    }
    __syncthreads();  // (s_w is used again)
    *total = sum;
    return before + inc - v;
}

}  // namespace
