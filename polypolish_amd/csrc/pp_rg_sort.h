// pp_rg_sort.h -- the stable radix sort of indices that pp_batch_regroup (pp_regroup.hip: 32-bit keys, the first record of a read) and
// pp_bam_sort (pp_bam_sort.hip: 64-bit keys, the coordinate of a record) share, and the aligned-rank map that carries the filter's
// verdicts over a permutation of the records (pp_regrouped_pass, pp_bam_sorted_pass).
//   k_rg_hist      a least-significant-digit pass over 8 bits of the key.  Every tile of RG_TILE keys counts its 256 digits (LDS); the
//   k_rg_scatter   counts, laid out digit by digit and inside a digit tile by tile, are scanned (scan_u32) into the place of every
//                  (digit, tile)'s first key; the scatter ranks a key among the equal digits of its tile WITHOUT atomics -- lanes
//                  below it in its wave's round (64-bit ballots, one per digit bit), the wave's earlier rounds, the tile's earlier
//                  waves (their counts through LDS) -- so that a pass is stable and the order never depends on how atomics land.  The
//                  cost is linear in the number of keys whatever their values.  K = u32 or u64: the key's word
//   k_rg_aligned   !(flag & 4) of the records in index order and behind a permutation; their scans give k_rg_map: aligned rank behind
//   k_rg_map       the permutation -> aligned rank in front of it
#pragma once
#include "pp_dev.h"

namespace {

constexpr u32 RG_BLOCK = 1024;                    // 16 waves ...
constexpr u32 RG_ROUNDS = 4;                      // ... each takes 4 x 64 adjacent keys: round by round, lane by lane
constexpr u32 RG_TILE = RG_BLOCK * RG_ROUNDS;     // keys per workgroup
constexpr u32 RG_WAVES = RG_BLOCK / 64u;

// the place of the key that lane `lane` of wave `wave` takes in round `j` of its tile
__device__ __forceinline__ u64 rg_index(u32 wave, u32 j, u32 lane) {
    return (u64)blockIdx.x * RG_TILE + wave * (64u * RG_ROUNDS) + j * 64u + lane;
}

__global__ __launch_bounds__(256) void k_rg_iota(u32 n, u32 *__restrict__ perm) {
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    if (i < n) perm[i] = (u32)i;
}

// cnt[digit * n_tiles + tile] = the tile's keys with that digit
template <class K>
__global__ __launch_bounds__(RG_BLOCK) void k_rg_hist(u32 n, const K *__restrict__ key, u32 shift, u32 n_tiles, u32 *__restrict__ cnt) {
    __shared__ u32 s_h[256];
    if (threadIdx.x < 256u) s_h[threadIdx.x] = 0;
    __syncthreads();
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (u32 j = 0; j < RG_ROUNDS; j++) {
        const u64 i = rg_index(wave, j, lane);
        if (i < n) atomicAdd(&s_h[(u32)(key[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 256u) cnt[(u64)threadIdx.x * n_tiles + blockIdx.x] = s_h[threadIdx.x];
}

// off[digit * n_tiles + tile] = where the tile's first key with that digit goes.  idx_in == nullptr: the keys stand in index order
// (the first pass).
template <class K>
__global__ __launch_bounds__(RG_BLOCK) void k_rg_scatter(u32 n, const K *__restrict__ key_in, const u32 *__restrict__ idx_in, u32 shift,
                                                         u32 n_tiles, const u32 *__restrict__ off, K *__restrict__ key_out,
                                                         u32 *__restrict__ idx_out) {
    __shared__ u32 s_c[RG_WAVES][256];  // keys of wave w with digit d so far; then the place of the wave's first such key
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (u32 t = threadIdx.x; t < RG_WAVES * 256u; t += RG_BLOCK) (&s_c[0][0])[t] = 0;
    __syncthreads();
    const u64 below = (1ull << lane) - 1ull;
    K key[RG_ROUNDS];
    u32 at[RG_ROUNDS];  // at: the key's rank among its wave's keys with its digit
    bool live[RG_ROUNDS];
#pragma unroll
    for (u32 j = 0; j < RG_ROUNDS; j++) {
        const u64 i = rg_index(wave, j, lane);
        live[j] = i < n;
        key[j] = live[j] ? key_in[i] : (K)0;
        const u32 d = (u32)(key[j] >> shift) & 255u;
        u64 peers = __ballot(live[j]);  // the round's live lanes with this lane's digit
#pragma unroll
        for (u32 b = 0; b < 8; b++) {
            const u64 m = __ballot((d >> b) & 1u);
            peers &= ((d >> b) & 1u) ? m : ~m;
        }
        // every lane reads the wave's count, then the digit's first lane adds the round's: a barrier between the two and behind
        // them (all waves make all rounds), so that neither the hardware nor the compiler may take one for the other
        at[j] = s_c[wave][d] + (u32)__popcll(peers & below);
        __syncthreads();
        if (live[j] && (peers & below) == 0) s_c[wave][d] += (u32)__popcll(peers);
        __syncthreads();
    }
    if (threadIdx.x < 256u) {  // a digit each: the waves in order, on top of the tile's place
        u32 run = off[(u64)threadIdx.x * n_tiles + blockIdx.x];
#pragma unroll
        for (u32 w = 0; w < RG_WAVES; w++) {
            const u32 c = s_c[w][threadIdx.x];
            s_c[w][threadIdx.x] = run;
            run += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (u32 j = 0; j < RG_ROUNDS; j++) {
        if (!live[j]) continue;
        const u64 i = rg_index(wave, j, lane);
        const u32 to = s_c[wave][(u32)(key[j] >> shift) & 255u] + at[j];
        if (to < n) {  // (it is: the places come from the counts of these very keys)
            key_out[to] = key[j];
            idx_out[to] = idx_in ? idx_in[i] : (u32)i;
        }
    }
}

// perm == nullptr: the records' own order
__global__ __launch_bounds__(256) void k_rg_aligned(u32 n, const uint16_t *__restrict__ flag, const u32 *__restrict__ perm, u32 *__restrict__ is_aln) {
    const u64 j = (u64)blockIdx.x * 256u + threadIdx.x;
    if (j < n) is_aln[j] = (flag[perm ? perm[j] : (u32)j] & 4u) ? 0u : 1u;
}

__global__ __launch_bounds__(256) void k_rg_map(u32 n, const uint16_t *__restrict__ flag, const u32 *__restrict__ perm, const u32 *__restrict__ rank_raw,
                                                const u32 *__restrict__ rank_new, u32 *__restrict__ amap) {
    const u64 j = (u64)blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    const u32 p = perm[j];
    if (!(flag[p] & 4u)) amap[rank_new[j]] = rank_raw[p];
}

}  // namespace
