// pp_k_index.h -- the table stage of a binning index, shared by pp_bam_index (pp_bam_out.hip: the .bai of a BAM file) and
// pp_tabix_index (pp_tabix.hip: the .tbi of a bgzipped text).  Both front ends hand over one row per record of the file, in file
// order -- {ref, pos, end} with ref < 0 for a record that stands on no reference -- its bin, a flag plane (bit 2: unmapped; all zero
// for text) and start[], the records' places in the uncompressed stream; the kernels here make the chunk table, the per-reference
// counts and spans and the linear index of them.  Moved function for function out of pp_bam_out.hip (profiles/index_move_isa.txt:
// instruction for instruction the same there).  Anonymous namespace, as pp_dev.h: each unit gets its own copies.
//   k_ix_run     a record starts a chunk where (ref, bin) changes; the scan of these flags numbers the chunks
//   k_ix_chunk   a chunk's key ref << 32 | bin, its first record's start and its last record's end
//   k_ix_ref     per reference: the windows it touches (atomicMax), its first record's start and last record's end, mapped and
//                unmapped records; the unplaced records
//   k_ix_lin     the window minima (64-bit atomicMin; a long record loops over its windows); k_ix_fill: the fill from the right
//   k_ix_gather  two 64-bit columns behind a permutation (the chunk table in the order k_rg_hist / k_rg_scatter of pp_rg_sort.h found)
#pragma once
#include "pp_bgzf_host.h"
#include "pp_dev.h"

namespace {

constexpr u32 IX_PAY = pp_bgzf_host::STORE_PAYLOAD;  // the uncompressed bytes of a BGZF block: the stream is cut every 65,280
constexpr u32 IX_MAX_END = 1u << 29;
constexpr u64 IX_MAX_WINDOWS = 1ull << 27;  // 1 GiB of linear index
constexpr u32 IX_MAX_REF = 1u << 24;

struct IxRec { int32_t ref, pos; u32 end; };

__device__ __forceinline__ u32 reg2bin(u32 beg, u32 end) {  // the SAM specification, section 5.3
    --end;
    if (beg >> 14 == end >> 14) return 4681u + (beg >> 14);
    if (beg >> 17 == end >> 17) return 585u + (beg >> 17);
    if (beg >> 20 == end >> 20) return 73u + (beg >> 20);
    if (beg >> 23 == end >> 23) return 9u + (beg >> 23);
    if (beg >> 26 == end >> 26) return 1u + (beg >> 26);
    return 0u;
}

__global__ __launch_bounds__(256) void k_ix_run(u32 n, const IxRec *__restrict__ rec, const u32 *__restrict__ bin, u32 *__restrict__ head) {
    const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
    if (r >= n) return;
    const int32_t ref = rec[r].ref;
    head[r] = (ref >= 0 && (r == 0 || rec[r - 1u].ref != ref || bin[r - 1u] != bin[r])) ? 1u : 0u;
}

struct IxWhere {  // where the records stand in the file
    const u64 *start;    // n + 2: start[r + 1] = record r's stream offset
    const u64 *blk_off;  // n_blk + 1
    __device__ __forceinline__ u64 at(u64 u) const { return blk_off[u / IX_PAY] << 16 | (u % IX_PAY); }
};

__global__ __launch_bounds__(256) void k_ix_chunk(u32 n, const IxRec *__restrict__ rec, const u32 *__restrict__ bin, const u32 *__restrict__ head,
                                                  const u32 *__restrict__ cidx, IxWhere W, u64 *__restrict__ key, u64 *__restrict__ beg, u64 *__restrict__ end) {
    const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
    if (r >= n || rec[r].ref < 0) return;
    const u32 c = cidx[r] + head[r] - 1u;  // (a placed record stands in or behind a run's first record)
    if (head[r]) {
        key[c] = (u64)(u32)rec[r].ref << 32 | bin[r];
        beg[c] = W.at(W.start[r + 1u]);
    }
    if (r + 1u == n || head[r + 1u] || rec[r + 1u].ref < 0) end[c] = W.at(W.start[r + 2u]);
}

// The records stand in coordinate order, so a wave almost always holds one reference: its lanes' counts and window maximum then meet
// in the wave (ballots, a shuffle maximum) and its first lane issues one atomic per word; a wave over a seam between two references
// or with unplaced records falls back to one atomic per lane.  All of it is commutative: the bytes do not depend on the path.
__global__ __launch_bounds__(256) void k_ix_ref(u32 n, const IxRec *__restrict__ rec, const uint16_t *__restrict__ flag, IxWhere W, u32 *__restrict__ n_intv,
                                                u64 *__restrict__ ref_beg, u64 *__restrict__ ref_end, u64 *__restrict__ mapped, u64 *__restrict__ unmapped,
                                                u64 *__restrict__ no_coor) {
    const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
    const bool in = r < n;
    const IxRec R = in ? rec[r] : IxRec{-1, 0, 1u};
    const bool placed = in && R.ref >= 0, un = in && (flag[r] & 4u);
    const u32 windows = placed ? ((R.end - 1u) >> 14) + 1u : 0u;
    const u64 live = __ballot(in), m_placed = __ballot(placed);
    const int32_t first = __shfl(R.ref, live ? (int)__builtin_ctzll(live) : 0, 64);
    const bool one = live != 0 && m_placed == live && __ballot(in && R.ref == first) == live;  // (the same for every lane of the wave)
    if (one) {
        u32 w = windows;
        for (int o = 32; o > 0; o >>= 1) w = max(w, (u32)__shfl_xor((int)w, o, 64));
        const u64 m_un = __ballot(un);
        if ((threadIdx.x & 63u) == (u32)__builtin_ctzll(live)) {
            atomicMax(&n_intv[first], w);
            const u64 k_un = (u64)__popcll(m_un), k_map = (u64)__popcll(live) - k_un;
            if (k_map) atomicAdd(&mapped[first], k_map);
            if (k_un) atomicAdd(&unmapped[first], k_un);
        }
    } else if (placed) {
        atomicMax(&n_intv[R.ref], windows);
        atomicAdd(un ? &unmapped[R.ref] : &mapped[R.ref], 1ull);
    } else if (in) atomicAdd(no_coor, 1ull);
    if (!placed) return;
    if (r == 0 || rec[r - 1u].ref != R.ref) ref_beg[R.ref] = W.at(W.start[r + 1u]);
    if (r + 1u == n || rec[r + 1u].ref != R.ref) ref_end[R.ref] = W.at(W.start[r + 2u]);
}

__global__ __launch_bounds__(256) void k_ix_lin(u32 n, const IxRec *__restrict__ rec, IxWhere W, const u64 *__restrict__ lin_off, u64 *__restrict__ lin) {
    const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
    if (r >= n || rec[r].ref < 0) return;
    const IxRec R = rec[r];
    const u64 v = W.at(W.start[r + 1u]), base = lin_off[R.ref];
    // The records stand in (reference, position) order and their starts grow with r: a window that the record in front reaches too
    // has a smaller start from it (or from one further in front), so only the windows behind that record's last one are this
    // record's to write -- about one atomic per window and not one per record.  (The minimum stays: a record may reach further
    // than a later one.)
    u32 w = (u32)R.pos >> 14;
    if (r > 0) {
        const IxRec P = rec[r - 1u];
        if (P.ref == R.ref) w = max(w, ((P.end - 1u) >> 14) + 1u);
    }
    for (; w <= (R.end - 1u) >> 14; w++) atomicMin(&lin[base + w], v);  // (w < n_intv[ref]: k_ix_ref took the maximum)
}

__global__ __launch_bounds__(256) void k_ix_fill(u32 n_ref, const u64 *__restrict__ lin_off, u64 *__restrict__ lin) {
    const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
    if (r >= n_ref) return;
    u64 next = 0;
    for (u64 w = lin_off[r + 1u]; w > lin_off[r]; w--) {  // from the right: an untouched window takes the next touched one's
        const u64 v = lin[w - 1u];
        if (v == ~0ull) lin[w - 1u] = next;
        else next = v;
    }
}

__global__ __launch_bounds__(256) void k_ix_gather(u32 n, const u32 *__restrict__ perm, const u64 *__restrict__ a, const u64 *__restrict__ b, u64 *__restrict__ oa,
                                                   u64 *__restrict__ ob) {
    const u64 j = (u64)blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    const u32 p = perm[j];
    oa[j] = a[p];
    ob[j] = b[p];
}

}  // namespace
