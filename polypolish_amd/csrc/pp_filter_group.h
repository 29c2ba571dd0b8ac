// pp_filter_group.h -- the filter's read grouping behind the interning, shared by the two device loaders: pp_filter_dev.hip
// (names in the SAM text) and pp_filter_rec.hip (the 64-bit ids of raw records).  Either interns its keys through an open-
// addressing table of record indices (the one over 64-bit ids is here: pp_regroup.hip interns a file's records with it, too) -- rep[i] = the first record, over both files, that carries record i's key -- and scans
// "is its own representative" into id_scan; from there on nothing depends on what a key is: read numbers (the rank of a key's
// first record), the files' group sizes, their scan, the scatter and the sort into file order.  Like pp_dev.h, which it
// builds on, everything lives in an anonymous namespace: each translation unit gets its own copies of the kernels.
#pragma once
#include "pp_dev.h"

namespace {

// ---- interning of 64-bit ids (pp_filter_rec.hip over both files' aligned records, pp_regroup.hip over one file's records): open
// addressing over record indices, a slot holds record index + 1; the representative of an id is its first record ----
__device__ __forceinline__ u32 hash_id(u64 x) {  // (the finaliser of MurmurHash3: every input bit reaches every output bit)
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return (u32)x;
}

__global__ __launch_bounds__(256) void k_rid_insert(u64 n, const u64 *__restrict__ ids, u32 *__restrict__ slots, u32 mask) {
    const u64 me = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (me >= n) return;
    const u64 a = ids[me];
    u32 i = hash_id(a) & mask;
    for (;;) {
        // look before touching the slot with an atomic (the mate's id is usually there already)
        u32 v = __atomic_load_n(&slots[i], __ATOMIC_RELAXED);
        if (v == 0) v = atomicCAS(&slots[i], 0u, (u32)me + 1u);
        if (v == 0) return;
        if (ids[v - 1] == a) {  // a slot only ever moves to a smaller index of the SAME id
            if ((u32)me + 1u < v) atomicMin(&slots[i], (u32)me + 1u);
            return;
        }
        i = (i + 1) & mask;
    }
}

__global__ __launch_bounds__(256) void k_rid_find(u64 n, const u64 *__restrict__ ids, const u32 *__restrict__ slots, u32 mask,
                                                  u32 *__restrict__ rep, u32 *__restrict__ is_rep) {
    const u64 me = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (me >= n) return;
    const u64 a = ids[me];
    u32 i = hash_id(a) & mask;
    for (;;) {
        const u32 v = slots[i];  // (never 0 on the way: the id was inserted)
        if (ids[v - 1] == a) {
            rep[me] = v - 1;
            is_rep[me] = (v - 1 == (u32)me);
            return;
        }
        i = (i + 1) & mask;
    }
}

// names of file 2 that file 1 holds as well (for the "alignments from N reads" line of file 2)
__global__ __launch_bounds__(256) void k_mark_shared(u64 n0, u64 n, const u32 *__restrict__ rep, u32 *__restrict__ hit) {
    const u64 i = n0 + (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && rep[i] < n0) hit[rep[i]] = 1;
}

__global__ __launch_bounds__(256) void k_assign(u32 n_aln, u64 base, const u32 *__restrict__ rep, const u32 *__restrict__ id_scan,
                                                const u32 *__restrict__ rep_ref, u32 *__restrict__ read,
                                                u32 *__restrict__ ref_id, u32 *__restrict__ grp_cnt) {
    const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_aln) return;
    const u32 id = id_scan[rep[base + r]];
    read[r] = id;
    if (rep_ref) ref_id[r] = rep_ref[base + r];  // (null: the caller's records carry their reference ids)
    atomicAdd(&grp_cnt[id], 1u);
}

__global__ __launch_bounds__(256) void k_grp_scatter(u32 n_aln, const u32 *__restrict__ read, const u32 *__restrict__ grp_off,
                                                     u32 *__restrict__ cursor, u32 *__restrict__ grp_idx) {
    const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_aln) return;
    const u32 id = read[r];
    grp_idx[grp_off[id] + atomicAdd(&cursor[id], 1u)] = r;
}

// file order inside every group (the scatter's order is whatever the atomics made it)
__global__ __launch_bounds__(256) void k_grp_sort(u32 n_reads, const u32 *__restrict__ grp_off, u32 *__restrict__ grp_idx) {
    const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_reads) return;
    const u32 lo = grp_off[r], hi = grp_off[r + 1];
    for (u32 i = lo + 1; i < hi; i++) {
        const u32 v = grp_idx[i];
        u32 j = i;
        while (j > lo && grp_idx[j - 1] > v) { grp_idx[j] = grp_idx[j - 1]; j--; }
        grp_idx[j] = v;
    }
}

// The groups of ONE file from the interned keys: read[], (ref_id[] from rep_ref -- both may be null: the caller has the ids
// already), grp_off[n_reads + 1] and grp_idx[] in file order inside a read.  base = the file's first record in rep[];
// cursor: n_reads words of scratch.
int file_groups(pp_ctx *ctx, u32 n_aln, u64 base, u32 n_reads, const u32 *rep, const u32 *id_scan, const u32 *rep_ref, u32 *read,
                u32 *ref_id, u32 *cursor, u32 *grp_off, u32 *grp_idx, pp::DevBuf &b_sums, pp::DevBuf &b_sums_off) {
    hipStream_t st = ctx->stream;
    const size_t cur_bytes = std::max<u64>(1, (u64)n_reads) * 4;
    PP_HIPCHK(ctx, hipMemsetAsync(cursor, 0, cur_bytes, st));
    if (n_aln)
        hipLaunchKernelGGL(k_assign, dim3((n_aln + 255) / 256), dim3(256), 0, st, n_aln, base, rep, id_scan, rep_ref, read, ref_id, cursor);
    if (int rc = scan_u32<u32>(ctx, b_sums, b_sums_off, (const u32 *)cursor, (u64)n_reads, grp_off)) return rc;
    PP_HIPCHK(ctx, hipMemsetAsync(cursor, 0, cur_bytes, st));
    if (n_aln) {
        hipLaunchKernelGGL(k_grp_scatter, dim3((n_aln + 255) / 256), dim3(256), 0, st, n_aln, (const u32 *)read, (const u32 *)grp_off, cursor, grp_idx);
        hipLaunchKernelGGL(k_grp_sort, dim3((n_reads + 255) / 256), dim3(256), 0, st, n_reads, (const u32 *)grp_off, grp_idx);
    }
    return PP_OK;
}

}  // namespace
