// pp_names.hip -- pp_names: a device-resident set of byte strings with dense ids, for a caller's QNAMEs and RNAMEs.
//
// pp_raw_batch.read_id and .contig are names as numbers: equal names <=> equal ids.  The reference keeps a HashMap<String, ..>
// for that; the text loaders intern the names of SAM text they uploaded themselves (k_ht_insert / k_ht_find, pp_filter_dev.hip).
// This is the same shape -- open addressing, the smallest index of a name is its representative, atomicCAS then atomicMin behind
// a plain atomic load -- over a caller's strings, with a table that stays: the id of a name is the number of distinct names in
// front of its first occurrence, over all calls.  One call:
//   k_nm_lookup   one lane per name: its range is checked before anything is read through it, then hashed eight bytes per load
//                 at any alignment and looked up among the RESIDENT names (slot = id + 1; the bytes compared are the caller's
//                 and the pool's).  The table is not written: a range defect, read back with the number of misses, leaves it
//                 unchanged.  No miss: the ids are all there.
//   k_nm_rehash   (the distinct names would pass half the slots) the resident names into a table twice as large, as often as
//                 needed, from the hashes the pool's entries keep.  Ids do not change.
//   k_nm_insert   the misses, with the call's own indices as candidates (slot = count + 1 + index, so a resident slot and a
//                 candidate cannot be mistaken; a miss equals no resident name and skips those without a look at their bytes).
//                 The bytes compared are the caller's.  Every miss notes the slot its name ended in.
//   k_nm_rank     a miss whose slot holds its own index is a new representative.  Their ranks -- new id = count + rank -- and
//                 the places of their bytes in the pool (a multiple of 8 each) by the workgroup scan of pp_dev.h and
//                 k_colscan over the workgroups' sums; second pass: the pool's entries, the slots pointed at the ids
//   k_nm_copy     eight lanes per new name: its bytes into the pool, zeros up to the next multiple of 8
//   k_nm_out      the ids, 64 and 32 bits wide
// No byte outside [0, n_bytes) is loaded: an 8-byte load is issued only where the array has eight bytes left, the last bytes of
// the array are read byte by byte.  Bytes behind a name are masked off before they reach the hash or a comparison.
#include "pp_dev.h"

namespace {

constexpr u32 NM_BLOCK = 1024;          // names per workgroup of the scanning kernel
constexpr u32 NM_NONE = 0xFFFFFFFFu;    // found[]: not among the resident names (ids end at 2^32 - 3)
constexpr u64 NM_MIN_SLOTS = 1024;
constexpr u32 NM_LOOKUP_BLOCKS = 2048;  // workgroups of k_nm_lookup at most (256 names a sweep each): eight on each of 256 CUs
constexpr u64 NM_CHUNK = 1ull << 26;    // names per pass over the kernels (bounds the scratch: 28 bytes per name)
constexpr u64 NM_MAX_NAMES = 0xFFFFFFFEull;  // distinct names a table holds at most (2^32 - 2)
// the spans of a call's kernels: range check and lookup | rehash | insert, rank, scan | entries and bytes | ids
enum : int { NM_T_LOOKUP = 0, NM_T_REHASH = 1, NM_T_INSERT = 2, NM_T_PLACE = 3, NM_T_OUT = 4, NM_STAGES = 5 };

struct NmEntry {  // a resident name: its bytes in the pool (off: a multiple of 8, zeros behind the name up to the next one), its hash
    u64 off;
    u32 len, hash;
};

struct NmSrc {  // the caller's names (device memory)
    const u8 *bytes;
    u64 n_bytes;
    const u64 *off;
    const u32 *len;
};

// The `live` (1..8) bytes at p + at as a little-endian word, zeros above them.  [at, at + live) lies inside [0, size): one
// 8-byte load at any alignment where the array has eight bytes left, else -- the array's last seven bytes -- byte by byte.
__device__ __forceinline__ u64 word_at(const u8 *__restrict__ p, u64 at, u32 live, u64 size) {
    u64 w = 0;
    if (size - at >= 8u) {
        __builtin_memcpy(&w, p + at, 8);  // (one global_load_dwordx2)
        if (live < 8u) w &= (1ull << (8u * live)) - 1ull;
    } else {
        for (u32 j = 0; j < live; j++) w |= (u64)p[at + j] << (8u * j);
    }
    return w;
}

__device__ __forceinline__ u64 mix(u64 h, u64 w) {
    h = (h ^ w) * 0x9E3779B97F4A7C15ull;
    return h ^ (h >> 29);
}
// (a name's words: w < ceil(len / 8) < 2^29, so 8 * w stays inside 32 bits)
__device__ __forceinline__ u32 words_of(u32 len) { return (u32)(((u64)len + 7u) >> 3); }
__device__ __forceinline__ u32 name_hash(const u8 *__restrict__ p, u64 off, u32 len, u64 size) {
    u64 h = 0xCBF29CE484222325ull ^ len;
    for (u32 w = 0, nw = words_of(len); w < nw; w++) h = mix(h, word_at(p, off + 8u * w, min(8u, len - 8u * w), size));
    h *= 0xD6E8FEB86659FD93ull;
    return (u32)(h >> 32);
}
// two names of `len` bytes in the caller's array
__device__ __forceinline__ bool same_names(const u8 *__restrict__ p, u64 a, u64 b, u32 len, u64 size) {
    if (a == b) return true;
    for (u32 w = 0, nw = words_of(len); w < nw; w++) {
        const u32 live = min(8u, len - 8u * w);
        if (word_at(p, a + 8u * w, live, size) != word_at(p, b + 8u * w, live, size)) return false;
    }
    return true;
}
// a name of the caller's and a resident one of the same length (the pool's words are aligned and padded with zeros)
__device__ __forceinline__ bool same_as_pool(const u8 *__restrict__ p, u64 a, u32 len, u64 size, const u64 *__restrict__ q) {
    for (u32 w = 0, nw = words_of(len); w < nw; w++)
        if (word_at(p, a + 8u * w, min(8u, len - 8u * w), size) != q[w]) return false;
    return true;
}

// the ranges alone (a call of several chunks: every range is known good before the first chunk touches the table)
__global__ __launch_bounds__(256) void k_nm_check(u64 n, NmSrc S, u64 *__restrict__ status) {
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    if (i < n && S.len[i] != 0 && !inside(S.off[i], S.len[i], S.n_bytes)) report(status, i);
}

// status[0]: the first name whose range does not lie inside the array; status[1]: names that are not resident.  At most
// NM_LOOKUP_BLOCKS workgroups stride over the names and each adds its misses to status[1] ONCE: a count per wave was 52,000
// atomics on one address for a file of 3.3 M new names, 0.5 ms of a 0.63 ms kernel (Guideline: sum on chip, then one atomic).
__global__ __launch_bounds__(256) void k_nm_lookup(u32 n, NmSrc S, u64 base, const u32 *__restrict__ slots, u64 mask,
                                                   const NmEntry *__restrict__ entries, const u8 *__restrict__ pool,
                                                   u32 *__restrict__ hash, u32 *__restrict__ found, u64 *__restrict__ status) {
    __shared__ u32 s_miss;
    if (threadIdx.x == 0) s_miss = 0;
    __syncthreads();
    u32 misses = 0;
    for (u64 i = (u64)blockIdx.x * 256u + threadIdx.x; i < n; i += (u64)gridDim.x * 256u) {
        const u64 o = S.off[i];
        const u32 l = S.len[i];
        if (l != 0 && !inside(o, l, S.n_bytes)) {
            report(status, base + i);
            continue;
        }
        const u32 h = name_hash(S.bytes, o, l, S.n_bytes);
        u32 id = NM_NONE;
        for (u64 s = h & mask;; s = (s + 1u) & mask) {  // (at most half the slots are taken)
            const u32 v = slots[s];
            if (v == 0) break;
            const NmEntry e = entries[v - 1u];
            if (e.hash == h && e.len == l && same_as_pool(S.bytes, o, l, S.n_bytes, (const u64 *)(pool + e.off))) {
                id = v - 1u;
                break;
            }
        }
        hash[i] = h;
        found[i] = id;
        misses += id == NM_NONE ? 1u : 0u;
    }
    const u32 wave_misses = pp::wave_scan_incl(misses);  // (lane 63: the wave's sum)
    if ((threadIdx.x & 63u) == 63u && wave_misses) atomicAdd(&s_miss, wave_misses);
    __syncthreads();
    if (threadIdx.x == 0 && s_miss) atomicAdd(status + 1, (u64)s_miss);
}

__global__ __launch_bounds__(256) void k_nm_rehash(u32 count, const NmEntry *__restrict__ entries, u32 *__restrict__ slots, u64 mask) {
    const u32 id = blockIdx.x * 256u + threadIdx.x;
    if (id >= count) return;
    for (u64 s = entries[id].hash & mask;; s = (s + 1u) & mask)
        if (__atomic_load_n(&slots[s], __ATOMIC_RELAXED) == 0 && atomicCAS(&slots[s], 0u, id + 1u) == 0) return;
}

__global__ __launch_bounds__(256) void k_nm_insert(u32 n, NmSrc S, const u32 *__restrict__ hash, const u32 *__restrict__ found,
                                                   u32 *__restrict__ slots, u64 mask, u32 count, u64 *__restrict__ slot_of) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n || found[i] != NM_NONE) return;
    const u32 h = hash[i], l = S.len[i], me = count + 1u + i;
    const u64 o = S.off[i];
    u64 s = h & mask;
    for (;; s = (s + 1u) & mask) {
        // look before touching the slot with an atomic: a million copies of one new name would serialise on its address
        u32 v = __atomic_load_n(&slots[s], __ATOMIC_RELAXED);
        if (v == 0) v = atomicCAS(&slots[s], 0u, me);
        if (v == 0) break;
        if (v <= count) continue;  // a resident name: the lookup found this one equal to none of them
        const u32 j = v - count - 1u;
        if (hash[j] == h && S.len[j] == l && same_names(S.bytes, o, S.off[j], l, S.n_bytes)) {
            if (me < v) atomicMin(&slots[s], me);  // a slot only ever moves to a smaller index of the SAME name
            break;
        }
    }
    slot_of[i] = s;
}

// PLACE == false: rep[] of every miss, and the workgroups' numbers of new representatives and of their pool words (blk2: two
// words per workgroup).  PLACE == true: blk2 holds their exclusive scan; every new representative gets its id and its entry,
// its slot is pointed at the id, found[] of it becomes the id and src_of[rank] its index.
template <bool PLACE>
__global__ __launch_bounds__(NM_BLOCK) void k_nm_rank(u32 n, NmSrc S, const u32 *__restrict__ hash, u32 *__restrict__ found,
                                                      u32 *__restrict__ slots, const u64 *__restrict__ slot_of, u32 count, u64 pool_used,
                                                      u32 *__restrict__ rep, u64 *__restrict__ blk2, NmEntry *__restrict__ entries,
                                                      u32 *__restrict__ src_of) {
    __shared__ u64 s_w[NM_BLOCK / 64];
    const u64 i = (u64)blockIdx.x * NM_BLOCK + threadIdx.x;
    u32 is_rep = 0, words = 0;
    if (i < n && found[i] == NM_NONE) {
        u32 r;
        if (!PLACE) rep[i] = r = slots[slot_of[i]] - count - 1u;
        else r = rep[i];
        if (r == (u32)i) {
            is_rep = 1;
            words = words_of(S.len[i]);
        }
    }
    u64 t_cnt, t_words;
    const u64 ex_cnt = block_scan_excl64<NM_BLOCK>(is_rep, s_w, &t_cnt);
    const u64 ex_words = block_scan_excl64<NM_BLOCK>(words, s_w, &t_words);
    u64 *const mine = blk2 + 2ull * blockIdx.x;
    if (!PLACE) {
        if (threadIdx.x == 0) { mine[0] = t_cnt; mine[1] = t_words; }
        return;
    }
    if (!is_rep) return;
    const u32 rank = (u32)(mine[0] + ex_cnt), id = count + rank;
    entries[id] = NmEntry{pool_used + 8ull * (mine[1] + ex_words), S.len[i], hash[i]};
    slots[slot_of[i]] = id + 1u;
    found[i] = id;
    src_of[rank] = (u32)i;
}

// the table as it was: the slots of the call's new representatives emptied again (the table would pass its limit)
__global__ __launch_bounds__(256) void k_nm_undo(u32 n, const u32 *__restrict__ found, const u32 *__restrict__ rep,
                                                 const u64 *__restrict__ slot_of, u32 *__restrict__ slots) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i < n && found[i] == NM_NONE && rep[i] == i) slots[slot_of[i]] = 0;
}

// the bytes of the new names into the pool: eight lanes per name, a word per lane and trip
__global__ __launch_bounds__(256) void k_nm_copy(u32 n_new, NmSrc S, const u32 *__restrict__ src_of, const NmEntry *__restrict__ fresh,
                                                 u8 *__restrict__ pool) {
    const u64 t = (u64)blockIdx.x * 256u + threadIdx.x;
    if ((t >> 3) >= n_new) return;
    const NmEntry e = fresh[t >> 3];
    const u64 o = S.off[src_of[t >> 3]];
    u64 *const out = (u64 *)(pool + e.off);
    for (u64 i = 8u * ((u32)t & 7u); i < e.len; i += 64u) out[i >> 3] = word_at(S.bytes, o + i, (u32)min((u64)8, e.len - i), S.n_bytes);
}

__global__ __launch_bounds__(256) void k_nm_out(u32 n, const u32 *__restrict__ found, const u32 *__restrict__ rep, u64 *__restrict__ id64,
                                                u32 *__restrict__ id32) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    u32 id = found[i];
    if (id == NM_NONE) id = found[rep[i]];
    if (id64) id64[i] = id;
    if (id32) id32[i] = id;
}

}  // namespace

struct pp_names {
    pp_ctx *ctx = nullptr;
    int device = 0;
    pp::DevBuf slots, entries, pool;  // u32[cap]: 0 or id + 1 | NmEntry[count] | the names' bytes
    u64 cap = 0, count = 0, pool_used = 0;
    // scratch of a call (grow-only): hash found rep src_of | slot_of | blk2 blk2off | status | a host array's copies
    pp::DevBuf hash, found, rep, src_of, slot_of, blk2, blk2off, status, up_bytes, up_off, up_len, dn64, dn32;
    StageMs<NM_STAGES> t;  // the last call's kernels by stage
};

namespace {

// the table with room for `need` distinct names at no more than half its slots
int names_reserve(pp_names *T, u64 need, StageTimer &timer) {
    pp_ctx *ctx = T->ctx;
    u64 cap = T->cap;
    while (2 * need > cap) cap <<= 1;
    if (cap == T->cap) return PP_OK;
    pp::DevBuf grown;
    if (int rc = pp::dev_ensure(ctx, grown, (size_t)cap * 4)) return rc;
    if (int rc = timer.begin(NM_T_REHASH)) return rc;
    PP_HIPCHK(ctx, hipMemsetAsync(grown.p, 0, (size_t)cap * 4, ctx->stream));
    if (T->count)
        hipLaunchKernelGGL(k_nm_rehash, dim3((unsigned)((T->count + 255) / 256)), dim3(256), 0, ctx->stream, (u32)T->count,
                           (const NmEntry *)T->entries.p, (u32 *)grown.p, cap - 1);
    if (int rc = timer.end()) return rc;
    PP_HIPCHK(ctx, hipGetLastError());
    PP_HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    pp::dev_free(T->slots);
    T->slots = grown;
    T->cap = cap;
    return PP_OK;
}

// One pass over the kernels: n <= NM_CHUNK names in device memory (base: the index of the chunk's first name in the call, for *bad).
// The table's room is reserved for every miss as if it were a new name: known before the first slot is written.
int names_chunk(pp_names *T, NmSrc S, u32 n, u64 base, u64 *id64, u32 *id32, StageTimer &timer, uint64_t *bad) {
    pp_ctx *ctx = T->ctx;
    hipStream_t st = ctx->stream;
    int rc;
    const unsigned g256 = (n + 255u) / 256u, nb = (n + NM_BLOCK - 1u) / NM_BLOCK;
    if ((rc = pp::dev_ensure(ctx, T->hash, (size_t)n * 4)) || (rc = pp::dev_ensure(ctx, T->found, (size_t)n * 4)) ||
        (rc = pp::dev_ensure(ctx, T->rep, (size_t)n * 4)) || (rc = pp::dev_ensure(ctx, T->src_of, (size_t)n * 4)) ||
        (rc = pp::dev_ensure(ctx, T->slot_of, (size_t)n * 8)) || (rc = pp::dev_ensure(ctx, T->blk2, (size_t)nb * 16)) ||
        (rc = pp::dev_ensure(ctx, T->blk2off, ((size_t)nb + 1) * 16)) || (rc = pp::dev_ensure(ctx, T->status, 16)))
        return rc;
    u32 *const d_hash = (u32 *)T->hash.p, *const d_found = (u32 *)T->found.p, *const d_rep = (u32 *)T->rep.p, *const d_src_of = (u32 *)T->src_of.p;
    u64 *const d_slot_of = (u64 *)T->slot_of.p, *const d_status = (u64 *)T->status.p;
    PP_HIPCHK(ctx, hipMemsetAsync(d_status, 0xFF, 8, st));
    PP_HIPCHK(ctx, hipMemsetAsync(d_status + 1, 0, 8, st));

    // ---- among the resident names ----
    if ((rc = timer.begin(NM_T_LOOKUP))) return rc;
    hipLaunchKernelGGL(k_nm_lookup, dim3(std::min(g256, NM_LOOKUP_BLOCKS)), dim3(256), 0, st, n, S, base, (const u32 *)T->slots.p, T->cap - 1,
                       (const NmEntry *)T->entries.p, (const u8 *)T->pool.p, d_hash, d_found, d_status);
    if ((rc = timer.end())) return rc;
    PP_HIPCHK(ctx, hipGetLastError());
    u64 status[2];
    if ((rc = fetch(ctx, d_status, status, 2))) return rc;
    if (status[0] != ~0ull) {
        if (bad) *bad = status[0];
        return ctx->fail(PP_ERR_ARG, "pp_names_ids: the range of name %llu does not lie inside the %llu bytes", (unsigned long long)status[0],
                         (unsigned long long)S.n_bytes);
    }
    const u64 n_miss = status[1];

    if (n_miss) {
        // ---- the misses: candidates, representatives, ranks ----
        if ((rc = names_reserve(T, std::min<u64>(T->count + n_miss, NM_MAX_NAMES), timer))) return rc;
        u32 *const d_slots = (u32 *)T->slots.p;
        const u32 count = (u32)T->count;
        if ((rc = timer.begin(NM_T_INSERT))) return rc;
        hipLaunchKernelGGL(k_nm_insert, dim3(g256), dim3(256), 0, st, n, S, (const u32 *)d_hash, (const u32 *)d_found, d_slots, T->cap - 1, count,
                           d_slot_of);
        hipLaunchKernelGGL(k_nm_rank<false>, dim3(nb), dim3(NM_BLOCK), 0, st, n, S, (const u32 *)d_hash, d_found, d_slots, (const u64 *)d_slot_of,
                           count, T->pool_used, d_rep, (u64 *)T->blk2.p, (NmEntry *)nullptr, (u32 *)nullptr);
        hipLaunchKernelGGL(k_colscan<2>, dim3(1), dim3(1024), 0, st, (const u64 *)T->blk2.p, (u64)nb, (u64 *)T->blk2off.p);
        if ((rc = timer.end())) return rc;
        PP_HIPCHK(ctx, hipGetLastError());
        u64 totals[2];
        if ((rc = fetch(ctx, (const u64 *)T->blk2off.p + 2ull * nb, totals, 2))) return rc;
        const u64 n_new = totals[0], new_bytes = 8ull * totals[1];
        if (T->count + n_new > NM_MAX_NAMES) {
            hipLaunchKernelGGL(k_nm_undo, dim3(g256), dim3(256), 0, st, n, (const u32 *)d_found, (const u32 *)d_rep, (const u64 *)d_slot_of, d_slots);
            PP_HIPCHK(ctx, hipGetLastError());
            PP_HIPCHK(ctx, hipStreamSynchronize(st));
            return ctx->fail(PP_ERR_LIMIT, "pp_names_ids: 2^32-1 or more distinct names in one table");
        }
        // ---- entries, bytes, slots ----
        if ((rc = pp::dev_grow_keep(ctx, T->entries, (size_t)(T->count + n_new) * sizeof(NmEntry), (size_t)T->count * sizeof(NmEntry))) ||
            (rc = pp::dev_grow_keep(ctx, T->pool, (size_t)(T->pool_used + new_bytes), (size_t)T->pool_used)))
            return rc;
        NmEntry *const d_entries = (NmEntry *)T->entries.p;
        if ((rc = timer.begin(NM_T_PLACE))) return rc;
        hipLaunchKernelGGL(k_nm_rank<true>, dim3(nb), dim3(NM_BLOCK), 0, st, n, S, (const u32 *)d_hash, d_found, d_slots, (const u64 *)d_slot_of, count,
                           T->pool_used, d_rep, (u64 *)T->blk2off.p, d_entries, d_src_of);
        hipLaunchKernelGGL(k_nm_copy, dim3((unsigned)((n_new * 8u + 255u) / 256u)), dim3(256), 0, st, (u32)n_new, S, (const u32 *)d_src_of,
                           (const NmEntry *)(d_entries + count), (u8 *)T->pool.p);
        if ((rc = timer.end())) return rc;
        T->count += n_new;
        T->pool_used += new_bytes;
    }
    if ((rc = timer.begin(NM_T_OUT))) return rc;
    hipLaunchKernelGGL(k_nm_out, dim3(g256), dim3(256), 0, st, n, (const u32 *)d_found, (const u32 *)d_rep, id64, id32);
    if ((rc = timer.end())) return rc;
    PP_HIPCHK(ctx, hipGetLastError());
    return PP_OK;
}

}  // namespace

extern "C" int pp_names_create(pp_ctx *ctx, uint64_t expect, pp_names **out) {
    if (!ctx) return PP_ERR_ARG;
    if (int rdy = pp_ctx_wait(ctx)) return rdy;
    if (!out) return ctx->fail(PP_ERR_ARG, "pp_names_create: null argument");
    *out = nullptr;
    PP_HIPCHK(ctx, hipSetDevice(ctx->device));
    pp_names *T = new pp_names;
    T->ctx = ctx;
    T->device = ctx->device;
    std::unique_ptr<pp_names, void (*)(pp_names *)> guard(T, pp_names_free);
    T->cap = NM_MIN_SLOTS;
    const u64 want = std::min<u64>(expect, NM_MAX_NAMES);
    while (2 * want > T->cap) T->cap <<= 1;
    int rc;
    if ((rc = pp::dev_ensure(ctx, T->slots, (size_t)T->cap * 4)) || (rc = pp::dev_ensure(ctx, T->entries, 16)) || (rc = pp::dev_ensure(ctx, T->pool, 16)))
        return rc;
    PP_HIPCHK(ctx, hipMemsetAsync(T->slots.p, 0, (size_t)T->cap * 4, ctx->stream));
    PP_HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    guard.release();
    *out = T;
    return PP_OK;
}

extern "C" void pp_names_free(pp_names *T) {
    if (!T) return;
    (void)hipSetDevice(T->device);  // (every call ends with the stream synchronised: nothing of the table's is in flight)
    pp::DevBuf *all[] = {&T->slots, &T->entries, &T->pool, &T->hash, &T->found, &T->rep, &T->src_of, &T->slot_of, &T->blk2, &T->blk2off,
                         &T->status, &T->up_bytes, &T->up_off, &T->up_len, &T->dn64, &T->dn32};
    for (pp::DevBuf *b : all) pp::dev_free(*b);
    delete T;
}

extern "C" uint64_t pp_names_count(const pp_names *T) { return T ? T->count : 0; }

extern "C" int pp_names_kernel_ms(const pp_names *T, float *ms) {
    return T ? T->t.total(T->ctx, "pp_names_kernel_ms", "at the table's last pp_names_ids", ms) : PP_ERR_ARG;
}

// (internal hook, not part of the header: tools/names_timing.py) the same time by stage: lookup | rehash | insert, rank | entries, bytes | ids
extern "C" int pp_names_stage_ms_(const pp_names *T, float *ms5) { return T ? T->t.stages(ms5) : PP_ERR_ARG; }

extern "C" int pp_names_name(const pp_names *T, uint64_t id, uint8_t *out, uint32_t cap, uint32_t *len) {
    if (!T) return PP_ERR_ARG;
    pp_ctx *ctx = T->ctx;
    if (!len || (cap && !out)) return ctx->fail(PP_ERR_ARG, "pp_names_name: null argument");
    if (id >= T->count) return ctx->fail(PP_ERR_ARG, "pp_names_name: the table holds %llu names, none with the id %llu", (unsigned long long)T->count, (unsigned long long)id);
    PP_HIPCHK(ctx, hipSetDevice(ctx->device));
    NmEntry e;
    if (int rc = fetch(ctx, (const NmEntry *)T->entries.p + id, &e)) return rc;
    *len = e.len;
    if (cap < e.len) return ctx->fail(PP_ERR_ARG, "pp_names_name: the name of id %llu has %u bytes, the buffer %u", (unsigned long long)id, e.len, cap);
    if (e.len)
        if (int rc = fetch(ctx, (const u8 *)T->pool.p + e.off, out, e.len)) return rc;
    return PP_OK;
}

extern "C" int pp_names_ids(pp_names *T, const uint8_t *bytes, uint64_t n_bytes, const uint64_t *off, const uint32_t *len, uint64_t n, int mem,
                            uint64_t *id64, uint32_t *id32, uint64_t *bad) {
    if (!T) return PP_ERR_ARG;
    pp_ctx *ctx = T->ctx;
    if (int rdy = pp_ctx_wait(ctx)) return rdy;
    if (bad) *bad = ~0ull;
    if (mem != PP_MEM_HOST && mem != PP_MEM_DEVICE)
        return ctx->fail(PP_ERR_ARG, "pp_names_ids: the names must be host memory or memory of the context's device");
    if (n == 0) return PP_OK;
    if (!id64 && !id32) return ctx->fail(PP_ERR_ARG, "pp_names_ids: neither id64 nor id32");
    if (!off || !len || (n_bytes && !bytes)) return ctx->fail(PP_ERR_ARG, "pp_names_ids: null array with n > 0");
    if (n >= 0xFFFFFFFFull) return ctx->fail(PP_ERR_LIMIT, "pp_names_ids: 2^32-1 or more names in one call");
    PP_HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    StageTimer timer(ctx, ctx->profiling != 0);
    T->t.timed = false;
    int rc;

    NmSrc S{bytes, n_bytes, (const u64 *)off, len};
    u64 *d64 = (u64 *)id64;
    u32 *d32 = id32;
    if (mem == PP_MEM_HOST) {
        if ((rc = pp::dev_ensure(ctx, T->up_bytes, (size_t)n_bytes)) || (rc = pp::dev_ensure(ctx, T->up_off, (size_t)n * 8)) ||
            (rc = pp::dev_ensure(ctx, T->up_len, (size_t)n * 4)) || (id64 && (rc = pp::dev_ensure(ctx, T->dn64, (size_t)n * 8))) ||
            (id32 && (rc = pp::dev_ensure(ctx, T->dn32, (size_t)n * 4))))
            return rc;
        if (n_bytes) PP_HIPCHK(ctx, hipMemcpyAsync(T->up_bytes.p, bytes, (size_t)n_bytes, hipMemcpyHostToDevice, st));
        PP_HIPCHK(ctx, hipMemcpyAsync(T->up_off.p, off, (size_t)n * 8, hipMemcpyHostToDevice, st));
        PP_HIPCHK(ctx, hipMemcpyAsync(T->up_len.p, len, (size_t)n * 4, hipMemcpyHostToDevice, st));
        S = NmSrc{(const u8 *)T->up_bytes.p, n_bytes, (const u64 *)T->up_off.p, (const u32 *)T->up_len.p};
        d64 = id64 ? (u64 *)T->dn64.p : nullptr;
        d32 = id32 ? (u32 *)T->dn32.p : nullptr;
    }
    if (n > NM_CHUNK) {  // several chunks: every range before the first of them reaches the table
        if ((rc = pp::dev_ensure(ctx, T->status, 16))) return rc;
        PP_HIPCHK(ctx, hipMemsetAsync(T->status.p, 0xFF, 8, st));
        if ((rc = timer.begin(NM_T_LOOKUP))) return rc;
        hipLaunchKernelGGL(k_nm_check, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, S, (u64 *)T->status.p);
        if ((rc = timer.end())) return rc;
        PP_HIPCHK(ctx, hipGetLastError());
        u64 first = ~0ull;
        if ((rc = fetch(ctx, T->status.p, &first))) return rc;
        if (first != ~0ull) {
            if (bad) *bad = first;
            return ctx->fail(PP_ERR_ARG, "pp_names_ids: the range of name %llu does not lie inside the %llu bytes", (unsigned long long)first,
                             (unsigned long long)n_bytes);
        }
    }
    for (u64 done = 0; done < n;) {
        // (a candidate is count + 1 + index in 32 bits: a table near its limit takes the names in smaller chunks)
        const u64 m = std::min<u64>(std::min<u64>(n - done, NM_CHUNK), 0xFFFFFFFFull - T->count);
        NmSrc C = S;
        C.off += done;
        C.len += done;
        if ((rc = names_chunk(T, C, (u32)m, done, d64 ? d64 + done : nullptr, d32 ? d32 + done : nullptr, timer, bad))) return rc;
        done += m;
    }
    if (mem == PP_MEM_HOST) {
        if (id64) PP_HIPCHK(ctx, hipMemcpyAsync(id64, T->dn64.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
        if (id32) PP_HIPCHK(ctx, hipMemcpyAsync(id32, T->dn32.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    }
    PP_HIPCHK(ctx, hipStreamSynchronize(st));  // the caller's arrays may be released
    return T->t.take(timer);
}
