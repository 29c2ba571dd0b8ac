// pp_bam_walk.hip -- pp_bam_walk_device: the block_size chain of UNCOMPRESSED BAM bytes walked on the device, exactly: the record
// offsets pp_bam_records takes as PP_MEM_DEVICE, for a caller whose bytes never leave device memory (pp_bgzf_bam_walk, pp_bgzf.hip, is
// a call of it).  The chain is serial by the format only along the true chain; a record takes 4 + block_size >= 36 bytes, so the
// record behind one at offset o starts at o + 36 or later, and everything here rests on that:
//   k_bamwalk_chunk   ONE WAVE per chunk of WALK_C bytes, the only kernel that touches all bytes.  The chunk goes into LDS (16-byte
//                     loads; the up to three bytes of the next chunk that a block_size word at the chunk's end reaches into stay in
//                     a register).  For every offset o of the chunk, from the top band of 32 offsets down, one word last | cnt << 16:
//                     the last offset inside the chunk on the chain from o -- the one whose step leaves the chunk, reaches n_bytes
//                     or is refused -- and the number of good records on the way.  The 32 offsets of a band do not depend on each
//                     other, and the record behind each starts in a band that is done: a band is one step of the wave, two
//                     dependent LDS reads, and the trip count is WALK_C / 32 whatever the bytes are.  The entries of the first
//                     WALK_Z offsets, the chunk's ENTRY ZONE, go to scratch.
//   k_bamwalk_group   the step over a group of WALK_G chunks, for each of the WALK_Z possible entries into the group's first chunk:
//                     per chunk one gather from its zone and one step at `last`.  An entry at or behind a chunk's end passes
//                     through (a record that skips the chunk).  A lane that lands behind a zone (the record in front is longer than
//                     WALK_Z) or on a refused step gives up: its entry says "serial".
//   k_bamwalk_chain   one thread chains the groups: the chunk that holds `from` is walked record by record, the rest of its group
//                     chunk by chunk, every later group through its table -- or chunk by chunk where the entry says so, a chunk
//                     entered behind its zone record by record (the SLOW PATH: at most WALK_C / 36 dependent loads on one lane).
//                     It leaves the total, the end or the first break (kind, record, offset, block_size) and the path counts in one
//                     status block, which the host reads once, and every group's entry.
//   k_bamwalk_replay  one thread per group, from the group's entry: every chunk's entry and record count.
//   k_bamwalk_emit    scan_u32 over the counts gives every chunk its base; one thread per chunk walks it and writes the offsets.
// EVERY LOOP IS BOUNDED BY THE INPUT: each trip takes at least 36 bytes or one chunk.  One record is hw::step (pp_bam_host.h), the
// function the host walk runs; the host words a break from what the status block holds with the host walk's own function.
// No byte outside [0, n_bytes) is loaded: a wide load is issued only where the array has that many bytes left, and step() looks at a
// block_size word only where four bytes are left.  Bytes in front of `from` and bytes off the chain are data: they fill table
// entries nobody follows.
#include "pp_bam_host.h"
#include "pp_dev.h"

extern "C" char *pp_bam_msg_buf_(size_t *cap);  // pp_bam.hip: the per-thread message behind pp_bam_last_error()

struct pp_bam_offs : DevOwner {
    using DevOwner::DevOwner;
    u64 *d_off = nullptr;  // DEVICE: n_rec offsets
    uint64_t n_rec = 0, end = 0;
    uint64_t stats[4] = {0, 0, 0, 0};  // along the true chain: chunks on it | entered through a zone | on the slow path | passed through
    StageMs<3> t;          // the chunk tables | groups, chain and replay | scan and offsets
};

namespace {

namespace hw = pp_bam_host;

constexpr u32 WALK_C = 16384;  // bytes per chunk: the table (64 KiB) and the bytes (16 KiB) of one chunk fill half a CU's LDS
constexpr u32 WALK_Z = 1024;   // offsets of a chunk's entry zone: a record of up to WALK_Z bytes in front lands inside it
constexpr u32 WALK_G = 64;     // chunks per group
constexpr u32 SERIAL = 0xFFFFFFFFu;
enum : u32 { VIA_ZONE = 0, VIA_SLOW = 1, VIA_PASS = 2, VIA_DIRECT = 3 };
enum : u32 { R_KIND = 0, R_COUNT = 1, R_END = 2, R_BS = 3, R_STATS = 4, R_WORDS = 8 };  // the status block

struct WalkSrc {
    const u8 *bytes;
    u64 n_bytes, from;
    u32 c0, nch;      // the chunk that holds `from`; the number of chunks
    const u32 *zone;  // WALK_Z entries per chunk, from chunk c0 + 1 on
};
struct GroupEntry {  // the step over a group from one entry of its first chunk
    u64 e;           // the entry of the next group
    u32 cnt, pass;   // records on the way; chunks passed through, or SERIAL: walk this group chunk by chunk
};
struct ChunkStep {
    u64 e;  // the entry of the next chunk, or the offending offset
    u32 cnt, kind, bs, via;
};

__global__ __launch_bounds__(64) void k_bamwalk_chunk(const u8 *__restrict__ B, u64 N, u32 c_first, u32 *__restrict__ zone) {
    __shared__ u32 s_bytes[WALK_C / 4];
    __shared__ u32 s_tab[WALK_C];
    const u32 lane = threadIdx.x;
    const u64 lo = (u64)(c_first + blockIdx.x) * WALK_C;  // < N: the chunk exists
    const u32 have = (u32)min((u64)WALK_C, N - lo);
    for (u32 i = lane * 16u; i < WALK_C; i += 64u * 16u) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (have >= 16u && i <= have - 16u) {
            __builtin_memcpy(&v, B + lo + i, 16);  // (any alignment: one global_load_dwordx4)
        } else if (i < have) {  // the array's last bytes
            u32 w[4] = {0u, 0u, 0u, 0u};
            for (u32 j = 0; j < 16u && i + j < have; j++) w[j >> 2] |= (u32)B[lo + i + j] << (8u * (j & 3u));
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        *(uint4 *)&s_bytes[i >> 2] = v;
    }
    u32 tail = 0;  // what a block_size word in the chunk's last three bytes takes from the next chunk
    for (u32 j = 0; j < 3u; j++)
        if (N - lo > (u64)WALK_C + j) tail |= (u32)B[lo + WALK_C + j] << (8u * j);
    __syncthreads();
    for (int band = (int)(WALK_C / 32u) - 1; band >= 0; band--) {
        const u32 o = (u32)band * 32u + (lane & 31u);
        if (lane < 32u) {
            const u32 wi = o >> 2, sh = (o & 3u) * 8u;
            const u32 w0 = s_bytes[wi], w1 = wi + 1u < WALK_C / 4u ? s_bytes[wi + 1u] : tail;
            const u32 bs = sh ? (w0 >> sh) | (w1 << (32u - sh)) : w0;
            u32 ent = o;  // last = o, no record
            if (o < have && hw::step_kind(N - lo - o, bs) == hw::W_OK) {
                const u64 t = (u64)o + 4u + bs;  // <= N - lo
                ent = t >= have ? (o | 1u << 16) : s_tab[(u32)t] + (1u << 16);
            }
            s_tab[o] = ent;
        }
        __syncthreads();  // (one wave: no barrier instruction, the LDS traffic in order)
    }
    u32 *const row = zone + (u64)blockIdx.x * WALK_Z;
    for (u32 z = lane; z < WALK_Z; z += 64u) row[z] = s_tab[z];
}

// the records of chunk c from e on, one by one (e >= the chunk's start)
__device__ __forceinline__ void walk_chunk(const WalkSrc &S, u32 c, ChunkStep &r) {
    const u64 hi = min(((u64)c + 1u) * WALK_C, S.n_bytes);
    while (r.e < hi) {
        uint64_t next = r.e;
        r.kind = hw::step(S.bytes, S.n_bytes, r.e, &next, &r.bs);
        if (r.kind != hw::W_OK) return;
        r.cnt++;
        r.e = next;
    }
}

// through chunk c's zone from e (inside the zone, inside the bytes): the table's entry and the step at its `last`
__device__ __forceinline__ void zone_step(const WalkSrc &S, u32 c, ChunkStep &r) {
    const u64 lo = (u64)c * WALK_C;
    const u32 v = S.zone[(u64)(c - S.c0 - 1u) * WALK_Z + (u32)(r.e - lo)];
    const u64 la = lo + (v & 0xFFFFu);
    uint64_t next = la;
    r.cnt = v >> 16;
    r.kind = hw::step(S.bytes, S.n_bytes, la, &next, &r.bs);
    r.e = r.kind == hw::W_OK ? next : la;
}

// entry e into chunk c (e >= the chunk's start) -> the entry of the next chunk and the records on the way, or the break
__device__ __forceinline__ ChunkStep chunk_step(const WalkSrc &S, u32 c, u64 e) {
    const u64 lo = (u64)c * WALK_C, hi = min(lo + WALK_C, S.n_bytes);
    ChunkStep r{e, 0u, hw::W_OK, 0u, VIA_PASS};
    if (c == S.c0) {  // the start is anywhere: no table
        r.via = VIA_DIRECT;
        walk_chunk(S, c, r);
    } else if (e >= hi) {  // a record skips the chunk
    } else if (e - lo < WALK_Z) {
        r.via = VIA_ZONE;
        zone_step(S, c, r);
    } else {  // the record in front is longer than the zone
        r.via = VIA_SLOW;
        walk_chunk(S, c, r);
    }
    return r;
}

__global__ __launch_bounds__(256) void k_bamwalk_group(WalkSrc S, u32 g_first, u32 n_groups, GroupEntry *__restrict__ gtab) {
    const u64 t = (u64)blockIdx.x * 256u + threadIdx.x;
    if (t / WALK_Z >= n_groups) return;
    const u32 g = g_first + (u32)(t / WALK_Z), cb = g * WALK_G, ce = min(cb + WALK_G, S.nch);
    u64 e = (u64)cb * WALK_C + (u32)(t % WALK_Z);
    GroupEntry out{e, 0u, SERIAL};
    if (e < S.n_bytes) {
        u32 cnt = 0, pass = 0, c = cb;
        for (; c < ce; c++) {
            const u64 lo = (u64)c * WALK_C, hi = min(lo + WALK_C, S.n_bytes);
            if (e >= hi) { pass++; continue; }
            if (e - lo >= WALK_Z) break;
            ChunkStep r{e, 0u, hw::W_OK, 0u, VIA_ZONE};
            zone_step(S, c, r);
            if (r.kind != hw::W_OK) break;
            cnt += r.cnt;
            e = r.e;
        }
        if (c == ce) out = GroupEntry{e, cnt, pass};
    }
    gtab[t] = out;
}

__global__ void k_bamwalk_chain(WalkSrc S, const GroupEntry *__restrict__ gtab, u64 *__restrict__ gentry, u64 *__restrict__ res) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const u32 g0 = S.c0 / WALK_G, n_groups = (S.nch + WALK_G - 1u) / WALK_G;
    u64 e = S.from, total = 0, st[4] = {0, 0, 0, 0};
    u32 kind = hw::W_OK, bs = 0;
    for (u32 g = g0; g < n_groups && kind == hw::W_OK; g++) {
        const u32 cb = g == g0 ? S.c0 : g * WALK_G, ce = min((g + 1u) * WALK_G, S.nch);
        gentry[g - g0] = e;
        if (g != g0) {
            if (e >= min((u64)ce * WALK_C, S.n_bytes)) {  // a record skips the group
                st[0] += ce - cb;
                st[3] += ce - cb;
                continue;
            }
            const u64 z = e - (u64)cb * WALK_C;
            if (z < WALK_Z) {
                const GroupEntry t = gtab[(u64)(g - g0 - 1u) * WALK_Z + z];
                if (t.pass != SERIAL) {
                    e = t.e;
                    total += t.cnt;
                    st[0] += ce - cb;
                    st[1] += ce - cb - t.pass;
                    st[3] += t.pass;
                    continue;
                }
            }
        }
        for (u32 c = cb; c < ce; c++) {
            const ChunkStep r = chunk_step(S, c, e);
            st[0]++;
            if (r.via != VIA_DIRECT) st[1 + r.via]++;
            total += r.cnt;
            e = r.e;
            if (r.kind != hw::W_OK) {
                kind = r.kind;
                bs = r.bs;
                break;
            }
        }
    }
    res[R_KIND] = kind;
    res[R_COUNT] = total;
    res[R_END] = e;
    res[R_BS] = bs;
    for (u32 i = 0; i < 4u; i++) res[R_STATS + i] = st[i];
}

__global__ __launch_bounds__(64) void k_bamwalk_replay(WalkSrc S, u32 n_groups, const u64 *__restrict__ gentry, u64 *__restrict__ centry,
                                                       u32 *__restrict__ ccnt) {
    const u32 gi = blockIdx.x * 64u + threadIdx.x;
    if (gi >= n_groups) return;
    const u32 g = S.c0 / WALK_G + gi, cb = gi == 0 ? S.c0 : g * WALK_G, ce = min((g + 1u) * WALK_G, S.nch);
    u64 e = gentry[gi];
    bool good = true;
    for (u32 c = cb; c < ce; c++) {
        ChunkStep r{e, 0u, hw::W_OK, 0u, VIA_PASS};
        if (good) r = chunk_step(S, c, e);
        good = good && r.kind == hw::W_OK;  // (the chain has been walked to its end: it holds)
        centry[c - S.c0] = e;
        ccnt[c - S.c0] = good ? r.cnt : 0u;
        e = r.e;
    }
}

__global__ __launch_bounds__(64) void k_bamwalk_emit(WalkSrc S, const u64 *__restrict__ centry, const u32 *__restrict__ ccnt,
                                                     const u64 *__restrict__ cbase, u64 n_rec, u64 *__restrict__ rec_off) {
    const u32 ci = blockIdx.x * 64u + threadIdx.x;
    if (ci >= S.nch - S.c0) return;
    const u64 base = cbase[ci];
    const u32 k = (u32)min((u64)ccnt[ci], n_rec - min(base, n_rec));  // (the counts sum to n_rec: nothing is written behind the array)
    u64 e = centry[ci];
    u64 *const out = rec_off + base;
    for (u32 i = 0; i < k && e < S.n_bytes; i++) {
        uint64_t next = e;
        u32 bs;
        out[i] = e;
        if (hw::step(S.bytes, S.n_bytes, e, &next, &bs) != hw::W_OK) break;
        e = next;
    }
}

int broken(pp_ctx *ctx, u32 kind, u64 n, u64 at, u32 bs, u64 n_bytes, uint64_t *n_rec, uint64_t *end) {
    size_t cap = 0;
    char *msg = pp_bam_msg_buf_(&cap);
    hw::walk_message(msg, cap, kind, n, at, bs, n_bytes);
    *n_rec = n;
    *end = at;
    return ctx->fail(PP_ERR_ARG, "pp_bam_walk_device: %s", msg);
}

}  // namespace

extern "C" void pp_bam_offs_free(pp_bam_offs *o) { delete o; }

extern "C" const uint64_t *pp_bam_offs_dev(const pp_bam_offs *o) { return o ? (const uint64_t *)o->d_off : nullptr; }

extern "C" uint64_t pp_bam_offs_count(const pp_bam_offs *o) { return o ? o->n_rec : 0; }

extern "C" int pp_bam_offs_kernel_ms(const pp_bam_offs *o, float *ms) {
    return o ? o->t.total(o->ctx, "pp_bam_offs_kernel_ms", "when the chain was walked", ms) : PP_ERR_ARG;
}

// (internal hooks, not part of the header: the tests and tools/bam_walk_timing.py) the same time by stage: the chunk tables | groups,
// chain and replay | scan and offsets; the bytes per chunk, the offsets of a zone, the chunks per group; the path counts
extern "C" int pp_bam_offs_stage_ms_(const pp_bam_offs *o, float *ms3) { return o ? o->t.stages(ms3) : PP_ERR_ARG; }

extern "C" void pp_bam_walk_geometry_(uint32_t *chunk, uint32_t *zone, uint32_t *group) {
    if (chunk) *chunk = WALK_C;
    if (zone) *zone = WALK_Z;
    if (group) *group = WALK_G;
}

extern "C" int pp_bam_offs_stats_(const pp_bam_offs *o, uint64_t out[4]) {
    if (!o || !out) return PP_ERR_ARG;
    for (int i = 0; i < 4; i++) out[i] = o->stats[i];
    return PP_OK;
}

extern "C" int pp_bam_walk_device(pp_ctx *ctx, const uint8_t *bytes, uint64_t n_bytes, uint64_t from, int mem, pp_bam_offs **out,
                                  uint64_t *n_rec, uint64_t *end) {
    if (!ctx) return PP_ERR_ARG;
    if (int rdy = pp_ctx_wait(ctx)) return rdy;
    if (out) *out = nullptr;
    if (n_rec) *n_rec = 0;
    if (end) *end = from;
    size_t mcap = 0;
    pp_bam_msg_buf_(&mcap)[0] = 0;
    if (!out || !n_rec || !end) return ctx->fail(PP_ERR_ARG, "pp_bam_walk_device: null argument");
    if (mem != PP_MEM_HOST && mem != PP_MEM_DEVICE)
        return ctx->fail(PP_ERR_ARG, "pp_bam_walk_device: the bytes must be host memory or memory of the context's device");
    if (n_bytes && !bytes) return ctx->fail(PP_ERR_ARG, "pp_bam_walk_device: null bytes with n_bytes > 0");
    if (from > n_bytes) return broken(ctx, hw::W_START, 0, from, 0, n_bytes, n_rec, end);
    if (n_bytes >= (1ull << 40)) return ctx->fail(PP_ERR_LIMIT, "pp_bam_walk_device: 2^40 or more bytes in one call");
    PP_HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;

    std::unique_ptr<pp_bam_offs> P(new pp_bam_offs(ctx));
    CallScratch T;  // the copy of host bytes and the tables: released when the call returns
    StageTimer timer(ctx, ctx->profiling != 0);
    int rc;
    if (from == n_bytes) {  // nothing to walk: no records, and with profiling no time
        if ((rc = P->alloc(P->d_off, 0))) return rc;
        PP_HIPCHK(ctx, hipStreamSynchronize(st));
        P->end = from;
        if ((rc = P->t.take(timer))) return rc;
        *out = P.release();
        return PP_OK;
    }
    WalkSrc S{};
    S.n_bytes = n_bytes;
    S.from = from;
    S.c0 = (u32)(from / WALK_C);  // < nch: from < n_bytes
    S.nch = (u32)((n_bytes + WALK_C - 1u) / WALK_C);
    if ((rc = on_device(ctx, T, mem, (const u8 *)bytes, (size_t)n_bytes, &S.bytes))) return rc;
    const u32 n_tab = S.nch - S.c0 - 1u;  // chunks with a table
    const u32 g0 = S.c0 / WALK_G, n_groups = (S.nch + WALK_G - 1u) / WALK_G - g0, n_gtab = n_groups - 1u;
    const u32 n_chunks = S.nch - S.c0;
    void *d_zone, *d_gtab, *d_gentry, *d_res, *d_centry, *d_ccnt, *d_cbase;
    if ((rc = T.get(ctx, &d_zone, (size_t)n_tab * WALK_Z * 4)) || (rc = T.get(ctx, &d_gtab, (size_t)n_gtab * WALK_Z * sizeof(GroupEntry))) ||
        (rc = T.get(ctx, &d_gentry, (size_t)n_groups * 8)) || (rc = T.get(ctx, &d_res, R_WORDS * 8)) || (rc = T.get(ctx, &d_centry, (size_t)n_chunks * 8)) ||
        (rc = T.get(ctx, &d_ccnt, (size_t)n_chunks * 4)) || (rc = T.get(ctx, &d_cbase, ((size_t)n_chunks + 1) * 8)))
        return rc;
    S.zone = (const u32 *)d_zone;
    pp::DevBuf b_sums, b_sums_off;
    struct Free {
        pp::DevBuf &a, &b;
        ~Free() { pp::dev_free(a); pp::dev_free(b); }
    } free_sums{b_sums, b_sums_off};

    // ---- the chunk tables, the chain ----
    if ((rc = timer.begin(0))) return rc;
    if (n_tab) hipLaunchKernelGGL(k_bamwalk_chunk, dim3(n_tab), dim3(64), 0, st, S.bytes, (u64)n_bytes, S.c0 + 1u, (u32 *)d_zone);
    if ((rc = timer.end()) || (rc = timer.begin(1))) return rc;
    if (n_gtab)
        hipLaunchKernelGGL(k_bamwalk_group, dim3((unsigned)(((u64)n_gtab * WALK_Z + 255u) / 256u)), dim3(256), 0, st, S, g0 + 1u, n_gtab, (GroupEntry *)d_gtab);
    hipLaunchKernelGGL(k_bamwalk_chain, dim3(1), dim3(64), 0, st, S, (const GroupEntry *)d_gtab, (u64 *)d_gentry, (u64 *)d_res);
    if ((rc = timer.end())) return rc;
    PP_HIPCHK(ctx, hipGetLastError());
    u64 res[R_WORDS];
    if ((rc = fetch(ctx, d_res, res, R_WORDS))) return rc;  // (the stream is synchronised)
    if (res[R_KIND] != hw::W_OK) return broken(ctx, (u32)res[R_KIND], res[R_COUNT], res[R_END], (u32)res[R_BS], n_bytes, n_rec, end);
    const u64 n = res[R_COUNT];
    if (n >= 0xFFFFFFFFull) return ctx->fail(PP_ERR_LIMIT, "more than 2^32-1 alignments in one batch");

    // ---- every chunk's entry and count, the offsets ----
    if ((rc = P->alloc(P->d_off, (size_t)n))) return rc;
    if ((rc = timer.begin(1))) return rc;
    hipLaunchKernelGGL(k_bamwalk_replay, dim3((n_groups + 63u) / 64u), dim3(64), 0, st, S, n_groups, (const u64 *)d_gentry, (u64 *)d_centry, (u32 *)d_ccnt);
    if ((rc = timer.end()) || (rc = timer.begin(2))) return rc;
    if ((rc = scan_u32<u64>(ctx, b_sums, b_sums_off, (const u32 *)d_ccnt, (u64)n_chunks, (u64 *)d_cbase))) return rc;
    hipLaunchKernelGGL(k_bamwalk_emit, dim3((n_chunks + 63u) / 64u), dim3(64), 0, st, S, (const u64 *)d_centry, (const u32 *)d_ccnt, (const u64 *)d_cbase,
                       (u64)n, (u64 *)P->d_off);
    if ((rc = timer.end())) return rc;
    PP_HIPCHK(ctx, hipGetLastError());
    PP_HIPCHK(ctx, hipStreamSynchronize(st));  // host bytes may be released, the scratch goes away
    if ((rc = P->t.take(timer))) return rc;
    P->n_rec = n;
    P->end = res[R_END];
    for (int i = 0; i < 4; i++) P->stats[i] = res[R_STATS + i];
    *out = P.release();
    *n_rec = n;
    *end = res[R_END];
    return PP_OK;
}
