// pp_dev.h -- what the device translation units share that is not text: the typedefs, the range and room arithmetic of a batch,
// the SEQ byte codes, the workgroup scans over the DPP wave scan of pp_wave.h, the multi-block exclusive scan, the host
// plumbing of one call (read-back, scratch, upload, stage timing), and the host side of the record chain's owned objects (the
// owner of their device memory, their stage times, the named arrays of a batch, a caller's batch checked and uploaded).  Included
// by pp_devtext.h (the SAM tokenizers' text utilities), by pp_textin.h (a borrowed text's: pp_sam_out.hip, pp_sam_bam.hip, pp_tabix.hip) and
// directly by the record chain: pp_bgzf.hip, pp_bgzf_deflate.hip,
// pp_bam.hip, pp_bam_walk.hip, pp_bam_out.hip, pp_names.hip, pp_filter_rec.hip and pp_regroup.hip (through pp_filter_group.h), pp_bam_sort.hip (through pp_rg_sort.h),
// pp_gate.hip and pp_prepare.hip, and by the units that make text from finished work: pp_fasta_out.hip and pp_polish_text.hip (the
// polish's TSV, VCF, BED and soft mask), both also through pp_cut16.h.  Everything lives in an anonymous namespace: each translation unit gets its own copies, and of
// the kernels that are templates only those it launches.
#pragma once
#include "pp_internal.h"
#include "pp_wave.h"

#include <algorithm>
#include <memory>
#include <vector>

namespace {

typedef unsigned long long u64;
typedef uint32_t u32;
typedef uint8_t u8;

__device__ __forceinline__ void report(u64 *status, u64 key) { atomicMin(status, key); }

// does [off, off + len) lie inside an array of `size` elements?  (no sum that could wrap)
__device__ __forceinline__ bool inside(u64 off, u32 len, u64 size) { return off <= size && (u64)len <= size - off; }

// the room of a read of `len` SEQ bytes in a batch's seq array: in units of PP_SEQ_ALIGN bytes, and in bytes
__device__ __forceinline__ u64 room_units(u64 len) { return (len + (u64)PP_SEQ_ALIGN - 1u) / (u64)PP_SEQ_ALIGN; }
__device__ __forceinline__ u64 room_bytes(u64 len) { return (len + (u64)PP_SEQ_ALIGN - 1u) & ~((u64)PP_SEQ_ALIGN - 1u); }

// ---- the complement of an upper-cased base: the tokenizer's k_tok_seq and the record gate's k_gate_seq fill a "*" record on the other
// strand with it ----------------------------------------------------------------------------------------
__device__ __forceinline__ u8 comp_upper(u8 c) {  // misc.rs:170-182 on the upper-cased base
    switch (c) {
    case 'A': return 'T'; case 'T': return 'A'; case 'G': return 'C'; case 'C': return 'G';
    case 'R': return 'Y'; case 'Y': return 'R'; case 'S': return 'S'; case 'W': return 'W';
    case 'K': return 'M'; case 'M': return 'K'; case 'B': return 'V'; case 'V': return 'B';
    case 'D': return 'H'; case 'H': return 'D'; case 'N': return 'N'; case '.': return '.';
    case '-': return '-'; case '?': return '?'; default: return 'N';
    }
}

// ---- the 4-bit mirror of SEQ bytes (pp_aln_batch.seq4), packed while the bytes are in registers (the tokenizer's k_tok_seq,
// pp_batch_prepare's k_prep_copy) ----------------------------------------------------------------------
__device__ __forceinline__ u32 seq4_code(u32 c) {
    const u32 t = (c >> 1) & 3u;  // A->0 C->1 T->2 G->3: the counter rows
    const u32 expect = (0x47544341u >> (t * 8u)) & 0xFFu;
    return c == expect ? t : (c == (u32)'N' ? (u32)PP_SEQ4_N : (c == (u32)'-' ? (u32)PP_SEQ4_DASH : (u32)PP_SEQ4_OTHER));
}
__device__ __forceinline__ uint2 pack4_16(const u32 w[4]) {  // 16 bytes -> 16 nibbles
    u32 o[2];
#pragma unroll
    for (int q = 0; q < 2; q++) {
        u32 v = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) v |= seq4_code((w[2 * q + (j >> 2)] >> (8 * (j & 3))) & 0xFFu) << (4 * j);
        o[q] = v;
    }
    return make_uint2(o[0], o[1]);
}

// ---- scans over one workgroup ----------------------------------------------------------------------------
// Exclusive prefix of v over the workgroup's BLOCK threads, *total = the workgroup's sum: the DPP wave scan, the waves' sums
// through LDS.  Every thread of the workgroup calls it; s_w has BLOCK / 64 words and may be used again after the return.
template <u32 BLOCK>
__device__ __forceinline__ u32 block_scan_excl(u32 v, u32 *s_w, u32 *total) {
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const u32 inc = pp::wave_scan_incl(v);
    if (lane == 63u) s_w[wave] = inc;
    __syncthreads();
    u32 before = 0, sum = 0;
#pragma unroll
    for (u32 i = 0; i < BLOCK / 64u; i++) {
        const u32 w = s_w[i];
        before += i < wave ? w : 0u;
        sum += w;
    }
    __syncthreads();  // (s_w is used again)
    *total = sum;
    return before + inc - v;
}
// ... of values whose sum over a workgroup does not fit 32 bits (rooms, CIGAR runs, pool words): v = hi << 16 | lo, the two
// halves scanned apart
template <u32 BLOCK>
__device__ __forceinline__ u64 block_scan_excl64(u32 v, u64 *s_w, u64 *total) {
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const u64 inc = ((u64)pp::wave_scan_incl(v >> 16) << 16) + (u64)pp::wave_scan_incl(v & 0xFFFFu);
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
    return before + inc - (u64)v;
}

// exclusive scan of the workgroups' C sums, column by column (one workgroup of 1024 threads; in: nb rows of C words, out: nb + 1)
template <u32 C>
__global__ __launch_bounds__(1024) void k_colscan(const u64 *__restrict__ in, u64 nb, u64 *__restrict__ out) {
    __shared__ u64 part[1024];
    const u32 t = threadIdx.x;
    const u64 per = (nb + 1023) / 1024;
    const u64 lo = min(nb, (u64)t * per), hi = min(nb, lo + per);
    for (u32 c = 0; c < C; c++) {
        u64 s = 0;
        for (u64 i = lo; i < hi; i++) s += in[C * i + c];
        part[t] = s;
        __syncthreads();
        for (u32 off = 1; off < 1024; off <<= 1) {
            const u64 v = (t >= off) ? part[t - off] : 0;
            __syncthreads();
            part[t] += v;
            __syncthreads();
        }
        u64 run = part[t] - s;
        for (u64 i = lo; i < hi; i++) {
            const u64 v = in[C * i + c];
            out[C * i + c] = run;
            run += v;
        }
        if (t == 1023) out[C * nb + c] = part[1023];
        __syncthreads();
    }
}

// ---- exclusive scan: u32 in -> T out (n + 1 entries) -- block sums, a single-block scan of the sums,
// then every block scans its own 8192 elements on top of its base ------------------------------------
constexpr u32 SCAN_PER_BLOCK = 1024 * 8;

__global__ __launch_bounds__(1024) void k_scan_sums(const u32 *__restrict__ in, u64 n, u32 *__restrict__ sums) {
    __shared__ u32 s_sum;
    if (threadIdx.x == 0) s_sum = 0;
    __syncthreads();
    const u64 base = (u64)blockIdx.x * SCAN_PER_BLOCK + (u64)threadIdx.x * 8u;
    u32 v = 0;
#pragma unroll
    for (u32 i = 0; i < 8; i++)
        if (base + i < n) v += in[base + i];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63u) == 0 && v) atomicAdd(&s_sum, v);
    __syncthreads();
    if (threadIdx.x == 0) sums[blockIdx.x] = s_sum;
}

template <typename T>
__global__ __launch_bounds__(1024) void k_tscan(const u32 *__restrict__ in, u64 n, T *__restrict__ out) {
    __shared__ u64 part[1024];
    const u32 t = threadIdx.x;
    const u64 per = (n + 1023) / 1024;
    const u64 lo = min(n, (u64)t * per), hi = min(n, lo + per);
    u64 s = 0;
    for (u64 i = lo; i < hi; i++) s += in[i];
    part[t] = s;
    __syncthreads();
    for (u32 off = 1; off < 1024; off <<= 1) {
        const u64 v = (t >= off) ? part[t - off] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    u64 run = part[t] - s;
    for (u64 i = lo; i < hi; i++) {
        out[i] = (T)run;
        run += in[i];
    }
    if (t == 1023) out[n] = (T)part[1023];
}

template <typename T>
__global__ __launch_bounds__(1024) void k_scan_apply(const u32 *__restrict__ in, u64 n, const u64 *__restrict__ sums_off,
                                                     T *__restrict__ out) {
    __shared__ u32 s_w[16];
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const u64 base = (u64)blockIdx.x * SCAN_PER_BLOCK + (u64)threadIdx.x * 8u;
    u32 v[8], sum = 0;
#pragma unroll
    for (u32 i = 0; i < 8; i++) {
        v[i] = base + i < n ? in[base + i] : 0u;
        sum += v[i];
    }
    u32 inc = sum;
    for (int o = 1; o < 64; o <<= 1) {
        const u32 t = __shfl_up(inc, o, 64);
        if ((int)lane >= o) inc += t;
    }
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    u64 run = sums_off[blockIdx.x] + (inc - sum);
    for (u32 i = 0; i < wave; i++) run += s_w[i];
#pragma unroll
    for (u32 i = 0; i < 8; i++) {
        if (base + i < n) out[base + i] = (T)run;
        run += v[i];
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) out[n] = (T)sums_off[gridDim.x];
}

// out[0..n] = exclusive scan of in[0..n); scratch: two small device buffers for the block sums
template <typename T>
int scan_u32(pp_ctx *ctx, pp::DevBuf &b_sums, pp::DevBuf &b_sums_off, const u32 *in, u64 n, T *out) {
    const u64 nb = std::max<u64>(1, (n + SCAN_PER_BLOCK - 1) / SCAN_PER_BLOCK);
    if (int rc = pp::dev_ensure(ctx, b_sums, nb * 4)) return rc;
    if (int rc = pp::dev_ensure(ctx, b_sums_off, (nb + 1) * 8)) return rc;
    hipLaunchKernelGGL(k_scan_sums, dim3((unsigned)nb), dim3(1024), 0, ctx->stream, in, n, (u32 *)b_sums.p);
    hipLaunchKernelGGL(k_tscan<u64>, dim3(1), dim3(1024), 0, ctx->stream, (const u32 *)b_sums.p, nb, (u64 *)b_sums_off.p);
    hipLaunchKernelGGL(k_scan_apply<T>, dim3((unsigned)nb), dim3(1024), 0, ctx->stream, in, n, (const u64 *)b_sums_off.p, out);
    return PP_OK;
}

// ---- the host side of one call ---------------------------------------------------------------------------
template <typename T>
int fetch(pp_ctx *ctx, const void *dev, T *host, size_t n = 1) {
    PP_HIPCHK(ctx, hipMemcpyAsync(host, dev, n * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
    PP_HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PP_OK;
}

struct CallScratch {  // device memory of one call, released when it returns
    std::vector<void *> p;
    CallScratch() = default;
    CallScratch(const CallScratch &) = delete;
    CallScratch &operator=(const CallScratch &) = delete;
    ~CallScratch() { for (void *q : p) (void)hipFree(q); }
    int get(pp_ctx *ctx, void **out, size_t bytes) {
        *out = nullptr;
        PP_HIPCHK(ctx, hipMalloc(out, std::max<size_t>(bytes, 16)));
        p.push_back(*out);
        return PP_OK;
    }
    template <class T>
    int alloc(pp_ctx *ctx, T *&a, size_t count) {  // get(), typed: `count` elements
        void *q;
        const int rc = get(ctx, &q, count * sizeof(T));
        a = (T *)q;
        return rc;
    }
};

// A call's device memory out of grow-only buffers of the context (pp_ctx::f_rec, g_rec), handed out in the order of the requests:
// the same request of the next call finds its buffer again.  Nothing in them outlives the call.  [0], [1]: scan_u32's block sums
struct CtxScratch {
    pp_ctx *ctx;
    pp::DevBuf *buf;
    size_t n_buf, k = 2;
    const char *who;
    template <size_t N>
    CtxScratch(pp_ctx *c, pp::DevBuf (&b)[N], const char *w) : ctx(c), buf(b), n_buf(N), who(w) {}
    pp::DevBuf &sums() { return buf[0]; }
    pp::DevBuf &sums_off() { return buf[1]; }
    int get(pp_ctx *, void **out, size_t bytes) {
        *out = nullptr;
        if (k >= n_buf) return ctx->fail(PP_ERR_HIP, "%s: out of buffer slots", who);
        if (int rc = pp::dev_ensure(ctx, buf[k], std::max<size_t>(bytes, 16))) return rc;
        *out = buf[k++].p;
        return PP_OK;
    }
};

// The base of the record chain's C objects: the context and the device memory the object owns, freed with it.  A creator holds the
// object in a std::unique_ptr until it hands it out: every early return frees what was made so far.  (Its get() is CallScratch's:
// on_device uploads into the object.)
struct DevOwner : CallScratch {
    pp_ctx *const ctx;
    explicit DevOwner(pp_ctx *c) : ctx(c) {}
    ~DevOwner() { (void)hipSetDevice(ctx->device); }  // (in front of the base's hipFree)
    template <class T>
    int alloc(T *&a, size_t count) { return CallScratch::alloc(ctx, a, count); }
    void release(const void *a) {  // one allocation early; an array that is not the object's is left alone
        const auto it = std::find(p.begin(), p.end(), a);
        if (it == p.end()) return;
        (void)hipFree(*it);
        p.erase(it);
    }
};

// `count` elements of a caller's array where the kernels can read them: device memory as it is, host memory copied into a buffer
// of `scratch` (anything with get(ctx, void **, bytes)) on the context's stream
template <class S, class T>
int on_device(pp_ctx *ctx, S &scratch, int mem, const T *src, size_t count, const T **dev) {
    if (mem == PP_MEM_DEVICE) {
        *dev = src;
        return PP_OK;
    }
    void *d;
    if (int rc = scratch.get(ctx, &d, count * sizeof(T))) return rc;
    if (count) PP_HIPCHK(ctx, hipMemcpyAsync(d, src, count * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    *dev = (const T *)d;
    return PP_OK;
}

// HIP-event time of one call's kernels by stage: begin(stage) ... end() around a stretch of launches on the context's stream, as
// often as the call likes; sums() once the stream is synchronised.  Off (a context without profiling), every call does nothing.
struct StageTimer {
    pp_ctx *ctx;
    bool on;
    std::vector<hipEvent_t> ev;  // pairs around the call's spans ...
    std::vector<int> stage;      // ... and the stage each pair belongs to
    StageTimer(pp_ctx *c, bool o) : ctx(c), on(o) {}
    StageTimer(const StageTimer &) = delete;
    StageTimer &operator=(const StageTimer &) = delete;
    ~StageTimer() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
    int begin(int s) {
        if (!on) return PP_OK;
        for (int i = 0; i < 2; i++) {  // (both events before the span opens)
            hipEvent_t e = nullptr;
            PP_HIPCHK(ctx, hipEventCreate(&e));
            ev.push_back(e);
        }
        stage.push_back(s);
        PP_HIPCHK(ctx, hipEventRecord(ev[ev.size() - 2], ctx->stream));
        return PP_OK;
    }
    int end() {
        if (on) PP_HIPCHK(ctx, hipEventRecord(ev.back(), ctx->stream));
        return PP_OK;
    }
    int sums(float *ms, int n_stages) {  // ms[s] = the time of the spans of stage s
        for (int s = 0; s < n_stages; s++) ms[s] = 0.f;
        for (size_t i = 0; i < stage.size(); i++) {
            float t = 0.f;
            PP_HIPCHK(ctx, hipEventElapsedTime(&t, ev[2 * i], ev[2 * i + 1]));
            ms[stage[i]] += t;
        }
        return PP_OK;
    }
};

// The time of an object's kernels by stage, kept when the context had profiling on.
template <int K>
struct StageMs {
    bool timed = false;
    float ms[K] = {};
    int take(StageTimer &t) {  // (once the stream is synchronised)
        if (!t.on) return PP_OK;
        if (int rc = t.sums(ms, K)) return rc;
        timed = true;
        return PP_OK;
    }
    // pp_X_kernel_ms: the stages from `first` on; `when` finishes the sentence of an object made without profiling
    int total(pp_ctx *ctx, const char *who, const char *when, float *out, int first = 0) const {
        if (!out) return PP_ERR_ARG;
        if (!timed) return ctx->fail(PP_ERR_ARG, "%s: the context had no profiling on %s (pp_ctx_set_profiling)", who, when);
        *out = 0.f;
        for (int i = first; i < K; i++) *out += ms[i];
        return PP_OK;
    }
    int stages(float *out) const {  // pp_X_stage_ms_
        if (!out || !timed) return PP_ERR_ARG;
        std::copy(ms, ms + K, out);
        return PP_OK;
    }
};

// ---- the arrays of a batch: an object's own, and a caller's made device-readable -----------------------------
struct RawArrays {  // pp_raw_batch
    uint16_t *flag = nullptr;
    u64 *read_id = nullptr, *seq_off = nullptr, *cig_off = nullptr;
    u32 *contig = nullptr, *ref_start = nullptr, *nm = nullptr, *seq_len = nullptr, *n_cig = nullptr, *cigar = nullptr;
    u8 *seq = nullptr;
    int alloc_records(DevOwner &o, size_t n) {  // the nine arrays per record
        int rc;
        if ((rc = o.alloc(flag, n)) || (rc = o.alloc(read_id, n)) || (rc = o.alloc(contig, n)) || (rc = o.alloc(ref_start, n)) ||
            (rc = o.alloc(nm, n)) || (rc = o.alloc(seq_off, n)) || (rc = o.alloc(seq_len, n)) || (rc = o.alloc(cig_off, n)))
            return rc;
        return o.alloc(n_cig, n);
    }
    pp_raw_batch view(u64 n, u64 seq_bytes, u64 n_cig_total) const {
        return pp_raw_batch{n, flag, (const uint64_t *)read_id, contig, ref_start, nm, (const uint64_t *)seq_off, seq_len,
                            (const uint64_t *)cig_off, n_cig, seq, seq_bytes, cigar, n_cig_total};
    }
};

struct AlnArrays {  // pp_aln_batch without its mirrors
    u32 *contig = nullptr, *ref_start = nullptr, *k = nullptr, *seq_len = nullptr, *n_cig = nullptr, *cigar = nullptr;
    u64 *seq_off = nullptr, *cig_off = nullptr;
    u8 *seq = nullptr;
    int alloc_records(DevOwner &o, size_t n) {  // the seven arrays per record
        int rc;
        if ((rc = o.alloc(contig, n)) || (rc = o.alloc(ref_start, n)) || (rc = o.alloc(k, n)) || (rc = o.alloc(seq_off, n)) ||
            (rc = o.alloc(seq_len, n)) || (rc = o.alloc(cig_off, n)))
            return rc;
        return o.alloc(n_cig, n);
    }
    pp_aln_batch view(u64 n, u64 seq_bytes, u64 n_cig_total) const {
        pp_aln_batch V{};
        V.n_aln = n;
        V.contig = contig; V.ref_start = ref_start; V.k = k; V.seq_off = (const uint64_t *)seq_off; V.seq_len = seq_len;
        V.cig_off = (const uint64_t *)cig_off; V.n_cig = n_cig; V.seq = seq; V.seq_bytes = seq_bytes; V.cigar = cigar;
        V.n_cig_total = n_cig_total;
        return V;
    }
};

// What a callee reads of a caller's raw batch beyond flag, read_id, contig, ref_start, cig_off and n_cig
enum : u32 { RAW_READS = 1 /* nm seq_off seq_len */, RAW_SEQ = 2, RAW_CIGAR = 4, RAW_ALL = 7, RAW_SEQ_LIMIT = 8 /* refuse 2^40 SEQ bytes */ };

// the refusals every taker of a raw batch shares, in the order and with the sentences they always had
int raw_check(pp_ctx *ctx, const char *who, const pp_raw_batch *raw, int mem, u32 which) {
    if (mem != PP_MEM_HOST && mem != PP_MEM_DEVICE)
        return ctx->fail(PP_ERR_ARG, "%s: the batch must be host memory or memory of the context's device", who);
    if (raw->n_rec >= 0xFFFFFFFFull) return ctx->fail(PP_ERR_LIMIT, "more than 2^32-1 alignments in one batch");
    if ((which & RAW_SEQ_LIMIT) && raw->seq_bytes >= (1ull << 40)) return ctx->fail(PP_ERR_LIMIT, "more than 2^40 SEQ bytes in one batch");
    const bool reads = (which & RAW_READS) != 0;
    if (raw->n_rec && (!raw->flag || !raw->read_id || !raw->contig || !raw->ref_start || !raw->cig_off || !raw->n_cig ||
                       (reads && (!raw->nm || !raw->seq_off || !raw->seq_len)) || ((which & RAW_SEQ) && raw->seq_bytes && !raw->seq) ||
                       ((which & RAW_CIGAR) && raw->n_cig_total && !raw->cigar)))
        return ctx->fail(PP_ERR_ARG, "%s: null array in a non-empty batch", who);
    return PP_OK;
}

// *dev = the batch with the arrays of `which` where the kernels can read them (on_device: uploads go to `scratch`), the others
// null.  The order of the uploads is pp_filter_records's: its scratch is the context's, found again by that order.
template <class S>
int raw_on_device(pp_ctx *ctx, S &scratch, int mem, const pp_raw_batch *raw, u32 which, pp_raw_batch *dev) {
    const size_t n = (size_t)raw->n_rec;
    *dev = pp_raw_batch{};
    dev->n_rec = raw->n_rec;
    dev->seq_bytes = raw->seq_bytes;
    dev->n_cig_total = raw->n_cig_total;
    int rc;
    if ((rc = on_device(ctx, scratch, mem, raw->flag, n, &dev->flag)) || (rc = on_device(ctx, scratch, mem, raw->read_id, n, &dev->read_id)) ||
        (rc = on_device(ctx, scratch, mem, raw->cig_off, n, &dev->cig_off)) || (rc = on_device(ctx, scratch, mem, raw->contig, n, &dev->contig)) ||
        (rc = on_device(ctx, scratch, mem, raw->ref_start, n, &dev->ref_start)) || (rc = on_device(ctx, scratch, mem, raw->n_cig, n, &dev->n_cig)))
        return rc;
    if ((which & RAW_READS) && ((rc = on_device(ctx, scratch, mem, raw->nm, n, &dev->nm)) || (rc = on_device(ctx, scratch, mem, raw->seq_off, n, &dev->seq_off)) ||
                                (rc = on_device(ctx, scratch, mem, raw->seq_len, n, &dev->seq_len))))
        return rc;
    if ((which & RAW_SEQ) && (rc = on_device(ctx, scratch, mem, raw->seq, (size_t)raw->seq_bytes, &dev->seq))) return rc;
    if ((which & RAW_CIGAR) && (rc = on_device(ctx, scratch, mem, raw->cigar, (size_t)raw->n_cig_total, &dev->cigar))) return rc;
    return PP_OK;
}

// ... and the nine arrays of a caller's pp_aln_batch (the mirrors are not read)
template <class S>
int aln_on_device(pp_ctx *ctx, S &scratch, int mem, const pp_aln_batch *b, pp_aln_batch *dev) {
    const size_t n = (size_t)b->n_aln;
    *dev = pp_aln_batch{};
    dev->n_aln = b->n_aln;
    dev->seq_bytes = b->seq_bytes;
    dev->n_cig_total = b->n_cig_total;
    int rc;
    if ((rc = on_device(ctx, scratch, mem, b->contig, n, &dev->contig)) || (rc = on_device(ctx, scratch, mem, b->ref_start, n, &dev->ref_start)) ||
        (rc = on_device(ctx, scratch, mem, b->k, n, &dev->k)) || (rc = on_device(ctx, scratch, mem, b->seq_off, n, &dev->seq_off)) ||
        (rc = on_device(ctx, scratch, mem, b->seq_len, n, &dev->seq_len)) || (rc = on_device(ctx, scratch, mem, b->cig_off, n, &dev->cig_off)) ||
        (rc = on_device(ctx, scratch, mem, b->n_cig, n, &dev->n_cig)) || (rc = on_device(ctx, scratch, mem, b->seq, (size_t)b->seq_bytes, &dev->seq)))
        return rc;
    return on_device(ctx, scratch, mem, b->cigar, (size_t)b->n_cig_total, &dev->cigar);
}

}  // namespace
