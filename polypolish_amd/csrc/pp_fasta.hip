// pp_fasta.hip -- pp_fasta_records: FASTA TEXT as contig bases in device memory, the device twin of load_fasta (pp_ingest.cpp), as
// pp_sam_records (pp_sam.hip) is the twin of the SAM ingest.  The text is read where it is (device memory at any alignment; host memory
// through one staging copy), once by each of the two passes; the object owns the bases and the contig table and nothing else.
//
// The geometry (pp_fasta_geometry_; the tests aim at these seams).  A lane takes FA_LANE = 16 bytes with one wide load, a workgroup of 256
// lanes a TILE of 4096 bytes at a time and FA_TILES = 16 tiles one after the other: WG = 65536 bytes.  Tiles are cut at multiples of 16
// bytes of ADDRESS: with shift = address of the text & 15, tile seams lie at the text offsets k * TILE - shift.  A 16-byte piece that
// is not wholly inside [0, n_bytes) is loaded byte by byte, each byte behind the test against n_bytes: no byte outside the text is
// loaded, by a wide load either.  Positions outside the text count as '\n': the text begins at a line start, a '\r' that is the text's
// last byte is dropped like one in front of a '\n' (LineReader of pp_ingest.cpp), and nothing behind n_bytes can be a base.
//
// What a byte is depends on the first byte of its line, which may lie any number of tiles back (a chromosome on one line).  So:
//   k_fasta<false>  per workgroup, with nothing known about the line that is open where it begins: the bases behind its first line start
//                   (cnt), the bytes in front of it that are bases if that line is a sequence line (pend), the header lines, and the two
//                   states it leaves behind: the kind of the open line, whether a NAMED header is open (inherit where it holds no line
//                   start, no header)
//   k_fasta_scan    one workgroup: the exclusive scan of those sums under the monoid that resolves `pend` and `inherit`; its first
//                   element is definite (the text begins at a line start, no header open), so every prefix is
//   k_fasta<true>   per workgroup with its definite prefix: the bases compacted and upper-cased -- through LDS, stored with 16-byte
//                   stores wherever 16 bytes of the destination are the tile's own --, per header line its offset and the bases in
//                   front of it, and the first offending sequence byte by atomicMin (offset << 8 | kind): a base with no named header
//                   open, a byte >= 0x80
// Inside a tile the states travel by ballot (the last lane below with a line start), across a workgroup's waves through LDS, across
// its tiles in registers.  A "\r\n" cut by a seam: every lane loads the byte behind its 16, guarded.
//   k_fasta_hdr_len / k_fasta_hdr_gather   one wave per header line: its end, then its bytes packed for one download
// The host part (pp_fasta_host.h) sees the header lines only; an offending line is found on the device, downloaded, and judged by the
// host's words (k_fasta_locate: its bounds and its number, on that path alone).
#include "pp_dev.h"
#include "pp_fasta_host.h"

#include <cstring>

struct pp_fasta : DevOwner {
    using DevOwner::DevOwner;
    u8 *bases = nullptr;  // DEVICE, n_bases bytes
    uint64_t n_bases = 0;
    pp_fasta_host::Contigs c;
    StageMs<4> t;  // the staging copy of a host text | the sums and their scan | bases and headers | header lines
};

namespace {

constexpr u32 FA_THREADS = 256, FA_LANE = 16, FA_TILE = FA_THREADS * FA_LANE, FA_TILES = 16, FA_WG = FA_TILE * FA_TILES;
enum : u32 { K_INHERIT = 0, K_SEQ = 1, K_HDR = 2 };     // the kind of the open line
enum : u32 { H_INHERIT = 0, H_NONE = 1, H_NAMED = 2 };  // is a named header open?
enum : u32 { FR_HEADLESS = 1, FR_NOT_ASCII = 2 };       // status: offset << 8 | why the byte offends

struct FaSum {
    u64 cnt, pend, nh;
    u32 kind, have;
};

__device__ __forceinline__ FaSum fa_join(const FaSum &a, const FaSum &b) {  // a in front of b
    FaSum r;
    r.cnt = a.cnt + b.cnt + (a.kind == K_SEQ ? b.pend : 0ull);
    r.pend = a.pend + (a.kind == K_INHERIT ? b.pend : 0ull);
    r.nh = a.nh + b.nh;
    r.kind = b.kind ? b.kind : a.kind;
    r.have = b.have ? b.have : a.have;
    return r;
}

// does the header line whose '>' is text[h] have a name?  (rust_ws_len of pp_host.h on the byte behind '>': a line end, the end of the
// text or a White_Space character there leaves the name empty; bytes behind the line's end cannot complete a multi-byte form)
__device__ bool hdr_named(const u8 *__restrict__ text, u64 n, u64 h) {
    if (h + 1 >= n) return false;
    const u8 c = text[h + 1];
    if (c == (u8)' ' || (c >= 0x09 && c <= 0x0D)) return false;  // ('\n': an empty name; "\r\n" and a lone '\r' alike)
    if (c < 0xC2) return true;
    const u8 d = h + 2 < n ? text[h + 2] : (u8)0, e = h + 3 < n ? text[h + 3] : (u8)0;
    if (c == 0xC2) return !(d == 0x85 || d == 0xA0);
    if (c == 0xE1 && d == 0x9A && e == 0x80) return false;
    if (c == 0xE2 && d == 0x80 && ((e >= 0x80 && e <= 0x8A) || e == 0xA8 || e == 0xA9 || e == 0xAF)) return false;
    if (c == 0xE2 && d == 0x81 && e == 0x9F) return false;
    if (c == 0xE3 && d == 0x80 && e == 0x80) return false;
    return true;
}

__device__ __forceinline__ u8 guarded(const u8 *__restrict__ text, u64 n, long long i) {
    return (i >= 0 && (u64)i < n) ? text[i] : (u8)'\n';
}

// PLACE == false: sums[workgroup] = its FaSum.  PLACE == true: sums holds the exclusive scan; bases, hdr_off, hdr_pre and status are written.
template <bool PLACE>
__global__ __launch_bounds__(FA_THREADS) void k_fasta(const u8 *__restrict__ text, u64 n, u32 shift, FaSum *__restrict__ sums,
                                                      u8 *__restrict__ bases, u64 n_bases, u64 *__restrict__ hdr_off,
                                                      u64 *__restrict__ hdr_pre, u64 n_hdr, u64 *__restrict__ status) {
    __shared__ u32 s_k[2][FA_THREADS / 64], s_h[2][FA_THREADS / 64], s_w[FA_THREADS / 64];
    __shared__ __attribute__((aligned(16))) u8 s_out[PLACE ? FA_TILE + 32 : 16];
    const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    u32 ck = K_INHERIT, ch = H_INHERIT;  // the states in front of the tile
    u64 seq_run = 0, hdr_run = 0;        // PLACE: bases and header lines in front of the tile
    if (PLACE) {
        const FaSum in = sums[blockIdx.x];
        ck = in.kind; ch = in.have; seq_run = in.cnt; hdr_run = in.nh;
    }
    u32 a_cnt = 0, a_pend = 0, a_nh = 0;
    const u64 v_end = n + shift;
    for (u32 ti = 0; ti < FA_TILES; ti++) {
        const u64 tv = (u64)blockIdx.x * FA_WG + (u64)ti * FA_TILE;
        if (tv >= v_end) break;  // (the same for every lane)
        const long long i0 = (long long)(tv + (u64)tid * FA_LANE) - (long long)shift;
        // ---- the lane's 16 bytes, the byte in front and the byte behind ----
        u32 w[4];
        if (i0 >= 0 && (u64)i0 + FA_LANE <= n) {
            const uint4 q = *(const uint4 *)(text + i0);
            w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
        } else {
#pragma unroll
            for (u32 q = 0; q < 4; q++) {
                u32 v = 0;
#pragma unroll
                for (u32 j = 0; j < 4; j++) v |= (u32)guarded(text, n, i0 + (long long)(4 * q + j)) << (8 * j);
                w[q] = v;
            }
        }
        const u32 prev_nl = guarded(text, n, i0 - 1) == (u8)'\n', next_nl = guarded(text, n, i0 + (long long)FA_LANE) == (u8)'\n';
        u32 nl = 0, gt = 0, cr = 0, hi = 0;
#pragma unroll
        for (u32 j = 0; j < FA_LANE; j++) {
            const u32 c = (w[j >> 2] >> (8 * (j & 3))) & 0xFFu;
            nl |= (c == (u32)'\n' ? 1u : 0u) << j;
            gt |= (c == (u32)'>' ? 1u : 0u) << j;
            cr |= (c == (u32)'\r' ? 1u : 0u) << j;
            hi |= (c >> 7) << j;
        }
        const u32 ls = ((nl << 1) | prev_nl) & 0xFFFFu;          // line starts
        const u32 hs = ls & gt;                                   // header lines' starts
        const u32 drop = nl | (cr & ((nl >> 1) | (next_nl << 15)));  // line ends: "\n", and the "\r" in front of one
        u32 nm = 0;                                               // ... with a name
        for (u32 m = hs; m; m &= m - 1) {
            const u32 j = (u32)__ffs((int)m) - 1u;
            if (hdr_named(text, n, (u64)(i0 + (long long)j))) nm |= 1u << j;
        }
        // ---- the states in front of the lane ----
        const bool has_ls = ls != 0, has_hs = hs != 0;
        const u64 B_ls = __ballot(has_ls), B_k = __ballot(has_ls && ((gt >> (31 - __clz((int)ls))) & 1u));
        const u64 B_hs = __ballot(has_hs), B_n = __ballot(has_hs && ((nm >> (31 - __clz((int)hs))) & 1u));
        const u32 buf = ti & 1u;
        if (lane == 0) {
            s_k[buf][wave] = B_ls ? (((B_k >> (63 - __clzll((long long)B_ls))) & 1ull) ? (u32)K_HDR : (u32)K_SEQ) : (u32)K_INHERIT;
            s_h[buf][wave] = B_hs ? (((B_n >> (63 - __clzll((long long)B_hs))) & 1ull) ? (u32)H_NAMED : (u32)H_NONE) : (u32)H_INHERIT;
        }
        __syncthreads();
        u32 kin = ck, hin = ch;
#pragma unroll
        for (u32 i = 0; i < FA_THREADS / 64; i++) {
            const u32 k = s_k[buf][i], h = s_h[buf][i];
            if (i < wave) { kin = k ? k : kin; hin = h ? h : hin; }
            ck = k ? k : ck;  // (behind the tile)
            ch = h ? h : ch;
        }
        const u64 below = (1ull << lane) - 1ull;
        if (B_ls & below) kin = ((B_k >> (63 - __clzll((long long)(B_ls & below)))) & 1ull) ? (u32)K_HDR : (u32)K_SEQ;
        if (B_hs & below) hin = ((B_n >> (63 - __clzll((long long)(B_hs & below)))) & 1ull) ? (u32)H_NAMED : (u32)H_NONE;
        // ---- which bytes are bases ----
        u32 hm;  // bytes of header lines
        if (!has_ls) hm = kin == K_HDR ? 0xFFFFu : 0u;
        else {
            u32 cur = kin == K_HDR ? 1u : 0u;
            hm = 0;
#pragma unroll
            for (u32 j = 0; j < FA_LANE; j++) {
                cur = ((ls >> j) & 1u) ? ((gt >> j) & 1u) : cur;
                hm |= cur << j;
            }
        }
        u32 seq = ~hm & ~drop & 0xFFFFu;
        if (!PLACE) {
            const u32 front = has_ls ? ((1u << ((u32)__ffs((int)ls) - 1u)) - 1u) : 0xFFFFu;  // in front of the lane's first line start
            if (kin == K_INHERIT) {
                a_pend += (u32)__popc(seq & front);
                seq &= ~front;
            }
            a_cnt += (u32)__popc(seq);
            a_nh += (u32)__popc(hs);
            continue;
        }
        // ---- PLACE: the offending bytes ----
        u32 headless;
        if (!has_hs) headless = hin == H_NAMED ? 0u : seq;
        else {
            u32 cur = hin == H_NAMED ? 1u : 0u;
            headless = 0;
#pragma unroll
            for (u32 j = 0; j < FA_LANE; j++) {
                cur = ((hs >> j) & 1u) ? ((nm >> j) & 1u) : cur;
                headless |= (cur ^ 1u) << j;
            }
            headless &= seq;
        }
        if (headless) report(status, ((u64)(i0 + (long long)__ffs((int)headless) - 1) << 8) | FR_HEADLESS);
        if (hi & seq) report(status, ((u64)(i0 + (long long)__ffs((int)(hi & seq)) - 1) << 8) | FR_NOT_ASCII);
        // ---- the lane's bases and header lines among the tile's ----
        const u32 mine = (u32)__popc(seq), mine_h = (u32)__popc(hs);
        u32 tot;
        const u32 ex = block_scan_excl<FA_THREADS>(mine | (mine_h << 16), s_w, &tot);
        const u32 ex_c = ex & 0xFFFFu, ex_h = ex >> 16, tot_c = tot & 0xFFFFu, tot_h = tot >> 16;
        // (the two passes count alike; were they not to, nothing is stored outside the arrays and the call fails: status 0)
        const bool fits = seq_run + tot_c <= n_bases && hdr_run + tot_h <= n_hdr;
        if (!fits && tid == 0) report(status, 0ull);
        u32 k = 0;
        for (u32 m = fits ? hs : 0u; m; m &= m - 1, k++) {
            const u32 j = (u32)__ffs((int)m) - 1u;
            hdr_off[hdr_run + ex_h + k] = (u64)(i0 + (long long)j);
            hdr_pre[hdr_run + ex_h + k] = seq_run + ex_c + (u32)__popc(seq & ((1u << j) - 1u));
        }
        // the tile's bases in LDS at the destination's offset inside its 16 bytes, then out in whole pieces of 16
        const u32 a = (u32)(seq_run & 15ull);
        if (mine) {
            u32 pos = a + ex_c;
#pragma unroll
            for (u32 j = 0; j < FA_LANE; j++) {
                if ((seq >> j) & 1u) {
                    const u32 c = (w[j >> 2] >> (8 * (j & 3))) & 0xFFu;
                    s_out[pos++] = (u8)(c - ((c - (u32)'a') < 26u ? 32u : 0u));
                }
            }
        }
        __syncthreads();
        if (tot_c && fits) {
            u8 *const dst0 = bases + (seq_run - a);  // (16-byte aligned: the allocation is)
            const u32 end = a + tot_c;
            for (u32 p = tid; p * 16u < end; p += FA_THREADS) {
                const u32 lo = p * 16u;
                if (lo >= a && lo + 16u <= end) *(uint4 *)(dst0 + lo) = *(const uint4 *)(s_out + lo);
                else
                    for (u32 b = max(lo, a); b < min(lo + 16u, end); b++) dst0[b] = s_out[b];
            }
        }
        seq_run += tot_c;
        hdr_run += tot_h;
    }
    if (!PLACE) {
        u32 t_cnt, t_pend, t_nh;
        (void)block_scan_excl<FA_THREADS>(a_cnt, s_w, &t_cnt);
        (void)block_scan_excl<FA_THREADS>(a_pend, s_w, &t_pend);
        (void)block_scan_excl<FA_THREADS>(a_nh, s_w, &t_nh);
        if (tid == 0) sums[blockIdx.x] = FaSum{t_cnt, t_pend, t_nh, ck, ch};
    }
}

// out[0 .. nwg] = the exclusive scan of in[0 .. nwg) under fa_join, in front of all of it: a sequence line's kind, no header open
__global__ __launch_bounds__(1024) void k_fasta_scan(const FaSum *__restrict__ in, u64 nwg, FaSum *__restrict__ out) {
    __shared__ FaSum part[1024];
    const u32 t = threadIdx.x;
    const u64 per = (nwg + 1023) / 1024;
    const u64 lo = min(nwg, (u64)t * per), hi = min(nwg, lo + per);
    FaSum acc = t == 0 ? FaSum{0, 0, 0, K_SEQ, H_NONE} : FaSum{0, 0, 0, K_INHERIT, H_INHERIT};
    for (u64 i = lo; i < hi; i++) acc = fa_join(acc, in[i]);
    part[t] = acc;
    __syncthreads();
    for (u32 off = 1; off < 1024; off <<= 1) {
        FaSum v = part[t];
        if (t >= off) v = fa_join(part[t - off], v);
        __syncthreads();
        part[t] = v;
        __syncthreads();
    }
    FaSum run = t == 0 ? FaSum{0, 0, 0, K_SEQ, H_NONE} : part[t - 1];
    for (u64 i = lo; i < hi; i++) {
        out[i] = run;
        run = fa_join(run, in[i]);
    }
    if (t == 1023) out[nwg] = part[1023];
}

// one wave per header line: its length without the line end
__global__ __launch_bounds__(256) void k_fasta_hdr_len(const u8 *__restrict__ text, u64 n, const u64 *__restrict__ hdr_off, u64 n_hdr,
                                                       u64 *__restrict__ hdr_len) {
    const u64 r = (u64)blockIdx.x * 4u + (threadIdx.x >> 6);
    const u32 lane = threadIdx.x & 63u;
    if (r >= n_hdr) return;
    const u64 h = hdr_off[r];
    u64 p = h + 1, e;
    for (;;) {
        const u64 i = p + lane;
        const u64 m = __ballot(i >= n || text[i] == (u8)'\n');
        if (m) { e = min(n, p + (u64)__ffsll((long long)m) - 1ull); break; }
        p += 64;
    }
    u64 len = e - h;
    if (lane == 0) {
        if (len > 1 && text[e - 1] == (u8)'\r') len--;
        hdr_len[r] = len;
    }
}

// ... and its bytes, packed at pk_off[r]
__global__ __launch_bounds__(256) void k_fasta_hdr_gather(const u8 *__restrict__ text, const u64 *__restrict__ hdr_off,
                                                          const u64 *__restrict__ hdr_len, const u64 *__restrict__ pk_off, u64 n_hdr,
                                                          u8 *__restrict__ packed) {
    const u64 r = (u64)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (r >= n_hdr) return;
    const u8 *src = text + hdr_off[r];
    u8 *dst = packed + pk_off[r];
    const u64 len = hdr_len[r];
    for (u64 k = threadIdx.x & 63u; k < len; k += 64) dst[k] = src[k];
}

// the line around text[pos]: out[0] = the "\n" in front of pos (its 0-based number), out[1] = its start, out[2] = its end (in: 0, 0, n)
__global__ __launch_bounds__(256) void k_fasta_locate(const u8 *__restrict__ text, u64 n, u64 pos, u64 *__restrict__ out) {
    u64 cnt = 0, start = 0, end = n;
    for (u64 i = (u64)blockIdx.x * 256u + threadIdx.x; i < n; i += (u64)gridDim.x * 256u) {
        if (text[i] != (u8)'\n') continue;
        if (i < pos) { cnt++; start = i + 1; }
        else end = min(end, i);
    }
    if (cnt) { atomicAdd(out, cnt); atomicMax(out + 1, start); }
    if (end != n) atomicMin(out + 2, end);
}

int locate(pp_ctx *ctx, const u8 *d_text, u64 n, u64 pos, u64 *d_loc, u64 loc[3]) {
    loc[0] = 0; loc[1] = 0; loc[2] = n;
    PP_HIPCHK(ctx, hipMemcpyAsync(d_loc, loc, 24, hipMemcpyHostToDevice, ctx->stream));
    PP_HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // (loc is changed below)
    const unsigned nb = (unsigned)std::min<u64>(1024, (n + 255) / 256);
    hipLaunchKernelGGL(k_fasta_locate, dim3(nb), dim3(256), 0, ctx->stream, d_text, n, pos, d_loc);
    PP_HIPCHK(ctx, hipGetLastError());
    return fetch(ctx, d_loc, loc, 3);
}

}  // namespace

extern "C" void pp_fasta_free(pp_fasta *f) { delete f; }

extern "C" void pp_fasta_bases(const pp_fasta *f, const uint8_t **dev, uint64_t *n_bases) {
    if (dev) *dev = f ? f->bases : nullptr;
    if (n_bases) *n_bases = f ? f->n_bases : 0;
}

extern "C" uint32_t pp_fasta_n_contigs(const pp_fasta *f) { return f ? (uint32_t)f->c.names.size() : 0; }
extern "C" const uint64_t *pp_fasta_offsets(const pp_fasta *f) { return f ? f->c.off.data() : nullptr; }
extern "C" const char *pp_fasta_name(const pp_fasta *f, uint32_t i) { return f && i < f->c.names.size() ? f->c.names[i].c_str() : nullptr; }
extern "C" const char *pp_fasta_description(const pp_fasta *f, uint32_t i) { return f && i < f->c.descs.size() ? f->c.descs[i].c_str() : nullptr; }

extern "C" int pp_fasta_kernel_ms(const pp_fasta *f, float *ms) {  // (from stage 1: the staging copy is no kernel)
    return f ? f->t.total(f->ctx, "pp_fasta_kernel_ms", "when the text was parsed", ms, 1) : PP_ERR_ARG;
}

// (internal hooks, not part of the header) the time by stage: the staging copy of a host text | the sums and their scan | bases and
// headers | header lines (tools/fasta_timing.py); the geometry: bytes per lane, per tile and per workgroup (the tests); the bases into
// host memory (pp_assembly_bases of an assembly made by pp_assembly_load_device)
extern "C" int pp_fasta_stage_ms_(const pp_fasta *f, float *ms4) { return f ? f->t.stages(ms4) : PP_ERR_ARG; }

extern "C" void pp_fasta_geometry_(uint32_t *lane, uint32_t *tile, uint32_t *group) {
    if (lane) *lane = FA_LANE;
    if (tile) *tile = FA_TILE;
    if (group) *group = FA_WG;
}

extern "C" int pp_fasta_download_(const pp_fasta *f, uint8_t *host) {
    if (!f || (f->n_bases && !host)) return PP_ERR_ARG;
    pp_ctx *ctx = f->ctx;
    PP_HIPCHK(ctx, hipSetDevice(ctx->device));
    if (f->n_bases) PP_HIPCHK(ctx, hipMemcpyAsync(host, f->bases, (size_t)f->n_bases, hipMemcpyDeviceToHost, ctx->stream));
    PP_HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PP_OK;
}

// pp_fasta_records with the path its messages name (pp_assembly_load_device: the file's; pp_fasta_records: "text")
extern "C" int pp_fasta_records_named_(pp_ctx *ctx, const uint8_t *text, uint64_t n_bytes, int mem, const char *path, pp_fasta **out,
                                       uint64_t *bad_line) {
    namespace fh = pp_fasta_host;
    if (!ctx) return PP_ERR_ARG;
    if (int rdy = pp_ctx_wait(ctx)) return rdy;
    if (bad_line) *bad_line = ~0ull;
    if (!out || !path) return ctx->fail(PP_ERR_ARG, "pp_fasta_records: null argument");
    *out = nullptr;
    if (mem != PP_MEM_HOST && mem != PP_MEM_DEVICE)
        return ctx->fail(PP_ERR_ARG, "pp_fasta_records: the text must be host memory or memory of the context's device");
    if (n_bytes && !text) return ctx->fail(PP_ERR_ARG, "pp_fasta_records: null text with n_bytes > 0");
    if (n_bytes >= (1ull << 40)) return ctx->fail(PP_ERR_LIMIT, "pp_fasta_records: the text is larger than the 1 TiB this parse indexes");
    PP_HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const u64 n = n_bytes;

    std::unique_ptr<pp_fasta> P(new pp_fasta(ctx));
    CallScratch T;
    StageTimer timer(ctx, ctx->profiling != 0 && n != 0);
    int rc;
    char msg[1024] = "";
    std::vector<fh::Header> hdr;
    std::vector<char> packed;
    if (n == 0) {  // no text: no sequences
        PP_HIPCHK(ctx, hipStreamSynchronize(st));
        return ctx->fail(fh::contigs(path, nullptr, nullptr, 0, 0, P->c, msg, sizeof msg), "%s", msg);
    }
    // ---- where the kernels read the text ----
    const u8 *d_text = text;
    if (mem == PP_MEM_HOST) {
        void *q;
        if ((rc = T.get(ctx, &q, (size_t)n)) || (rc = timer.begin(0))) return rc;
        PP_HIPCHK(ctx, hipMemcpyAsync(q, text, (size_t)n, hipMemcpyHostToDevice, st));
        if ((rc = timer.end())) return rc;
        d_text = (const u8 *)q;
    }
    const u32 shift = (u32)((uintptr_t)d_text & 15u);
    const u64 nwg = (n + shift + FA_WG - 1) / FA_WG;
    if (nwg > 0x7FFFFFFFull) return ctx->fail(PP_ERR_LIMIT, "pp_fasta_records: the text is larger than the 1 TiB this parse indexes");
    // ---- the workgroups' sums and their scan ----
    void *d_sums, *d_pre, *d_status, *d_loc;
    if ((rc = T.get(ctx, &d_sums, (size_t)nwg * sizeof(FaSum))) || (rc = T.get(ctx, &d_pre, ((size_t)nwg + 1) * sizeof(FaSum))) ||
        (rc = T.get(ctx, &d_status, 8)) || (rc = T.get(ctx, &d_loc, 24)))
        return rc;
    PP_HIPCHK(ctx, hipMemsetAsync(d_status, 0xFF, 8, st));
    if ((rc = timer.begin(1))) return rc;
    hipLaunchKernelGGL(k_fasta<false>, dim3((unsigned)nwg), dim3(FA_THREADS), 0, st, d_text, n, shift, (FaSum *)d_sums, (u8 *)nullptr, 0ull, (u64 *)nullptr,
                       (u64 *)nullptr, 0ull, (u64 *)nullptr);
    hipLaunchKernelGGL(k_fasta_scan, dim3(1), dim3(1024), 0, st, (const FaSum *)d_sums, nwg, (FaSum *)d_pre);
    if ((rc = timer.end())) return rc;
    PP_HIPCHK(ctx, hipGetLastError());
    FaSum total;
    if ((rc = fetch(ctx, (const FaSum *)d_pre + nwg, &total))) return rc;
    const u64 n_bases = total.cnt, n_hdr = total.nh;
    if (n_bases > n || n_hdr > n) return ctx->fail(PP_ERR_HIP, "pp_fasta_records: the scan counts more bytes than the text holds");
    // ---- the bases, the header lines ----
    void *d_hoff, *d_hpre, *d_hlen;
    if ((rc = P->alloc(P->bases, (size_t)n_bases + 64)) || (rc = T.get(ctx, &d_hoff, (size_t)n_hdr * 8)) || (rc = T.get(ctx, &d_hpre, (size_t)n_hdr * 8)) ||
        (rc = T.get(ctx, &d_hlen, (size_t)n_hdr * 8)))
        return rc;
    P->n_bases = n_bases;
    if ((rc = timer.begin(2))) return rc;
    hipLaunchKernelGGL(k_fasta<true>, dim3((unsigned)nwg), dim3(FA_THREADS), 0, st, d_text, n, shift, (FaSum *)d_pre, P->bases, n_bases, (u64 *)d_hoff,
                       (u64 *)d_hpre, n_hdr, (u64 *)d_status);
    if ((rc = timer.end())) return rc;
    PP_HIPCHK(ctx, hipGetLastError());
    u64 status = ~0ull;
    if ((rc = fetch(ctx, d_status, &status))) return rc;
    if (status != ~0ull && (status & 0xFFu) == 0) return ctx->fail(PP_ERR_HIP, "pp_fasta_records: the two passes over the text disagree");
    if (n_hdr) {
        std::vector<u64> off((size_t)n_hdr), pre((size_t)n_hdr), len((size_t)n_hdr), pk((size_t)n_hdr);
        if ((rc = timer.begin(3))) return rc;
        hipLaunchKernelGGL(k_fasta_hdr_len, dim3((unsigned)((n_hdr + 3) / 4)), dim3(256), 0, st, d_text, n, (const u64 *)d_hoff, n_hdr, (u64 *)d_hlen);
        if ((rc = timer.end())) return rc;
        PP_HIPCHK(ctx, hipGetLastError());
        if ((rc = fetch(ctx, d_hoff, off.data(), off.size())) || (rc = fetch(ctx, d_hpre, pre.data(), pre.size())) ||
            (rc = fetch(ctx, d_hlen, len.data(), len.size())))
            return rc;
        hdr.resize((size_t)n_hdr);
        u64 pk_total = 0;
        for (size_t i = 0; i < hdr.size(); i++) {
            if (off[i] >= n || len[i] > n - off[i]) return ctx->fail(PP_ERR_HIP, "pp_fasta_records: a header line outside the text");
            hdr[i] = fh::Header{off[i], len[i], pre[i]};
            pk[i] = pk_total;
            pk_total += len[i];
        }
        void *d_pk, *d_packed;
        if ((rc = T.get(ctx, &d_pk, (size_t)n_hdr * 8)) || (rc = T.get(ctx, &d_packed, (size_t)pk_total))) return rc;
        PP_HIPCHK(ctx, hipMemcpyAsync(d_pk, pk.data(), (size_t)n_hdr * 8, hipMemcpyHostToDevice, st));
        if ((rc = timer.begin(3))) return rc;
        hipLaunchKernelGGL(k_fasta_hdr_gather, dim3((unsigned)((n_hdr + 3) / 4)), dim3(256), 0, st, d_text, (const u64 *)d_hoff, (const u64 *)d_hlen,
                           (const u64 *)d_pk, n_hdr, (u8 *)d_packed);
        if ((rc = timer.end())) return rc;
        PP_HIPCHK(ctx, hipGetLastError());
        packed.resize((size_t)pk_total);
        if ((rc = fetch(ctx, d_packed, packed.data(), packed.size()))) return rc;  // (synchronises: pk may go)
    }
    PP_HIPCHK(ctx, hipStreamSynchronize(st));  // the caller's text may be released, the scratch goes away
    if ((rc = P->t.take(timer))) return rc;
    // ---- the first offending line in file order: a header that is not valid UTF-8, or the line of the device's byte ----
    const u64 s_off = status == ~0ull ? ~0ull : status >> 8;
    const size_t ib = fh::first_bad_header(packed.data(), hdr.data(), hdr.size(), s_off);
    u64 loc[3];
    if (ib < hdr.size()) {
        if ((rc = locate(ctx, d_text, n, hdr[ib].off, (u64 *)d_loc, loc))) return rc;
        if (bad_line) *bad_line = loc[0];
        return ctx->fail(PP_ERR_QUIT, "unable to load \"%s\"", path);
    }
    if (status != ~0ull) {
        if (s_off >= n) return ctx->fail(PP_ERR_HIP, "pp_fasta_records: an offending byte outside the text");
        if ((rc = locate(ctx, d_text, n, s_off, (u64 *)d_loc, loc))) return rc;
        if (bad_line) *bad_line = loc[0];
        const u64 a = loc[1], b = loc[2];
        std::vector<char> line((size_t)(b - a));
        if (mem == PP_MEM_HOST) memcpy(line.data(), text + a, (size_t)(b - a));
        else if ((rc = fetch(ctx, d_text + a, line.data(), line.size()))) return rc;
        // (the text's last byte, if it is a "\r", ends its line as one in front of a "\n" does: sequence_line drops either)
        const int code = fh::sequence_line(path, line.data(), line.size(), (status & 0xFFu) != FR_HEADLESS, msg, sizeof msg);
        if (code == PP_OK) return ctx->fail(PP_ERR_HIP, "pp_fasta_records: the device refused line %llu but the host loader takes it", (unsigned long long)(loc[0] + 1));
        return ctx->fail(code, "%s", msg);
    }
    if (int code = fh::contigs(path, packed.data(), hdr.data(), hdr.size(), n_bases, P->c, msg, sizeof msg)) return ctx->fail(code, "%s", msg);
    if (P->c.names.size() >= 0xFFFFFFFFull) return ctx->fail(PP_ERR_LIMIT, "pp_fasta_records: 2^32-1 or more contigs in one text");
    *out = P.release();
    return PP_OK;
}

extern "C" int pp_fasta_records(pp_ctx *ctx, const uint8_t *text, uint64_t n_bytes, int mem, pp_fasta **out, uint64_t *bad_line) {
    return pp_fasta_records_named_(ctx, text, n_bytes, mem, "text", out, bad_line);
}
