// pp_fasta_out.hip -- pp_fasta_text: contig bases in device memory as FASTA TEXT at a chosen line width, the mirror of pp_fasta_records
// (pp_fasta.hip) and the link in front of pp_bgzf_deflate: the polished assembly leaves the device as the file a user wants (wrapped,
// bgzipped, indexed).  tests/fasta_text_model.py defines the bytes.  The bases are read where they are (device memory at any alignment;
// host memory through one staging copy); the object owns the text and nothing else.
//
// The geometry (pp_fasta_out_geometry_; the tests aim at these seams).  The OUTPUT is cut, not the input: a lane owns FT_LANE = 16 bytes
// of text and writes them with ONE aligned 16-byte store, a workgroup of 256 lanes a TILE of 4096 bytes at a time and FT_TILES = 4 tiles
// one after the other: FT_WG = 16384 bytes.  The text's allocation is padded to a multiple of 16 (zeros behind the text), so every
// lane that owns a byte stores 16.
//
// What a byte of text is follows from the contig table the host uploads once (pp_fasta_out_host.h: per contig the text offset of its
// '>', of its body, its base offset, its length, where its header's bytes lie among the uploaded ones; one more row closes the table):
//   the workgroup  two lanes search the table for the contigs of the stretch's first and last byte; every lane then searches between
//                  the two for the contig of ITS first byte (no step at all inside a long contig)
//   the bulk       a lane whose 16 bytes lie inside one body and hold at most one "\n" (width 0, or 16 and more): ONE division gives
//                  the line and the place in it, the 15 or 16 bases are one run of the source.  The source's alignment is whatever
//                  the offsets make it: the run is taken from the one or two 16-byte pieces of ADDRESS that hold it, each with one
//                  wide load where the piece lies wholly inside the bases, byte by byte behind the test otherwise; v_alignbyte shifts
//                  the run into place (piece16, bytes_from: pp_cut16.h, shared with k_vcf_text), the "\n" goes in with three masks
//   the seams      any other lane -- a header, a contig's end, several whole contigs, a width below 16 -- walks its 16 bytes one at a
//                  time: one division when it enters a body, increments from there
// No byte outside bases[0, contig_off[n] - contig_off[0]) and outside the header bytes is loaded, by a wide load either.  Plain C++,
// vector stores, no cross-workgroup wait, nothing depends on the order in which lanes run.
#include "pp_dev.h"
#include "pp_cut16.h"
#include "pp_fasta_out_host.h"

#include <cstring>

namespace fo = pp_fasta_out_host;

struct pp_fasta_out : DevOwner {
    using DevOwner::DevOwner;
    u8 *text = nullptr;  // DEVICE, n_text bytes (allocated up to a multiple of 16)
    uint64_t n_text = 0;
    std::string fai;
    StageMs<2> t;  // the staging copy of host bases | the kernel
};

namespace {

constexpr u32 FT_THREADS = 256, FT_LANE = 16, FT_TILE = FT_THREADS * FT_LANE, FT_TILES = 4, FT_WG = FT_TILE * FT_TILES;
static_assert(sizeof(fo::Row) == 40, "the table's rows as the kernel reads them");

// the largest c in [lo, hi] with rows[c].hdr_at <= t (rows[lo].hdr_at <= t)
__device__ __forceinline__ u32 contig_of(const fo::Row *__restrict__ rows, u32 lo, u32 hi, u64 t) {
    while (lo < hi) {
        const u32 mid = lo + (hi - lo + 1u) / 2u;
        if (rows[mid].hdr_at <= t) lo = mid;
        else hi = mid - 1u;
    }
    return lo;
}

// the mask of the bytes below byte k (k in 0..16) of word i of 16 bytes
__device__ __forceinline__ u32 below(u32 k, u32 i) { return k >= 4u * i + 4u ? 0xFFFFFFFFu : (k <= 4u * i ? 0u : (1u << (8u * (k - 4u * i))) - 1u); }

__global__ __launch_bounds__(FT_THREADS) void k_fasta_text(const u8 *__restrict__ bases, u64 n_bases, const u8 *__restrict__ hdr,
                                                           const fo::Row *__restrict__ rows, u32 nc, u64 n_text, u32 W, u8 *__restrict__ out) {
    __shared__ u32 s_c[2];
    const u32 tid = threadIdx.x;
    const u64 g0 = (u64)blockIdx.x * FT_WG, g1 = min(n_text, g0 + (u64)FT_WG);  // (g0 < n_text: the grid)
    if (tid < 2) s_c[tid] = contig_of(rows, 0, nc - 1u, tid ? g1 - 1u : g0);
    __syncthreads();
    const u32 c_lo = s_c[0], c_hi = s_c[1];
    const u64 W1 = (u64)W + 1u;
    for (u32 ti = 0; ti < FT_TILES; ti++) {
        const u64 t0 = g0 + (u64)ti * FT_TILE + (u64)tid * FT_LANE;
        if (t0 >= n_text) break;  // (no lane waits for another below)
        u32 c = contig_of(rows, c_lo, c_hi, t0);
        fo::Row R = rows[c];
        u64 next = rows[c + 1u].hdr_at;
        uint4 v;
        bool done = false;
        if (t0 >= R.body_at && t0 + FT_LANE <= next && (W == 0 || W >= FT_LANE)) {
            // ---- the bulk: 16 bytes of one body ----
            const u64 r0 = t0 - R.body_at, last = next - R.body_at - 1u;  // the body's last byte is a "\n"
            u64 src = r0;
            u32 k = 16;  // where the "\n" goes
            const u32 k_end = last - r0 < 16u ? (u32)(last - r0) : 16u;
            if (W == 0) k = k_end;
            else {
                const u64 q = r0 / W1, m = r0 - q * W1;
                src = r0 - q;
                const u32 k_line = (u64)W - m < 16u ? (u32)((u64)W - m) : 16u;
                k = min(k_line, k_end);
                done = !(k_line < 16u && k_end < 16u && k_line != k_end);  // (a short last line may bring a second "\n": the walk below)
            }
            if (W == 0 || done) {
                done = true;
                const u8 *p = bases + R.base_off + src;
                const u32 a = (u32)((uintptr_t)p & 15u), cnt = k < 16u ? 15u : 16u;
                const uint4 p0 = piece16(p - a, bases, bases + n_bases);
                const uint4 p1 = a + cnt > 16u ? piece16(p - a + 16, bases, bases + n_bases) : make_uint4(0, 0, 0, 0);
                v = bytes_from(p0, p1, a);
                if (k < 16u) {  // bytes below k stay, byte k is "\n", the bytes behind it move up by one
                    const uint4 up = make_uint4(v.x << 8, (v.y << 8) | (v.x >> 24), (v.z << 8) | (v.y >> 24), (v.w << 8) | (v.z >> 24));
                    const u32 nl = 0x0Au << (8u * (k & 3u));
                    const u32 b0 = below(k, 0), b1 = below(k, 1), b2 = below(k, 2), b3 = below(k, 3);
                    const u32 a0 = below(k + 1u, 0), a1 = below(k + 1u, 1), a2 = below(k + 1u, 2), a3 = below(k + 1u, 3);
                    v.x = (v.x & b0) | (up.x & ~a0) | ((k >> 2) == 0u ? nl : 0u);
                    v.y = (v.y & b1) | (up.y & ~a1) | ((k >> 2) == 1u ? nl : 0u);
                    v.z = (v.z & b2) | (up.z & ~a2) | ((k >> 2) == 2u ? nl : 0u);
                    v.w = (v.w & b3) | (up.w & ~a3) | ((k >> 2) == 3u ? nl : 0u);
                }
            }
        }
        if (!done) {
            // ---- the seams: one byte at a time ----
            u32 w[4] = {0, 0, 0, 0};
            bool in_body = false;  // m, si hold for the byte at hand
            u64 m = 0, si = 0;     // the place in the line, the base's index in the contig
            for (u32 j = 0; j < FT_LANE; j++) {
                const u64 t = t0 + j;
                if (t >= n_text) break;
                while (t >= next) {  // (a contig without a body line ends where its header does)
                    c++;
                    R = rows[c];
                    next = rows[c + 1u].hdr_at;
                    in_body = false;
                }
                u32 b;
                if (t < R.body_at) {
                    const u64 i = t - R.hdr_at;
                    b = i == 0 ? (u32)'>' : (t + 1u == R.body_at ? (u32)'\n' : (u32)hdr[R.hsrc + i - 1u]);
                } else {
                    const u64 r = t - R.body_at;
                    if (!in_body) {
                        in_body = true;
                        if (W == 0) { m = 0; si = r; }
                        else {
                            const u64 q = r / W1;
                            m = r - q * W1;
                            si = r - q;
                        }
                    }
                    if (t + 1u == next || (W != 0 && m == (u64)W)) { b = (u32)'\n'; m = 0; }
                    else {
                        b = si < R.len && R.base_off + si < n_bases ? (u32)bases[R.base_off + si] : 0u;
                        si++;
                        m++;
                    }
                }
                w[j >> 2] |= b << (8 * (j & 3));
            }
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        *(uint4 *)(out + t0) = v;
    }
}

}  // namespace

extern "C" void pp_fasta_out_free(pp_fasta_out *o) { delete o; }

extern "C" void pp_fasta_out_bytes(const pp_fasta_out *o, const uint8_t **dev, uint64_t *n_bytes) {
    if (dev) *dev = o ? o->text : nullptr;
    if (n_bytes) *n_bytes = o ? o->n_text : 0;
}

extern "C" int pp_fasta_out_fai(const pp_fasta_out *o, pp_bytes *fai) {
    if (!o || !fai) return PP_ERR_ARG;
    fai->len = o->fai.size();
    fai->data = (uint8_t *)malloc(o->fai.size() + 1);
    if (!fai->data) {
        fai->len = 0;
        return o->ctx->fail(PP_ERR_HIP, "pp_fasta_out_fai: out of host memory");
    }
    memcpy(fai->data, o->fai.data(), o->fai.size());
    return PP_OK;
}

extern "C" int pp_fasta_out_write(const pp_fasta_out *o, const char *path) {
    if (!o || !o->ctx) return PP_ERR_ARG;
    if (!path) return o->ctx->fail(PP_ERR_ARG, "pp_fasta_out_write: null argument");
    return pp::write_device_file(o->ctx, "pp_fasta_out_write", o->text, o->n_text, path);
}

extern "C" int pp_fasta_out_kernel_ms(const pp_fasta_out *o, float *ms) {  // (from stage 1: the staging copy is no kernel)
    return o ? o->t.total(o->ctx, "pp_fasta_out_kernel_ms", "when the text was made", ms, 1) : PP_ERR_ARG;
}

// (internal hooks, not part of the header) the time by stage: the staging copy of host bases | the kernel (tools/fasta_text_timing.py);
// the geometry: bytes per store and per workgroup (the tests)
extern "C" int pp_fasta_out_stage_ms_(const pp_fasta_out *o, float *ms2) { return o ? o->t.stages(ms2) : PP_ERR_ARG; }

extern "C" void pp_fasta_out_geometry_(uint32_t *bytes_per_store, uint32_t *bytes_per_workgroup) {
    if (bytes_per_store) *bytes_per_store = FT_LANE;
    if (bytes_per_workgroup) *bytes_per_workgroup = FT_WG;
}

extern "C" int pp_fasta_text(pp_ctx *ctx, const uint8_t *bases, int mem, uint32_t n_contigs, const uint64_t *contig_off, const uint8_t *headers,
                             const uint64_t *header_off, uint32_t width, pp_fasta_out **out) {
    if (!ctx) return PP_ERR_ARG;
    if (int rdy = pp_ctx_wait(ctx)) return rdy;
    if (!out) return ctx->fail(PP_ERR_ARG, "pp_fasta_text: null argument");
    *out = nullptr;
    // ---- the host's part, all of it before anything is uploaded ----
    fo::Plan plan;
    char msg[256] = "";
    if (int code = fo::plan(bases != nullptr, mem == PP_MEM_HOST || mem == PP_MEM_DEVICE, n_contigs, contig_off, headers, header_off, width, plan, msg, sizeof msg))
        return ctx->fail(code, "%s", msg);
    PP_HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    std::unique_ptr<pp_fasta_out> P(new pp_fasta_out(ctx));
    fo::fai(plan, headers, header_off, width, P->fai);
    P->n_text = plan.n_text;
    CallScratch T;
    StageTimer timer(ctx, ctx->profiling != 0);
    int rc;
    if ((rc = P->alloc(P->text, (size_t)((plan.n_text + 15u) & ~15ull)))) return rc;
    if (plan.n_text) {
        const u8 *d_bases = nullptr, *d_hdr = nullptr;
        const fo::Row *d_rows = nullptr;
        if ((rc = timer.begin(0))) return rc;
        if ((rc = on_device(ctx, T, mem, (const u8 *)(bases ? bases + contig_off[0] : nullptr), (size_t)plan.n_bases, &d_bases))) return rc;
        if ((rc = timer.end())) return rc;
        if ((rc = on_device(ctx, T, PP_MEM_HOST, (const u8 *)(headers ? headers + header_off[0] : nullptr), (size_t)plan.n_hdr, &d_hdr)) ||
            (rc = on_device(ctx, T, PP_MEM_HOST, plan.rows.data(), plan.rows.size(), &d_rows)))
            return rc;
        const u64 nwg = (plan.n_text + FT_WG - 1) / FT_WG;  // (below 2^26: the text is below 2^40)
        if ((rc = timer.begin(1))) return rc;
        hipLaunchKernelGGL(k_fasta_text, dim3((unsigned)nwg), dim3(FT_THREADS), 0, st, d_bases, plan.n_bases, d_hdr, d_rows, n_contigs, plan.n_text, width, P->text);
        if ((rc = timer.end())) return rc;
        PP_HIPCHK(ctx, hipGetLastError());
    }
    PP_HIPCHK(ctx, hipStreamSynchronize(st));  // host inputs may be released, the scratch goes away
    if ((rc = P->t.take(timer))) return rc;
    *out = P.release();
    return PP_OK;
}

// ---- the form of the file drivers' FASTA (pp_driver.cpp) ----
extern "C" int pp_ctx_set_fasta_form(pp_ctx *ctx, int64_t width, int bgzf) {
    if (!ctx) return PP_ERR_ARG;
    if (width > (int64_t)fo::WIDTH_MAX) return ctx->fail(PP_ERR_LIMIT, "pp_ctx_set_fasta_form: a line width above 2^31-1");
    ctx->fasta_width = width < 0 ? -1 : width;
    ctx->fasta_bgzf = width >= 0 && bgzf != 0;
    return PP_OK;
}

static int bytes_of(pp_ctx *ctx, const std::string &s, pp_bytes *out) {
    if (!out) return PP_OK;
    out->len = 0;
    out->data = (uint8_t *)malloc(s.size() + 1);
    if (!out->data) return ctx->fail(PP_ERR_HIP, "pp_ctx_fasta_index: out of host memory");
    memcpy(out->data, s.data(), s.size());
    out->len = s.size();
    return PP_OK;
}

extern "C" int pp_ctx_fasta_index(pp_ctx *ctx, pp_bytes *fai, pp_bytes *gzi) {
    if (!ctx) return PP_ERR_ARG;
    if (fai) *fai = pp_bytes{nullptr, 0};
    if (gzi) *gzi = pp_bytes{nullptr, 0};
    if (!ctx->fasta_indexed) return ctx->fail(PP_ERR_ARG, "pp_ctx_fasta_index: no driver has made a FASTA with pp_ctx_set_fasta_form on this context");
    if (int rc = bytes_of(ctx, ctx->fasta_fai, fai)) return rc;
    return bytes_of(ctx, ctx->fasta_gzi, gzi);
}

// (internal, the file drivers: pp_driver.cpp) what pp_ctx_set_fasta_form was given; the indexes of the text a driver made; the name
// of the file the caller will write the FASTA to (bin/polypolish --out, Python's out=: the log's last section names it), "" for none
extern "C" int pp_ctx_fasta_form_(const pp_ctx *ctx, int64_t *width, int *bgzf) {
    if (width) *width = ctx ? ctx->fasta_width : -1;
    if (bgzf) *bgzf = ctx && ctx->fasta_bgzf ? 1 : 0;
    return ctx && ctx->fasta_width >= 0 ? 1 : 0;
}
extern "C" void pp_ctx_keep_fasta_index_(pp_ctx *ctx, const uint8_t *fai, uint64_t n_fai, const uint8_t *gzi, uint64_t n_gzi) {
    ctx->fasta_fai.assign((const char *)fai, (size_t)n_fai);
    ctx->fasta_gzi.assign((const char *)gzi, (size_t)n_gzi);
    ctx->fasta_indexed = true;
}
extern "C" int pp_ctx_set_fasta_out_name_(pp_ctx *ctx, const char *path) {
    if (!ctx) return PP_ERR_ARG;
    ctx->fasta_out_name = path ? path : "";
    return PP_OK;
}
extern "C" const char *pp_ctx_fasta_out_name_(const pp_ctx *ctx) { return ctx ? ctx->fasta_out_name.c_str() : ""; }
