// pp_polish_text.hip -- the post-passes that make text from a finished polish job, each on the device: the --debug TSV
// (pp_polish_debug_tsv, pp_k_debug.h), the edits as VCF (pp_polish_vcf, pp_k_vcf.h, pp_vcf_host.h), the undecided regions as BED and
// the soft-masked polished bytes (pp_status_bed, pp_polish_bed, pp_polish_masked, pp_k_bed.h, pp_bed_host.h), the read depth as bedGraph
// (pp_depth_bedgraph, pp_polish_depth, pp_k_depth.h, pp_depth_host.h), and what the file drivers keep of them on the context.  Nothing here runs unless a caller asks for it: the polish pipeline (pp_kernels.hip) is
// untouched, and this unit reads of it only what a finished job leaves in the context (pp_internal.h).  The call's scratch, the
// result objects' device memory and the stage times are pp_dev.h's (CallScratch, DevOwner, StageTimer, StageMs), the single-workgroup
// scan of the workgroups' sums its k_colscan<1>.
#include "pp_dev.h"
#include "pp_vcf_host.h"
#include "pp_bed_host.h"
#include "pp_depth_host.h"

#include <cstring>

// The kernels (they define __global__ kernels: included here and nowhere else), each header after the one it takes helpers from
#include "pp_k_debug.h"
#include "pp_k_vcf.h"
#include "pp_k_bed.h"
#include "pp_k_depth.h"

using namespace pp;

namespace {
// A call's stages lie back to back on the stream: stage s begins where the one in front of it ends.
int next_stage(StageTimer &t, int s) {
    if (int rc = t.end()) return rc;
    return t.begin(s);
}
}  // namespace

// ---- the --debug TSV on the device (pp_k_debug.h) ----------------------------------------------------------------------
constexpr uint64_t DFMT_STAGE = 64ull << 20;     // device staging of a chunk that goes to host memory
constexpr uint64_t DFMT_MAX_POS = 1ull << 22;    // positions per chunk (and so the room of its length array)

// the formatter's tables of the finished job: contig names and emit ranges on the device, key records and multi-byte winners
// grouped by position
static int dfmt_prepare(pp_ctx *ctx, const char *const *names) {
    if (ctx->dfmt_ready) return PP_OK;
    hipStream_t st = ctx->stream;
    const uint32_t nc = ctx->n_contigs;
    const uint64_t G = ctx->G;
    std::vector<uint64_t> noff((size_t)nc + 1, 0);
    for (uint32_t c = 0; c < nc; c++) {
        if (!names[c]) return ctx->fail(PP_ERR_ARG, "pp_polish_debug_tsv: contig name %u is NULL", c);
        noff[c + 1] = noff[c] + strlen(names[c]);
    }
    std::vector<uint8_t> nb(noff[nc] ? noff[nc] : 1);
    for (uint32_t c = 0; c < nc; c++) memcpy(nb.data() + noff[c], names[c], noff[c + 1] - noff[c]);
    int rc;
    if ((rc = dev_ensure(ctx, ctx->b_dfmt_names, nb.size())) || (rc = dev_ensure(ctx, ctx->b_dfmt_noff, noff.size() * 8)) ||
        (rc = dev_ensure(ctx, ctx->b_dfmt_emit, (size_t)nc * 8)))
        return rc;
    PP_HIPCHK(ctx, hipMemcpyAsync(ctx->b_dfmt_names.p, nb.data(), nb.size(), hipMemcpyHostToDevice, st));
    PP_HIPCHK(ctx, hipMemcpyAsync(ctx->b_dfmt_noff.p, noff.data(), noff.size() * 8, hipMemcpyHostToDevice, st));
    if (!ctx->emit.empty()) PP_HIPCHK(ctx, hipMemcpyAsync(ctx->b_dfmt_emit.p, ctx->emit.data(), (size_t)nc * 8, hipMemcpyHostToDevice, st));
    const uint64_t nk = ctx->n_keys, nm = ctx->n_multi, nr = nk + nm;
    if (nr >= 0xFFFFFFFFull) return ctx->fail(PP_ERR_LIMIT, "more than 2^32-1 key records in one --debug job");
    if ((rc = dev_ensure(ctx, ctx->b_dfmt_idx, G * 4)) || (rc = dev_ensure(ctx, ctx->b_dfmt_rec, nr * 4))) return rc;
    PP_HIPCHK(ctx, hipMemsetAsync(ctx->b_dfmt_idx.p, 0, G * 4, st));
    if (nr) {
        const uint64_t per_blk = 256ull * DFMT_SCAN_PER, nb_scan = (G + per_blk - 1) / per_blk;
        if ((rc = dev_ensure(ctx, ctx->b_dfmt_bsum, nb_scan * 8)) || (rc = dev_ensure(ctx, ctx->b_dfmt_boff, (nb_scan + 1) * 8))) return rc;
        const unsigned g = (unsigned)((nr + 255) / 256);
        u32 *idx = (u32 *)ctx->b_dfmt_idx.p;
        hipLaunchKernelGGL(k_dfmt_count, dim3(g), dim3(256), 0, st, (const KeyRec *)ctx->b_keys.p, (u32)nk, (const MultiEnt *)ctx->b_multi.p,
                           (u32)nm, (u64)G, idx);
        hipLaunchKernelGGL(k_dfmt_bsum, dim3((unsigned)nb_scan), dim3(256), 0, st, (const u32 *)idx, (u64)G, (u64 *)ctx->b_dfmt_bsum.p);
        hipLaunchKernelGGL(k_colscan<1>, dim3(1), dim3(1024), 0, st, (const u64 *)ctx->b_dfmt_bsum.p, (u64)nb_scan, (u64 *)ctx->b_dfmt_boff.p);
        hipLaunchKernelGGL(k_dfmt_apply, dim3((unsigned)nb_scan), dim3(256), 0, st, idx, (u64)G, (const u64 *)ctx->b_dfmt_boff.p);
        hipLaunchKernelGGL(k_dfmt_scatter, dim3(g), dim3(256), 0, st, (const KeyRec *)ctx->b_keys.p, (u32)nk, (const MultiEnt *)ctx->b_multi.p,
                           (u32)nm, (u64)G, idx, (u32 *)ctx->b_dfmt_rec.p);
        PP_HIPCHK(ctx, hipGetLastError());
    }
    ctx->dfmt_ready = true;
    return PP_OK;
}

extern "C" int pp_polish_debug_tsv(pp_ctx *ctx, const char *const *contig_names, uint64_t pos_lo, uint64_t pos_hi, uint8_t *out,
                                   int out_mem, uint64_t cap, uint64_t *len, uint64_t *pos_next) {
    if (!ctx) return PP_ERR_ARG;
    if (len) *len = 0;
    if (pos_next) *pos_next = pos_lo;
    if (!ctx->job_done || !ctx->job_debug || !ctx->b_dbg_depth.p)
        return ctx->fail(PP_ERR_ARG, "the --debug TSV needs pp_polish_set_debug(1) before pp_polish_finish");
    if (!contig_names || !out || !len || !pos_next || cap == 0 || (out_mem != PP_MEM_HOST && out_mem != PP_MEM_DEVICE))
        return ctx->fail(PP_ERR_ARG, "pp_polish_debug_tsv: null argument, cap 0 or unknown memory kind");
    if (pos_lo > pos_hi || pos_hi > ctx->G)
        return ctx->fail(PP_ERR_ARG, "pp_polish_debug_tsv: positions [%llu, %llu) are not inside the assembly",
                         (unsigned long long)pos_lo, (unsigned long long)pos_hi);
    PP_HIPCHK(ctx, hipSetDevice(ctx->device));
    if (int rc = dfmt_prepare(ctx, contig_names)) return rc;
    hipStream_t st = ctx->stream;
    DfmtJob J;
    J.depth = (const double *)ctx->b_dbg_depth.p;
    J.counts = (const u32 *)ctx->b_dbg_counts.p;
    J.status = (const u8 *)ctx->b_dbg_status.p;
    J.code = (const u8 *)ctx->b_code.p;
    J.bases = ctx->d_bases;
    J.seq = ctx->have_batch ? ctx->dbatch.seq : nullptr;
    J.contig_off = (const u64 *)ctx->b_contig_off.p;
    J.nc = ctx->n_contigs;
    J.n_keys = (u32)ctx->n_keys;
    J.names = (const u8 *)ctx->b_dfmt_names.p;
    J.name_off = (const u64 *)ctx->b_dfmt_noff.p;
    J.emit = ctx->emit.empty() ? nullptr : (const u32 *)ctx->b_dfmt_emit.p;
    J.keys = (const KeyRec *)ctx->b_keys.p;
    J.multi = (const MultiEnt *)ctx->b_multi.p;
    J.rec_end = (const u32 *)ctx->b_dfmt_idx.p;
    J.rec = (const u32 *)ctx->b_dfmt_rec.p;
    J.G = ctx->G;
    const bool host = out_mem == PP_MEM_HOST;
    int rc;
    if (host && (rc = dev_ensure(ctx, ctx->b_dfmt_stage, (size_t)std::min<uint64_t>(cap, DFMT_STAGE)))) return rc;
    if ((rc = dev_ensure(ctx, ctx->b_dfmt_res, 16))) return rc;
    uint64_t written = 0, p = pos_lo;
    // Chunks of at most DFMT_MAX_POS positions (and no more than the room could take at 16 bytes a line -- a line has 22 at
    // least): size pass, scan of the workgroups' sums, write pass, then how far it got.  To host memory through the staging
    // buffer, DFMT_STAGE bytes at a time.
    while (p < pos_hi && written < cap) {
        const uint64_t caller_room = cap - written;
        const uint64_t room = host ? std::min<uint64_t>(caller_room, DFMT_STAGE) : caller_room;
        const uint32_t N = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(pos_hi - p, room / 16 + 1), DFMT_MAX_POS);
        const uint32_t nb = (N + DFMT_THREADS - 1) / DFMT_THREADS;
        if ((rc = dev_ensure(ctx, ctx->b_dfmt_len, (size_t)N * 4)) || (rc = dev_ensure(ctx, ctx->b_dfmt_bsum, (size_t)nb * 8)) ||
            (rc = dev_ensure(ctx, ctx->b_dfmt_boff, ((size_t)nb + 1) * 8)))
            return rc;
        u8 *dst = host ? (u8 *)ctx->b_dfmt_stage.p : out + written;
        PP_HIPCHK(ctx, hipMemsetAsync(ctx->b_dfmt_res.p, 0, 16, st));
        hipLaunchKernelGGL(k_dfmt_len, dim3(nb), dim3(DFMT_THREADS), 0, st, J, (u64)p, N, (u32 *)ctx->b_dfmt_len.p, (u64 *)ctx->b_dfmt_bsum.p);
        hipLaunchKernelGGL(k_colscan<1>, dim3(1), dim3(1024), 0, st, (const u64 *)ctx->b_dfmt_bsum.p, (u64)nb, (u64 *)ctx->b_dfmt_boff.p);
        hipLaunchKernelGGL(k_dfmt_write, dim3(nb), dim3(DFMT_THREADS), 0, st, J, (u64)p, N, (const u32 *)ctx->b_dfmt_len.p,
                           (const u64 *)ctx->b_dfmt_boff.p, (u64)room, dst, (u64 *)ctx->b_dfmt_res.p);
        PP_HIPCHK(ctx, hipGetLastError());
        uint64_t res[2] = {0, 0};
        PP_HIPCHK(ctx, hipMemcpyAsync(res, ctx->b_dfmt_res.p, 16, hipMemcpyDeviceToHost, st));
        PP_HIPCHK(ctx, hipStreamSynchronize(st));
        const uint64_t n_fit = res[0], bytes = res[1];
        if (bytes == 0 && n_fit < N) {  // the next line does not fit
            if (room == caller_room && written == 0)
                return ctx->fail(PP_ERR_ARG, "pp_polish_debug_tsv: %llu bytes of room do not take the line of position %llu",
                                 (unsigned long long)cap, (unsigned long long)(p + n_fit));
            if (room == caller_room) {
                p += n_fit;
                break;
            }
            return ctx->fail(PP_ERR_LIMIT, "a --debug line longer than %llu bytes", (unsigned long long)DFMT_STAGE);
        }
        if (host && bytes) {
            PP_HIPCHK(ctx, hipMemcpyAsync(out + written, ctx->b_dfmt_stage.p, bytes, hipMemcpyDeviceToHost, st));
            PP_HIPCHK(ctx, hipStreamSynchronize(st));
        }
        written += bytes;
        p += n_fit;
        if (n_fit < N && room == caller_room) break;  // the caller's buffer is full
    }
    *len = written;
    *pos_next = p;
    return PP_OK;
}

// ---- the polish's edits as VCF text on the device (pp_k_vcf.h, pp_vcf_host.h) ---------------------------------------------
struct pp_vcf_out : DevOwner {
    using DevOwner::DevOwner;
    u8 *text = nullptr;  // DEVICE, n_text bytes (allocated up to a multiple of 16)
    uint64_t n_text = 0, n_records = 0;
    StageMs<4> t;  // mark | runs | records | text
};

namespace {
// The finished job as the post-passes read it (pp_polish_vcf, pp_polish_masked), and where each workgroup's emitted bytes begin: the
// multi-byte winners' lengths as a table (J.mlen, when the job has any), the emitted bytes per workgroup of VCF_TILE positions
// (d_bsum: nb words, free for the caller afterwards) and their scan (d_boff: nb + 1).  G > 0.
VcfJob vcf_job_of(const pp_ctx *ctx) {
    VcfJob J;
    J.bases = ctx->d_bases; J.code = (const u8 *)ctx->b_code.p; J.out = (const u8 *)ctx->b_out.p; J.mlen = nullptr;
    J.contig_off = (const u64 *)ctx->b_contig_off.p; J.nc = ctx->n_contigs; J.G = ctx->G; J.total_out = ctx->total_out;
    return J;
}
int vcf_emit_offsets(pp_ctx *ctx, CallScratch &T, VcfJob &J, uint64_t nb, u64 *&d_bsum, u64 *&d_boff) {
    hipStream_t st = ctx->stream;
    const uint64_t nm = ctx->n_multi;
    int rc;
    if ((rc = T.alloc(ctx, d_bsum, nb)) || (rc = T.alloc(ctx, d_boff, nb + 1))) return rc;
    if (nm) {
        u32 *d_mlen = nullptr;
        if ((rc = T.alloc(ctx, d_mlen, J.G))) return rc;
        hipLaunchKernelGGL(k_vcf_multi, dim3((unsigned)((nm + 255) / 256)), dim3(256), 0, st, (const MultiEnt *)ctx->b_multi.p, (u32)nm, J.code, (u64)J.G, d_mlen);
        J.mlen = d_mlen;
    }
    hipLaunchKernelGGL(k_vcf_sum, dim3((unsigned)nb), dim3(VCF_THREADS), 0, st, J, d_bsum);
    hipLaunchKernelGGL(k_colscan<1>, dim3(1), dim3(1024), 0, st, (const u64 *)d_bsum, (u64)nb, d_boff);
    return PP_OK;
}
}  // namespace

extern "C" void pp_vcf_out_free(pp_vcf_out *o) { delete o; }

extern "C" void pp_vcf_out_bytes(const pp_vcf_out *o, const uint8_t **dev, uint64_t *n_bytes, uint64_t *n_records) {
    if (dev) *dev = o ? o->text : nullptr;
    if (n_bytes) *n_bytes = o ? o->n_text : 0;
    if (n_records) *n_records = o ? o->n_records : 0;
}

extern "C" int pp_vcf_out_write(const pp_vcf_out *o, const char *path) {
    if (!o || !o->ctx) return PP_ERR_ARG;
    if (!path) return o->ctx->fail(PP_ERR_ARG, "pp_vcf_out_write: null argument");
    return write_device_file(o->ctx, "pp_vcf_out_write", o->text, o->n_text, path);
}

extern "C" int pp_vcf_out_kernel_ms(const pp_vcf_out *o, float *ms) {
    return o ? o->t.total(o->ctx, "pp_vcf_out_kernel_ms", "when the text was made", ms) : PP_ERR_ARG;
}

// (internal hooks, not part of the header) the time by stage: mark | runs | records | text (tools/vcf_timing.py); the geometry:
// positions per thread and per workgroup of the position passes, text bytes per store and per workgroup (the tests)
extern "C" int pp_vcf_out_stage_ms_(const pp_vcf_out *o, float *ms4) { return o ? o->t.stages(ms4) : PP_ERR_ARG; }
extern "C" void pp_vcf_geometry_(uint32_t *pos_per_thread, uint32_t *pos_per_workgroup, uint32_t *bytes_per_store, uint32_t *bytes_per_workgroup) {
    if (pos_per_thread) *pos_per_thread = VCF_PPT;
    if (pos_per_workgroup) *pos_per_workgroup = VCF_TILE;
    if (bytes_per_store) *bytes_per_store = VCF_LANE;
    if (bytes_per_workgroup) *bytes_per_workgroup = VCF_TEXT_WG;
}

extern "C" int pp_polish_vcf(pp_ctx *ctx, const char *const *contig_names, pp_vcf_out **out) {
    if (!ctx) return PP_ERR_ARG;
    if (int rdy = pp_ctx_wait(ctx)) return rdy;
    if (out) *out = nullptr;
    // ---- the host's part, all of it before anything is launched ----
    pp_vcf_host::Plan plan;
    char msg[256] = "";
    const pp_vcf_host::JobState S{ctx->job_done, !ctx->emit.empty() || !ctx->run_full_of.empty()};
    if (int code = pp_vcf_host::plan(out != nullptr, S, ctx->n_contigs, ctx->contig_off.data(), contig_names, pp_version(), plan, msg, sizeof msg))
        return ctx->fail(code, "%s", msg);
    PP_HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint64_t G = ctx->G, H = plan.header.size();
    const uint32_t nc = ctx->n_contigs;
    std::unique_ptr<pp_vcf_out> P(new pp_vcf_out(ctx));
    CallScratch T;
    StageTimer timer(ctx, ctx->profiling != 0);
    int rc;
    uint64_t n_rec = 0, rec_bytes = 0;
    VcfRec *d_rec = nullptr;
    u64 *d_rec_at = nullptr, *d_noff = nullptr;
    VcfJob J = vcf_job_of(ctx);
    if ((rc = timer.begin(0))) return rc;
    if (G) {
        const uint64_t nb = (G + VCF_TILE - 1) / VCF_TILE;  // (below 2^21: G is below 2^32)
        u8 *d_flag = nullptr, *d_flag2 = nullptr;
        u64 *d_bsum = nullptr, *d_boff = nullptr, *d_roff = nullptr;
        if ((rc = T.alloc(ctx, d_flag, nb * VCF_TILE)) || (rc = T.alloc(ctx, d_flag2, nb * VCF_TILE)) || (rc = T.alloc(ctx, d_roff, nb + 1)) ||
            (rc = vcf_emit_offsets(ctx, T, J, nb, d_bsum, d_boff)))
            return rc;
        hipLaunchKernelGGL(k_vcf_mark, dim3((unsigned)nb), dim3(VCF_THREADS), 0, st, J, (const u64 *)d_boff, d_flag);
        if ((rc = next_stage(timer, 1))) return rc;
        hipLaunchKernelGGL(k_vcf_runs, dim3((unsigned)nb), dim3(VCF_THREADS), 0, st, J, (const u8 *)d_flag, d_flag2, d_bsum);
        hipLaunchKernelGGL(k_colscan<1>, dim3(1), dim3(1024), 0, st, (const u64 *)d_bsum, (u64)nb, d_roff);
        if ((rc = next_stage(timer, 2))) return rc;
        PP_HIPCHK(ctx, hipGetLastError());
        PP_HIPCHK(ctx, hipMemcpyAsync(&n_rec, d_roff + nb, 8, hipMemcpyDeviceToHost, st));
        PP_HIPCHK(ctx, hipStreamSynchronize(st));
        if (n_rec) {
            const uint64_t nbr = (n_rec + VCF_THREADS - 1) / VCF_THREADS;
            u64 *d_rsum = nullptr, *d_rsoff = nullptr;
            if ((rc = T.alloc(ctx, d_rec, n_rec)) || (rc = T.alloc(ctx, d_rec_at, n_rec + 1)) || (rc = T.alloc(ctx, d_rsum, nbr)) ||
                (rc = T.alloc(ctx, d_rsoff, nbr + 1)) || (rc = T.alloc(ctx, d_noff, (size_t)nc + 1)))
                return rc;
            PP_HIPCHK(ctx, hipMemsetAsync(d_rec, 0, n_rec * sizeof(VcfRec), st));
            PP_HIPCHK(ctx, hipMemcpyAsync(d_noff, plan.name_off.data(), ((size_t)nc + 1) * 8, hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(k_vcf_recs, dim3((unsigned)nb), dim3(VCF_THREADS), 0, st, J, (const u8 *)d_flag2, (const u64 *)d_boff, (const u64 *)d_roff, (u64)n_rec, d_rec);
            hipLaunchKernelGGL(k_vcf_reclen, dim3((unsigned)nbr), dim3(VCF_THREADS), 0, st, (const VcfRec *)d_rec, (u64)n_rec, J.contig_off, nc, (const u64 *)d_noff, d_rec_at, d_rsum);
            hipLaunchKernelGGL(k_colscan<1>, dim3(1), dim3(1024), 0, st, (const u64 *)d_rsum, (u64)nbr, d_rsoff);
            hipLaunchKernelGGL(k_vcf_recoff, dim3((unsigned)nbr), dim3(VCF_THREADS), 0, st, (u64)n_rec, (const u64 *)d_rsoff, (u64)H, d_rec_at);
            PP_HIPCHK(ctx, hipGetLastError());
            PP_HIPCHK(ctx, hipMemcpyAsync(&rec_bytes, d_rsoff + nbr, 8, hipMemcpyDeviceToHost, st));
            PP_HIPCHK(ctx, hipStreamSynchronize(st));
            P->n_records = n_rec;
        }
    }
    if ((rc = next_stage(timer, 3))) return rc;
    uint64_t n_text = 0;
    if (int code = pp_vcf_host::text_size(H, rec_bytes, &n_text, msg, sizeof msg)) return ctx->fail(code, "%s", msg);
    const size_t room = (size_t)((n_text + 15u) & ~15ull);
    if ((rc = P->alloc(P->text, room))) return rc;
    P->n_text = n_text;
    PP_HIPCHK(ctx, hipMemsetAsync(P->text, 0, std::max<size_t>(room, 16), st));
    u8 *d_hdr = nullptr, *d_names = nullptr;
    if ((rc = T.alloc(ctx, d_hdr, (size_t)((H + 15u) & ~15ull))) || (rc = T.alloc(ctx, d_names, plan.names.size()))) return rc;
    PP_HIPCHK(ctx, hipMemcpyAsync(d_hdr, plan.header.data(), H, hipMemcpyHostToDevice, st));
    if (!plan.names.empty()) PP_HIPCHK(ctx, hipMemcpyAsync(d_names, plan.names.data(), plan.names.size(), hipMemcpyHostToDevice, st));
    {
        VcfText X;
        X.bases = J.bases; X.out = J.out; X.hdr = d_hdr; X.names = d_names;
        X.name_off = d_noff;
        X.contig_off = J.contig_off; X.rec_at = d_rec_at; X.rec = d_rec;
        X.nc = nc; X.n_rec = n_rec; X.G = G; X.total_out = ctx->total_out; X.H = H; X.n_text = n_text;
        const uint64_t nwg = (n_text + VCF_TEXT_WG - 1) / VCF_TEXT_WG;  // (below 2^26: the text is below 2^40)
        hipLaunchKernelGGL(k_vcf_text, dim3((unsigned)nwg), dim3(VCF_THREADS), 0, st, X, P->text);
        PP_HIPCHK(ctx, hipGetLastError());
    }
    if ((rc = timer.end())) return rc;
    PP_HIPCHK(ctx, hipStreamSynchronize(st));  // the header's and the names' host bytes may go, the scratch goes away
    if ((rc = P->t.take(timer))) return rc;
    *out = P.release();
    return PP_OK;
}

// ---- the file drivers' VCF (pp_driver.cpp) ----
extern "C" int pp_ctx_set_vcf(pp_ctx *ctx, int on, int bgzf) {
    if (!ctx) return PP_ERR_ARG;
    ctx->vcf_on = on != 0;
    ctx->vcf_bgzf = on != 0 && bgzf != 0;
    return PP_OK;
}
extern "C" int pp_ctx_vcf(pp_ctx *ctx, pp_bytes *vcf) {
    if (!ctx) return PP_ERR_ARG;
    if (!vcf) return ctx->fail(PP_ERR_ARG, "pp_ctx_vcf: null argument");
    *vcf = pp_bytes{nullptr, 0};
    if (!ctx->vcf_made) return ctx->fail(PP_ERR_ARG, "pp_ctx_vcf: no driver has made a VCF with pp_ctx_set_vcf on this context");
    vcf->data = (uint8_t *)malloc(ctx->vcf_bytes.size() + 1);
    if (!vcf->data) return ctx->fail(PP_ERR_HIP, "pp_ctx_vcf: out of host memory");
    memcpy(vcf->data, ctx->vcf_bytes.data(), ctx->vcf_bytes.size());
    vcf->len = ctx->vcf_bytes.size();
    return PP_OK;
}
// (internal, the file drivers) what pp_ctx_set_vcf was given; the file a driver made (data == NULL: none, the run begins or failed)
extern "C" int pp_ctx_vcf_form_(const pp_ctx *ctx, int *bgzf) {
    if (bgzf) *bgzf = ctx && ctx->vcf_bgzf ? 1 : 0;
    return ctx && ctx->vcf_on ? 1 : 0;
}
extern "C" void pp_ctx_keep_vcf_(pp_ctx *ctx, const uint8_t *data, uint64_t n) {
    ctx->vcf_made = data != nullptr;
    ctx->vcf_bytes.assign(data ? (const char *)data : "", data ? (size_t)n : 0);
    if (!data) ctx->vcf_bytes.shrink_to_fit();
}

// ---- undecided regions: the status runs as BED text, the soft-masked polished bytes (pp_k_bed.h, pp_bed_host.h) ---------------
struct pp_bed_out : DevOwner {
    using DevOwner::DevOwner;
    u8 *text = nullptr;  // DEVICE, n_text bytes (allocated up to a multiple of 16)
    uint64_t n_text = 0, n_records = 0;
    uint64_t positions[6] = {0, 0, 0, 0, 0, 0};
    StageMs<3> t;  // runs | records | text
};
struct pp_masked : DevOwner {
    using DevOwner::DevOwner;
    u8 *bytes = nullptr;  // DEVICE, n bytes
    uint64_t n = 0;
    StageMs<1> t;
};

extern "C" void pp_bed_out_free(pp_bed_out *o) { delete o; }
extern "C" void pp_bed_out_bytes(const pp_bed_out *o, const uint8_t **dev, uint64_t *n_bytes, uint64_t *n_records) {
    if (dev) *dev = o ? o->text : nullptr;
    if (n_bytes) *n_bytes = o ? o->n_text : 0;
    if (n_records) *n_records = o ? o->n_records : 0;
}
extern "C" void pp_bed_out_counts(const pp_bed_out *o, uint64_t positions[6]) {
    if (!positions) return;
    for (int s = 0; s < 6; s++) positions[s] = o ? o->positions[s] : 0;
}
extern "C" int pp_bed_out_write(const pp_bed_out *o, const char *path) {
    if (!o || !o->ctx) return PP_ERR_ARG;
    if (!path) return o->ctx->fail(PP_ERR_ARG, "pp_bed_out_write: null argument");
    return write_device_file(o->ctx, "pp_bed_out_write", o->text, o->n_text, path);
}
extern "C" int pp_bed_out_kernel_ms(const pp_bed_out *o, float *ms) {
    return o ? o->t.total(o->ctx, "pp_bed_out_kernel_ms", "when the text was made", ms) : PP_ERR_ARG;
}
// (internal hooks, not part of the header) the time by stage: runs | records | text (tools/bed_timing.py); the geometry: positions
// per thread and per workgroup of the position passes, text bytes per store and per workgroup (the tests)
extern "C" int pp_bed_out_stage_ms_(const pp_bed_out *o, float *ms3) { return o ? o->t.stages(ms3) : PP_ERR_ARG; }
extern "C" void pp_bed_geometry_(uint32_t *pos_per_thread, uint32_t *pos_per_workgroup, uint32_t *bytes_per_store, uint32_t *bytes_per_workgroup) {
    if (pos_per_thread) *pos_per_thread = BED_PPT;
    if (pos_per_workgroup) *pos_per_workgroup = BED_TILE;
    if (bytes_per_store) *bytes_per_store = BED_LANE;
    if (bytes_per_workgroup) *bytes_per_workgroup = BED_TEXT_WG;
}

// the passes over d_status (DEVICE, plan.G bytes, any alignment); the arguments have been judged (pp_bed_host::plan)
static int status_bed_on_device(pp_ctx *ctx, const char *who, const u8 *d_status, uint32_t nc, const uint64_t *contig_off, const pp_bed_host::Plan &plan,
                                uint32_t mask, pp_bed_out **out, uint64_t *bad_pos) {
    hipStream_t st = ctx->stream;
    const uint64_t G = plan.G;
    std::unique_ptr<pp_bed_out> P(new pp_bed_out(ctx));
    CallScratch T;
    StageTimer timer(ctx, ctx->profiling != 0);
    int rc;
    char msg[256] = "";
    uint64_t n_rec = 0, n_text = 0;
    if ((rc = timer.begin(0))) return rc;
    if (G) {
        const uint64_t nb = (G + BED_TILE - 1) / BED_TILE;  // (below 2^21: G is below 2^32)
        u64 *d_coff = nullptr, *d_bcnt = nullptr, *d_roff = nullptr, *d_word = nullptr;  // d_word: the first bad position | positions per status
        if ((rc = T.alloc(ctx, d_coff, (size_t)nc + 1)) || (rc = T.alloc(ctx, d_bcnt, nb)) || (rc = T.alloc(ctx, d_roff, nb + 1)) || (rc = T.alloc(ctx, d_word, 7)))
            return rc;
        uint64_t word[7] = {~0ull, 0, 0, 0, 0, 0, 0};
        PP_HIPCHK(ctx, hipMemcpyAsync(d_coff, contig_off, ((size_t)nc + 1) * 8, hipMemcpyHostToDevice, st));
        PP_HIPCHK(ctx, hipMemcpyAsync(d_word, word, sizeof word, hipMemcpyHostToDevice, st));
        BedJob J;
        J.status = d_status; J.contig_off = d_coff; J.nc = nc; J.mask = mask; J.G = G;
        hipLaunchKernelGGL(k_bed_runs, dim3((unsigned)nb), dim3(BED_THREADS), 0, st, J, d_bcnt, d_word);
        hipLaunchKernelGGL(k_colscan<1>, dim3(1), dim3(1024), 0, st, (const u64 *)d_bcnt, (u64)nb, d_roff);
        PP_HIPCHK(ctx, hipGetLastError());
        PP_HIPCHK(ctx, hipMemcpyAsync(&n_rec, d_roff + nb, 8, hipMemcpyDeviceToHost, st));
        PP_HIPCHK(ctx, hipMemcpyAsync(word, d_word, 8, hipMemcpyDeviceToHost, st));
        if ((rc = next_stage(timer, 1))) return rc;
        PP_HIPCHK(ctx, hipStreamSynchronize(st));
        if (word[0] != ~0ull) {
            if (bad_pos) *bad_pos = word[0];
            return ctx->fail(PP_ERR_ARG, "%s: a status byte above 5 (PP_ST_TOO_CLOSE) at position %llu", who, (unsigned long long)word[0]);
        }
        if (n_rec) {
            const uint64_t nbr = (n_rec + BED_THREADS - 1) / BED_THREADS;
            BedRec *d_rec = nullptr;
            u64 *d_rec_at = nullptr, *d_rsum = nullptr, *d_rsoff = nullptr, *d_noff = nullptr;
            u8 *d_names = nullptr;
            if ((rc = T.alloc(ctx, d_rec, n_rec)) || (rc = T.alloc(ctx, d_rec_at, n_rec + 1)) || (rc = T.alloc(ctx, d_rsum, nbr)) ||
                (rc = T.alloc(ctx, d_rsoff, nbr + 1)) || (rc = T.alloc(ctx, d_noff, (size_t)nc + 1)) || (rc = T.alloc(ctx, d_names, plan.names.size())))
                return rc;
            PP_HIPCHK(ctx, hipMemsetAsync(d_rec, 0, n_rec * sizeof(BedRec), st));
            PP_HIPCHK(ctx, hipMemcpyAsync(d_noff, plan.name_off.data(), ((size_t)nc + 1) * 8, hipMemcpyHostToDevice, st));
            if (!plan.names.empty()) PP_HIPCHK(ctx, hipMemcpyAsync(d_names, plan.names.data(), plan.names.size(), hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(k_bed_recs, dim3((unsigned)nb), dim3(BED_THREADS), 0, st, J, (const u64 *)d_roff, (u64)n_rec, d_rec);
            hipLaunchKernelGGL(k_bed_reclen, dim3((unsigned)nbr), dim3(BED_THREADS), 0, st, (const BedRec *)d_rec, (u64)n_rec, (const u64 *)d_coff, nc,
                               (const u64 *)d_noff, d_rec_at, d_rsum, d_word + 1);
            hipLaunchKernelGGL(k_colscan<1>, dim3(1), dim3(1024), 0, st, (const u64 *)d_rsum, (u64)nbr, d_rsoff);
            hipLaunchKernelGGL(k_vcf_recoff, dim3((unsigned)nbr), dim3(VCF_THREADS), 0, st, (u64)n_rec, (const u64 *)d_rsoff, (u64)0, d_rec_at);
            PP_HIPCHK(ctx, hipGetLastError());
            PP_HIPCHK(ctx, hipMemcpyAsync(&n_text, d_rsoff + nbr, 8, hipMemcpyDeviceToHost, st));
            PP_HIPCHK(ctx, hipMemcpyAsync(P->positions, d_word + 1, 6 * 8, hipMemcpyDeviceToHost, st));
            if ((rc = next_stage(timer, 2))) return rc;
            PP_HIPCHK(ctx, hipStreamSynchronize(st));
            if (int code = pp_bed_host::text_size(who, n_text, msg, sizeof msg)) return ctx->fail(code, "%s", msg);
            const size_t room = (size_t)((n_text + 15u) & ~15ull);
            if ((rc = P->alloc(P->text, room))) return rc;
            P->n_text = n_text;
            P->n_records = n_rec;
            PP_HIPCHK(ctx, hipMemsetAsync(P->text, 0, room, st));
            BedText X;
            X.names = d_names; X.name_off = d_noff; X.contig_off = d_coff; X.rec_at = d_rec_at; X.rec = d_rec;
            X.nc = nc; X.n_rec = n_rec; X.n_text = n_text;
            const uint64_t nwg = (n_text + BED_TEXT_WG - 1) / BED_TEXT_WG;  // (below 2^26: the text is below 2^40)
            hipLaunchKernelGGL(k_bed_text, dim3((unsigned)nwg), dim3(BED_THREADS), 0, st, X, P->text);
            PP_HIPCHK(ctx, hipGetLastError());
        }
    }
    if ((rc = timer.end())) return rc;
    PP_HIPCHK(ctx, hipStreamSynchronize(st));  // the scratch goes away
    if ((rc = P->t.take(timer))) return rc;
    *out = P.release();
    return PP_OK;
}

extern "C" int pp_status_bed(pp_ctx *ctx, const uint8_t *status, int mem, uint32_t n_contigs, const uint64_t *contig_off, const char *const *contig_names,
                             uint32_t status_mask, pp_bed_out **out, uint64_t *bad_pos) {
    if (!ctx) return PP_ERR_ARG;
    if (int rdy = pp_ctx_wait(ctx)) return rdy;
    if (out) *out = nullptr;
    if (bad_pos) *bad_pos = 0;
    pp_bed_host::Plan plan;
    char msg[256] = "";
    if (int code = pp_bed_host::plan("pp_status_bed", out != nullptr, status != nullptr, mem == PP_MEM_HOST || mem == PP_MEM_DEVICE, n_contigs, contig_off,
                                     contig_names, status_mask, plan, msg, sizeof msg))
        return ctx->fail(code, "%s", msg);
    PP_HIPCHK(ctx, hipSetDevice(ctx->device));
    CallScratch T;
    const u8 *d_status = status;
    if (mem == PP_MEM_HOST && plan.G) {
        u8 *up = nullptr;
        if (int rc = T.alloc(ctx, up, (size_t)plan.G)) return rc;
        PP_HIPCHK(ctx, hipMemcpyAsync(up, status, plan.G, hipMemcpyHostToDevice, ctx->stream));
        d_status = up;
    }
    return status_bed_on_device(ctx, "pp_status_bed", d_status, n_contigs, contig_off, plan, status_mask, out, bad_pos);
}

static pp_bed_host::JobState bed_job_state(const pp_ctx *ctx) {
    return pp_bed_host::JobState{ctx->job_done, ctx->job_debug && ctx->b_dbg_status.p != nullptr, !ctx->emit.empty() || !ctx->run_full_of.empty()};
}

extern "C" int pp_polish_bed(pp_ctx *ctx, const char *const *contig_names, uint32_t status_mask, pp_bed_out **out) {
    if (!ctx) return PP_ERR_ARG;
    if (int rdy = pp_ctx_wait(ctx)) return rdy;
    if (out) *out = nullptr;
    char msg[256] = "";
    if (!out || !contig_names) return ctx->fail(PP_ERR_ARG, "pp_polish_bed: null argument");
    if (int code = pp_bed_host::check_job("pp_polish_bed", bed_job_state(ctx), msg, sizeof msg)) return ctx->fail(code, "%s", msg);
    pp_bed_host::Plan plan;
    if (int code = pp_bed_host::plan("pp_polish_bed", true, true, true, ctx->n_contigs, ctx->contig_off.data(), contig_names, status_mask, plan, msg, sizeof msg))
        return ctx->fail(code, "%s", msg);
    PP_HIPCHK(ctx, hipSetDevice(ctx->device));
    uint64_t bad = 0;
    return status_bed_on_device(ctx, "pp_polish_bed", (const u8 *)ctx->b_dbg_status.p, ctx->n_contigs, ctx->contig_off.data(), plan, status_mask, out, &bad);
}

extern "C" void pp_masked_free(pp_masked *o) { delete o; }
extern "C" void pp_masked_bytes(const pp_masked *o, const uint8_t **dev, uint64_t *n_bytes) {
    if (dev) *dev = o ? o->bytes : nullptr;
    if (n_bytes) *n_bytes = o ? o->n : 0;
}
extern "C" int pp_masked_kernel_ms(const pp_masked *o, float *ms) {
    return o ? o->t.total(o->ctx, "pp_masked_kernel_ms", "when the bytes were made", ms) : PP_ERR_ARG;
}

extern "C" int pp_polish_masked(pp_ctx *ctx, uint32_t status_mask, pp_masked **out) {
    if (!ctx) return PP_ERR_ARG;
    if (int rdy = pp_ctx_wait(ctx)) return rdy;
    if (out) *out = nullptr;
    char msg[256] = "";
    if (!out) return ctx->fail(PP_ERR_ARG, "pp_polish_masked: null argument");
    if (int code = pp_bed_host::check_job("pp_polish_masked", bed_job_state(ctx), msg, sizeof msg)) return ctx->fail(code, "%s", msg);
    if (int code = pp_bed_host::check_mask("pp_polish_masked", status_mask, msg, sizeof msg)) return ctx->fail(code, "%s", msg);
    PP_HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint64_t G = ctx->G, n = ctx->total_out;
    std::unique_ptr<pp_masked> P(new pp_masked(ctx));
    CallScratch T;
    StageTimer timer(ctx, ctx->profiling != 0);
    int rc;
    if ((rc = timer.begin(0)) || (rc = P->alloc(P->bytes, (size_t)n))) return rc;
    P->n = n;
    if (n) PP_HIPCHK(ctx, hipMemcpyAsync(P->bytes, ctx->b_out.p, n, hipMemcpyDeviceToDevice, st));
    if (G && n) {
        const uint64_t nb = (G + VCF_TILE - 1) / VCF_TILE;
        VcfJob J = vcf_job_of(ctx);
        u64 *d_bsum = nullptr, *d_boff = nullptr;
        if ((rc = vcf_emit_offsets(ctx, T, J, nb, d_bsum, d_boff))) return rc;
        hipLaunchKernelGGL(k_bed_mask, dim3((unsigned)nb), dim3(VCF_THREADS), 0, st, J, (const u64 *)d_boff, (const u8 *)ctx->b_dbg_status.p, status_mask, P->bytes);
        PP_HIPCHK(ctx, hipGetLastError());
    }
    if ((rc = timer.end())) return rc;
    PP_HIPCHK(ctx, hipStreamSynchronize(st));
    if ((rc = P->t.take(timer))) return rc;
    *out = P.release();
    return PP_OK;
}

// ---- the file drivers' BED and soft mask (pp_driver.cpp) ----
extern "C" int pp_ctx_set_bed(pp_ctx *ctx, int on, uint32_t status_mask, int bgzf) {
    if (!ctx) return PP_ERR_ARG;
    char msg[256] = "";
    if (on)
        if (int code = pp_bed_host::check_mask("pp_ctx_set_bed", status_mask, msg, sizeof msg)) return ctx->fail(code, "%s", msg);
    ctx->bed_on = on != 0;
    ctx->bed_mask = on ? status_mask : 0u;
    ctx->bed_bgzf = on != 0 && bgzf != 0;
    return PP_OK;
}
extern "C" int pp_ctx_bed(pp_ctx *ctx, pp_bytes *bed) {
    if (!ctx) return PP_ERR_ARG;
    if (!bed) return ctx->fail(PP_ERR_ARG, "pp_ctx_bed: null argument");
    *bed = pp_bytes{nullptr, 0};
    if (!ctx->bed_made) return ctx->fail(PP_ERR_ARG, "pp_ctx_bed: no driver has made a BED with pp_ctx_set_bed on this context");
    bed->data = (uint8_t *)malloc(ctx->bed_bytes.size() + 1);
    if (!bed->data) return ctx->fail(PP_ERR_HIP, "pp_ctx_bed: out of host memory");
    memcpy(bed->data, ctx->bed_bytes.data(), ctx->bed_bytes.size());
    bed->len = ctx->bed_bytes.size();
    return PP_OK;
}
extern "C" int pp_ctx_set_soft_mask(pp_ctx *ctx, uint32_t status_mask) {
    if (!ctx) return PP_ERR_ARG;
    if (status_mask & ~pp_bed_host::MASK_ALL) return ctx->fail(PP_ERR_ARG, "pp_ctx_set_soft_mask: a status mask with a bit above 5");
    ctx->soft_mask = status_mask;
    return PP_OK;
}
// (internal, the file drivers) what pp_ctx_set_bed / pp_ctx_set_soft_mask were given; the file a driver made (data == NULL: none)
extern "C" int pp_ctx_bed_form_(const pp_ctx *ctx, uint32_t *status_mask, int *bgzf) {
    if (status_mask) *status_mask = ctx ? ctx->bed_mask : 0u;
    if (bgzf) *bgzf = ctx && ctx->bed_bgzf ? 1 : 0;
    return ctx && ctx->bed_on ? 1 : 0;
}
extern "C" uint32_t pp_ctx_soft_mask_(const pp_ctx *ctx) { return ctx ? ctx->soft_mask : 0u; }
extern "C" void pp_ctx_keep_bed_(pp_ctx *ctx, const uint8_t *data, uint64_t n) {
    ctx->bed_made = data != nullptr;
    ctx->bed_bytes.assign(data ? (const char *)data : "", data ? (size_t)n : 0);
    if (!data) ctx->bed_bytes.shrink_to_fit();
}

// ---- read depth: the per-position depth as bedGraph text, runs or bins (pp_k_depth.h, pp_depth_host.h) ----------------------------
struct pp_depth_out : DevOwner {
    using DevOwner::DevOwner;
    u8 *text = nullptr;  // DEVICE, n_text bytes (allocated up to a multiple of 16)
    uint64_t n_text = 0, n_records = 0;
    uint64_t zero_positions = 0, max_tenths = 0, sum_tenths = 0;
    StageMs<4> t;  // values | records | lengths | text
};

extern "C" void pp_depth_out_free(pp_depth_out *o) { delete o; }
extern "C" void pp_depth_out_bytes(const pp_depth_out *o, const uint8_t **dev, uint64_t *n_bytes, uint64_t *n_records) {
    if (dev) *dev = o ? o->text : nullptr;
    if (n_bytes) *n_bytes = o ? o->n_text : 0;
    if (n_records) *n_records = o ? o->n_records : 0;
}
extern "C" void pp_depth_out_summary(const pp_depth_out *o, uint64_t *zero_positions, uint64_t *max_tenths, uint64_t *sum_tenths) {
    if (zero_positions) *zero_positions = o ? o->zero_positions : 0;
    if (max_tenths) *max_tenths = o ? o->max_tenths : 0;
    if (sum_tenths) *sum_tenths = o ? o->sum_tenths : 0;
}
extern "C" int pp_depth_out_write(const pp_depth_out *o, const char *path) {
    if (!o || !o->ctx) return PP_ERR_ARG;
    if (!path) return o->ctx->fail(PP_ERR_ARG, "pp_depth_out_write: null argument");
    return write_device_file(o->ctx, "pp_depth_out_write", o->text, o->n_text, path);
}
extern "C" int pp_depth_out_kernel_ms(const pp_depth_out *o, float *ms) {
    return o ? o->t.total(o->ctx, "pp_depth_out_kernel_ms", "when the text was made", ms) : PP_ERR_ARG;
}
// (internal hooks, not part of the header) the time by stage: values | records | lengths | text (tools/depth_timing.py); the geometry:
// positions per thread and per workgroup of the position passes, text bytes per store and per workgroup (the tests)
extern "C" int pp_depth_out_stage_ms_(const pp_depth_out *o, float *ms4) { return o ? o->t.stages(ms4) : PP_ERR_ARG; }
extern "C" void pp_depth_geometry_(uint32_t *pos_per_thread, uint32_t *pos_per_workgroup, uint32_t *bytes_per_store, uint32_t *bytes_per_workgroup) {
    if (pos_per_thread) *pos_per_thread = DEP_PPT;
    if (pos_per_workgroup) *pos_per_workgroup = DEP_TILE;
    if (bytes_per_store) *bytes_per_store = DEP_LANE;
    if (bytes_per_workgroup) *bytes_per_workgroup = DEP_TEXT_WG;
}

// the passes over d_depth (DEVICE, plan.names.G doubles, aligned to 8 bytes); the arguments have been judged (pp_depth_host::plan)
static int depth_on_device(pp_ctx *ctx, const char *who, const double *d_depth, uint32_t nc, const uint64_t *contig_off, const pp_depth_host::Plan &plan,
                           uint32_t bin, pp_depth_out **out, uint64_t *bad_pos) {
    hipStream_t st = ctx->stream;
    const uint64_t G = plan.names.G;
    std::unique_ptr<pp_depth_out> P(new pp_depth_out(ctx));
    CallScratch T;
    StageTimer timer(ctx, ctx->profiling != 0);
    int rc;
    char msg[256] = "";
    if ((rc = timer.begin(0))) return rc;
    if (G) {
        const uint64_t nb = (G + DEP_TILE - 1) / DEP_TILE;  // (below 2^21: G is below 2^32)
        uint64_t n_rec = bin ? plan.bin_base[nc] : 0, n_text = 0;
        u64 *d_coff = nullptr, *d_bcnt = nullptr, *d_roff = nullptr, *d_word = nullptr, *d_binbase = nullptr, *d_bins = nullptr;
        if ((rc = T.alloc(ctx, d_coff, (size_t)nc + 1)) || (rc = T.alloc(ctx, d_word, 4))) return rc;
        uint64_t word[4] = {~0ull, 0, 0, 0};  // the first bad position | zero positions | the largest tenths | their sum
        PP_HIPCHK(ctx, hipMemcpyAsync(d_coff, contig_off, ((size_t)nc + 1) * 8, hipMemcpyHostToDevice, st));
        PP_HIPCHK(ctx, hipMemcpyAsync(d_word, word, sizeof word, hipMemcpyHostToDevice, st));
        DepJob J;
        J.depth = d_depth; J.contig_off = d_coff; J.bin_base = nullptr; J.nc = nc; J.bin = bin; J.G = G;
        if (bin) {
            if ((rc = T.alloc(ctx, d_binbase, (size_t)nc + 1)) || (rc = T.alloc(ctx, d_bins, n_rec))) return rc;
            PP_HIPCHK(ctx, hipMemcpyAsync(d_binbase, plan.bin_base.data(), ((size_t)nc + 1) * 8, hipMemcpyHostToDevice, st));
            PP_HIPCHK(ctx, hipMemsetAsync(d_bins, 0, n_rec * 8, st));
            J.bin_base = d_binbase;
            hipLaunchKernelGGL(k_dep_values<true>, dim3((unsigned)nb), dim3(DEP_THREADS), 0, st, J, (u64 *)nullptr, d_bins, d_word);
            PP_HIPCHK(ctx, hipGetLastError());
        } else {
            if ((rc = T.alloc(ctx, d_bcnt, nb)) || (rc = T.alloc(ctx, d_roff, nb + 1))) return rc;
            hipLaunchKernelGGL(k_dep_values<false>, dim3((unsigned)nb), dim3(DEP_THREADS), 0, st, J, d_bcnt, (u64 *)nullptr, d_word);
            hipLaunchKernelGGL(k_colscan<1>, dim3(1), dim3(1024), 0, st, (const u64 *)d_bcnt, (u64)nb, d_roff);
            PP_HIPCHK(ctx, hipGetLastError());
            PP_HIPCHK(ctx, hipMemcpyAsync(&n_rec, d_roff + nb, 8, hipMemcpyDeviceToHost, st));
        }
        PP_HIPCHK(ctx, hipMemcpyAsync(word, d_word, sizeof word, hipMemcpyDeviceToHost, st));
        if ((rc = next_stage(timer, 1))) return rc;
        PP_HIPCHK(ctx, hipStreamSynchronize(st));
        if (word[0] != ~0ull) {
            if (bad_pos) *bad_pos = word[0];
            return ctx->fail(PP_ERR_ARG, "%s: a depth that is negative, not a number or 2^32 and more at position %llu", who, (unsigned long long)word[0]);
        }
        P->zero_positions = word[1];
        P->max_tenths = word[2];
        P->sum_tenths = word[3];
        // (G > 0: there is a record)
        const uint64_t nbr = (n_rec + DEP_THREADS - 1) / DEP_THREADS;
        const uint32_t frac = bin ? 2u : 1u;
        DepRec *d_rec = nullptr;
        u64 *d_rec_at = nullptr, *d_rsum = nullptr, *d_rsoff = nullptr, *d_noff = nullptr;
        u8 *d_names = nullptr;
        if ((rc = T.alloc(ctx, d_rec, n_rec)) || (rc = T.alloc(ctx, d_rec_at, n_rec + 1)) || (rc = T.alloc(ctx, d_rsum, nbr)) ||
            (rc = T.alloc(ctx, d_rsoff, nbr + 1)) || (rc = T.alloc(ctx, d_noff, (size_t)nc + 1)) || (rc = T.alloc(ctx, d_names, plan.names.names.size())))
            return rc;
        PP_HIPCHK(ctx, hipMemcpyAsync(d_noff, plan.names.name_off.data(), ((size_t)nc + 1) * 8, hipMemcpyHostToDevice, st));
        if (!plan.names.names.empty()) PP_HIPCHK(ctx, hipMemcpyAsync(d_names, plan.names.names.data(), plan.names.names.size(), hipMemcpyHostToDevice, st));
        if (bin) {
            hipLaunchKernelGGL(k_dep_binrecs, dim3((unsigned)nbr), dim3(DEP_THREADS), 0, st, J, (const u64 *)d_bins, (u64)n_rec, d_rec);
        } else {
            PP_HIPCHK(ctx, hipMemsetAsync(d_rec, 0, n_rec * sizeof(DepRec), st));
            hipLaunchKernelGGL(k_dep_recs, dim3((unsigned)nb), dim3(DEP_THREADS), 0, st, J, (const u64 *)d_roff, (u64)n_rec, d_rec);
        }
        PP_HIPCHK(ctx, hipGetLastError());
        if ((rc = next_stage(timer, 2))) return rc;
        hipLaunchKernelGGL(k_dep_reclen, dim3((unsigned)nbr), dim3(DEP_THREADS), 0, st, (const DepRec *)d_rec, (u64)n_rec, (const u64 *)d_coff, nc,
                           (const u64 *)d_noff, frac, d_rec_at, d_rsum);
        hipLaunchKernelGGL(k_colscan<1>, dim3(1), dim3(1024), 0, st, (const u64 *)d_rsum, (u64)nbr, d_rsoff);
        hipLaunchKernelGGL(k_vcf_recoff, dim3((unsigned)nbr), dim3(VCF_THREADS), 0, st, (u64)n_rec, (const u64 *)d_rsoff, (u64)0, d_rec_at);
        PP_HIPCHK(ctx, hipGetLastError());
        PP_HIPCHK(ctx, hipMemcpyAsync(&n_text, d_rsoff + nbr, 8, hipMemcpyDeviceToHost, st));
        if ((rc = next_stage(timer, 3))) return rc;
        PP_HIPCHK(ctx, hipStreamSynchronize(st));
        if (int code = pp_bed_host::text_size(who, n_text, msg, sizeof msg)) return ctx->fail(code, "%s", msg);
        const size_t room = (size_t)((n_text + 15u) & ~15ull);
        if ((rc = P->alloc(P->text, room))) return rc;
        P->n_text = n_text;
        P->n_records = n_rec;
        PP_HIPCHK(ctx, hipMemsetAsync(P->text, 0, room, st));
        DepText X;
        X.names = d_names; X.name_off = d_noff; X.contig_off = d_coff; X.rec_at = d_rec_at; X.rec = d_rec;
        X.nc = nc; X.frac = frac; X.n_rec = n_rec; X.n_text = n_text;
        const uint64_t nwg = (n_text + DEP_TEXT_WG - 1) / DEP_TEXT_WG;  // (below 2^26: the text is below 2^40)
        hipLaunchKernelGGL(k_dep_text, dim3((unsigned)nwg), dim3(DEP_THREADS), 0, st, X, P->text);
        PP_HIPCHK(ctx, hipGetLastError());
    }
    if ((rc = timer.end())) return rc;
    PP_HIPCHK(ctx, hipStreamSynchronize(st));  // the scratch goes away
    if ((rc = P->t.take(timer))) return rc;
    *out = P.release();
    return PP_OK;
}

extern "C" int pp_depth_bedgraph(pp_ctx *ctx, const double *depth, int mem, uint32_t n_contigs, const uint64_t *contig_off, const char *const *contig_names,
                                 uint32_t bin, pp_depth_out **out, uint64_t *bad_pos) {
    if (!ctx) return PP_ERR_ARG;
    if (int rdy = pp_ctx_wait(ctx)) return rdy;
    if (out) *out = nullptr;
    if (bad_pos) *bad_pos = 0;
    pp_depth_host::Plan plan;
    char msg[256] = "";
    if (int code = pp_depth_host::plan("pp_depth_bedgraph", out != nullptr, depth != nullptr, mem == PP_MEM_HOST || mem == PP_MEM_DEVICE,
                                       mem != PP_MEM_DEVICE || ((uintptr_t)depth & 7u) == 0u, n_contigs, contig_off, contig_names, bin, plan, msg, sizeof msg))
        return ctx->fail(code, "%s", msg);
    PP_HIPCHK(ctx, hipSetDevice(ctx->device));
    CallScratch T;
    const double *d_depth = depth;
    if (mem == PP_MEM_HOST && plan.names.G) {
        double *up = nullptr;
        if (int rc = T.alloc(ctx, up, (size_t)plan.names.G)) return rc;
        PP_HIPCHK(ctx, hipMemcpyAsync(up, depth, plan.names.G * 8, hipMemcpyHostToDevice, ctx->stream));
        d_depth = up;
    }
    return depth_on_device(ctx, "pp_depth_bedgraph", d_depth, n_contigs, contig_off, plan, bin, out, bad_pos);
}

extern "C" int pp_polish_depth(pp_ctx *ctx, const char *const *contig_names, uint32_t bin, pp_depth_out **out) {
    if (!ctx) return PP_ERR_ARG;
    if (int rdy = pp_ctx_wait(ctx)) return rdy;
    if (out) *out = nullptr;
    char msg[256] = "";
    if (!out || !contig_names) return ctx->fail(PP_ERR_ARG, "pp_polish_depth: null argument");
    const pp_bed_host::JobState S{ctx->job_done, ctx->job_debug && ctx->b_dbg_depth.p != nullptr, !ctx->emit.empty() || !ctx->run_full_of.empty()};
    if (int code = pp_bed_host::check_job("pp_polish_depth", S, msg, sizeof msg)) return ctx->fail(code, "%s", msg);
    pp_depth_host::Plan plan;
    if (int code = pp_depth_host::plan("pp_polish_depth", true, true, true, true, ctx->n_contigs, ctx->contig_off.data(), contig_names, bin, plan, msg, sizeof msg))
        return ctx->fail(code, "%s", msg);
    PP_HIPCHK(ctx, hipSetDevice(ctx->device));
    uint64_t bad = 0;
    return depth_on_device(ctx, "pp_polish_depth", (const double *)ctx->b_dbg_depth.p, ctx->n_contigs, ctx->contig_off.data(), plan, bin, out, &bad);
}

// ---- the file drivers' depth track (pp_driver.cpp) ----
extern "C" int pp_ctx_set_depth(pp_ctx *ctx, int on, uint32_t bin, int bgzf) {
    if (!ctx) return PP_ERR_ARG;
    if (on && bin > pp_depth_host::BIN_MAX) return ctx->fail(PP_ERR_ARG, "pp_ctx_set_depth: a bin of more than 2^24 positions");
    ctx->depth_on = on != 0;
    ctx->depth_bin = on ? bin : 0u;
    ctx->depth_bgzf = on != 0 && bgzf != 0;
    return PP_OK;
}
extern "C" int pp_ctx_depth(pp_ctx *ctx, pp_bytes *depth) {
    if (!ctx) return PP_ERR_ARG;
    if (!depth) return ctx->fail(PP_ERR_ARG, "pp_ctx_depth: null argument");
    *depth = pp_bytes{nullptr, 0};
    if (!ctx->depth_made) return ctx->fail(PP_ERR_ARG, "pp_ctx_depth: no driver has made a depth track with pp_ctx_set_depth on this context");
    depth->data = (uint8_t *)malloc(ctx->depth_bytes.size() + 1);
    if (!depth->data) return ctx->fail(PP_ERR_HIP, "pp_ctx_depth: out of host memory");
    memcpy(depth->data, ctx->depth_bytes.data(), ctx->depth_bytes.size());
    depth->len = ctx->depth_bytes.size();
    return PP_OK;
}
// (internal, the file drivers) what pp_ctx_set_depth was given; the file a driver made (data == NULL: none)
extern "C" int pp_ctx_depth_form_(const pp_ctx *ctx, uint32_t *bin, int *bgzf) {
    if (bin) *bin = ctx ? ctx->depth_bin : 0u;
    if (bgzf) *bgzf = ctx && ctx->depth_bgzf ? 1 : 0;
    return ctx && ctx->depth_on ? 1 : 0;
}
extern "C" void pp_ctx_keep_depth_(pp_ctx *ctx, const uint8_t *data, uint64_t n) {
    ctx->depth_made = data != nullptr;
    ctx->depth_bytes.assign(data ? (const char *)data : "", data ? (size_t)n : 0);
    if (!data) ctx->depth_bytes.shrink_to_fit();
}
