// pp_bam_sam.hip -- pp_bam_sam: uncompressed BAM decoded to SAM TEXT, on the device.  The inverse of pp_sam_bam (pp_sam_bam.hip) and
// the last side of the square SAM <-> BAM: from the BAM bytes, the records' offsets and -- where the caller has them -- one verdict
// byte per aligned record it makes the text `polypolish filter` would have written had the input been that text: the header's lines,
// one line per record in index order, "\tZP:Z:fail" behind the aligned ones that failed.  The result is a pp_sam_out, the object
// pp_sam_tagged makes (pp_sam_out.hip owns the type): pp_sam_out_write puts it on disk, pp_bgzf_deflate compresses its bytes.
// The bytes are defined by a plain model, tests/bam_sam_model.py; include/polypolish_hip.h states the contract.  The bytes are
// BORROWED: no byte outside [0, n_bytes) is loaded, by a wide load either.
//
// The geometry (pp_bam_sam_geometry_; the tests aim at these seams):
//   BS_RECS  = 1,024    records per workgroup of pass A and of the placing kernel
//   BS_TILE  = 16,384   output bytes per workgroup of pass B
//   BS_STORE = 16       bytes per store of pass B, aligned on the OUTPUT
//   BS_LANE  = 16       output bytes per lane and step of the wide parts (a group of BS_GROUP = 32 lanes per record: 512 per step)
//
//   k_bs_scan   pass A, one lane per record: the record's range (pp_bam_host::step_kind, as pp_bam_tagged), its inner structure in
//               pp_bam_records' order -- nothing read through a length before it is checked, no sum that could wrap -- the bytes a
//               SAM line cannot hold, then the line's length and where SEQ starts in it: emit_line with a counting emitter, the same
//               walk pass B writes with.  A refusal is status = record << 8 | why by atomicMin: the first record in index order wins; inside a record a
//               structural defect goes in front of a limit.  Also the workgroups' numbers of aligned records
//   k_bs_off    the aligned rank, the verdict at that rank, a 64-bit scan of the lengths; then off[r], the failing bit, and
//               tile_first[tile] = the record that holds the first byte of pass B's tile
//   k_bs_emit   pass B, output-centric: a workgroup owns BS_TILE output bytes as an image in LDS (zeros and the header's bytes first).
//               (1) one lane per record writes what is serial by nature: the numbers, the names of the references, the CIGAR, the
//               aux fields, the appended tag, the tabs and the newline; (2) a group of 32 lanes per record writes what is wide:
//               QNAME (a copy), SEQ (eight bytes of nibbles become sixteen letters), QUAL (sixteen bytes plus 33 in one step);
//               (3) the image leaves through 16-byte stores aligned on the output.  Every write into the image is clipped to the
//               tile, so a record longer than a tile spans workgroups; the wide parts start at the tile's first chunk.
// "%g" of an aux float is pp_fmt_g.h: integer arithmetic, exact over all of float32.  Its limbs live in scratch memory; floats are
// rare (bwa writes none) and no other register does.
// What happens to ONE record -- check_record, emit_line and its emitters, wide_parts -- is pp_bam_sam_lines.h: plain C++ for host
// and device, so that tools/bam_sam_host_check.cpp runs the same code in loops over tiles, records and lanes under a sanitizer.
#include "pp_bam_sam_host.h"
#include "pp_bam_sam_lines.h"
#include "pp_textin.h"

#include <cstring>
#include <new>
#include <string>

extern "C" char *pp_bam_msg_buf_(size_t *cap);  // pp_bam.hip: the per-thread message behind pp_bam_last_error()
// pp_sam_out.hip, the owner of the type: an object with room for `alloc` bytes of text; then what it holds
extern "C" int pp_sam_out_new_(pp_ctx *ctx, uint64_t alloc, pp_sam_out **out, uint8_t **d_out);
extern "C" void pp_sam_out_set_(pp_sam_out *o, uint64_t n_out, uint64_t pass_count, uint64_t fail_count, uint64_t n_lines, const float *ms4);

namespace {

// status: the first refusal, record << 8 | why
__global__ __launch_bounds__(BS_RECS) void k_bs_scan(u32 n_rec, const u8 *__restrict__ B, u64 N, const u64 *__restrict__ rec_off, RefTab R,
                                                     u64 *__restrict__ len, u64 *__restrict__ seq_at, u8 *__restrict__ kind, u64 *__restrict__ blk_al, u64 *__restrict__ status) {
    __shared__ u64 s_w[BS_RECS / 64];
    const u64 r = (u64)blockIdx.x * BS_RECS + threadIdx.x;
    u32 al = 0;
    if (r < n_rec) {
        u64 c = 0, n = 1, mark = 0;
        u32 bs = 0;
        const u32 why = check_record(B, N, rec_off[r], R, &al, &c, &bs);
        if (why) {
            report(status, (r << 8) | why);
            al = 0;
        } else {
            Count cnt;
            emit_line(cnt, B, c, bs, R, false);
            n = cnt.n;
            mark = cnt.seq_at;
        }
        len[r] = n;
        seq_at[r] = mark;
        kind[r] = (u8)al;
    }
    u64 total;
    (void)block_scan_excl64<BS_RECS>(al, s_w, &total);
    if (threadIdx.x == 0) blk_al[blockIdx.x] = total;
}

// PLACE == false: the workgroups' output bytes and failing records (blk2: two words per workgroup).  PLACE == true: blk2 holds their
// exclusive scan: off[r] (from the output's first byte), off[n_rec], the verdict into kind bit 1, the tiles the record starts.
template <bool PLACE>
__global__ __launch_bounds__(BS_RECS) void k_bs_off(u32 n_rec, const u64 *__restrict__ len, u8 *__restrict__ kind, const u64 *__restrict__ al_base,
                                                    const u8 *__restrict__ pass /* or null: no verdicts */, u64 hdr_len, u64 *__restrict__ blk2,
                                                    u64 *__restrict__ off, u32 *__restrict__ tile_first) {
    __shared__ u64 s_w[BS_RECS / 64];
    const u64 r = (u64)blockIdx.x * BS_RECS + threadIdx.x;
    const u32 al = r < n_rec ? (u32)kind[r] & 1u : 0u;
    u64 t_al, t_len, t_fail;
    const u64 rank = al_base[blockIdx.x] + block_scan_excl64<BS_RECS>(al, s_w, &t_al);
    const u32 fail = (al && pass && pass[rank] == 0) ? 1u : 0u;
    const u64 n = r < n_rec ? len[r] + 10u * fail : 0u;
    const u64 ex_len = block_scan_excl_u64<BS_RECS>(n, s_w, &t_len);
    (void)block_scan_excl64<BS_RECS>(fail, s_w, &t_fail);
    u64 *const mine = blk2 + 2ull * blockIdx.x;
    if (!PLACE) {
        if (threadIdx.x == 0) { mine[0] = t_len; mine[1] = t_fail; }
        return;
    }
    if (r >= n_rec) return;
    const u64 s = hdr_len + mine[0] + ex_len, e = s + n;
    off[r] = s;
    if (r + 1 == n_rec) off[n_rec] = e;
    kind[r] = (u8)(al | (fail << 1));
    for (u64 tile = (s + BS_TILE - 1u) / BS_TILE; tile * BS_TILE < e; tile++) tile_first[tile] = (u32)r;
}

// ---- pass B --------------------------------------------------------------------------------------------------------------------------
struct EmitArgs {
    const u8 *bytes;
    u64 n_bytes;
    const u64 *rec_off;
    const u64 *off;          // n_rec + 1 entries: where a line starts in the output
    const u64 *seq_at;       // where SEQ starts in the line (pass A)
    const u8 *kind;          // aligned | fail << 1
    const u32 *tile_first;   // the record of every tile's first byte (tiles that begin at or behind hdr_len)
    const u8 *hdr;           // the header's text, zeros up to a multiple of BS_STORE
    RefTab R;
    u64 hdr_len, n_rec, total;
    u8 *out;                 // ... in an allocation of a multiple of BS_STORE
};
__global__ __launch_bounds__(BS_THREADS) void k_bs_emit(EmitArgs A) {
    __shared__ __attribute__((aligned(16))) u8 img[BS_TILE];
    const u8 *__restrict__ const B = A.bytes;
    const u32 t = threadIdx.x;
    const u64 t0 = (u64)blockIdx.x * BS_TILE, t1 = min(A.total, t0 + (u64)BS_TILE);
    // ---- the image starts as the header's bytes and zeros
    const u64 hdr_pad = (A.hdr_len + BS_STORE - 1u) / BS_STORE * BS_STORE;
#pragma unroll
    for (u32 j = 0; j < BS_TILE / BS_STORE / BS_THREADS; j++) {
        const u32 c = BS_STORE * (t + j * BS_THREADS);
        uint4 v = make_uint4(0, 0, 0, 0);
        if (t0 + c < hdr_pad) v = *(const uint4 *)(A.hdr + t0 + c);
        *(uint4 *)(img + c) = v;
    }
    __syncthreads();
    if (A.n_rec && t1 > A.hdr_len) {
        const u64 r_lo = t0 <= A.hdr_len ? 0 : (u64)A.tile_first[blockIdx.x];
        const u64 r_hi = t0 + BS_TILE < A.total ? (u64)A.tile_first[blockIdx.x + 1u] : A.n_rec - 1u;
        // ---- (1) what is serial: one lane per record
        for (u64 r = r_lo + t; r <= r_hi; r += BS_THREADS) {
            const u64 c = A.rec_off[r] + 4u;
            Img W{img, (i64)(A.off[r] - t0)};
            emit_line(W, B, c, ld32(B, c - 4u), A.R, ((u32)A.kind[r] >> 1) & 1u);
        }
        // ---- (2) what is wide: QNAME, SEQ, QUAL; a group of lanes per record, sixteen output bytes per lane and step
        const u32 grp = t / BS_GROUP, hl = t % BS_GROUP;
        for (u64 r = r_lo + grp; r <= r_hi; r += BS_THREADS / BS_GROUP) wide_parts(img, B, A.n_bytes, A.rec_off[r] + 4u, (i64)(A.off[r] - t0), A.seq_at[r], hl);
        __syncthreads();
    }
    // ---- (3) the image leaves through 16-byte stores aligned on the output
#pragma unroll
    for (u32 j = 0; j < BS_TILE / BS_STORE / BS_THREADS; j++) {
        const u32 c = BS_STORE * (t + j * BS_THREADS);
        if (t0 + c < t1) *(uint4 *)(A.out + t0 + c) = *(const uint4 *)(img + c);
    }
}

// ---- the host side ---------------------------------------------------------------------------------------------------------------------
struct Why { int code; const char *what; };
Why why_of(u32 w) {
    switch (w) {
    case pp_bam_host::W_CUT: return {PP_ERR_ARG, "has an offset outside the bytes, or the bytes end inside its block_size"};
    case pp_bam_host::W_SMALL: return {PP_ERR_ARG, "has a block_size below the 32 bytes of its fixed part"};
    case pp_bam_host::W_PAST: return {PP_ERR_ARG, "runs past the end of the bytes"};
    case Y_BLOCK: return {PP_ERR_ARG, "has a block_size below what its l_read_name, n_cigar_op and l_seq ask for"};
    case Y_NAME: return {PP_ERR_ARG, "has an empty read_name or one without its NUL"};
    case Y_CIGAR_OP: return {PP_ERR_ARG, "has a CIGAR op above 8"};
    case Y_REF_ID: return {PP_ERR_ARG, "has a refID or next_refID outside [-1, n_ref)"};
    case Y_AUX: return {PP_ERR_ARG, "has an aux field that is cut, of unknown type or without its end inside the record"};
    case Y_POS: return {PP_ERR_ARG, "has a pos or next_pos below -1"};
    case Y_QNAME: return {PP_ERR_LIMIT, "has a QNAME no SAM line holds (empty, '@' in front, or a byte outside 0x21..0x7E)"};
    case Y_REF_NAME: return {PP_ERR_LIMIT, "names a reference whose name no SAM line holds (empty, \"*\", \"=\", or a byte outside 0x21..0x7E)"};
    case Y_QUAL: return {PP_ERR_LIMIT, "has a QUAL byte above 93"};
    case Y_TAG: return {PP_ERR_LIMIT, "has an aux tag that is not [A-Za-z][A-Za-z0-9]"};
    case Y_A: return {PP_ERR_LIMIT, "has an aux A value outside 0x21..0x7E"};
    case Y_Z: return {PP_ERR_LIMIT, "has an aux Z byte outside 0x20..0x7E"};
    case Y_H: return {PP_ERR_LIMIT, "has an aux H that is not an even number of hex digits"};
    default: return {PP_ERR_LIMIT, "has an aux float that is inf or nan"};
    }
}

int decode(pp_ctx *ctx, const char *who, const uint8_t *bytes, uint64_t n_bytes, uint64_t records_at, const uint64_t *rec_off, uint64_t n_rec, int mem,
           const uint8_t *pass, uint64_t n_pass, pp_sam_out **out, uint64_t *bad_record) {
    if (bad_record) *bad_record = ~0ull;
    if (!out) return ctx->fail(PP_ERR_ARG, "%s: null argument", who);
    *out = nullptr;
    if (mem != PP_MEM_HOST && mem != PP_MEM_DEVICE) return ctx->fail(PP_ERR_ARG, "%s: the bytes must be host memory or memory of the context's device", who);
    if ((n_bytes && !bytes) || (n_rec && !rec_off)) return ctx->fail(PP_ERR_ARG, "%s: null bytes with n_bytes > 0, or null rec_off with n_rec > 0", who);
    if (records_at > n_bytes) return ctx->fail(PP_ERR_ARG, "%s: records_at %llu lies behind the %llu bytes", who, (unsigned long long)records_at, (unsigned long long)n_bytes);
    if (n_rec >= 0xFFFFFFFFull) return ctx->fail(PP_ERR_LIMIT, "more than 2^32-1 alignments in one batch");
    if (n_bytes >= (1ull << 40)) return ctx->fail(PP_ERR_LIMIT, "%s: 2^40 or more bytes in one call", who);
    PP_HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const u32 n = (u32)n_rec;
    CallScratch T;  // the copy of host bytes, the header and the per-record arrays: released when the call returns
    StageTimer timer(ctx, ctx->profiling != 0);
    int rc;

    // ---- the header: on the host, from bytes[0, records_at) ----
    std::vector<u8> head;  // ... downloaded, where the bytes are the device's
    const u8 *h_bytes = (const u8 *)bytes;
    if (mem == PP_MEM_DEVICE) {
        try {
            head.resize((size_t)records_at);
        } catch (const std::bad_alloc &) {
            return ctx->fail(PP_ERR_LIMIT, "%s: no host memory for a header of %llu bytes", who, (unsigned long long)records_at);
        }
        if (records_at && (rc = fetch(ctx, bytes, head.data(), (size_t)records_at))) return rc;
        h_bytes = head.data();
    }
    pp_bam_sam_host::Header H;
    {
        size_t cap = 0;
        char *msg = pp_bam_msg_buf_(&cap);
        if (cap) msg[0] = 0;
        if ((rc = pp_bam_sam_host::header_text(h_bytes, records_at, &H, msg, cap))) return ctx->fail(rc, "%s: %s", who, msg);
    }
    const u64 hdr_len = H.text.size();
    std::vector<u8> hdr(H.text.begin(), H.text.end());
    hdr.resize((size_t)((hdr_len + BS_STORE - 1) / BS_STORE * BS_STORE), 0);
    void *d_hdr, *d_names, *d_name_off, *d_ok;
    const u32 n_ref = (u32)H.ok.size();
    if ((rc = T.get(ctx, &d_hdr, hdr.size())) || (rc = T.get(ctx, &d_names, H.names.size())) || (rc = T.get(ctx, &d_name_off, H.name_off.size() * 8)) ||
        (rc = T.get(ctx, &d_ok, H.ok.size())))
        return rc;
    if (!hdr.empty()) PP_HIPCHK(ctx, hipMemcpyAsync(d_hdr, hdr.data(), hdr.size(), hipMemcpyHostToDevice, st));
    if (!H.names.empty()) PP_HIPCHK(ctx, hipMemcpyAsync(d_names, H.names.data(), H.names.size(), hipMemcpyHostToDevice, st));
    PP_HIPCHK(ctx, hipMemcpyAsync(d_name_off, H.name_off.data(), H.name_off.size() * 8, hipMemcpyHostToDevice, st));
    if (n_ref) PP_HIPCHK(ctx, hipMemcpyAsync(d_ok, H.ok.data(), H.ok.size(), hipMemcpyHostToDevice, st));
    const RefTab R{(const u8 *)d_names, (const u64 *)d_name_off, (const u8 *)d_ok, n_ref};

    const u8 *d_bytes = nullptr;
    const u64 *d_rec_off = nullptr;
    if ((rc = on_device(ctx, T, mem, (const u8 *)bytes, (size_t)n_bytes, &d_bytes)) || (rc = on_device(ctx, T, mem, (const u64 *)rec_off, (size_t)n, &d_rec_off)))
        return rc;
    const u32 nb = std::max(1u, (n + BS_RECS - 1u) / BS_RECS);
    void *d_len, *d_seq_at, *d_kind, *d_blk_al, *d_al_base, *d_blk2, *d_blk2off, *d_off, *d_status, *d_pass = nullptr, *d_tile = nullptr;
    if ((rc = T.get(ctx, &d_len, (size_t)n * 8)) || (rc = T.get(ctx, &d_seq_at, (size_t)n * 8)) || (rc = T.get(ctx, &d_kind, (size_t)n)) || (rc = T.get(ctx, &d_blk_al, (size_t)nb * 8)) ||
        (rc = T.get(ctx, &d_al_base, ((size_t)nb + 1) * 8)) || (rc = T.get(ctx, &d_blk2, (size_t)nb * 16)) || (rc = T.get(ctx, &d_blk2off, ((size_t)nb + 1) * 16)) ||
        (rc = T.get(ctx, &d_off, ((size_t)n + 1) * 8)) || (rc = T.get(ctx, &d_status, 16)))
        return rc;

    // ---- pass A: the records, their lengths, the aligned ones ----
    u64 n_al = 0, total = hdr_len, n_fail = 0;
    if (n) {
        PP_HIPCHK(ctx, hipMemsetAsync(d_status, 0xFF, 16, st));
        if ((rc = timer.begin(1))) return rc;
        hipLaunchKernelGGL(k_bs_scan, dim3(nb), dim3(BS_RECS), 0, st, n, d_bytes, (u64)n_bytes, d_rec_off, R, (u64 *)d_len, (u64 *)d_seq_at, (u8 *)d_kind, (u64 *)d_blk_al, (u64 *)d_status);
        if ((rc = timer.end()) || (rc = timer.begin(2))) return rc;
        hipLaunchKernelGGL(k_colscan<1>, dim3(1), dim3(1024), 0, st, (const u64 *)d_blk_al, (u64)nb, (u64 *)d_al_base);
        if ((rc = timer.end())) return rc;
        PP_HIPCHK(ctx, hipGetLastError());
        u64 status = ~0ull;
        if ((rc = fetch(ctx, d_status, &status)) || (rc = fetch(ctx, (const u64 *)d_al_base + nb, &n_al))) return rc;
        if (status != ~0ull) {
            const u64 r = status >> 8;
            const Why w = why_of((u32)(status & 0xFFu));
            if (bad_record) *bad_record = r;
            return ctx->fail(w.code, "%s: record %llu %s", who, (unsigned long long)r, w.what);
        }
    }
    const bool tags = pass != nullptr || n_pass != 0;  // (neither: no verdicts, no tags)
    if (tags) {
        if (n_al && !pass) return ctx->fail(PP_ERR_ARG, "%s: null pass with %llu aligned records", who, (unsigned long long)n_al);
        if (n_pass != n_al) return ctx->fail(PP_ERR_ARG, "%s: %llu verdicts for %llu aligned records", who, (unsigned long long)n_pass, (unsigned long long)n_al);
        if ((rc = T.get(ctx, &d_pass, (size_t)n_al))) return rc;
        if (n_al) PP_HIPCHK(ctx, hipMemcpyAsync(d_pass, pass, (size_t)n_al, hipMemcpyHostToDevice, st));
    }

    // ---- the offsets ----
    if (n) {
        if ((rc = timer.begin(2))) return rc;
        hipLaunchKernelGGL(k_bs_off<false>, dim3(nb), dim3(BS_RECS), 0, st, n, (const u64 *)d_len, (u8 *)d_kind, (const u64 *)d_al_base, (const u8 *)d_pass, hdr_len,
                           (u64 *)d_blk2, (u64 *)nullptr, (u32 *)nullptr);
        hipLaunchKernelGGL(k_colscan<2>, dim3(1), dim3(1024), 0, st, (const u64 *)d_blk2, (u64)nb, (u64 *)d_blk2off);
        if ((rc = timer.end())) return rc;
        PP_HIPCHK(ctx, hipGetLastError());
        u64 totals[2] = {0, 0};
        if ((rc = fetch(ctx, (const u64 *)d_blk2off + 2ull * nb, totals, 2))) return rc;
        total = hdr_len + totals[0];
        n_fail = totals[1];
    }
    if (total >= (1ull << 40)) return ctx->fail(PP_ERR_LIMIT, "%s: an output of 2^40 or more bytes", who);
    if (n) {
        if ((rc = T.get(ctx, &d_tile, (size_t)(total / BS_TILE + 2) * 4)) || (rc = timer.begin(2))) return rc;
        hipLaunchKernelGGL(k_bs_off<true>, dim3(nb), dim3(BS_RECS), 0, st, n, (const u64 *)d_len, (u8 *)d_kind, (const u64 *)d_al_base, (const u8 *)d_pass, hdr_len,
                           (u64 *)d_blk2off, (u64 *)d_off, (u32 *)d_tile);
        if ((rc = timer.end())) return rc;
    }

    // ---- pass B: the bytes ----
    pp_sam_out *P = nullptr;
    uint8_t *d_out = nullptr;
    if ((rc = pp_sam_out_new_(ctx, (total + BS_STORE - 1) / BS_STORE * BS_STORE, &P, &d_out))) return rc;
    std::unique_ptr<pp_sam_out, void (*)(pp_sam_out *)> owner(P, pp_sam_out_free);
    if (total) {
        if ((rc = timer.begin(3))) return rc;
        hipLaunchKernelGGL(k_bs_emit, dim3((unsigned)((total + BS_TILE - 1) / BS_TILE)), dim3(BS_THREADS), 0, st,
                           EmitArgs{d_bytes, (u64)n_bytes, d_rec_off, (const u64 *)d_off, (const u64 *)d_seq_at, (const u8 *)d_kind, (const u32 *)d_tile, (const u8 *)d_hdr, R, hdr_len,
                                    (u64)n, total, d_out});
        if ((rc = timer.end())) return rc;
        PP_HIPCHK(ctx, hipGetLastError());
    }
    PP_HIPCHK(ctx, hipStreamSynchronize(st));  // host inputs may be released, the scratch goes away
    float ms[4] = {0.f, 0.f, 0.f, 0.f};
    if (timer.on && (rc = timer.sums(ms, 4))) return rc;
    u64 hdr_lines = 0;
    for (const char ch : H.text) hdr_lines += ch == '\n' ? 1u : 0u;
    pp_sam_out_set_(P, total, n_al - n_fail, n_fail, hdr_lines + n, timer.on ? ms : nullptr);
    *out = owner.release();
    return PP_OK;
}

}  // namespace

extern "C" int pp_bam_sam(pp_ctx *ctx, const uint8_t *bytes, uint64_t n_bytes, uint64_t records_at, const uint64_t *rec_off, uint64_t n_rec,
                          int mem, const uint8_t *pass, uint64_t n_pass, pp_sam_out **out, uint64_t *bad_record) {
    if (!ctx) return PP_ERR_ARG;
    if (int rdy = pp_ctx_wait(ctx)) return rdy;
    return decode(ctx, "pp_bam_sam", bytes, n_bytes, records_at, rec_off, n_rec, mem, pass, n_pass, out, bad_record);
}

extern "C" int pp_bam_sam_encoded(pp_ctx *ctx, const pp_bam_enc *e, const uint8_t *pass, uint64_t n_pass, pp_sam_out **out, uint64_t *bad_record) {
    if (!ctx) return PP_ERR_ARG;
    if (int rdy = pp_ctx_wait(ctx)) return rdy;
    if (bad_record) *bad_record = ~0ull;
    if (out) *out = nullptr;
    if (!e || !out) return ctx->fail(PP_ERR_ARG, "pp_bam_sam_encoded: null argument");
    const uint8_t *dev = nullptr;  // the object's own device memory
    uint64_t n_bytes = 0, records_at = 0, n_rec = 0;
    pp_bam_enc_bytes(e, &dev, &n_bytes, &records_at);
    const uint64_t *rec_off = pp_bam_enc_rec_off(e, &n_rec);
    return decode(ctx, "pp_bam_sam_encoded", dev, n_bytes, records_at, rec_off, n_rec, PP_MEM_DEVICE, pass, n_pass, out, bad_record);
}

// (internal hook, not part of the header: the tests) the geometry: records per workgroup of pass A, output bytes per workgroup of
// pass B, bytes per store, output bytes per lane and step of the wide parts, lanes per record's group there
extern "C" void pp_bam_sam_geometry_(uint32_t *recs, uint32_t *tile, uint32_t *store, uint32_t *lane, uint32_t *group) {
    if (recs) *recs = BS_RECS;
    if (tile) *tile = BS_TILE;
    if (store) *store = BS_STORE;
    if (lane) *lane = BS_LANE;
    if (group) *group = BS_GROUP;
}

extern "C" int pp_ctx_set_out_sam(pp_ctx *ctx, int on) {
    if (!ctx) return PP_ERR_ARG;
    ctx->out_sam = on != 0;
    return PP_OK;
}

// (internal, the filter drivers: pp_filter_host.cpp)
extern "C" int pp_ctx_out_sam_(const pp_ctx *ctx) { return ctx && ctx->out_sam ? 1 : 0; }
