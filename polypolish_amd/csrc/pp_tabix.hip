// pp_tabix.hip -- pp_tabix_index: the .tbi of a bgzipped, position-sorted, tab-separated text (the polish's VCF, BED and bedGraph, or a
// caller's own), made on the device from the UNCOMPRESSED text and the block table of its pp_bgzf_deflate.
//   newline index   k_in_nl_count, the scan, k_in_nl_write (pp_textin.h): where the lines are
//   rows            k_tx_meta, the scan of the data lines, k_tx_row and -- for the lines whose columns are not closed inside
//                   PP_TBX_LANE_BYTES -- k_tx_long (pp_k_tabix.h): {name length, beg, end} per line, the first refused line
//   names           k_tx_name, the scan of the run heads, k_tx_rec, k_tx_names: the name ids; the heads' names go to the host, which
//                   checks that no name comes back and writes the name list (pp_tabix_host.h)
//   chunks, linear  the table stage of pp_bam_index (pp_k_index.h, pp_rg_sort.h) on one row per line, a meta line a row on no
//                   reference, the flag plane zero; k_tx_span writes a name's span again, over the meta rows between its lines
// The host (pp_tabix_host.h) writes the downloaded tables out; pp_bgzf_deflate compresses them into the .tbi's bytes.
#include "pp_k_tabix.h"
#include "pp_rg_sort.h"
#include "pp_tabix_host.h"

#include <cstring>

namespace {

enum : int { TX_T_NL = 0, TX_T_ROWS = 1, TX_T_NAMES = 2, TX_T_CHUNKS = 3, TX_T_LINEAR = 4 };

const char *tx_what(u32 kind) {
    switch (kind) {
    case TX_EMPTY: return "is an empty data line";
    case TX_NAME: return "has an empty name";
    case TX_COLUMN: return "lacks a column";
    case TX_NUMBER: return "has a position that is not 1 to 10 decimal digits";
    case TX_POS0: return "has POS 0";
    case TX_REF: return "has an empty REF";
    case TX_ENDBEG: return "ends in front of its begin";
    case TX_ORDER: return "begins in front of the line before it: the lines of a name are not in position order";
    default: return "ends behind 2^29: TBI holds positions below 2^29";
    }
}

int to_bytes(pp_ctx *ctx, const std::vector<uint8_t> &v, pp_bytes *out) {
    out->data = (uint8_t *)malloc(v.size() + 1);
    if (!out->data) return ctx->fail(PP_ERR_HIP, "pp_tabix_index: out of host memory");
    if (!v.empty()) memcpy(out->data, v.data(), v.size());
    out->len = v.size();
    return PP_OK;
}

}  // namespace

extern "C" int pp_tabix_index(pp_ctx *ctx, const uint8_t *text, uint64_t n_bytes, int mem, int preset, const uint64_t *blk_off, uint64_t n_blk,
                              int blk_mem, pp_bytes *tbi, pp_bytes *raw, uint64_t *bad_line) {
    if (!ctx) return PP_ERR_ARG;
    if (int rdy = pp_ctx_wait(ctx)) return rdy;
    if (bad_line) *bad_line = ~0ull;
    if (raw) {
        raw->data = nullptr;
        raw->len = 0;
    }
    if (!tbi) return ctx->fail(PP_ERR_ARG, "pp_tabix_index: null argument");
    tbi->data = nullptr;
    tbi->len = 0;
    if ((mem != PP_MEM_HOST && mem != PP_MEM_DEVICE) || (blk_mem != PP_MEM_HOST && blk_mem != PP_MEM_DEVICE))
        return ctx->fail(PP_ERR_ARG, "pp_tabix_index: the text and the block offsets must be host memory or memory of the context's device");
    if (preset != PP_TBX_VCF && preset != PP_TBX_BED) return ctx->fail(PP_ERR_ARG, "pp_tabix_index: unknown preset %d", preset);
    if ((n_bytes && !text) || !blk_off) return ctx->fail(PP_ERR_ARG, "pp_tabix_index: null text or blk_off");
    if (n_bytes >= (1ull << 40)) return ctx->fail(PP_ERR_LIMIT, "pp_tabix_index: 2^40 or more bytes in one call");
    if (n_blk != (n_bytes + IX_PAY - 1u) / IX_PAY)
        return ctx->fail(PP_ERR_ARG, "pp_tabix_index: %llu block offsets and one for a stream of %llu bytes, which has %llu blocks", (unsigned long long)n_blk,
                         (unsigned long long)n_bytes, (unsigned long long)((n_bytes + IX_PAY - 1u) / IX_PAY));
    PP_HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    CallScratch T;
    CtxScratch S(ctx, ctx->g_rec, "pp_tabix_index");  // (scan_u32's block sums)
    StageTimer timer(ctx, ctx->profiling != 0);       // newline index | rows | names | chunks | linear (pp_tabix_stage_ms_)
    ctx->tbx_timed = false;
    int rc;
    const u8 *d_text = nullptr;
    const u64 *d_blk = nullptr;
    if ((rc = on_device(ctx, T, mem, (const u8 *)text, (size_t)n_bytes, &d_text)) || (rc = on_device(ctx, T, blk_mem, (const u64 *)blk_off, (size_t)n_blk + 1, &d_blk)))
        return rc;
    u64 *d_status;
    if ((rc = T.alloc(ctx, d_status, 4))) return rc;
    PP_HIPCHK(ctx, hipMemsetAsync(d_status, 0xFF, 32, st));
    {
        hipLaunchKernelGGL(k_tx_blk, dim3((unsigned)((n_blk + 256u) / 256u)), dim3(256), 0, st, (u64)n_blk + 1u, d_blk, d_status + 1);
        PP_HIPCHK(ctx, hipGetLastError());
        u64 far = ~0ull;
        if ((rc = fetch(ctx, d_status + 1, &far))) return rc;
        if (far != ~0ull) return ctx->fail(PP_ERR_LIMIT, "pp_tabix_index: block %llu starts at 2^48 or behind: a virtual offset cannot hold it", (unsigned long long)far);
    }

    // ---- the newline index ----
    const u64 nlb = std::max<u64>(1, (n_bytes + IN_NL_BLOCK - 1u) / IN_NL_BLOCK);
    u32 *d_nl_cnt;
    u64 *d_nl_off, *d_nl_pos;
    u64 n_nl = 0, last_nl = ~0ull;
    if ((rc = T.alloc(ctx, d_nl_cnt, (size_t)nlb)) || (rc = T.alloc(ctx, d_nl_off, (size_t)nlb + 1))) return rc;
    if ((rc = timer.begin(TX_T_NL))) return rc;
    hipLaunchKernelGGL(k_in_nl_count<false>, dim3((unsigned)nlb), dim3(1024), 0, st, d_text, (u64)n_bytes, d_nl_cnt);
    if ((rc = scan_u32<u64>(ctx, S.sums(), S.sums_off(), d_nl_cnt, nlb, d_nl_off))) return rc;
    if ((rc = timer.end())) return rc;
    PP_HIPCHK(ctx, hipGetLastError());
    if ((rc = fetch(ctx, d_nl_off + nlb, &n_nl))) return rc;
    if ((rc = T.alloc(ctx, d_nl_pos, (size_t)n_nl))) return rc;
    if (n_nl) {
        if ((rc = timer.begin(TX_T_NL))) return rc;
        hipLaunchKernelGGL(k_in_nl_write, dim3((unsigned)nlb), dim3(1024), 0, st, d_text, (u64)n_bytes, (const u64 *)d_nl_off, d_nl_pos);
        if ((rc = timer.end())) return rc;
        PP_HIPCHK(ctx, hipGetLastError());
        if ((rc = fetch(ctx, d_nl_pos + (n_nl - 1u), &last_nl))) return rc;
    }
    const u64 n_lines = n_nl + ((n_bytes && (n_nl == 0 || last_nl + 1u != n_bytes)) ? 1u : 0u);  // (last bytes without a '\n' are a line)
    if (n_lines > 0xFFFFFFFEull) return ctx->fail(PP_ERR_LIMIT, "pp_tabix_index: more than 2^32 - 2 lines");
    const u32 n = (u32)n_lines;
    const TxLines Ln{d_nl_pos, n_nl, n_bytes};
    const unsigned gb = std::max(1u, (unsigned)(((u64)n + 255u) / 256u));

    // ---- the rows and the names ----
    namespace ih = pp_bam_index_host;
    namespace th = pp_tabix_host;
    std::vector<uint64_t> h_key, h_beg, h_end, h_lin, h_name_off(1, 0), h_ref[4];
    std::vector<u32> h_intv;
    std::vector<uint8_t> h_names;
    uint64_t n_chunk = 0;
    u32 n_ref = 0;
    u32 *d_is_data, *d_didx, *d_dline, *d_long, *d_n_long, *d_head, *d_hidx, *d_bin, *d_head_line, *d_head_len;
    u64 *d_start, *d_name_off;
    TxRow *d_row;
    IxRec *d_rec;
    uint16_t *d_flag;
    if (n) {
        if ((rc = T.alloc(ctx, d_is_data, (size_t)n)) || (rc = T.alloc(ctx, d_didx, (size_t)n + 1)) || (rc = T.alloc(ctx, d_dline, (size_t)n)) ||
            (rc = T.alloc(ctx, d_long, (size_t)n)) || (rc = T.alloc(ctx, d_n_long, 4)) || (rc = T.alloc(ctx, d_head, (size_t)n)) ||
            (rc = T.alloc(ctx, d_hidx, (size_t)n + 1)) || (rc = T.alloc(ctx, d_bin, (size_t)n)) || (rc = T.alloc(ctx, d_start, (size_t)n + 2)) ||
            (rc = T.alloc(ctx, d_row, (size_t)n)) || (rc = T.alloc(ctx, d_rec, (size_t)n)) || (rc = T.alloc(ctx, d_flag, (size_t)n)))
            return rc;
        PP_HIPCHK(ctx, hipMemsetAsync(d_n_long, 0, 16, st));
        PP_HIPCHK(ctx, hipMemsetAsync(d_flag, 0, std::max<size_t>((size_t)n * 2, 16), st));
        if ((rc = timer.begin(TX_T_ROWS))) return rc;
        hipLaunchKernelGGL(k_tx_meta, dim3(gb), dim3(256), 0, st, n, d_text, Ln, d_is_data, d_start);
        if ((rc = scan_u32<u32>(ctx, S.sums(), S.sums_off(), (const u32 *)d_is_data, (u64)n, d_didx))) return rc;
        hipLaunchKernelGGL(k_tx_row, dim3(gb), dim3(256), 0, st, n, d_text, Ln, preset, (const u32 *)d_is_data, (const u32 *)d_didx, d_dline, d_row, d_long, d_n_long,
                           d_status);
        if ((rc = timer.end())) return rc;
        PP_HIPCHK(ctx, hipGetLastError());
        u32 n_long = 0;
        if ((rc = fetch(ctx, d_n_long, &n_long))) return rc;
        if ((rc = timer.begin(TX_T_ROWS))) return rc;
        if (n_long)
            hipLaunchKernelGGL(k_tx_long, dim3(std::min(n_long, 1u << 20)), dim3(256), 0, st, n_long, (const u32 *)d_long, d_text, Ln, preset, d_row, d_status);
        if ((rc = timer.end()) || (rc = timer.begin(TX_T_NAMES))) return rc;
        hipLaunchKernelGGL(k_tx_name, dim3(gb), dim3(256), 0, st, n, d_text, Ln, (const TxRow *)d_row, (const u32 *)d_didx, (const u32 *)d_dline, d_head, d_status);
        if ((rc = scan_u32<u32>(ctx, S.sums(), S.sums_off(), (const u32 *)d_head, (u64)n, d_hidx))) return rc;
        if ((rc = timer.end())) return rc;
        PP_HIPCHK(ctx, hipGetLastError());
        u64 bad = ~0ull;
        u32 n_head = 0;
        if ((rc = fetch(ctx, d_status, &bad)) || (rc = fetch(ctx, d_hidx + n, &n_head))) return rc;
        // the run heads' lines, name lengths and names (with a refused line: of the heads in front of it, whose rows are good)
        std::vector<u32> h_head_line(n_head), h_head_len(n_head);
        if (n_head) {
            if ((rc = T.alloc(ctx, d_head_line, (size_t)n_head)) || (rc = T.alloc(ctx, d_head_len, (size_t)n_head)) || (rc = T.alloc(ctx, d_name_off, (size_t)n_head + 1)))
                return rc;
            if ((rc = timer.begin(TX_T_NAMES))) return rc;
            hipLaunchKernelGGL(k_tx_rec, dim3(gb), dim3(256), 0, st, n, (const TxRow *)d_row, (const u32 *)d_head, (const u32 *)d_hidx, d_rec, d_bin, d_head_line, d_head_len);
            if ((rc = scan_u32<u64>(ctx, S.sums(), S.sums_off(), (const u32 *)d_head_len, (u64)n_head, d_name_off))) return rc;
            if ((rc = timer.end())) return rc;
            PP_HIPCHK(ctx, hipGetLastError());
            h_name_off.resize((size_t)n_head + 1);
            if ((rc = fetch(ctx, d_head_line, h_head_line.data(), n_head)) || (rc = fetch(ctx, d_name_off, h_name_off.data(), (size_t)n_head + 1))) return rc;
        }
        u32 n_good = n_head;  // the heads in front of the first refused line
        if (bad != ~0ull) n_good = (u32)(std::lower_bound(h_head_line.begin(), h_head_line.end(), (u32)(bad >> 8)) - h_head_line.begin());
        if (n_good && h_name_off[n_good] >= th::MAX_L_NM && bad == ~0ull)
            return ctx->fail(PP_ERR_LIMIT, "pp_tabix_index: the names take 2^31 bytes or more");
        if (n_good && h_name_off[n_good] < th::MAX_L_NM) {
            u8 *d_names;
            const u64 l_names = h_name_off[n_good];
            if ((rc = T.alloc(ctx, d_names, (size_t)l_names))) return rc;
            if ((rc = timer.begin(TX_T_NAMES))) return rc;
            hipLaunchKernelGGL(k_tx_names, dim3(std::min(n_good, 1u << 20)), dim3(256), 0, st, n_good, d_text, Ln, (const u32 *)d_head_line, (const u64 *)d_name_off, d_names);
            if ((rc = timer.end())) return rc;
            PP_HIPCHK(ctx, hipGetLastError());
            h_names.resize((size_t)l_names);
            if ((rc = fetch(ctx, d_names, h_names.data(), (size_t)l_names))) return rc;
            const uint64_t back = th::first_repeat(h_names.data(), h_name_off.data(), n_good);
            if (back < n_good) {  // (in front of the refused line, if there is one)
                if (bad_line) *bad_line = h_head_line[back];
                return ctx->fail(PP_ERR_ARG, "pp_tabix_index: line %llu names a sequence that other names followed: the lines of a name are not consecutive",
                                 (unsigned long long)h_head_line[back]);
            }
        }
        if (bad != ~0ull) {
            const u32 kind = (u32)(bad & 0xFFu);
            if (bad_line) *bad_line = bad >> 8;
            return ctx->fail(kind == TX_END ? PP_ERR_LIMIT : PP_ERR_ARG, "pp_tabix_index: line %llu %s", (unsigned long long)(bad >> 8), tx_what(kind));
        }
        if (n_head > IX_MAX_REF) return ctx->fail(PP_ERR_LIMIT, "pp_tabix_index: more than 2^24 names");
        n_ref = n_head;
    }
    h_intv.assign(n_ref, 0);
    std::vector<uint64_t> h_lin_off((size_t)n_ref + 1, 0);
    for (auto &v : h_ref) v.assign(n_ref, 0);

    // ---- the tables: pp_bam_index's, the name's index as the reference id ----
    if (n_ref) {
        const IxWhere W{(const u64 *)d_start, d_blk};
        u32 *d_chead, *d_cidx, *d_intv;
        u64 *d_ref4, *d_nc;
        if ((rc = T.alloc(ctx, d_chead, (size_t)n)) || (rc = T.alloc(ctx, d_cidx, (size_t)n + 1)) || (rc = T.alloc(ctx, d_intv, (size_t)n_ref)) ||
            (rc = T.alloc(ctx, d_ref4, (size_t)n_ref * 4)) || (rc = T.alloc(ctx, d_nc, 1)))
            return rc;
        u64 *const d_rb = d_ref4, *const d_re = d_rb + n_ref, *const d_map = d_re + n_ref, *const d_unm = d_map + n_ref;
        PP_HIPCHK(ctx, hipMemsetAsync(d_intv, 0, std::max<size_t>((size_t)n_ref * 4, 16), st));
        PP_HIPCHK(ctx, hipMemsetAsync(d_ref4, 0, std::max<size_t>((size_t)n_ref * 32, 16), st));
        PP_HIPCHK(ctx, hipMemsetAsync(d_nc, 0, 8, st));
        if ((rc = timer.begin(TX_T_CHUNKS))) return rc;
        hipLaunchKernelGGL(k_ix_run, dim3(gb), dim3(256), 0, st, n, (const IxRec *)d_rec, (const u32 *)d_bin, d_chead);
        if ((rc = scan_u32<u32>(ctx, S.sums(), S.sums_off(), (const u32 *)d_chead, (u64)n, d_cidx))) return rc;
        if ((rc = timer.end()) || (rc = timer.begin(TX_T_LINEAR))) return rc;
        hipLaunchKernelGGL(k_ix_ref, dim3(gb), dim3(256), 0, st, n, (const IxRec *)d_rec, (const uint16_t *)d_flag, W, d_intv, d_rb, d_re, d_map, d_unm, d_nc);
        hipLaunchKernelGGL(k_tx_span, dim3(gb), dim3(256), 0, st, n, (const IxRec *)d_rec, (const u32 *)d_head, (const u32 *)d_didx, (const u32 *)d_dline, W, d_rb, d_re);
        if ((rc = timer.end())) return rc;
        PP_HIPCHK(ctx, hipGetLastError());
        u32 nc32 = 0;
        if ((rc = fetch(ctx, d_cidx + n, &nc32)) || (rc = fetch(ctx, d_intv, h_intv.data(), n_ref))) return rc;
        n_chunk = nc32;
        for (int k = 0; k < 4; k++)
            if ((rc = fetch(ctx, d_rb + (size_t)k * n_ref, h_ref[k].data(), n_ref))) return rc;
        for (u32 r = 0; r < n_ref; r++) h_lin_off[r + 1] = h_lin_off[r] + h_intv[r];
        const u64 n_win = h_lin_off[n_ref];
        if (n_win > IX_MAX_WINDOWS) return ctx->fail(PP_ERR_LIMIT, "pp_tabix_index: %llu windows of 16,384 bases in the linear index, above 2^27", (unsigned long long)n_win);
        if (n_win) {
            u64 *d_lin_off, *d_lin;
            if ((rc = T.alloc(ctx, d_lin_off, (size_t)n_ref + 1)) || (rc = T.alloc(ctx, d_lin, (size_t)n_win))) return rc;
            PP_HIPCHK(ctx, hipMemcpyAsync(d_lin_off, h_lin_off.data(), ((size_t)n_ref + 1) * 8, hipMemcpyHostToDevice, st));
            PP_HIPCHK(ctx, hipMemsetAsync(d_lin, 0xFF, (size_t)n_win * 8, st));
            if ((rc = timer.begin(TX_T_LINEAR))) return rc;
            hipLaunchKernelGGL(k_ix_lin, dim3(gb), dim3(256), 0, st, n, (const IxRec *)d_rec, W, (const u64 *)d_lin_off, d_lin);
            hipLaunchKernelGGL(k_ix_fill, dim3((n_ref + 255u) / 256u), dim3(256), 0, st, n_ref, (const u64 *)d_lin_off, d_lin);
            if ((rc = timer.end())) return rc;
            PP_HIPCHK(ctx, hipGetLastError());
            h_lin.resize((size_t)n_win);
            if ((rc = fetch(ctx, d_lin, h_lin.data(), (size_t)n_win))) return rc;
        }
        if (n_chunk) {  // the chunk table, then its order
            const u32 m = (u32)n_chunk;
            const unsigned gm = (unsigned)(((u64)m + 255u) / 256u);
            const u32 m_tiles = (u32)(((u64)m + RG_TILE - 1u) / RG_TILE);
            const u64 m_cnt = 256ull * m_tiles;
            u64 *d_key[2], *d_beg, *d_end, *d_sb, *d_se;
            u32 *d_idx[2], *d_cnt, *d_off;
            if ((rc = T.alloc(ctx, d_key[0], (size_t)m)) || (rc = T.alloc(ctx, d_key[1], (size_t)m)) || (rc = T.alloc(ctx, d_beg, (size_t)m)) ||
                (rc = T.alloc(ctx, d_end, (size_t)m)) || (rc = T.alloc(ctx, d_idx[0], (size_t)m)) || (rc = T.alloc(ctx, d_idx[1], (size_t)m)) ||
                (rc = T.alloc(ctx, d_cnt, (size_t)m_cnt)) || (rc = T.alloc(ctx, d_off, (size_t)m_cnt + 1)) || (rc = T.alloc(ctx, d_sb, (size_t)m)) ||
                (rc = T.alloc(ctx, d_se, (size_t)m)))
                return rc;
            if ((rc = timer.begin(TX_T_CHUNKS))) return rc;
            hipLaunchKernelGGL(k_ix_chunk, dim3(gb), dim3(256), 0, st, n, (const IxRec *)d_rec, (const u32 *)d_bin, (const u32 *)d_chead, (const u32 *)d_cidx, W, d_key[0],
                               d_beg, d_end);
            u32 shifts[6], passes = 0;
            shifts[passes++] = 0;
            shifts[passes++] = 8;  // bins are below 2^16
            for (u32 top = n_ref - 1u, b = 0; top; top >>= 8, b++) shifts[passes++] = 32u + 8u * b;
            const u32 *idx_in = nullptr;
            for (u32 p = 0; p < passes; p++) {
                const u64 *const key_in = d_key[p & 1u];
                u64 *const key_out = d_key[(p + 1u) & 1u];
                u32 *const idx_out = d_idx[p & 1u];
                hipLaunchKernelGGL(k_rg_hist<u64>, dim3(m_tiles), dim3(RG_BLOCK), 0, st, m, key_in, shifts[p], m_tiles, d_cnt);
                if ((rc = scan_u32<u32>(ctx, S.sums(), S.sums_off(), (const u32 *)d_cnt, m_cnt, d_off))) return rc;
                hipLaunchKernelGGL(k_rg_scatter<u64>, dim3(m_tiles), dim3(RG_BLOCK), 0, st, m, key_in, idx_in, shifts[p], m_tiles, (const u32 *)d_off, key_out, idx_out);
                idx_in = idx_out;
            }
            hipLaunchKernelGGL(k_ix_gather, dim3(gm), dim3(256), 0, st, m, idx_in, (const u64 *)d_beg, (const u64 *)d_end, d_sb, d_se);
            if ((rc = timer.end())) return rc;
            PP_HIPCHK(ctx, hipGetLastError());
            h_key.resize(m);
            h_beg.resize(m);
            h_end.resize(m);
            if ((rc = fetch(ctx, d_key[passes & 1u], h_key.data(), m)) || (rc = fetch(ctx, d_sb, h_beg.data(), m)) || (rc = fetch(ctx, d_se, h_end.data(), m))) return rc;
        }
    }
    PP_HIPCHK(ctx, hipStreamSynchronize(st));
    if (timer.on) {
        if ((rc = timer.sums(ctx->tbx_ms, 5))) return rc;
        ctx->tbx_timed = true;
    }
    ih::Tables Tb;
    Tb.n_ref = n_ref;
    Tb.n_chunk = n_chunk;
    Tb.chunk_key = h_key.data();
    Tb.chunk_beg = h_beg.data();
    Tb.chunk_end = h_end.data();
    Tb.n_intv = h_intv.data();
    Tb.lin_off = h_lin_off.data();
    Tb.lin = h_lin.data();
    Tb.ref_beg = h_ref[0].data();
    Tb.ref_end = h_ref[1].data();
    Tb.mapped = h_ref[2].data();
    Tb.unmapped = h_ref[3].data();
    Tb.n_no_coor = 0;  // (a meta line is on no name, and is not counted)
    th::Head H;
    H.format = preset == PP_TBX_VCF ? 2 : 0x10000;
    H.col_seq = 1;
    H.col_beg = 2;
    H.col_end = preset == PP_TBX_VCF ? 0 : 3;
    std::vector<uint8_t> file;
    char msg[200];
    msg[0] = 0;
    if ((rc = th::serialise(Tb, H, h_names.data(), h_name_off.data(), &file, msg, sizeof msg))) return ctx->fail(rc, "%s", msg);

    // ---- the .tbi: the raw bytes as a BGZF file ----
    pp_bgzf_out *z = nullptr;
    if ((rc = pp_bgzf_deflate(ctx, file.data(), file.size(), PP_MEM_HOST, &z))) return rc;
    const uint8_t *d_z = nullptr;
    uint64_t n_z = 0;
    pp_bgzf_out_bytes(z, &d_z, &n_z);
    std::vector<uint8_t> packed((size_t)n_z);
    rc = PP_OK;
    if (n_z && hipMemcpyAsync(packed.data(), d_z, (size_t)n_z, hipMemcpyDeviceToHost, st) != hipSuccess) rc = PP_ERR_HIP;
    if (!rc && hipStreamSynchronize(st) != hipSuccess) rc = PP_ERR_HIP;
    pp_bgzf_out_free(z);
    if (rc) return ctx->fail(rc, "pp_tabix_index: the download of the compressed index failed");
    if ((rc = to_bytes(ctx, packed, tbi))) return rc;
    if (raw && (rc = to_bytes(ctx, file, raw))) {
        pp_bytes_free(tbi);
        return rc;
    }
    return PP_OK;
}

// (internal hook, not part of the header: tools/tabix_timing.py) the HIP-event time of the context's last pp_tabix_index by stage:
// newline index | rows | names | chunks | linear; PP_ERR_ARG where the context had no profiling on
extern "C" int pp_tabix_stage_ms_(const pp_ctx *ctx, float *ms5) {
    if (!ctx || !ms5 || !ctx->tbx_timed) return PP_ERR_ARG;
    std::copy(ctx->tbx_ms, ctx->tbx_ms + 5, ms5);
    return PP_OK;
}

// ---- the file drivers' indexes (pp_driver.cpp) ----
extern "C" int pp_ctx_set_tbi(pp_ctx *ctx, int vcf, int bed, int depth) {
    if (!ctx) return PP_ERR_ARG;
    ctx->tbi_on[PP_TBI_VCF] = vcf != 0;
    ctx->tbi_on[PP_TBI_BED] = bed != 0;
    ctx->tbi_on[PP_TBI_DEPTH] = depth != 0;
    return PP_OK;
}
extern "C" int pp_ctx_tbi(pp_ctx *ctx, int which, pp_bytes *tbi) {
    if (!ctx) return PP_ERR_ARG;
    if (!tbi) return ctx->fail(PP_ERR_ARG, "pp_ctx_tbi: null argument");
    *tbi = pp_bytes{nullptr, 0};
    if (which < 0 || which > PP_TBI_DEPTH) return ctx->fail(PP_ERR_ARG, "pp_ctx_tbi: unknown track %d", which);
    if (!ctx->tbi_made[which]) return ctx->fail(PP_ERR_ARG, "pp_ctx_tbi: no driver has made that index with pp_ctx_set_tbi on this context");
    tbi->data = (uint8_t *)malloc(ctx->tbi_bytes[which].size() + 1);
    if (!tbi->data) return ctx->fail(PP_ERR_HIP, "pp_ctx_tbi: out of host memory");
    memcpy(tbi->data, ctx->tbi_bytes[which].data(), ctx->tbi_bytes[which].size());
    tbi->len = ctx->tbi_bytes[which].size();
    return PP_OK;
}
// (internal, the file drivers) what pp_ctx_set_tbi was given; the index a driver made (data == NULL: none)
extern "C" int pp_ctx_tbi_form_(const pp_ctx *ctx, int which) { return ctx && which >= 0 && which <= PP_TBI_DEPTH && ctx->tbi_on[which] ? 1 : 0; }
extern "C" void pp_ctx_keep_tbi_(pp_ctx *ctx, int which, const uint8_t *data, uint64_t n) {
    ctx->tbi_made[which] = data != nullptr;
    ctx->tbi_bytes[which].assign(data ? (const char *)data : "", data ? (size_t)n : 0);
    if (!data) ctx->tbi_bytes[which].shrink_to_fit();
}
