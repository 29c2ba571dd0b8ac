// pp_sam.hip -- pp_sam_records: the lines of SAM TEXT as a pp_raw_batch, decoded on the device: the second front end of the record
// chain names -> filter -> regroup -> gate -> prepare -> polish, the text twin of pp_bam_records (pp_bam.hip).  The two fused text
// routes (pp_tokenize.hip: text -> gated pp_aln_batch; pp_filter_dev.hip: text -> the filter's input) leave no raw records behind;
// this one leaves nothing else.  The chain's write side for text is pp_sam_out.hip: pp_sam_tagged_records reads this object's copy
// of the text (through pp_sam_names) and splices the filter's verdicts into it.
//
// The object owns ONE device copy of the text, padded with zeros behind its end as pp_devtext.h asks (the newline kernels read whole
// blocks, stage_wave_lines and find_tab read a few bytes past a line).  Every kernel reads that copy and nothing else; raw.seq IS the
// copy, seq_off[r] the offset of the record's SEQ column in it, and the QNAME / RNAME ranges point into it: no rooms, no upper-casing,
// no second set of SEQ bytes.
//   newline_index  pp_devtext.h: count, scan, write
//   k_sam_scan     the hot pass, one lane per line, the wave's 64 lines through LDS (stage_wave_lines, three stage sizes):
//                  Alignment::new (src/alignment.rs:49-98) as tok_parse_line of pp_tokenize.hip and parse_chunk of pp_ingest.cpp
//                  restate it -- the eleven columns, FLAG, POS, the tag walk for NM:i: and ZP:Z:fail, get_expanded_cigar with its runs
//                  counted -- then what a raw batch cannot hold.  A refusal is status = line << 8 | kind by atomicMin: the first line
//                  in file order wins, whatever its kind.  Per line: kind (skipped | unaligned record | aligned record) and a SamLine
//   k_sam_place    the record index of every line, the aligned rank of every record and cig_off by the workgroup scan of pp_dev.h
//                  (sums per workgroup, k_colscan over them), then the per-line results compacted into the per-record arrays, the
//                  ranges, the line numbers, and the pass byte at the aligned rank
//   k_sam_cigar    one lane per record: the CIGAR text (validated by the scan) packed into its runs, as k_tok_meta's loop does
// k_sam_scan does not share tok_parse_line: that one looks the contig up, drops unaligned lines and keeps other fields; it is left
// as it is, and this parse stands on the same small helpers (find_tab, parse_u, op_code, report).
// The sentence of a refused line is the host ingest's: the device only decides WHICH line, the host parser then runs on that line.
#include "pp_devtext.h"

#include <cstring>

extern "C" int pp_ingest_line_error_(const char *path, const char *line, size_t n, uint64_t line_no, char *err, size_t errlen);

struct pp_sam : DevOwner {
    using DevOwner::DevOwner;
    RawArrays a;                       // a.seq: the owned device copy of the text, zeros behind n_bytes
    u64 *name_off = nullptr, *rname_off = nullptr;  // the QNAME and RNAME ranges, in the text
    u32 *name_len = nullptr, *rname_len = nullptr, *line = nullptr;
    uint64_t n_bytes = 0;
    pp_raw_batch view{};
    std::vector<uint8_t> pass;         // HOST: one byte per aligned record, 0 = ZP:Z:fail
    uint64_t first_empty = ~0ull;      // the first line without a byte (or with "\r" only), 0-based; ~0: none
    uint64_t first_nameless = ~0ull;   // the first record line whose QNAME is empty; ~0: none (pp_sam_empty_qname_rule_ has work only then)
    StageMs<5> t;                      // the device copy | newline index | scan | scans and compaction | CIGAR pack
};

namespace {

constexpr u32 SAM_BLOCK = 1024;  // lines per workgroup of the placing kernel
enum : u32 { SK_SKIP = 0, SK_UNALIGNED = 1, SK_ALIGNED = 2 };          // kind[line]
enum : u32 { SR_PARSE = 1, SR_FLAG = 2, SR_POS = 3, SR_SEQ = 4 };      // status: line << 8 | why it is refused

struct SamLine {  // one record line (offsets relative to the start of the line, where its QNAME begins)
    u32 flag, ref_start, nm, n_runs;  // flag: FLAG | ZP:Z:fail << 16
    u32 name_len, rname_off, rname_len, cig_off;
    u32 cig_len, seq_off, seq_len, pad;  // seq_len 0: SEQ is "*"
};

struct SamOut {  // the per-record arrays (device memory)
    uint16_t *flag;
    u32 *ref_start, *nm, *seq_len, *n_cig, *name_len, *rname_len, *line;
    u64 *seq_off, *cig_off, *name_off, *rname_off;
    u8 *pass;
};

// Alignment::new on one line.  kind[li] is written for every line; rec[li] for the records.  status[0]: the first refused line;
// status[1]: the first empty line (pp_sam_first_empty_line), which this parse skips; status[2]: the first record with an empty QNAME.
__device__ __forceinline__ void sam_parse_line(const u8 *L, u32 n, u64 li, SamLine *__restrict__ rec, u32 *__restrict__ kind,
                                               u64 *__restrict__ status) {
    kind[li] = SK_SKIP;  // (a refused line, too: the scans behind this kernel run before anybody looks at the status)
    if (n == 0) { report(status + 1, li); return; }
    if (L[0] == (u8)'@') return;  // alignment.rs:241
    const u64 refused = (li << 8) | SR_PARSE;
    u32 cs[11], cl[11], nc = 0, q = 0;
    while (nc < 11) {
        const u32 t = find_tab(L, q, n);
        cs[nc] = q;
        cl[nc] = t - q;
        nc++;
        if (t >= n) { q = n + 1; break; }
        q = t + 1;
    }
    if (nc < 11) { report(status, refused); return; }  // too few columns
    u64 flags, pos;
    if (!parse_u(L + cs[1], cl[1], 0xFFFFFFFFull, flags) || !parse_u(L + cs[3], cl[3], ~0ull, pos)) { report(status, refused); return; }
    u32 nm = 0xFFFFFFFFu, zp_fail = 0;
    u32 tg = q;  // start of the tag fields; q == n means one empty field after a trailing tab; n + 1: none
    while (tg <= n) {
        const u32 t = find_tab(L, tg, n);
        const u32 tl = t - tg;
        const u8 *f = L + tg;
        if (tl >= 5 && f[0] == 'N' && f[1] == 'M' && f[2] == ':' && f[3] == 'i' && f[4] == ':') {
            u64 v;
            if (!parse_u(f + 5, tl - 5, 0xFFFFFFFFull, v)) { report(status, refused); return; }
            nm = (u32)v;
        }
        if (tl == 9 && (f[0] | 32) == 'z' && (f[1] | 32) == 'p' && f[2] == ':' && (f[3] | 32) == 'z' && f[4] == ':' &&
            (f[5] | 32) == 'f' && (f[6] | 32) == 'a' && (f[7] | 32) == 'i' && (f[8] | 32) == 'l')
            zp_fail = 1;
        if (t >= n) break;
        tg = t + 1;
    }
    if (nm == 0xFFFFFFFFu && (flags & 4) == 0) { report(status, refused); return; }  // missing NM tag
    // get_expanded_cigar (alignment.rs:325-346), kept as runs: zero-length runs vanish, long runs are cut
    const u8 *cg = L + cs[5];
    const u32 cgl = cl[5];
    u32 n_runs = 0;
    if (!(cgl == 1 && cg[0] == (u8)'*')) {
        u32 i = 0;
        while (i < cgl) {
            u32 j = i;
            while (j < cgl && cg[j] >= (u8)'0' && cg[j] <= (u8)'9') j++;
            const int op = j < cgl ? op_code(cg[j]) : -1;
            u64 num;
            if (j == i || op < 0 || !parse_u(cg + i, j - i, 0xFFFFFFFFull, num)) { report(status, refused); return; }
            n_runs += (u32)((num + 0x0FFFFFFEull) / 0x0FFFFFFFull);  // pieces of at most 2^28-1
            i = j + 1;
        }
    }
    // the reference takes the line: what a raw batch cannot hold
    const bool aligned = (flags & 4) == 0;
    const u32 limit = flags > 0xFFFFull ? SR_FLAG : (pos > 0xFFFFFFFFull ? SR_POS : ((aligned && cl[9] == 0) ? SR_SEQ : 0u));
    if (limit) { report(status, (li << 8) | limit); return; }
    SamLine r;
    r.flag = (u32)flags | (zp_fail << 16);
    r.ref_start = (u32)(pos > 0 ? pos - 1 : 0);
    r.nm = nm;
    r.n_runs = n_runs;
    r.name_len = cl[0];
    if (cl[0] == 0) report(status + 2, li);
    r.rname_off = cs[2];
    r.rname_len = cl[2];
    r.cig_off = cs[5];
    r.cig_len = cgl;
    r.seq_off = cs[9];
    r.seq_len = (cl[9] == 1 && L[cs[9]] == (u8)'*') ? 0u : cl[9];
    r.pad = 0;
    rec[li] = r;
    kind[li] = aligned ? SK_ALIGNED : SK_UNALIGNED;
}

template <u32 TOK_STAGE>
__global__ __launch_bounds__(64) void k_sam_scan(const u8 *__restrict__ text, u64 size, const u64 *__restrict__ nl_pos, u64 n_nl,
                                                 u64 n_lines, SamLine *__restrict__ rec, u32 *__restrict__ kind,
                                                 u64 *__restrict__ status) {
    __shared__ __attribute__((aligned(16))) u8 stage[TOK_STAGE + 32];
    const u8 *L;
    u32 n;
    u64 li;
    if (stage_wave_lines<TOK_STAGE>(text, size, nl_pos, n_nl, n_lines, stage, &L, &n, &li)) sam_parse_line(L, n, li, rec, kind, status);
}

// PLACE == false: the workgroups' numbers of records, of aligned records and of CIGAR runs (blk3: three words per workgroup).
// PLACE == true: blk3 holds their exclusive scan: every record line's results go to the record's place, the pass byte to its rank.
template <bool PLACE>
__global__ __launch_bounds__(SAM_BLOCK) void k_sam_place(u64 n_lines, const u32 *__restrict__ kind, const SamLine *__restrict__ rec,
                                                         const u64 *__restrict__ nl_pos, u64 *__restrict__ blk3, SamOut O) {
    __shared__ u64 s_w[SAM_BLOCK / 64];
    const u64 li = (u64)blockIdx.x * SAM_BLOCK + threadIdx.x;
    const u32 k = li < n_lines ? kind[li] : (u32)SK_SKIP;
    const u32 is_rec = k != SK_SKIP ? 1u : 0u, al = k == SK_ALIGNED ? 1u : 0u;
    const u32 nr = is_rec ? rec[li].n_runs : 0u;
    u64 t_rec, t_al, t_cig;
    const u64 ex_rec = block_scan_excl64<SAM_BLOCK>(is_rec, s_w, &t_rec);
    const u64 ex_al = block_scan_excl64<SAM_BLOCK>(al, s_w, &t_al);
    const u64 ex_cig = block_scan_excl64<SAM_BLOCK>(nr, s_w, &t_cig);
    u64 *const mine = blk3 + 3ull * blockIdx.x;
    if (!PLACE) {
        if (threadIdx.x == 0) { mine[0] = t_rec; mine[1] = t_al; mine[2] = t_cig; }
        return;
    }
    if (!is_rec) return;
    const SamLine a = rec[li];
    const u64 r = mine[0] + ex_rec, ls = li ? nl_pos[li - 1] + 1 : 0;
    O.flag[r] = (uint16_t)a.flag;
    O.ref_start[r] = a.ref_start;
    O.nm[r] = a.nm;
    O.seq_off[r] = ls + a.seq_off;
    O.seq_len[r] = a.seq_len;
    O.cig_off[r] = mine[2] + ex_cig;
    O.n_cig[r] = a.n_runs;
    O.name_off[r] = ls;
    O.name_len[r] = a.name_len;
    O.rname_off[r] = ls + a.rname_off;
    O.rname_len[r] = a.rname_len;
    O.line[r] = (u32)li;
    if (al) O.pass[mine[1] + ex_al] = (a.flag >> 16) & 1u ? 0 : 1;
}

// The CIGAR text of every record as packed runs at cig_off (validated by k_sam_scan: digits, then one of MIDNSHP=X, to the column's
// end; zero-length runs vanish, a run above 2^28-1 is cut: get_expanded_cigar).  One lane per record.
__global__ __launch_bounds__(256) void k_sam_cigar(u32 n_rec, const u8 *__restrict__ text, const u64 *__restrict__ nl_pos,
                                                   const SamLine *__restrict__ rec, const u32 *__restrict__ line,
                                                   const u64 *__restrict__ cig_off, u32 *__restrict__ cigar) {
    const u32 r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n_rec) return;
    const u32 li = line[r];
    const SamLine &a = rec[li];
    if (a.n_runs == 0) return;  // "*", or nothing but zero-length runs
    const u8 *cg = text + (li ? nl_pos[li - 1] + 1 : 0) + a.cig_off;
    u32 *runs = cigar + cig_off[r];
    u32 i = 0, nw = 0;
    while (i < a.cig_len) {
        u64 num = 0;
        while (cg[i] >= (u8)'0' && cg[i] <= (u8)'9') num = num * 10 + (u64)(cg[i++] - (u8)'0');
        const u32 op = (u32)op_code(cg[i++]);
        while (num > 0) {
            const u32 piece = num > 0x0FFFFFFFull ? 0x0FFFFFFFu : (u32)num;
            runs[nw++] = (piece << 4) | op;
            num -= piece;
        }
    }
}

struct NlBufs {  // the newline index of one call
    pp::DevBuf blk, blkoff, nl;
    ~NlBufs() { pp::dev_free(blk); pp::dev_free(blkoff); pp::dev_free(nl); }
};

const char *limit_text(u32 why) {
    switch (why) {
    case SR_FLAG: return "a FLAG above 65535, which a raw batch's 16 bits cannot hold";
    case SR_POS: return "a POS above 4294967295, which a raw batch's 32 bits cannot hold";
    default: return "an aligned record with an empty SEQ column, which a raw batch cannot tell from \"*\"";
    }
}

}  // namespace

extern "C" void pp_sam_free(pp_sam *s) { delete s; }

extern "C" void pp_sam_raw(const pp_sam *s, pp_raw_batch *out) {
    if (out) *out = s ? s->view : pp_raw_batch{};
}

extern "C" uint64_t *pp_sam_read_id(pp_sam *s) { return s ? (uint64_t *)s->a.read_id : nullptr; }
extern "C" uint32_t *pp_sam_contig(pp_sam *s) { return s ? s->a.contig : nullptr; }

static void sam_ranges(const pp_sam *s, const u64 *r_off, const u32 *r_len, const uint8_t **bytes_dev, uint64_t *n_bytes, const uint64_t **off,
                       const uint32_t **len) {
    if (bytes_dev) *bytes_dev = s ? s->a.seq : nullptr;
    if (n_bytes) *n_bytes = s ? s->n_bytes : 0;
    if (off) *off = (const uint64_t *)r_off;
    if (len) *len = r_len;
}

extern "C" void pp_sam_names(const pp_sam *s, const uint8_t **bytes_dev, uint64_t *n_bytes, const uint64_t **off, const uint32_t **len) {
    sam_ranges(s, s ? s->name_off : nullptr, s ? s->name_len : nullptr, bytes_dev, n_bytes, off, len);
}

extern "C" void pp_sam_rnames(const pp_sam *s, const uint8_t **bytes_dev, uint64_t *n_bytes, const uint64_t **off, const uint32_t **len) {
    sam_ranges(s, s ? s->rname_off : nullptr, s ? s->rname_len : nullptr, bytes_dev, n_bytes, off, len);
}

extern "C" const uint32_t *pp_sam_lines(const pp_sam *s) { return s ? s->line : nullptr; }

extern "C" void pp_sam_pass(const pp_sam *s, const uint8_t **zp, uint64_t *n_aligned) {
    if (zp) *zp = (s && !s->pass.empty()) ? s->pass.data() : nullptr;
    if (n_aligned) *n_aligned = s ? s->pass.size() : 0;
}

extern "C" int pp_sam_kernel_ms(const pp_sam *s, float *ms) {  // (from stage 1: the copy of the text is no kernel)
    return s ? s->t.total(s->ctx, "pp_sam_kernel_ms", "when the text was decoded", ms, 1) : PP_ERR_ARG;
}

// (internal hook, not part of the header: tools/sam_records_timing.py) the time by stage: the device copy of the text | newline index |
// scan | scans and compaction | CIGAR pack
extern "C" int pp_sam_stage_ms_(const pp_sam *s, float *ms5) { return s ? s->t.stages(ms5) : PP_ERR_ARG; }

extern "C" int pp_sam_first_empty_line(const pp_sam *s, uint64_t *line) {
    if (!s || s->first_empty == ~0ull) return 0;
    if (line) *line = s->first_empty;
    return 1;
}

// pp_sam_records (line_limit = ~0) and pp_sam_records_lines: the first line_limit lines of the text.  Where the limit cuts, the text
// behind the cut is zeroed in the object's copy and the call goes on as pp_sam_records of the prefix.
static int sam_records(pp_ctx *ctx, const uint8_t *text, uint64_t n_bytes, int mem, u64 line_limit, pp_sam **out, uint64_t *bad_line) {
    const char *const sym = line_limit != ~0ull ? "pp_sam_records_lines" : "pp_sam_records";  // who the refusals speak as
    if (!ctx) return PP_ERR_ARG;
    if (int rdy = pp_ctx_wait(ctx)) return rdy;
    if (bad_line) *bad_line = ~0ull;
    if (!out) return ctx->fail(PP_ERR_ARG, "%s: null argument", sym);
    *out = nullptr;
    if (mem != PP_MEM_HOST && mem != PP_MEM_DEVICE)
        return ctx->fail(PP_ERR_ARG, "%s: the text must be host memory or memory of the context's device", sym);
    if (n_bytes && !text) return ctx->fail(PP_ERR_ARG, "%s: null text with n_bytes > 0", sym);
    if (n_bytes >= (1ull << 40)) return ctx->fail(PP_ERR_LIMIT, "%s: the text is larger than the 1 TiB this decode indexes", sym);
    PP_HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const bool limited = line_limit != ~0ull;
    u64 size = line_limit ? n_bytes : 0;  // (no line: no byte of the text is looked at)

    std::unique_ptr<pp_sam> P(new pp_sam(ctx));
    RawArrays &A = P->a;
    CallScratch T;
    NlBufs N;
    StageTimer timer(ctx, ctx->profiling != 0 && size != 0);
    int rc;
    // ---- the owned copy: the text, zeros up to a multiple of NL_BLOCK and 64 more ----
    const u64 n_blk = (size + NL_BLOCK - 1) / NL_BLOCK, padded = std::max<u64>(1, n_blk) * NL_BLOCK;
    if ((rc = P->alloc(A.seq, (size_t)(padded + 64)))) return rc;
    if ((rc = timer.begin(0))) return rc;
    if (size) PP_HIPCHK(ctx, hipMemcpyAsync(A.seq, text, (size_t)size, mem == PP_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, st));
    PP_HIPCHK(ctx, hipMemsetAsync(A.seq + size, 0, (size_t)(padded + 64 - size), st));
    if ((rc = timer.end())) return rc;
    const u8 *const d_text = A.seq;
    auto done = [&](u64 n_rec, u64 n_cig_total) {  // (an empty batch: the text and no other array)
        P->n_bytes = size;
        P->view = A.view(n_rec, size, n_cig_total);
        *out = P.release();
        return PP_OK;
    };
    if (size == 0) {  // no text: an empty batch
        PP_HIPCHK(ctx, hipStreamSynchronize(st));
        return done(0, 0);
    }
    // ---- the newline index ----
    u64 n_nl = 0;
    u32 not_ascii = 0;
    if ((rc = timer.begin(1))) return rc;
    if ((rc = newline_index(ctx, d_text, size, N.blk, N.blkoff, N.nl, &n_nl, &not_ascii, limited))) return rc;
    if (limited && line_limit <= n_nl) {
        // Line line_limit starts behind newline line_limit - 1 (there may be no byte of it: the limit is the line count then).  From
        // there on the copy is zeros, as behind the end of any text, and the prefix is the text: its first line_limit newlines are
        // indexed already; whether IT holds a byte outside ASCII is asked again only where the whole text does.
        u64 cut = 0;
        if ((rc = fetch(ctx, (const u64 *)N.nl.p + (line_limit - 1), &cut))) return rc;
        cut += 1;
        if (cut < size) PP_HIPCHK(ctx, hipMemsetAsync(A.seq + cut, 0, (size_t)(size - cut), st));
        size = cut;
        n_nl = line_limit;
        if (not_ascii && (rc = newline_index(ctx, d_text, size, N.blk, N.blkoff, N.nl, &n_nl, &not_ascii))) return rc;
    }
    if ((rc = timer.end())) return rc;
    if (not_ascii)  // as pp_dev_ingest_sam: which lines are valid UTF-8 is the host parsers' to say
        return ctx->fail(PP_ERR_NOT_ASCII, "the text holds bytes outside ASCII: left to the host ingest");
    u8 last = 0;
    if ((rc = fetch(ctx, d_text + size - 1, &last))) return rc;
    const u64 n_lines = n_nl + (last != (u8)'\n' ? 1 : 0);
    if (n_lines >= 0xFFFFFFFFull) return ctx->fail(PP_ERR_LIMIT, "%s: 2^32-1 or more lines in one text", sym);
    const u64 *const d_nl = (const u64 *)N.nl.p;

    // ---- the scan, and the sums ----
    const u32 nb = (u32)((n_lines + SAM_BLOCK - 1) / SAM_BLOCK);
    void *d_rec, *d_kind, *d_blk3, *d_blk3off, *d_status;
    if ((rc = T.get(ctx, &d_rec, (size_t)n_lines * sizeof(SamLine))) || (rc = T.get(ctx, &d_kind, (size_t)n_lines * 4)) ||
        (rc = T.get(ctx, &d_blk3, (size_t)nb * 24)) || (rc = T.get(ctx, &d_blk3off, ((size_t)nb + 1) * 24)) || (rc = T.get(ctx, &d_status, 24)))
        return rc;
    PP_HIPCHK(ctx, hipMemsetAsync(d_status, 0xFF, 24, st));
    if ((rc = timer.begin(2))) return rc;
    with_stage(tok_stage_for(size, n_lines), [&](auto stage) {
        hipLaunchKernelGGL(k_sam_scan<decltype(stage)::value>, dim3((unsigned)((n_lines + 63) / 64)), dim3(64), 0, st, d_text, size, d_nl, n_nl,
                           n_lines, (SamLine *)d_rec, (u32 *)d_kind, (u64 *)d_status);
    });
    if ((rc = timer.end()) || (rc = timer.begin(3))) return rc;
    hipLaunchKernelGGL(k_sam_place<false>, dim3(nb), dim3(SAM_BLOCK), 0, st, n_lines, (const u32 *)d_kind, (const SamLine *)d_rec, d_nl, (u64 *)d_blk3,
                       SamOut{});
    hipLaunchKernelGGL(k_colscan<3>, dim3(1), dim3(1024), 0, st, (const u64 *)d_blk3, (u64)nb, (u64 *)d_blk3off);
    if ((rc = timer.end())) return rc;
    PP_HIPCHK(ctx, hipGetLastError());
    u64 status2[3] = {~0ull, ~0ull, ~0ull}, totals[3] = {0, 0, 0};
    if ((rc = fetch(ctx, d_status, status2, 3)) || (rc = fetch(ctx, (const u64 *)d_blk3off + 3ull * nb, totals, 3))) return rc;
    const u64 status = status2[0];
    P->first_empty = status2[1];
    P->first_nameless = status2[2];
    if (status != ~0ull) {  // the first refused line: its bytes, and what the host parser says to them
        const u64 li = status >> 8;
        const u32 why = (u32)(status & 0xFFu);
        if (bad_line) *bad_line = li;
        if (why != SR_PARSE)
            return ctx->fail(PP_ERR_LIMIT, "%s: %s in \"text\" (line %llu)", sym, limit_text(why), (unsigned long long)(li + 1));
        u64 a = 0, b = size;
        if (li) {
            if ((rc = fetch(ctx, d_nl + (li - 1), &a))) return rc;
            a += 1;
        }
        if (li < n_nl && (rc = fetch(ctx, d_nl + li, &b))) return rc;
        std::vector<char> line((size_t)(b - a));
        if (b > a) {
            if (mem == PP_MEM_HOST) memcpy(line.data(), text + a, (size_t)(b - a));
            else if ((rc = fetch(ctx, d_text + a, line.data(), (size_t)(b - a)))) return rc;
        }
        char err[1024] = "";
        const int code = pp_ingest_line_error_("text", line.data(), line.size(), li + 1, err, sizeof err);
        if (code == PP_OK) return ctx->fail(PP_ERR_HIP, "%s: the device refused line %llu but the host ingest takes it", sym, (unsigned long long)(li + 1));
        return ctx->fail(code, "%s", err);
    }
    const u64 n_rec = totals[0], n_al = totals[1], n_cig_total = totals[2];
    if (n_rec == 0) {  // header lines only: an empty batch
        PP_HIPCHK(ctx, hipStreamSynchronize(st));
        if ((rc = P->t.take(timer))) return rc;
        return done(0, 0);
    }
    const u32 n = (u32)n_rec;

    // ---- the per-record arrays, the CIGAR runs ----
    if ((rc = A.alloc_records(*P, n)) || (rc = P->alloc(A.cigar, (size_t)n_cig_total)) || (rc = P->alloc(P->name_off, n)) ||
        (rc = P->alloc(P->name_len, n)) || (rc = P->alloc(P->rname_off, n)) || (rc = P->alloc(P->rname_len, n)) || (rc = P->alloc(P->line, n)))
        return rc;
    PP_HIPCHK(ctx, hipMemsetAsync(A.read_id, 0, (size_t)n * 8, st));  // read_id and contig: the caller's (pp_names_ids)
    PP_HIPCHK(ctx, hipMemsetAsync(A.contig, 0, (size_t)n * 4, st));
    void *d_pass;
    if ((rc = T.get(ctx, &d_pass, (size_t)n_al))) return rc;
    SamOut O{A.flag, A.ref_start, A.nm, A.seq_len, A.n_cig, P->name_len, P->rname_len, P->line,
             A.seq_off, A.cig_off, P->name_off, P->rname_off, (u8 *)d_pass};
    if ((rc = timer.begin(3))) return rc;
    hipLaunchKernelGGL(k_sam_place<true>, dim3(nb), dim3(SAM_BLOCK), 0, st, n_lines, (const u32 *)d_kind, (const SamLine *)d_rec, d_nl,
                       (u64 *)d_blk3off, O);
    if ((rc = timer.end()) || (rc = timer.begin(4))) return rc;
    hipLaunchKernelGGL(k_sam_cigar, dim3((n + 255u) / 256u), dim3(256), 0, st, n, d_text, d_nl, (const SamLine *)d_rec, (const u32 *)P->line,
                       (const u64 *)A.cig_off, A.cigar);
    if ((rc = timer.end())) return rc;
    PP_HIPCHK(ctx, hipGetLastError());
    P->pass.resize((size_t)n_al);
    if (n_al) PP_HIPCHK(ctx, hipMemcpyAsync(P->pass.data(), d_pass, (size_t)n_al, hipMemcpyDeviceToHost, st));
    PP_HIPCHK(ctx, hipStreamSynchronize(st));  // the caller's text may be released, the scratch goes away
    if ((rc = P->t.take(timer))) return rc;
    return done(n, n_cig_total);
}

extern "C" int pp_sam_records(pp_ctx *ctx, const uint8_t *text, uint64_t n_bytes, int mem, pp_sam **out, uint64_t *bad_line) {
    return sam_records(ctx, text, n_bytes, mem, ~0ull, out, bad_line);
}

extern "C" int pp_sam_records_lines(pp_ctx *ctx, const uint8_t *text, uint64_t n_bytes, int mem, uint64_t n_lines, pp_sam **out,
                                    uint64_t *bad_line) {
    return sam_records(ctx, text, n_bytes, mem, n_lines == ~0ull ? n_lines - 1 : n_lines, out, bad_line);
}

// (internal hook, the command drivers' text front: pp_bam_files.cpp)  The reference's grouping quirk on top of interned ids, for the
// gate: an ALIGNED record joins the aligned record in front of it also when THAT one's QNAME is empty (src/alignment.rs:255), which
// ids from a name table do not know.  Where the decoded text has a record with an empty QNAME -- the scan has noted the first --
// read_id is rewritten as tests/names_model.empty_qname_rule has it: such a successor copies its predecessor's id, and a group that
// follows with the id the group in front borrowed that way gets a fresh one (from 2^40 up).  One sequential walk on the host over
// flag, name_len and read_id; a text without such a record (every text `bwa mem` writes) costs nothing.  Call it behind the QNAME
// pp_names_ids, and behind a filter: filter::filter keys its reads by name and has no such rule.
extern "C" int pp_sam_empty_qname_rule_(pp_sam *s) {
    if (!s) return PP_ERR_ARG;
    const uint64_t n = s->view.n_rec;
    if (s->first_nameless == ~0ull || n == 0) return PP_OK;
    s->first_nameless = ~0ull;  // (once)
    pp_ctx *ctx = s->ctx;
    PP_HIPCHK(ctx, hipSetDevice(ctx->device));
    std::vector<uint16_t> flag((size_t)n);
    std::vector<u32> len((size_t)n);
    std::vector<u64> id((size_t)n), was;
    int rc;
    if ((rc = fetch(ctx, s->a.flag, flag.data(), (size_t)n)) || (rc = fetch(ctx, s->name_len, len.data(), (size_t)n)) ||
        (rc = fetch(ctx, s->a.read_id, id.data(), (size_t)n)))
        return rc;
    was = id;
    u64 fresh = 1ull << 40, prev = ~0ull;
    for (u64 r = 0; r < n; r++) {
        if (flag[r] & 4) continue;
        if (prev != ~0ull && (len[prev] == 0 || was[prev] == was[r])) id[r] = id[prev];
        else if (prev != ~0ull && id[r] == id[prev]) id[r] = fresh++;
        prev = r;
    }
    PP_HIPCHK(ctx, hipMemcpyAsync(s->a.read_id, id.data(), (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
    PP_HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PP_OK;
}
