// pp_filter_rec.hip -- pp_filter_records: filter::filter (src/filter.rs:26-37) between loading and writing over a caller's RAW
// alignment records (pp_raw_batch, the arrays pp_batch_gate takes next), on the device.
//
// The file drivers reach pp_filter_begin through a loader welded to SAM text (pp_filter_load on the host, pp_filter_load_device:
// keys are pointers into the uploaded file).  This is the loader for a caller who holds records: pp_raw_batch.read_id is the
// QNAME as a number already, contig the RNAME.
//   k_rec_aligned   1 for every record without FLAG & 4; its scan is the record's index among the file's aligned records (the
//                   numbering of pp_filter_file and of the verdicts)
//   k_rec_compact   the aligned records of a file into the arrays of pp_filter_file: flags, ref_start, ref_id (= contig, compared
//                   for equality only), ref_end from the runs (Alignment::get_ref_end, alignment.rs:138-149; PP_OP_UNPARSEABLE ->
//                   PP_REF_END_UNPARSEABLE) -- the later passes need no CIGAR -- and the id into the list of both files' ids.  A
//                   CIGAR range outside the array is reported before anything is read through it
//   k_rid_insert    (pp_filter_group.h) the reference's HashMap<String, Vec<Alignment>> (filter.rs:91-145) over 64-bit keys: open addressing, a slot
//   k_rid_find      holds record index + 1 (over both files, file 1 first), a key's representative is its first record.  Equality
//                   is equality of the ids: no value is reserved.  The hash mixes all 64 bits (ids that differ only above bit 32,
//                   or that are multiples of the table's capacity, spread like any others)
// and from there the grouping both device loaders share (pp_filter_group.h): read numbers, group sizes, scan, scatter, sort into
// file order.  Then pp_filter_begin(PP_MEM_DEVICE), pp_filter_thresholds, pp_filter_pairs.
#include "pp_filter_group.h"
#include "pp_host.h"


namespace {

struct RecRaw {  // what the filter reads of a raw batch (device memory)
    const uint16_t *flag;
    const u64 *read_id, *cig_off;
    const u32 *contig, *ref_start, *n_cig, *cigar;
    u64 n_cig_total;
};

__global__ __launch_bounds__(256) void k_rec_aligned(u32 n_rec, const uint16_t *__restrict__ flag, u32 *__restrict__ is_aln) {
    const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
    if (r < n_rec) is_aln[r] = (flag[r] & 4u) ? 0u : 1u;
}

// status: (file << 32 | raw index) of the first aligned record whose CIGAR range does not lie inside the cigar array
__global__ __launch_bounds__(256) void k_rec_compact(u32 n_rec, RecRaw R, const u32 *__restrict__ rank_of, u64 base, u32 file,
                                                     u32 *__restrict__ flags, u32 *__restrict__ ref_start, u32 *__restrict__ ref_id,
                                                     u64 *__restrict__ ref_end, u64 *__restrict__ ids, u64 *__restrict__ status) {
    const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
    if (r >= n_rec) return;
    const u32 fl = R.flag[r];
    if (fl & 4u) return;
    const u32 a = rank_of[r], nc = R.n_cig[r], start = R.ref_start[r];
    const u64 co = R.cig_off[r];
    u64 end = start;  // (n_cig == 0: the end is the start)
    if (nc && !inside(co, nc, R.n_cig_total)) {
        report(status, ((u64)file << 32) | r);
    } else {
        const u32 *cg = R.cigar + co;
        for (u32 i = 0; i < nc; i++) {
            const u32 op = cg[i], o = op & 15u;
            if (o == PP_OP_M || o == PP_OP_D || o == PP_OP_N || o == PP_OP_EQ || o == PP_OP_X) end += op >> 4;
            else if (o == (u32)PP_OP_UNPARSEABLE) { end = PP_REF_END_UNPARSEABLE; break; }
        }
    }
    flags[a] = fl;
    ref_start[a] = start;
    ref_id[a] = R.contig[r];
    ref_end[a] = end;
    ids[base + a] = R.read_id[r];
}

enum : int { SPAN_COMPACT = 0, SPAN_INTERN = 1, SPAN_GROUPS = 2 };
static const char *const SPAN_NAME[3] = {"rec_compact", "rec_intern", "rec_groups"};

}  // namespace

extern "C" int pp_filter_records(pp_ctx *ctx, const pp_raw_batch raw[2], int mem, const char *orientation, double low, double high,
                                 uint8_t *pass1, uint8_t *pass2, pp_filter_file_counts counts[2], pp_filter_report *report) {
    if (!ctx) return PP_ERR_ARG;
    if (int rdy = pp_ctx_wait(ctx)) return rdy;
    if (!raw || !orientation) return ctx->fail(PP_ERR_ARG, "pp_filter_records: null argument");
    if (mem != PP_MEM_HOST && mem != PP_MEM_DEVICE)
        return ctx->fail(PP_ERR_ARG, "pp_filter_records: the batches must be host memory or memory of the context's device");
    pp_filter_file_counts local_counts[2];
    pp_filter_report local_report;
    if (!counts) counts = local_counts;
    if (!report) report = &local_report;
    memset(counts, 0, 2 * sizeof(pp_filter_file_counts));
    memset(report, 0, sizeof *report);
    int rc;
    for (int f = 0; f < 2; f++)  // (the filter reads no nm and no SEQ)
        if ((rc = raw_check(ctx, "pp_filter_records", &raw[f], mem, RAW_CIGAR))) return rc;
    // check_inputs comes before anything is loaded (filter.rs:40-53)
    if (const char *msg = pph::percentile_options_error(low, high)) return ctx->fail(PP_ERR_QUIT, "%s", msg);
    PP_HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    uint8_t *const pass[2] = {pass1, pass2};

    CtxScratch T(ctx, ctx->f_rec, "pp_filter_records");
    StageTimer spans(ctx, ctx->profiling != 0);  // (pp_filter_begin starts the context's own timers afresh)
    // ---- the source on the device ----
    RecRaw R[2];
    u32 n_rec[2];
    for (int f = 0; f < 2; f++) {
        pp_raw_batch D = raw[f];  // (a batch without records uploads nothing)
        n_rec[f] = (u32)D.n_rec;
        if (n_rec[f] && (rc = raw_on_device(ctx, T, mem, &raw[f], RAW_CIGAR, &D))) return rc;
        R[f] = RecRaw{D.flag, (const u64 *)D.read_id, (const u64 *)D.cig_off, D.contig, D.ref_start, D.n_cig, D.cigar, D.n_cig_total};
    }

    // ---- the aligned records of either file, numbered in file order ----
    u32 n_al[2] = {0, 0};
    void *d_rank[2] = {nullptr, nullptr};
    for (int f = 0; f < 2; f++) {
        if (!n_rec[f]) continue;
        void *d_isaln;
        if ((rc = T.get(ctx, &d_isaln, (size_t)n_rec[f] * 4)) || (rc = T.get(ctx, &d_rank[f], ((size_t)n_rec[f] + 1) * 4))) return rc;
        if ((rc = spans.begin(SPAN_COMPACT))) return rc;
        hipLaunchKernelGGL(k_rec_aligned, dim3((n_rec[f] + 255u) / 256u), dim3(256), 0, st, n_rec[f], R[f].flag, (u32 *)d_isaln);
        if ((rc = scan_u32<u32>(ctx, T.sums(), T.sums_off(), (const u32 *)d_isaln, (u64)n_rec[f], (u32 *)d_rank[f]))) return rc;
        if ((rc = spans.end())) return rc;
        PP_HIPCHK(ctx, hipGetLastError());
        if ((rc = fetch(ctx, (const u32 *)d_rank[f] + n_rec[f], &n_al[f]))) return rc;
    }
    const u64 n0 = n_al[0], n1 = n_al[1], N = n0 + n1;
    if (N >= 0xFFFFFFFFull) return ctx->fail(PP_ERR_LIMIT, "more than 2^32-1 alignments in the two files");
    for (int f = 0; f < 2; f++)
        if (n_al[f] && !pass[f]) return ctx->fail(PP_ERR_ARG, "pp_filter_records: null output");

    // ---- the arrays of pp_filter_file, the ids of both files ----
    void *d_flags[2], *d_start[2], *d_refid[2], *d_end[2], *d_read[2], *d_grpidx[2], *d_grpoff[2], *d_ids, *d_status;
    if ((rc = T.get(ctx, &d_ids, std::max<u64>(1, N) * 8)) || (rc = T.get(ctx, &d_status, 8))) return rc;
    PP_HIPCHK(ctx, hipMemsetAsync(d_status, 0xFF, 8, st));
    for (int f = 0; f < 2; f++) {
        const size_t n = std::max<u32>(1, n_al[f]);
        if ((rc = T.get(ctx, &d_flags[f], n * 4)) || (rc = T.get(ctx, &d_start[f], n * 4)) || (rc = T.get(ctx, &d_refid[f], n * 4)) ||
            (rc = T.get(ctx, &d_end[f], n * 8)) || (rc = T.get(ctx, &d_read[f], n * 4)) || (rc = T.get(ctx, &d_grpidx[f], n * 4)))
            return rc;
        if (!n_al[f]) continue;
        if ((rc = spans.begin(SPAN_COMPACT))) return rc;
        hipLaunchKernelGGL(k_rec_compact, dim3((n_rec[f] + 255u) / 256u), dim3(256), 0, st, n_rec[f], R[f], (const u32 *)d_rank[f], f == 0 ? 0ull : n0,
                           (u32)f, (u32 *)d_flags[f], (u32 *)d_start[f], (u32 *)d_refid[f], (u64 *)d_end[f], (u64 *)d_ids, (u64 *)d_status);
        if ((rc = spans.end())) return rc;
    }
    PP_HIPCHK(ctx, hipGetLastError());
    u64 status = ~0ull;
    if ((rc = fetch(ctx, d_status, &status))) return rc;
    if (status != ~0ull)
        return ctx->fail(PP_ERR_ARG, "pp_filter_records: the CIGAR range of record %llu of file %d does not lie inside the batch's cigar array",
                         (unsigned long long)(status & 0xFFFFFFFFull), (int)(status >> 32) + 1);
    counts[0].alignments = n0;
    counts[1].alignments = n1;
    if (n0 == 0) return ctx->fail(PP_ERR_QUIT, "no alignments found in file 1");

    // ---- intern the ids (file 1, then file 2) ----
    u32 cap = 1024;
    while (cap < 2 * N + 2) cap <<= 1;
    void *d_slots, *d_rep, *d_isrep, *d_idscan;
    if ((rc = T.get(ctx, &d_slots, (size_t)cap * 4)) || (rc = T.get(ctx, &d_rep, N * 4)) || (rc = T.get(ctx, &d_isrep, N * 4)) ||
        (rc = T.get(ctx, &d_idscan, (N + 1) * 4)))
        return rc;
    if ((rc = spans.begin(SPAN_INTERN))) return rc;
    PP_HIPCHK(ctx, hipMemsetAsync(d_slots, 0, (size_t)cap * 4, st));
    {
        const unsigned gb = (unsigned)((N + 255) / 256);
        hipLaunchKernelGGL(k_rid_insert, dim3(gb), dim3(256), 0, st, N, (const u64 *)d_ids, (u32 *)d_slots, cap - 1);
        hipLaunchKernelGGL(k_rid_find, dim3(gb), dim3(256), 0, st, N, (const u64 *)d_ids, (const u32 *)d_slots, cap - 1, (u32 *)d_rep, (u32 *)d_isrep);
        if ((rc = scan_u32<u32>(ctx, T.sums(), T.sums_off(), (const u32 *)d_isrep, N, (u32 *)d_idscan))) return rc;
    }
    if ((rc = spans.end())) return rc;
    PP_HIPCHK(ctx, hipGetLastError());
    u32 ids_f1 = 0, n_reads = 0, shared = 0;
    if ((rc = fetch(ctx, (const u32 *)d_idscan + n0, &ids_f1)) || (rc = fetch(ctx, (const u32 *)d_idscan + N, &n_reads))) return rc;
    if (n1) {  // ids of file 2 that file 1 holds as well (file 2's count of distinct ids)
        void *d_hit, *d_hitscan;
        if ((rc = T.get(ctx, &d_hit, n0 * 4)) || (rc = T.get(ctx, &d_hitscan, (n0 + 1) * 4))) return rc;
        if ((rc = spans.begin(SPAN_INTERN))) return rc;
        PP_HIPCHK(ctx, hipMemsetAsync(d_hit, 0, n0 * 4, st));
        hipLaunchKernelGGL(k_mark_shared, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, st, n0, N, (const u32 *)d_rep, (u32 *)d_hit);
        if ((rc = scan_u32<u32>(ctx, T.sums(), T.sums_off(), (const u32 *)d_hit, n0, (u32 *)d_hitscan))) return rc;
        if ((rc = spans.end())) return rc;
        if ((rc = fetch(ctx, (const u32 *)d_hitscan + n0, &shared))) return rc;
    }
    counts[0].reads = ids_f1;
    counts[0].loaded = 1;
    counts[1].reads = (u64)(n_reads - ids_f1) + shared;
    counts[1].loaded = 1;

    // ---- read numbers and the per-file groups in file order ----
    void *d_cursor;
    if ((rc = T.get(ctx, &d_cursor, (size_t)n_reads * 4))) return rc;
    if ((rc = spans.begin(SPAN_GROUPS))) return rc;
    for (int f = 0; f < 2; f++) {
        if ((rc = T.get(ctx, &d_grpoff[f], ((size_t)n_reads + 1) * 4))) return rc;
        if ((rc = file_groups(ctx, n_al[f], f == 0 ? 0ull : n0, n_reads, (const u32 *)d_rep, (const u32 *)d_idscan, (const u32 *)nullptr, (u32 *)d_read[f],
                              (u32 *)nullptr, (u32 *)d_cursor, (u32 *)d_grpoff[f], (u32 *)d_grpidx[f], T.sums(), T.sums_off())))
            return rc;
    }
    if ((rc = spans.end())) return rc;
    PP_HIPCHK(ctx, hipGetLastError());

    // ---- the filter itself ----
    pp_filter_input in{};
    in.n_reads = n_reads;
    for (int f = 0; f < 2; f++) {
        pp_filter_file &d = in.file[f];
        d.n_aln = n_al[f];
        d.ref_id = (const u32 *)d_refid[f]; d.ref_start = (const u32 *)d_start[f]; d.flags = (const u32 *)d_flags[f];
        d.read = (const u32 *)d_read[f]; d.grp_off = (const u32 *)d_grpoff[f]; d.grp_idx = (const u32 *)d_grpidx[f];
        d.ref_end = (const uint64_t *)d_end[f];
    }
    struct Close {  // the job's arrays are the next call's scratch: nothing may be asked of it afterwards
        pp_ctx *ctx;
        ~Close() {
            (void)hipStreamSynchronize(ctx->stream);
            ctx->filter_open = false;
        }
    } close{ctx};
    if ((rc = pp_filter_begin(ctx, &in, PP_MEM_DEVICE))) return rc;
    if ((rc = pp_filter_thresholds(ctx, orientation, low, high, report))) return rc;
    if ((rc = pp_filter_pairs(ctx, report->low_threshold, report->high_threshold, (uint8_t)report->orientation, pass1, pass2))) return rc;
    for (int f = 0; f < 2; f++)
        for (u64 i = 0; i < n_al[f]; i++) report->after_count += pass[f][i] != 0;
    if (spans.on) {  // (the stream has been synchronised)
        float ms[3];
        if ((rc = spans.sums(ms, 3))) return rc;
        pp_kernel_times &t = ctx->last_times;
        for (int k = 0; k < 3 && t.n < PP_MAX_KERNELS; k++) {
            t.name[t.n] = SPAN_NAME[k];
            t.ms[t.n++] = ms[k];
        }
    }
    return PP_OK;
}
