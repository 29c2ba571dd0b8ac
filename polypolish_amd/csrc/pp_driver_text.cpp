// pp_driver_text.cpp -- the polish driver's routes for SAM text on one context: the device tokenizer (pp_tokenize.hip) and the host
// ingest (multi-threaded parse, PP_DEVICE_INGEST=0), whose batches go up file by file while the next file is parsed.  The host
// ingest's file step also serves the multi-context job (pp_driver_multi.cpp), which plans over the files' batches.
#include "pp_driver.h"

namespace ppd {

int TextRoute::wait_pending() {
    int r = PP_OK;
    for (auto &p : pending)
        if (const int ri = p.get()) r = r ? r : ri;
    pending.clear();
    return r;
}

void TextRoute::reset() {
    (void)wait_pending();  // uploads in flight are joined before the batches they read are freed
    for (pp_ingest *x : gs) pp_ingest_free(x);
    pp_ingest_free(g);
    pp_dev_ingest_free(dg);
    gs.clear();
    g = nullptr;
    dg = nullptr;
}

int tokenizer_create(PolishJob &J) {
    int rc = pp_dev_ingest_create(J.ctx, J.a, J.opt->max_errors, J.opt->careful, &J.text.dg);
    uint64_t largest = 0, total = 0;
    for (uint64_t b : J.sam_bytes) { largest = std::max(largest, b); total += b; }
    if (rc == PP_OK && largest) rc = pp_dev_ingest_reserve_text_(J.text.dg, largest);
    if (rc == PP_OK && J.n_sams > 1) rc = pp_dev_ingest_expect(J.text.dg, total);  // the batch's arrays sized once, for all the files
    return rc;
}

int ingest_file_device(PolishJob &J, int i, pp_sam_counts &c) {
    pp_dev_ingest *const dg = J.text.dg;
    // the text of the NEXT file goes up (second text buffer, upload stream) while this one is tokenized
    if (i + 1 < J.n_sams) pp_dev_ingest_prefetch_(dg, J.sams[i + 1], *std::max_element(J.sam_bytes.begin(), J.sam_bytes.end()));
    return hand_back_if_text_defect(J.pass ? pp_dev_ingest_sam_filtered(dg, J.sams[i], J.pass[i], J.n_pass[i], &c)
                                           : pp_dev_ingest_sam(dg, J.sams[i], &c));
}

// The host ingest `gi` refused file i with (rc, J.err).  The reference streams: every read group before the failing point
// had already gone through add_alignment (alignment.rs:297-303), so a record there that only the CIGAR walk rejects
// (unexpected op, CIGAR / SEQ length mismatch, past the contig end) is what it reports.  Run the device over exactly those
// records: the earlier files and this file up to the group that was pending.  Returns the error that stands.
static int replay_records_before_defect(PolishJob &J, int i, const pp_ingest *gi, int rc) {
    pp_ctx *const ctx = J.ctx;
    TextRoute &T = J.text;
    uint64_t cut = 0;
    if (!pp_ingest_fail_cut_(gi, &cut) || T.wait_pending() != PP_OK) return rc;
    int rd = T.begun ? PP_OK : begin_job(J, ctx);
    T.begun = true;
    auto add = [&](const pp_ingest *x) {
        pp_aln_batch b;
        pp_ingest_batch(x, &b);
        if (rd == PP_OK && b.n_aln) rd = pp_polish_add(ctx, &b, PP_MEM_HOST);
    };
    if (J.route == Route::HOST_ONE) add(T.g);
    if (J.route == Route::MULTI_HOST)  // (the earlier files' batches have not gone anywhere yet: the first context takes them whole)
        for (size_t q = 0; q + 1 < T.gs.size(); q++) add(T.gs[q]);
    pp_ingest *gp = nullptr;
    char err2[256];
    pp_sam_counts c2;
    if (rd == PP_OK && cut > 0 && pp_ingest_create(J.a, J.opt->max_errors, J.opt->careful, &gp) == PP_OK &&
        pp_ingest_sam_prefix_(gp, J.sams[i], cut, J.pass ? J.pass[i] : nullptr, J.pass ? J.n_pass[i] : 0, &c2, err2, sizeof err2) == PP_OK)
        add(gp);
    if (rd == PP_OK) rd = pp_polish_finish(ctx);
    pp_ingest_free(gp);
    return replayed_or_refusal(ctx, rd, rc, J.err);
}

int ingest_file_host(PolishJob &J, int i, pp_sam_counts &c) {
    pp_ctx *const ctx = J.ctx;
    TextRoute &T = J.text;
    pp_ingest *gi = T.g;
    if (J.route != Route::HOST_ONE) {  // an object per file
        if (int rc = pp_ingest_create(J.a, J.opt->max_errors, J.opt->careful, &gi)) return rc;
        T.gs.push_back(gi);
    }
    int rc = J.pass ? pp_ingest_sam_filtered(gi, J.sams[i], J.pass[i], J.n_pass[i], &c, J.err, sizeof J.err)
                    : pp_ingest_sam(gi, J.sams[i], &c, J.err, sizeof J.err);
    if (rc) {
        set_err(ctx, rc, J.err);
        return replay_records_before_defect(J, i, gi, rc);
    }
    if (J.route != Route::HOST_STREAMED) return PP_OK;
    if ((rc = T.wait_pending())) return rc;  // the upload of the file before
    const bool first = !T.begun;
    T.begun = true;
    // room for all files at once: this file's batch scaled by the files' sizes on disk
    double scale = 1.0;
    if (first && J.n_sams > 1 && J.sam_bytes[(size_t)i] > 0) scale = scale_to_all_files(bytes_on_disk(J, J.n_sams), (double)J.sam_bytes[(size_t)i]);
    T.pending.push_back(std::async(std::launch::async, [&J, ctx, gi, first, scale]() {
        int r = first ? begin_job(J, ctx) : PP_OK;
        pp_aln_batch bi;
        pp_ingest_batch(gi, &bi);
        if (r == PP_OK && first && scale > 1.0) r = reserve_scaled(ctx, bi.n_aln, bi.seq_bytes, bi.n_cig_total, scale);
        if (r == PP_OK) r = pp_polish_add(ctx, &bi, PP_MEM_HOST);
        return r;
    }));
    return PP_OK;
}

// the batches that are not in the job yet: the tokenizer's one batch, the one host ingest object's -- or none (streamed adds: every
// file's went up as it was parsed; no SAM files at all)
int text_hand_over(PolishJob &J) {
    TextRoute &T = J.text;
    if (T.begun) return PP_OK;
    pp_aln_batch batch{};
    const int rc = begin_job(J, J.ctx);
    if (rc || J.route == Route::HOST_STREAMED) return rc;
    if (J.route == Route::HOST_ONE) pp_ingest_batch(T.g, &batch);
    else pp_dev_ingest_batch(T.dg, &batch);
    return pp_polish_add(J.ctx, &batch, J.route == Route::HOST_ONE ? PP_MEM_HOST : PP_MEM_DEVICE);
}

}  // namespace ppd
