// pp_driver.cpp -- whole-command drivers behind the `polypolish` CLI contract.
//   pp_polish_files  = polish::polish   (src/polish.rs:26-38)
// Output bytes (FASTA on stdout, filtered SAMs) are the contract; the stderr log reproduces the
// reference's numbers (counts, depth, changed positions, Q-score) in plain text -- the
// reference's colours, wrapping and timestamps (src/log.rs) are cosmetic and not reproduced.
// This unit: the stages every input route shares, the one place that sends a stage to the job's route, the polish on one
// context and the entry points.  The routes: pp_driver_text.cpp, pp_driver_multi.cpp, pp_driver_bam.cpp (pp_driver.h).
#include <sys/stat.h>

#include <cmath>

#include "pp_driver.h"

using pph::commas;
using pph::format_duration;
using pph::qscore;

// (internal, bin/polypolish only) the process exits right after the command: see pph::process_leaving_soon
extern "C" void pp_process_leaving_soon_(int yes) { pph::process_leaving_soon() = yes != 0; }

extern "C" void pp_bytes_free(pp_bytes *b) {
    if (!b) return;
    free(b->data);
    b->data = nullptr;
    b->len = 0;
}

// write_debug_line (polish.rs:257-266) for the positions [lo, hi) of ctx's job: formatted on its device (pp_polish_debug_tsv,
// pp_k_debug.h) a chunk at a time into two pinned buffers in turn -- the fwrite of one chunk runs on a helper thread while
// the next one is formatted and copied out.  Host memory: two chunks, whatever the TSV's size.
namespace ppd {

int write_debug_tsv(pp_ctx *ctx, FILE *f, const std::vector<const char *> &names, uint64_t lo, uint64_t hi) {
    constexpr uint64_t CHUNK = 32ull << 20;
    uint8_t *buf[2] = {nullptr, nullptr};
    bool pinned[2] = {false, false};
    for (int k = 0; k < 2; k++) {
        buf[k] = (uint8_t *)pp_host_pinned_alloc_(ctx, CHUNK);
        pinned[k] = buf[k] != nullptr;
        if (!buf[k]) buf[k] = (uint8_t *)malloc(CHUNK);
    }
    int rc = buf[0] && buf[1] ? PP_OK : pp_ctx_set_error_(ctx, PP_ERR_HIP, "out of host memory for the --debug file");
    std::future<bool> pending;  // the fwrite of the chunk before
    auto written = [&]() { return !pending.valid() || pending.get(); };
    for (uint64_t p = lo; rc == PP_OK && p < hi;) {
        uint8_t *const b = buf[0];
        uint64_t n = 0, next = p;
        rc = pp_polish_debug_tsv(ctx, names.data(), p, hi, b, PP_MEM_HOST, CHUNK, &n, &next);
        if (rc == PP_OK && next == p) rc = pp_ctx_set_error_(ctx, PP_ERR_HIP, "the --debug formatter made no progress");
        if (!written() && rc == PP_OK) rc = pp_ctx_set_error_(ctx, PP_ERR_QUIT, "unable to write to the --debug file");
        if (rc) break;
        if (n) pending = std::async(std::launch::async, [f, b, n] { return fwrite(b, 1, n, f) == n; });
        std::swap(buf[0], buf[1]);
        std::swap(pinned[0], pinned[1]);
        p = next;
    }
    if (!written() && rc == PP_OK) rc = pp_ctx_set_error_(ctx, PP_ERR_QUIT, "unable to write to the --debug file");
    for (int k = 0; k < 2; k++) {
        if (pinned[k]) pp_host_pinned_free_(buf[k]);
        else free(buf[k]);
    }
    return rc;
}

bool origin_of(const std::vector<Stretch> &sent, uint64_t local, Origin *o) {
    uint64_t at = 0;
    for (const Stretch &s : sent) {
        if (local < at + s.n) {
            uint32_t v = 0;
            if (s.mem == PP_MEM_HOST) v = s.orig[local - at];
            else if (pp_ctx_download(s.holder, &v, s.orig + (local - at), 4) != PP_OK) return false;
            *o = Origin{&s, local - at, s.base + v};
            return true;
        }
        at += s.n;
    }
    return false;
}

double bytes_on_disk(const PolishJob &J, int n_files) {
    double sum = 0;
    for (int f = 0; f < n_files; f++) sum += (double)J.sam_bytes[(size_t)f];
    return sum;
}

int reserve_scaled(pp_ctx *ctx, uint64_t n_aln, uint64_t seq_bytes, uint64_t n_cig_total, double scale) {
    return pp_polish_reserve(ctx, (uint64_t)((double)n_aln * scale) + 1024, (uint64_t)((double)seq_bytes * scale) + 4096,
                             (uint64_t)((double)n_cig_total * scale) + 1024);
}

int replayed_or_refusal(pp_ctx *ctx, int replayed, int refusal, const char *refusal_msg) {
    if (replayed == PP_ERR_QUIT || replayed == PP_ERR_PANIC) return replayed;  // the device's message stands
    return set_err(ctx, refusal, refusal_msg);
}

int on_all(PolishJob &J, const std::function<int(int)> &f) {
    std::vector<std::future<int>> jobs;
    for (int d = 0; d < J.n_ctx; d++) jobs.push_back(std::async(std::launch::async, f, d));
    int r = PP_OK;
    for (int d = 0; d < J.n_ctx; d++) {
        const int rd = jobs[(size_t)d].get();
        if (rd && !r) {
            r = rd;
            if (d) set_err(J.ctx, rd, pp_last_error(J.ctxs[d]));
        }
    }
    return r;
}

static bool exists(const char *p) {
    struct stat st;
    return stat(p, &st) == 0;
}
static bool off_by_env(const char *name) { return getenv(name) && atoi(getenv(name)) == 0; }

static int check_options_and_inputs(PolishJob &J) {
    const pp_polish_options *opt = J.opt;
    // check_option_values (polish.rs:277-287) is repeated by pp_polish_begin; do it first as the reference does
    if (opt->fraction_valid <= 0.0 || opt->fraction_valid >= 1.0)
        return set_err(J.ctx, PP_ERR_QUIT, "--fraction_valid must be between 0 and 1 (exclusive)");
    if (opt->fraction_invalid <= 0.0 || opt->fraction_invalid >= 1.0)
        return set_err(J.ctx, PP_ERR_QUIT, "--fraction_invalid must be between 0 and 1 (exclusive)");
    if (opt->fraction_invalid >= opt->fraction_valid)
        return set_err(J.ctx, PP_ERR_QUIT, "--fraction_invalid must be less than --fraction_valid");
    // check_inputs_exist, polish.rs:269-274
    for (int i = -1; i < J.n_sams; i++) {
        const char *path = i < 0 ? J.assembly : J.sams[i];
        if (exists(path)) continue;
        snprintf(J.err, sizeof J.err, "\"%s\" file does not exist", path);
        return set_err(J.ctx, PP_ERR_QUIT, J.err);
    }
    // SAM text or BAM, told by the files' heads (pp_aln_file_kind); all files of a command are of one kind
    std::vector<int> &kinds = J.bam.kinds;
    // (with pp_ctx_set_text_chain, pp_aln_file_kind_text: bgzipped SAM text is text.  The second look at a text the chain handed
    // back is the host ingest's, as without it.)
    const bool text_chain = pp_ctx_text_chain_(J.ctx) != 0 && J.resume_log_at < 0;
    kinds.assign((size_t)J.n_sams, J.bam.borrowed ? J.bam.fronts[0]->kind : PP_ALN_SAM);
    int first_sam = -1, first_bam = -1;
    for (int i = 0; i < J.n_sams; i++) {
        if (!J.bam.borrowed)
            if (int rc = ppb::file_kind(J.ctx, J.sams[i], &kinds[(size_t)i])) return rc;
        int &first = ppb::is_text(kinds[(size_t)i]) ? first_sam : first_bam;
        if (first < 0) first = i;
    }
    if (first_sam >= 0 && first_bam >= 0)
        return ppb::fail(J.ctx, PP_ERR_QUIT, "the alignment files of one command must all be SAM text or all be BAM: \"%s\" is SAM text, \"%s\" is BAM",
                         J.sams[first_sam], J.sams[first_bam]);
    if (first_sam >= 0 && pp_ctx_regroup_(J.ctx) && !text_chain)
        return ppb::fail(J.ctx, PP_ERR_QUIT, "--regroup takes BAM input: \"%s\" is SAM text (its records are regrouped on the device, which holds none of a text file)",
                         J.sams[first_sam]);
    // the job's route, decided here and nowhere else
    const bool tokenize = J.resume_log_at < 0 && !off_by_env("PP_DEVICE_INGEST");
    J.route = first_bam >= 0 ? Route::BAM
              : text_chain   ? Route::TEXT_CHAIN
              : J.n_ctx > 1  ? (tokenize ? Route::SHARDED : Route::MULTI_HOST)
              : tokenize     ? Route::TOKENIZER
                             : (off_by_env("PP_STREAM_ADDS") ? Route::HOST_ONE : Route::HOST_STREAMED);
    if (J.route == Route::BAM && J.n_ctx > 1)
        return ppb::fail(J.ctx, PP_ERR_QUIT, "BAM input (\"%s\") runs on one GPU: polish it without PP_GPUS / several contexts, or convert it to SAM text",
                         J.sams[first_bam]);
    if (J.route == Route::TEXT_CHAIN && J.n_ctx > 1)
        return ppb::fail(J.ctx, PP_ERR_QUIT, "SAM text on the record chain (--text_chain, \"%s\") runs on one GPU: polish it without PP_GPUS / several contexts, or without --text_chain",
                         J.sams[first_sam]);
    // The device tokenizer uploads the SAM text as it is: map the files and pre-fault the mappings NOW, on background
    // threads, while the HIP runtime is still initialising (a copy out of an untouched mapping runs at a quarter of
    // the link's rate).
    for (int i = 0; tokenize && i < J.n_sams; i++) pph::prefetch_file(J.sams[i], J.ctx);
    J.sam_bytes.assign((size_t)J.n_sams, 0);
    for (int i = 0; i < J.n_sams; i++) {
        struct stat st;
        if (stat(J.sams[i], &st) == 0 && S_ISREG(st.st_mode)) J.sam_bytes[(size_t)i] = (uint64_t)st.st_size;
    }
    return PP_OK;
}

// starting_message, polish.rs:41-73
static void log_banner(const PolishJob &J) {
    const pp_polish_options *opt = J.opt;
    J.log("\nStarting Polypolish polish\n%s\n\nInput assembly:\n  %s\n\nInput short-read alignments:\n", pp_version(), J.assembly);
    for (int i = 0; i < J.n_sams; i++) J.log("  %s\n", J.sams[i]);
    J.log("\nSettings:\n  --fraction_invalid %g\n  --fraction_valid %g\n  --max_errors %u\n  --min_depth %u\n",
          opt->fraction_invalid, opt->fraction_valid, opt->max_errors, opt->min_depth);
    if (opt->careful) J.log("  --careful\n");
    if (opt->debug_path) J.log("  --debug %s\n\n", opt->debug_path);
    else J.log("  not logging debugging information\n\n");
}

// load_assembly, polish.rs:93-106
static int load_assembly(PolishJob &J) {
    J.log("Loading assembly\n");
    if (!J.a_borrowed)  // (else: loaded for the filter's RNAME table already)
        if (int rc = ppb::load_assembly_file(J.ctx, J.n_ctx, J.assembly, &J.a, J.err, sizeof J.err)) return set_err(J.ctx, rc, J.err);
    J.nc = pp_assembly_n_contigs(J.a);
    J.off = pp_assembly_offsets(J.a);
    J.names.resize(J.nc);
    for (uint32_t c = 0; c < J.nc; c++) {
        J.names[c] = pp_assembly_name(J.a, c);
        J.log("%s (%s bp)\n", J.names[c], commas(J.off[c + 1] - J.off[c]).c_str());
    }
    J.log("\n");
    J.out_off.resize(J.nc + 1);
    J.stats.resize(J.nc);
    return PP_OK;
}

// The FASTA that will be returned: headers + polished bytes.  Its buffer is allocated for an upper bound NOW and touched
// by a helper thread while the alignments are loaded -- the polished bytes then come off the device straight into their
// place in it (a fresh 250 MB destination took 30 ms of page faults inside the copy, and assembling the FASTA from a
// second buffer another 40 ms of memcpy).
static void reserve_fasta(PolishJob &J) {
    size_t cap = 0;
    for (uint32_t c = 0; c < J.nc; c++) cap += strlen(J.names[c]) + strlen(pp_assembly_description(J.a, c)) + 16;
    J.fasta.header_bytes = cap;
    cap += (size_t)(J.off[J.nc] + J.off[J.nc] / 8) + 2 * (size_t)J.nc + 65536;  // (every planted insertion adds a byte: far below 1/8)
    J.fasta.cap = cap;
    uint8_t *out = J.fasta.buf = (uint8_t *)malloc(cap);
    if (out) J.fasta.toucher = std::thread([out, cap] { for (size_t q = 0; q < cap; q += 4096) out[q] = 0; });
}

// ---- the one place that sends a stage to the job's route: create, ingest one file, hand the batches to the polish, name a job
// record's origin (the multi-context polish, polish_on_several_contexts, is chosen in polish_once) ----
// the ingest objects of the job's route -- the device tokenizer (pp_tokenize.hip), one per context when sharded, or the host's
// (multi-threaded parse) with PP_DEVICE_INGEST=0
static int create_ingests(PolishJob &J) {
    if (several_contexts(J.route)) pp_ctx_enable_peers_(J.ctxs, J.n_ctx);
    int rc = PP_OK;
    switch (J.route) {
    case Route::BAM:
    case Route::TEXT_CHAIN: return bam_create(J);
    case Route::SHARDED: rc = sharded_create(J); break;
    case Route::TOKENIZER: rc = tokenizer_create(J); break;
    case Route::HOST_ONE: rc = pp_ingest_create(J.a, J.opt->max_errors, J.opt->careful, &J.text.g); break;
    case Route::HOST_STREAMED:
    case Route::MULTI_HOST: break;  // an object per file, as the files come
    }
    if (tokenizes(J.route)) J.lap("device ready, tokenizer created");  // (pp_dev_ingest_create waits for the HIP runtime's start-up)
    return rc;
}
static int ingest_file(PolishJob &J, int i, pp_sam_counts &c) {
    switch (J.route) {
    case Route::BAM:
    case Route::TEXT_CHAIN: return ingest_file_bam(J, i, c);
    case Route::SHARDED: return ingest_file_sharded(J, i, c);
    case Route::TOKENIZER: return ingest_file_device(J, i, c);
    default: return ingest_file_host(J, i, c);
    }
}
static int hand_over_batches(PolishJob &J) { return chained(J.route) ? (int)PP_OK : text_hand_over(J); }  // (the chain: added file by file)
static int said_about_its_source(PolishJob &J, int rc) { return chained(J.route) ? bam_polish_error(J, rc) : rc; }

// load_alignments, polish.rs:109-134.  A device tokenizer that meets a defect in the text (or bytes outside ASCII, which the
// host parsers must judge) only says so: which defect the reference reports FIRST also depends on what its CIGAR walk makes of
// the records before it, and the host ingest works that out (replay_records_before_defect): HAND_BACK, at J.handed_back_at.
static int load_alignments(PolishJob &J) {
    uint64_t alignment_total = 0, used_total = 0;
    J.log("Loading alignments\n");
    if (int rc = create_ingests(J)) return rc;
    for (int i = 0; i < J.n_sams; i++) {
        pp_sam_counts c{0, 0, 0};
        if (i == J.resume_log_at) J.log.quiet = J.opt->quiet != 0;
        const int rc = ingest_file(J, i, c);
        if (rc == HAND_BACK) J.handed_back_at = i;
        if (rc) return rc;
        J.log("%s: %s alignments from %s reads\n", J.sams[i], commas(c.alignments).c_str(), commas(c.reads).c_str());
        if (J.lap.on) { char what[64]; snprintf(what, sizeof what, "file %d ingested", i + 1); J.lap(what); }
        alignment_total += c.alignments;
        used_total += c.used;
    }
    if (int rc = J.text.wait_pending()) return rc;
    J.log("\nFiltering for high-quality end-to-end alignments%s:\n  %s alignments kept\n  %s alignments discarded\n\n",
          J.opt->careful ? " from reads with only one alignment" : "", commas(used_total).c_str(),
          commas(alignment_total - used_total).c_str());
    J.lap("alignments ingested");
    return PP_OK;
}

// create_debug_file, polish.rs:230-245: the file is created (and the header written) before polishing
static int create_debug_file(PolishJob &J) {
    if (J.opt->debug_path) {
        J.dbg = fopen(J.opt->debug_path, "wb");
        if (!J.dbg) {
            snprintf(J.err, sizeof J.err, "unable to create \"%s\"", J.opt->debug_path);
            return set_err(J.ctx, PP_ERR_QUIT, J.err);
        }
        fputs("name\tpos\tbase\tdepth\tinvalid\tvalid\tpileup\tstatus\tnew_base\n", J.dbg);
    }
    J.debug_set = true;
    for (int d = 0; d < J.n_ctx; d++) pp_polish_set_debug(J.ctxs[d], J.dbg || J.wants_status() ? 1 : 0);  // (--bed, --soft_mask, --depth: the records without a file)
    return PP_OK;
}
// ... and closed once the contexts have written their lines; they keep no per-position records from here on
int close_debug_file(PolishJob &J, int rc, bool say) {
    FILE *f = J.dbg;
    J.dbg = nullptr;
    if (f && fclose(f) && rc == PP_OK) rc = set_err(J.ctx, PP_ERR_QUIT, "unable to write to the --debug file");
    if (f && say) J.lap("--debug file written");
    for (int d = 0; d < J.n_ctx; d++) pp_polish_set_debug(J.ctxs[d], 0);
    J.debug_set = false;
    return rc;
}

// the polished bytes in the context's device memory: the job's own, or their soft-masked copy (pp_ctx_set_soft_mask)
static const uint8_t *polished_on_device(PolishJob &J) {
    if (!J.masked) return pp_polish_result_device(J.ctx);
    const uint8_t *dev = nullptr;
    pp_masked_bytes(J.masked, &dev, nullptr);
    return dev;
}

// The .tbi of pp_ctx_set_tbi for one track: pp_tabix_index on the track's device text and on the block table of its pp_bgzf_deflate,
// both read where they lie; one copy of the index into the job (J.tbi_file[which]).
static int make_tbi(PolishJob &J, int which, int preset, const uint8_t *text, uint64_t n_text, const pp_bgzf_out *z) {
    uint64_t n_blk = 0, bad = 0;
    const uint64_t *blk = pp_bgzf_out_blk_off(z, &n_blk);
    pp_bytes tbi{nullptr, 0};
    const int rc = pp_tabix_index(J.ctx, text, n_text, PP_MEM_DEVICE, preset, blk, n_blk, PP_MEM_DEVICE, &tbi, nullptr, &bad);
    if (rc == PP_OK) J.tbi_file[which].assign(tbi.data, tbi.data + tbi.len);
    pp_bytes_free(&tbi);
    return rc;
}

// The BED of pp_ctx_set_bed: pp_polish_bed on the finished job, pp_bgzf_deflate on the device text with bgzf, one copy off the
// device into the job (J.bed_file).  Nothing is logged.
static int make_bed(PolishJob &J) {
    pp_ctx *const ctx = J.ctx;
    pp_bed_out *text = nullptr;
    pp_bgzf_out *z = nullptr;
    const uint8_t *dev = nullptr;
    uint64_t n = 0;
    int rc = pp_polish_bed(ctx, J.names.data(), J.bed_mask, &text);
    if (rc == PP_OK) pp_bed_out_bytes(text, &dev, &n, nullptr);
    if (rc == PP_OK && J.bed_bgzf) {
        rc = pp_bgzf_deflate(ctx, dev, n, PP_MEM_DEVICE, &z);
        if (rc == PP_OK && J.tbi_on[PP_TBI_BED]) rc = make_tbi(J, PP_TBI_BED, PP_TBX_BED, dev, n, z);
        if (rc == PP_OK) pp_bgzf_out_bytes(z, &dev, &n);
    }
    if (rc == PP_OK) {  // (handed to the context once the whole run has succeeded: polish_once)
        J.bed_file.resize((size_t)n);
        if (n) rc = pp_ctx_download(ctx, J.bed_file.data(), dev, n);
    }
    pp_bgzf_out_free(z);
    pp_bed_out_free(text);
    J.lap(J.tbi_on[PP_TBI_BED] ? "BED made, compressed and indexed on the device" : J.bed_bgzf ? "BED made and compressed on the device" : "BED made on the device");
    return rc;
}

// The depth track of pp_ctx_set_depth, as make_bed: pp_polish_depth on the finished job, pp_bgzf_deflate on the device text with bgzf, one
// copy off the device into the job (J.depth_file).  Nothing is logged.
static int make_depth(PolishJob &J) {
    pp_ctx *const ctx = J.ctx;
    pp_depth_out *text = nullptr;
    pp_bgzf_out *z = nullptr;
    const uint8_t *dev = nullptr;
    uint64_t n = 0;
    int rc = pp_polish_depth(ctx, J.names.data(), J.depth_bin, &text);
    if (rc == PP_OK) pp_depth_out_bytes(text, &dev, &n, nullptr);
    if (rc == PP_OK && J.depth_bgzf) {
        rc = pp_bgzf_deflate(ctx, dev, n, PP_MEM_DEVICE, &z);
        if (rc == PP_OK && J.tbi_on[PP_TBI_DEPTH]) rc = make_tbi(J, PP_TBI_DEPTH, PP_TBX_BED, dev, n, z);
        if (rc == PP_OK) pp_bgzf_out_bytes(z, &dev, &n);
    }
    if (rc == PP_OK) {  // (handed to the context once the whole run has succeeded: polish_once)
        J.depth_file.resize((size_t)n);
        if (n) rc = pp_ctx_download(ctx, J.depth_file.data(), dev, n);
    }
    pp_bgzf_out_free(z);
    pp_depth_out_free(text);
    J.lap(J.tbi_on[PP_TBI_DEPTH] ? "depth track made, compressed and indexed on the device"
          : J.depth_bgzf         ? "depth track made and compressed on the device"
                                 : "depth track made on the device");
    return rc;
}

static int polish_on_one_context(PolishJob &J) {
    pp_ctx *const ctx = J.ctx;
    int rc = hand_over_batches(J);
    if (rc == PP_OK) rc = pp_polish_finish(ctx);
    if (rc) rc = said_about_its_source(J, rc);
    J.lap("uploaded + polished on device");
    if (rc == PP_OK && J.dbg) {
        rc = write_debug_tsv(ctx, J.dbg, J.names, 0, J.off[J.nc]);
        J.lap("--debug file written");
    }
    // (the BED and the masked bytes read the job's status: made before the records are closed)
    if (rc == PP_OK && J.bed_on) rc = make_bed(J);
    if (rc == PP_OK && J.depth_on) rc = make_depth(J);
    if (rc == PP_OK && J.soft_mask) {
        rc = pp_polish_masked(ctx, J.soft_mask, &J.masked);
        J.lap("polished bytes soft-masked on the device");
    }
    rc = close_debug_file(J, rc, false);
    if (rc == PP_OK) rc = pp_polish_result_size(ctx, &J.total);
    // offsets and statistics now; the bytes go straight into the FASTA buffer below (contig by contig) when that is a
    // handful of copies, else through one copy of everything
    // (with pp_ctx_set_fasta_form the bytes stay on the device for pp_fasta_text)
    J.direct_fetch = rc == PP_OK && (J.form_on || (J.fasta.buf && J.nc <= 256 && J.fasta.header_bytes + J.total + J.nc <= J.fasta.cap));
    if (!J.direct_fetch) J.polished.resize(J.total ? J.total : 1);
    if (rc == PP_OK) rc = pp_polish_result(ctx, J.direct_fetch || J.masked ? nullptr : J.polished.data(), PP_MEM_HOST, J.out_off.data(), J.stats.data());
    if (rc == PP_OK && J.masked && !J.direct_fetch && J.total) rc = pp_ctx_download(ctx, J.polished.data(), polished_on_device(J), J.total);
    return rc;
}

// print_polishing_info, polish.rs:206-227
static void log_polishing_info(PolishJob &J, uint32_t c) {
    const uint64_t *off = J.off;
    const char *name = J.names[c];
    const pp_contig_stats &s = J.stats[c];
    const double len = (double)(off[c + 1] - off[c]);
    const double changed_pct = 100.0 * (double)s.changed / len;
    J.log("Polishing %s (%s bp):\n  mean read depth: %.1fx\n  %s bp %s a depth of zero (%.4f%% coverage)\n"
          "  %s %s changed (%.4f%% of total positions)\n  estimated pre-polishing sequence accuracy: %.4f%% (%s)\n\n",
          name, commas(off[c + 1] - off[c]).c_str(), s.depth_sum / len, commas(s.zero_depth).c_str(),
          s.zero_depth == 1 ? "has" : "have", 100.0 * (len - (double)s.zero_depth) / len,
          commas(s.changed).c_str(), s.changed == 1 ? "position" : "positions", changed_pct,
          100.0 - changed_pct, qscore(100.0 - changed_pct).c_str());
}

// print_seq_to_stdout (polish.rs:196-203), one contig after the other in FASTA order, with print_polishing_info's lines
static int write_fasta_and_log(PolishJob &J, pp_bytes *fasta) {
    const uint32_t nc = J.nc;
    const uint64_t *out_off = J.out_off.data();
    J.fasta.join();
    if (!J.fasta.buf || J.fasta.header_bytes + J.total + nc > J.fasta.cap) {  // (a job whose polished bytes outgrow the bound: a buffer of the exact size)
        free(J.fasta.buf);
        J.fasta.buf = (uint8_t *)malloc(J.fasta.header_bytes + J.total + nc + 1);
        if (!J.fasta.buf) return set_err(J.ctx, PP_ERR_HIP, "out of host memory for the FASTA");
    }
    uint8_t *out = J.fasta.buf;
    const uint8_t *d_polished = J.direct_fetch ? polished_on_device(J) : nullptr;
    size_t w = 0;
    for (uint32_t c = 0; c < nc; c++) {
        const char *name = J.names[c], *desc = pp_assembly_description(J.a, c);
        out[w++] = '>';
        memcpy(out + w, name, strlen(name)); w += strlen(name);
        if (desc[0]) {
            out[w++] = ' ';
            memcpy(out + w, desc, strlen(desc)); w += strlen(desc);
        }
        memcpy(out + w, " polypolish\n", 12); w += 12;
        if (J.direct_fetch) {
            if (int rd = pp_ctx_download(J.ctx, out + w, d_polished + out_off[c], out_off[c + 1] - out_off[c])) return rd;
        } else memcpy(out + w, J.polished.data() + out_off[c], out_off[c + 1] - out_off[c]);
        w += out_off[c + 1] - out_off[c];
        out[w++] = '\n';
        log_polishing_info(J, c);
    }
    fasta->data = out;
    fasta->len = w;
    J.fasta.buf = nullptr;  // the caller's now (pp_bytes_free)
    J.lap("FASTA assembled");
    return PP_OK;
}

// The same FASTA in the form pp_ctx_set_fasta_form chose, made on the device: the headers go up, pp_fasta_text writes the text at the
// line width from the polished bytes where they lie -- in device memory on one context, in the host bytes the ranks' results were
// assembled into on several --, pp_bgzf_deflate follows on the device bytes, and what is returned comes off the device in one copy.
// The indexes stay with the context (pp_ctx_fasta_index).  The log's lines are write_fasta_and_log's.
static int write_fasta_form_and_log(PolishJob &J, pp_bytes *fasta) {
    const uint32_t nc = J.nc;
    pp_ctx *const ctx = J.ctx;
    std::string headers;
    std::vector<uint64_t> header_off(nc + 1, 0);
    for (uint32_t c = 0; c < nc; c++) {
        const char *desc = pp_assembly_description(J.a, c);
        headers += J.names[c];
        if (desc[0]) { headers += ' '; headers += desc; }
        headers += " polypolish";
        header_off[c + 1] = headers.size();
    }
    const bool on_device = J.direct_fetch;
    const uint8_t *src = on_device ? polished_on_device(J) : J.polished.data();
    pp_fasta_out *text = nullptr;
    pp_bgzf_out *z = nullptr;
    pp_bytes fai{nullptr, 0}, gzi{nullptr, 0};
    const uint8_t *dev = nullptr;
    uint64_t n = 0;
    int rc = pp_fasta_text(ctx, src, on_device ? PP_MEM_DEVICE : PP_MEM_HOST, nc, J.out_off.data(), (const uint8_t *)headers.data(), header_off.data(),
                           (uint32_t)J.form_width, &text);
    if (rc == PP_OK) rc = pp_fasta_out_fai(text, &fai);
    if (rc == PP_OK) pp_fasta_out_bytes(text, &dev, &n);
    if (rc == PP_OK && J.form_bgzf) {
        rc = pp_bgzf_deflate(ctx, dev, n, PP_MEM_DEVICE, &z);
        if (rc == PP_OK) rc = pp_bgzf_out_gzi(z, &gzi);
        if (rc == PP_OK) pp_bgzf_out_bytes(z, &dev, &n);
    }
    uint8_t *out = rc == PP_OK ? (uint8_t *)malloc((size_t)n + 1) : nullptr;
    if (rc == PP_OK && !out) rc = set_err(ctx, PP_ERR_HIP, "out of host memory for the FASTA");
    if (rc == PP_OK && n) rc = pp_ctx_download(ctx, out, dev, n);
    if (rc == PP_OK) pp_ctx_keep_fasta_index_(ctx, fai.data, fai.len, gzi.data, gzi.len);
    pp_bytes_free(&fai);
    pp_bytes_free(&gzi);
    pp_bgzf_out_free(z);
    pp_fasta_out_free(text);
    if (rc) {
        free(out);
        return rc;
    }
    for (uint32_t c = 0; c < nc; c++) log_polishing_info(J, c);
    fasta->data = out;
    fasta->len = n;
    J.lap(J.form_bgzf ? "FASTA text made and compressed on the device" : "FASTA text made on the device");
    return PP_OK;
}

// The VCF of pp_ctx_set_vcf: pp_polish_vcf on the finished job, pp_bgzf_deflate on the device text with bgzf, one copy off the
// device; the bytes stay with the context (pp_ctx_vcf).  Nothing is logged.
static int make_vcf(PolishJob &J, int bgzf) {
    pp_ctx *const ctx = J.ctx;
    pp_vcf_out *text = nullptr;
    pp_bgzf_out *z = nullptr;
    const uint8_t *dev = nullptr;
    uint64_t n = 0;
    int rc = pp_polish_vcf(ctx, J.names.data(), &text);
    if (rc == PP_OK) pp_vcf_out_bytes(text, &dev, &n, nullptr);
    if (rc == PP_OK && bgzf) {
        rc = pp_bgzf_deflate(ctx, dev, n, PP_MEM_DEVICE, &z);
        if (rc == PP_OK && J.tbi_on[PP_TBI_VCF]) rc = make_tbi(J, PP_TBI_VCF, PP_TBX_VCF, dev, n, z);
        if (rc == PP_OK) pp_bgzf_out_bytes(z, &dev, &n);
    }
    std::vector<uint8_t> host;
    if (rc == PP_OK) {
        host.resize((size_t)n + 1);
        if (n) rc = pp_ctx_download(ctx, host.data(), dev, n);
    }
    if (rc == PP_OK) pp_ctx_keep_vcf_(ctx, host.data(), n);
    pp_bgzf_out_free(z);
    pp_vcf_out_free(text);
    J.lap(J.tbi_on[PP_TBI_VCF] ? "VCF made, compressed and indexed on the device" : bgzf ? "VCF made and compressed on the device" : "VCF made on the device");
    return rc;
}

// finished_message, polish.rs:76-90
static void log_finished(const PolishJob &J) {
    const char *to = pp_ctx_fasta_out_name_(J.ctx);
    if (to[0]) J.log("Finished!\nPolished sequence (to %s):\n", to);
    else J.log("Finished!\nPolished sequence (to stdout):\n");
    for (uint32_t c = 0; c < J.nc; c++) J.log("  %s_polypolish (%s bp)\n", J.names[c], commas(J.stats[c].polished_len).c_str());
    J.log("\nTime to run: %s\n\n", format_duration(J.lap.seconds()).c_str());
}

// polish::polish (src/polish.rs:26-38) for one look at the input.  HAND_BACK: nothing was polished, the host ingest is to
// take the input, its log resuming at file J.handed_back_at.
static int polish_once(PolishJob &J, pp_bytes *fasta) {
    int vcf_bgzf = 0;
    const bool vcf_on = pp_ctx_vcf_form_(J.ctx, &vcf_bgzf) != 0;
    pp_ctx_keep_vcf_(J.ctx, nullptr, 0);  // (the file of the run before)
    if (vcf_on && J.n_ctx > 1)  // (a rank's share has no defined runs at its edges: pp_polish_vcf)
        return set_err(J.ctx, PP_ERR_QUIT, "--vcf runs on one GPU: polish without PP_GPUS / several contexts, or without --vcf");
    J.bed_on = pp_ctx_bed_form_(J.ctx, &J.bed_mask, &J.bed_bgzf) != 0;
    J.soft_mask = pp_ctx_soft_mask_(J.ctx);
    pp_ctx_keep_bed_(J.ctx, nullptr, 0);  // (the file of the run before)
    if (J.bed_on && J.n_ctx > 1)  // (the status plane of a rank is its share's: pp_polish_bed)
        return set_err(J.ctx, PP_ERR_QUIT, "--bed runs on one GPU: polish without PP_GPUS / several contexts, or without --bed");
    if (J.soft_mask && J.n_ctx > 1)
        return set_err(J.ctx, PP_ERR_QUIT, "--soft_mask runs on one GPU: polish without PP_GPUS / several contexts, or without --soft_mask");
    J.depth_on = pp_ctx_depth_form_(J.ctx, &J.depth_bin, &J.depth_bgzf) != 0;
    pp_ctx_keep_depth_(J.ctx, nullptr, 0);  // (the file of the run before)
    if (J.depth_on && J.n_ctx > 1)  // (the depth plane of a rank is its share's: pp_polish_depth)
        return set_err(J.ctx, PP_ERR_QUIT, "--depth runs on one GPU: polish without PP_GPUS / several contexts, or without --depth");
    for (int w = 0; w <= PP_TBI_DEPTH; w++) {
        J.tbi_on[w] = pp_ctx_tbi_form_(J.ctx, w) != 0;
        pp_ctx_keep_tbi_(J.ctx, w, nullptr, 0);  // (the index of the run before)
    }
    if ((J.tbi_on[PP_TBI_VCF] && !(vcf_on && vcf_bgzf)) || (J.tbi_on[PP_TBI_BED] && !(J.bed_on && J.bed_bgzf)) || (J.tbi_on[PP_TBI_DEPTH] && !(J.depth_on && J.depth_bgzf)))
        return set_err(J.ctx, PP_ERR_ARG, "pp_ctx_set_tbi: a .tbi indexes a bgzipped track: switch the track on with bgzf (pp_ctx_set_vcf, pp_ctx_set_bed, pp_ctx_set_depth)");
    if (int rc = check_options_and_inputs(J)) return rc;
    log_banner(J);
    J.lap("driver entered");
    if (int rc = load_assembly(J)) return rc;
    J.lap("assembly loaded");
    J.form_on = pp_ctx_fasta_form_(J.ctx, &J.form_width, &J.form_bgzf) != 0;
    if (!J.form_on) reserve_fasta(J);  // (the form's text is made on the device)
    if (int rc = load_alignments(J)) return rc;
    // polish_sequences, polish.rs:137-154 -- on the device
    J.log("Polishing assembly sequences\n");
    if (int rc = create_debug_file(J)) return rc;
    if (int rc = several_contexts(J.route) ? polish_on_several_contexts(J) : polish_on_one_context(J)) return rc;
    J.lap(J.direct_fetch ? "result: offsets fetched" : "result fetched");
    if (vcf_on)
        if (int rc = make_vcf(J, vcf_bgzf)) return rc;
    if (int rc = J.form_on ? write_fasta_form_and_log(J, fasta) : write_fasta_and_log(J, fasta)) return rc;
    if (J.bed_on) {  // (a run that fails leaves no file: pp_ctx_bed)
        J.bed_file.push_back(0);
        pp_ctx_keep_bed_(J.ctx, J.bed_file.data(), J.bed_file.size() - 1);
    }
    if (J.depth_on) {  // (as the BED: pp_ctx_depth)
        J.depth_file.push_back(0);
        pp_ctx_keep_depth_(J.ctx, J.depth_file.data(), J.depth_file.size() - 1);
    }
    for (int w = 0; w <= PP_TBI_DEPTH; w++)  // (as the tracks: pp_ctx_tbi)
        if (J.tbi_on[w]) pp_ctx_keep_tbi_(J.ctx, w, J.tbi_file[w].data(), J.tbi_file[w].size());
    log_finished(J);
    J.release();
    J.lap("device and host buffers released");
    return PP_OK;
}

}  // namespace ppd

using namespace ppd;

static int polish_files_impl(pp_ctx *const *ctxs, int n_ctx, const char *assembly, const char *const *sams, int n_sams,
                             const pp_polish_options *opt, pp_bytes *fasta, const uint8_t *const *pass, const uint64_t *n_pass,
                             const BamGiven *given = nullptr) {
    if (!ctxs[0] || !assembly || !opt || !fasta || (n_sams > 0 && !sams)) return PP_ERR_ARG;
    fasta->data = nullptr;
    fasta->len = 0;
    // The second look, if the device tokenizer hands a file back: a job of its own on the host ingest, after everything of
    // the first has been released.
    for (int resume_log_at = -1;;) {
        PolishJob job{ctxs, n_ctx, assembly, sams, n_sams, opt, pass, n_pass, resume_log_at};
        if (given) job.borrow(*given);
        const int rc = polish_once(job, fasta);
        if (rc != HAND_BACK) return rc;
        resume_log_at = job.handed_back_at;
    }
}

extern "C" int pp_polish_files_filtered_(pp_ctx *ctx, const char *assembly, const char *const *sams, int n_sams,
                                         const pp_polish_options *opt, pp_bytes *fasta,
                                         const uint8_t *const *pass, const uint64_t *n_pass) {
    return polish_files_impl(&ctx, 1, assembly, sams, n_sams, opt, fasta, pass, n_pass);
}

int ppb::polish_bam_fronts(pp_ctx *ctx, const char *assembly, pp_assembly *a, ppb::Front *const *fronts, pp_names *rnames, pp_names *qnames,
                           const char *const *paths, int n, const pp_polish_options *opt, pp_bytes *fasta, const uint8_t *const *pass,
                           const uint64_t *n_pass) {
    const BamGiven given{a, fronts, rnames, qnames};
    return polish_files_impl(&ctx, 1, assembly, paths, n, opt, fasta, pass, n_pass, &given);
}

extern "C" int pp_polish_files(pp_ctx *ctx, const char *assembly, const char *const *sams, int n_sams,
                               const pp_polish_options *opt, pp_bytes *fasta) {
    return polish_files_impl(&ctx, 1, assembly, sams, n_sams, opt, fasta, nullptr, nullptr);
}

// One process, several GPUs (polish::polish has no counterpart: src/polish.rs:137-154 is one thread): every context
// uploads and tokenizes its own slice of every SAM file (or the host ingest parses once), the records are partitioned --
// a context is sent the records that reach its units (pp_shard_split) -- the contexts polish side by side on their own
// threads, and every device copies its own share of the polished bytes out for the host to put together -- or, with
// PP_GATHER=rccl, the bytes meet on the first context's GPU in ONE RCCL gather over xGMI (pp_polish_gather: the north
// star's "single RCCL gather for the final FASTA") followed by one device-to-host copy.  The RCCL route of THIS driver is
// opt-in until it has run on a multi-GPU node (see below); it cannot run without librccl or with two contexts on one
// device (PP_SHARE_GPU, tests).  PP_TIMING prints the route that was taken.
extern "C" int pp_polish_files_multi(pp_ctx *const *ctxs, int n_ctx, const char *assembly, const char *const *sams,
                                     int n_sams, const pp_polish_options *opt, pp_bytes *fasta) {
    if (!ctxs || n_ctx < 1) return PP_ERR_ARG;
    for (int i = 0; i < n_ctx; i++)
        if (!ctxs[i]) return PP_ERR_ARG;
    return polish_files_impl(ctxs, n_ctx, assembly, sams, n_sams, opt, fasta, nullptr, nullptr);
}

extern "C" int pp_log_text(int what, double value, char *out, size_t cap) {
    if (!out || cap == 0) return PP_ERR_ARG;
    std::string s;
    switch (what) {
    case PP_TEXT_QSCORE: s = pph::qscore(value); break;
    case PP_TEXT_DURATION: s = pph::format_duration_us((uint64_t)value); break;
    case PP_TEXT_PERCENTILE_NAME: s = pph::percentile_name(value); break;
    default: return PP_ERR_ARG;
    }
    if (s.size() + 1 > cap) return PP_ERR_ARG;
    memcpy(out, s.c_str(), s.size() + 1);
    return PP_OK;
}
