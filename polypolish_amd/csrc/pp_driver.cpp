// pp_driver.cpp -- whole-command drivers behind the `polypolish` CLI contract.
//   pp_polish_files  = polish::polish   (src/polish.rs:26-38)
// Output bytes (FASTA on stdout, filtered SAMs) are the contract; the stderr log reproduces the
// reference's numbers (counts, depth, changed positions, Q-score) in plain text -- the
// reference's colours, wrapping and timestamps (src/log.rs) are cosmetic and not reproduced.
#include <sys/stat.h>

#include <chrono>
#include <functional>
#include <future>
#include <memory>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include <algorithm>

#include "polypolish_hip.h"
#include "pp_host.h"
#include "pp_bam_files.h"

namespace {

using pph::commas;
using pph::format_duration;
using pph::Log;
using pph::qscore;

bool exists(const char *p) {
    struct stat st;
    return stat(p, &st) == 0;
}

int set_err(pp_ctx *ctx, int code, const char *msg) { return pp_ctx_set_error_(ctx, code, msg); }

}  // namespace

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
static int write_debug_tsv(pp_ctx *ctx, FILE *f, const std::vector<const char *> &names, uint64_t lo, uint64_t hi) {
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

namespace {

// ---- several GPUs, ONE copy of the text: every GPU uploads and tokenizes a slice of each SAM file ---------------------
// Where may a file be cut?  At the start of a line that opens a read group (src/alignment.rs:255-263: an aligned record
// joins the group of the aligned record before it when that one's QNAME is empty or equal; header, empty and unaligned
// lines neither join nor close anything).  Returns the first such line start at or after `from`, or `size`.
struct LineView { const char *q; size_t qlen; bool aligned; };
LineView look_at_line(const char *text, size_t ls, size_t le) {
    LineView v{text + ls, 0, false};
    if (le == ls || text[ls] == '@') return v;
    const char *tab = (const char *)memchr(text + ls, '\t', le - ls);
    if (!tab) return v;
    v.qlen = (size_t)(tab - (text + ls));
    const char *f = tab + 1, *end = text + le;
    if (f < end && *f == '+') f++;
    unsigned long long flag = 0;
    const char *d = f;
    while (d < end && *d >= '0' && *d <= '9' && d - f < 12) flag = flag * 10 + (unsigned long long)(*d++ - '0');
    if (d == f || (d < end && *d != '\t')) return v;  // not a number: the tokenizer will say so; no cut here
    v.aligned = (flag & 4ull) == 0;
    return v;
}
size_t group_cut(const char *text, size_t size, size_t from) {
    if (from == 0) return 0;
    if (from >= size) return size;
    // the start of the first line at or after `from`
    size_t p = from;
    if (text[p - 1] != '\n') {
        const char *nl = (const char *)memchr(text + p, '\n', size - p);
        if (!nl) return size;
        p = (size_t)(nl - text) + 1;
    }
    // the aligned record before it (scan back over header / empty / unaligned lines; give up after a while: then the
    // first aligned line at or after p is compared with nothing and the search just moves on one group)
    bool have_prev = false, unknown_prev = false;
    const char *pq = nullptr;
    size_t pql = 0;
    {
        size_t e = p;  // e = one past the '\n' that ends the line being looked at
        for (int tries = 0; tries < 4096 && e > 0; tries++) {
            const size_t le = e - 1;  // the '\n'
            size_t ls = le;
            while (ls > 0 && text[ls - 1] != '\n') ls--;
            const LineView v = look_at_line(text, ls, le);
            if (v.aligned) { have_prev = true; pq = v.q; pql = v.qlen; break; }
            e = ls;
        }
        // A long stretch without aligned records (unmapped reads grouped together): the aligned record before it is out
        // of sight, so the first aligned line from p on may still belong to ITS group.  It is then taken as the record to
        // compare with, and the cut falls on the first QNAME change after it -- a boundary whatever came before.  (Until
        // round 4 this gave up and returned `size`: every later cut then fell on `size` too and one GPU tokenized the rest
        // of the file.)
        unknown_prev = !have_prev && e > 0;
    }
    while (p < size) {
        const char *nl = (const char *)memchr(text + p, '\n', size - p);
        const size_t le = nl ? (size_t)(nl - text) : size;
        const LineView v = look_at_line(text, p, le);
        if (v.aligned) {
            if (unknown_prev) unknown_prev = false;
            else if (!have_prev || (pql != 0 && (pql != v.qlen || memcmp(pq, v.q, pql) != 0))) return p;
            have_prev = true; pq = v.q; pql = v.qlen;
        }
        p = le + 1;
    }
    return size;
}

// one stretch of records handed to a destination context, for turning its rank-local record numbers back into the job's
struct Piece { pp_shard_part *part; int src; uint64_t base, n; };

// the job-wide number of the record a context's device error is about, or ~0 (not a record-level error)
uint64_t job_record_of(pp_ctx *cd, pp_ctx *const *ctxs, const std::vector<Piece> &pieces, uint32_t *kind) {
    uint64_t local = 0;
    if (!pp_polish_error_record(cd, &local, kind)) return ~0ull;
    uint64_t at = 0;
    for (const Piece &pc : pieces) {
        if (local < at + pc.n) {
            const uint32_t *orig = nullptr;
            pp_shard_part_batch(pc.part, nullptr, &orig);
            uint32_t o = 0;
            if (pp_shard_part_mem(pc.part) == PP_MEM_HOST) o = orig[local - at];
            else if (pp_ctx_download(ctxs[pc.src], &o, orig + (local - at), 4) != PP_OK) return ~0ull;
            return pc.base + o;
        }
        at += pc.n;
    }
    return ~0ull;
}

// ---- the polish command: one job object, stages over it ----------------------------------------------------------------
// a source batch of the multi-context job, in file order: sharded -> a (file, slice) piece living on a context's GPU; host
// ingest -> a file
struct Src { pp_aln_batch view; int owner; uint64_t base; uint32_t wo_base; std::vector<uint64_t> runs; };
// what a context brought back
struct RankResult {
    int rc = PP_OK;
    uint64_t total = 0;
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> off;
    std::vector<pp_contig_stats> stats;
};

// what an ingest_file_* returns for a file the host ingest must look at again (not a PP_ERR_* code); the caller decides
constexpr int HAND_BACK = -1;
int hand_back_if_text_defect(int rc) { return rc == PP_ERR_QUIT || rc == PP_ERR_PANIC || rc == PP_ERR_NOT_ASCII ? HAND_BACK : rc; }

struct BamGiven { pp_assembly *a; ppb::BamFile *const *fronts; pp_names *rnames, *qnames; };
// a gated batch that went into the job: its file, and where its records start among the job's (a device error names a job record)
struct BamAdded { int file; uint64_t base, n; const pp_gated *g; };
constexpr uint32_t KIND_BAD_CONTIG = 4;  // DE_BAD_CONTIG (pp_internal.h), as pp_polish_error_record reports it

// Everything one `polish` command allocates, opens or starts.  release() gives all of it back -- uploads in flight are joined
// before the batches they read are freed, the FASTA buffer's toucher before the buffer -- and the destructor calls it: every
// way out of the driver is a plain return.
struct PolishJob {
    pp_ctx *const *ctxs;
    int n_ctx;
    const char *assembly;
    const char *const *sams;
    int n_sams;
    const pp_polish_options *opt;
    // optional per-file filter verdicts (pp_ingest_sam_filtered), used by pp_filter_polish_files
    const uint8_t *const *pass;
    const uint64_t *n_pass;
    // resume_log_at >= 0: the second look at an input the device tokenizer handed back, on the host ingest only.  The banner,
    // the assembly section and the lines of the files before that one are on stderr already: the log resumes at that file.
    int resume_log_at;
    // BAM files that pp_filter_polish_files has opened and decoded already (all borrowed), or NULL
    const BamGiven *given = nullptr;
    int handed_back_at = -1;  // the file at which this look ended with HAND_BACK
    pp_ctx *ctx = ctxs[0];    // carries the error text
    // Several contexts: every GPU uploads and tokenizes its own slice of each file (`sharded`), so a byte of text crosses
    // PCIe once; the host ingest (PP_DEVICE_INGEST=0, or a file the tokenizer handed back) parses once and sends every
    // context the records that reach its units.
    // Host ingest: one ingest object per SAM file (`per_file`), and (one context: `stream_adds`) the batch of file i goes to the
    // device (pp_polish_begin + pp_polish_add on a helper thread) while file i+1 is parsed -- the reference streams its files
    // one after the other as well (alignment.rs:238-265).  Several contexts: the files' batches wait until the plan is known,
    // then every context is sent its part.
    static bool off_by_env(const char *name) { return getenv(name) && atoi(getenv(name)) == 0; }
    bool multi = n_ctx > 1;
    bool dev_ingest = resume_log_at < 0 && !off_by_env("PP_DEVICE_INGEST");
    bool sharded = multi && dev_ingest;
    bool per_file = !dev_ingest && (multi || !off_by_env("PP_STREAM_ADDS"));
    bool stream_adds = per_file && !multi;
    Log log{opt->quiet != 0 || resume_log_at >= 0};
    pph::Lap lap{"", 36, true};  // "[timing] <stage>  <seconds since the driver was entered>  (process <seconds>)"
    pp_params prm{opt->min_depth, opt->fraction_valid, opt->fraction_invalid};
    char err[1024] = "";
    pp_assembly *a = nullptr;
    uint32_t nc = 0;
    const uint64_t *off = nullptr;
    std::vector<const char *> names;
    uint8_t *out = nullptr;  // the FASTA that will be returned (reserve_fasta)
    size_t fasta_cap = 0;
    size_t header_bytes = 0;
    std::thread out_toucher;
    std::vector<uint64_t> sam_bytes;  // the SAM files' sizes on disk (0: not a regular file)
    pp_ingest *g = nullptr;           // host ingest, all files in one ...
    std::vector<pp_ingest *> gs;      // ... or one per file
    pp_dev_ingest *dg = nullptr;
    std::vector<pp_dev_ingest *> dgs;       // sharded ingest: one per context
    // BAM input (all files of a command are of one kind): the record chain on the device, file by file (ingest_file_bam).  The gated
    // batches (and the prepared ones, PP_BAM_PREPARE=1) live until pp_polish_finish has returned.
    bool bam = given != nullptr;
    std::vector<int> kinds;  // pp_aln_file_kind of every file
    std::vector<std::unique_ptr<ppb::BamFile>> fronts;
    pp_names *rnames = nullptr, *qnames = nullptr;  // RNAME -> contig index (seeded with the assembly's names); QNAME -> read_id
    std::vector<pp_gated *> gated;
    std::vector<pp_prepared *> prepared;
    std::vector<BamAdded> added;
    bool bam_prepare = getenv("PP_BAM_PREPARE") && atoi(getenv("PP_BAM_PREPARE")) != 0;
    std::vector<std::future<int>> pending;  // the upload of the file before
    bool begun = false;                     // pp_polish_begin has run on ctx
    uint64_t alignment_total = 0;
    uint64_t used_total = 0;
    // sharded: the records of file i's slice on context s are records [slice_end[i-1][s], slice_end[i][s]) of its batch
    std::vector<std::vector<uint64_t>> slice_end;
    std::vector<Src> srcs;
    pp_shard_plan *plan = nullptr;
    std::vector<std::vector<Piece>> pieces;  // [context][source]: the parts (owned here from the split on) in file order
    bool use_rccl = false;                   // the gather route
    bool comms = false;                      // the communicators exist
    std::vector<RankResult> ranks;
    std::vector<uint8_t> gathered;
    FILE *dbg = nullptr;
    bool debug_set = false;  // pp_polish_set_debug was called on the contexts
    uint64_t total = 0;
    bool direct_fetch = false;
    std::vector<uint8_t> polished = std::vector<uint8_t>(1);
    std::vector<uint64_t> out_off;
    std::vector<pp_contig_stats> stats;

    // (an input that is handed back keeps its pre-faulted mappings: the host ingest of the second look takes them)
    ~PolishJob() {
        release();
        if (handed_back_at < 0) pph::prefetch_drop_all(ctx);
    }
    int wait_pending() {
        int r = PP_OK;
        for (auto &p : pending)
            if (const int ri = p.get()) r = r ? r : ri;
        pending.clear();
        return r;
    }
    // the communicators, the plan and what the contexts brought back: not needed once the FASTA's bytes are in `polished`
    void release_exchange() {
        for (int d = 0; comms && d < n_ctx; d++) pp_comm_destroy(ctxs[d]);
        comms = false;
        pp_shard_plan_free(plan);
        plan = nullptr;
        ranks = {};
        gathered = {};
    }
    void release() {
        (void)wait_pending();
        if (dbg) fclose(dbg);
        for (int d = 0; debug_set && d < n_ctx; d++) pp_polish_set_debug(ctxs[d], 0);
        release_exchange();
        for (auto &v : pieces)
            for (Piece &pc : v) pp_shard_part_free(pc.part);
        for (pp_ingest *x : gs) pp_ingest_free(x);
        pp_ingest_free(g);
        pp_dev_ingest_free(dg);
        for (pp_dev_ingest *x : dgs) pp_dev_ingest_free(x);
        for (pp_prepared *x : prepared) pp_prepared_free(x);
        for (pp_gated *x : gated) pp_gated_free(x);
        prepared.clear();
        gated.clear();
        added.clear();
        fronts.clear();
        if (!given) {
            pp_names_free(qnames);
            pp_names_free(rnames);
        }
        qnames = rnames = nullptr;
        if (!given) pp_assembly_free(a);
        if (out_toucher.joinable()) out_toucher.join();
        free(out);
        pieces.clear();
        gs.clear();
        dgs.clear();
        dbg = nullptr;
        g = nullptr;
        dg = nullptr;
        a = nullptr;
        out = nullptr;
        debug_set = false;
    }
};

// run f(d) for every context on its own thread; the first failure (lowest d) is returned, its text put on ctxs[0]
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

int check_options_and_inputs(PolishJob &J) {
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
    J.kinds.assign((size_t)J.n_sams, J.given ? PP_ALN_BAM : PP_ALN_SAM);
    int first_sam = -1, first_bam = -1;
    for (int i = 0; i < J.n_sams; i++) {
        if (!J.given)
            if (int rc = ppb::file_kind(J.ctx, J.sams[i], &J.kinds[(size_t)i])) return rc;
        int &first = J.kinds[(size_t)i] == PP_ALN_SAM ? first_sam : first_bam;
        if (first < 0) first = i;
    }
    if (first_sam >= 0 && first_bam >= 0)
        return ppb::fail(J.ctx, PP_ERR_QUIT, "the alignment files of one command must all be SAM text or all be BAM: \"%s\" is SAM text, \"%s\" is BAM",
                         J.sams[first_sam], J.sams[first_bam]);
    J.bam = first_bam >= 0;
    if (J.bam && J.multi)
        return ppb::fail(J.ctx, PP_ERR_QUIT, "BAM input (\"%s\") runs on one GPU: polish it without PP_GPUS / several contexts, or convert it to SAM text",
                         J.sams[first_bam]);
    // The device tokenizer uploads the SAM text as it is: map the files and pre-fault the mappings NOW, on background
    // threads, while the HIP runtime is still initialising (a copy out of an untouched mapping runs at a quarter of
    // the link's rate).
    for (int i = 0; J.dev_ingest && i < J.n_sams; i++) pph::prefetch_file(J.sams[i], J.ctx);
    J.sam_bytes.assign((size_t)J.n_sams, 0);
    for (int i = 0; i < J.n_sams; i++) {
        struct stat st;
        if (stat(J.sams[i], &st) == 0 && S_ISREG(st.st_mode)) J.sam_bytes[(size_t)i] = (uint64_t)st.st_size;
    }
    return PP_OK;
}

// starting_message, polish.rs:41-73
void log_banner(const PolishJob &J) {
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
int load_assembly(PolishJob &J) {
    J.log("Loading assembly\n");
    if (J.given) J.a = J.given->a;  // (loaded for the filter's RNAME table already)
    else if (int rc = pp_assembly_load(J.assembly, &J.a, J.err, sizeof J.err)) return set_err(J.ctx, rc, J.err);
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
void reserve_fasta(PolishJob &J) {
    size_t cap = 0;
    for (uint32_t c = 0; c < J.nc; c++) cap += strlen(J.names[c]) + strlen(pp_assembly_description(J.a, c)) + 16;
    J.header_bytes = cap;
    cap += (size_t)(J.off[J.nc] + J.off[J.nc] / 8) + 2 * (size_t)J.nc + 65536;  // (every planted insertion adds a byte: far below 1/8)
    J.fasta_cap = cap;
    uint8_t *out = J.out = (uint8_t *)malloc(cap);
    if (out) J.out_toucher = std::thread([out, cap] { for (size_t q = 0; q < cap; q += 4096) out[q] = 0; });
}

// the ingest objects of the job's route -- the device tokenizer (pp_tokenize.hip), one per context when sharded, or the host's
// (multi-threaded parse) with PP_DEVICE_INGEST=0
int create_ingests(PolishJob &J) {
    const pp_polish_options *opt = J.opt;
    int rc = PP_OK;
    if (J.bam) {  // no ingest object: the two name tables of the record chain, and the job the gated batches are added to
        if (J.given) {
            J.rnames = J.given->rnames;
            J.qnames = J.given->qnames;
        } else {
            rc = pp_names_create(J.ctx, J.nc, &J.rnames);
            if (rc == PP_OK) rc = ppb::seed_names(J.rnames, J.a);
            if (rc == PP_OK) rc = pp_names_create(J.ctx, 0, &J.qnames);
        }
        if (rc == PP_OK) rc = pp_polish_begin(J.ctx, J.nc, J.off, pp_assembly_bases(J.a), PP_MEM_HOST, &J.prm);
        J.begun = rc == PP_OK;
        J.lap("device ready, polish job open");
        return rc;
    }
    if (J.multi) pp_ctx_enable_peers_(J.ctxs, J.n_ctx);
    if (J.sharded) {
        J.dgs.assign((size_t)J.n_ctx, nullptr);
        rc = on_all(J, [&](int d) { return pp_dev_ingest_create(J.ctxs[d], J.a, opt->max_errors, opt->careful, &J.dgs[(size_t)d]); });
    } else if (J.dev_ingest) {
        rc = pp_dev_ingest_create(J.ctx, J.a, opt->max_errors, opt->careful, &J.dg);
        uint64_t largest = 0, total = 0;
        for (uint64_t b : J.sam_bytes) { largest = std::max(largest, b); total += b; }
        if (rc == PP_OK && largest) rc = pp_dev_ingest_reserve_text_(J.dg, largest);
        if (rc == PP_OK && J.n_sams > 1) rc = pp_dev_ingest_expect(J.dg, total);  // the batch's arrays sized once, for all the files
    } else if (!J.per_file) {
        rc = pp_ingest_create(J.a, opt->max_errors, opt->careful, &J.g);
    }
    if (J.dev_ingest) J.lap("device ready, tokenizer created");  // (pp_dev_ingest_create waits for the HIP runtime's start-up)
    return rc;
}

// cut the file into one slice per context at read-group boundaries; every context uploads and tokenizes its own
int ingest_file_sharded(PolishJob &J, int i, pp_sam_counts &c) {
    const size_t n = (size_t)J.n_ctx;
    pph::FileText F;
    if (!F.open_file(J.sams[i])) {
        snprintf(J.err, sizeof J.err, "unable to load alignments from \"%s\"", J.sams[i]);
        return set_err(J.ctx, PP_ERR_QUIT, J.err);
    }
    std::vector<size_t> cut(n + 1, F.size);
    cut[0] = 0;
    for (size_t d = 1; d < n; d++) cut[d] = std::max(cut[d - 1], group_cut(F.text, F.size, F.size / n * d));
    std::vector<pp_sam_counts> cs(n);
    int rs = on_all(J, [&](int d) {
        const size_t s = (size_t)d;
        return pp_dev_ingest_slice_(J.dgs[s], J.sams[i], F.text + cut[s], cut[s + 1] - cut[s], &cs[s]);
    });
    for (auto &x : cs) { c.alignments += x.alignments; c.used += x.used; c.reads += x.reads; }
    if (rs == PP_OK && c.alignments == 0) rs = PP_ERR_PANIC;  // a file without aligned records: the host path has the message
    if (rs) return hand_back_if_text_defect(rs);  // as for one context
    std::vector<uint64_t> ends(n);
    for (size_t d = 0; d < n; d++) {
        pp_aln_batch bd;
        pp_dev_ingest_batch(J.dgs[d], &bd);
        ends[d] = bd.n_aln;
    }
    J.slice_end.push_back(ends);
    return PP_OK;
}

int ingest_file_device(PolishJob &J, int i, pp_sam_counts &c) {
    // the text of the NEXT file goes up (second text buffer, upload stream) while this one is tokenized
    if (i + 1 < J.n_sams) pp_dev_ingest_prefetch_(J.dg, J.sams[i + 1], *std::max_element(J.sam_bytes.begin(), J.sam_bytes.end()));
    return hand_back_if_text_defect(J.pass ? pp_dev_ingest_sam_filtered(J.dg, J.sams[i], J.pass[i], J.n_pass[i], &c)
                                           : pp_dev_ingest_sam(J.dg, J.sams[i], &c));
}

// The host ingest `gi` refused file i with (rc, J.err).  The reference streams: every read group before the failing point
// had already gone through add_alignment (alignment.rs:297-303), so a record there that only the CIGAR walk rejects
// (unexpected op, CIGAR / SEQ length mismatch, past the contig end) is what it reports.  Run the device over exactly those
// records: the earlier files and this file up to the group that was pending.  Returns the error that stands.
int replay_records_before_defect(PolishJob &J, int i, const pp_ingest *gi, int rc) {
    pp_ctx *const ctx = J.ctx;
    uint64_t cut = 0;
    if (!pp_ingest_fail_cut_(gi, &cut) || J.wait_pending() != PP_OK) return rc;
    int rd = J.begun ? PP_OK : pp_polish_begin(ctx, J.nc, J.off, pp_assembly_bases(J.a), PP_MEM_HOST, &J.prm);
    J.begun = true;
    auto add = [&](const pp_ingest *x) {
        pp_aln_batch b;
        pp_ingest_batch(x, &b);
        if (rd == PP_OK && b.n_aln) rd = pp_polish_add(ctx, &b, PP_MEM_HOST);
    };
    if (!J.per_file && J.g) add(J.g);
    if (J.multi)  // (the earlier files' batches have not gone anywhere yet: the first context takes them whole)
        for (size_t q = 0; q + 1 < J.gs.size(); q++) add(J.gs[q]);
    pp_ingest *gp = nullptr;
    char err2[256];
    pp_sam_counts c2;
    if (rd == PP_OK && cut > 0 && pp_ingest_create(J.a, J.opt->max_errors, J.opt->careful, &gp) == PP_OK &&
        pp_ingest_sam_prefix_(gp, J.sams[i], cut, J.pass ? J.pass[i] : nullptr, J.pass ? J.n_pass[i] : 0, &c2, err2, sizeof err2) == PP_OK)
        add(gp);
    if (rd == PP_OK) rd = pp_polish_finish(ctx);
    pp_ingest_free(gp);
    if (rd == PP_ERR_QUIT || rd == PP_ERR_PANIC) return rd;  // the device's message stands
    return set_err(ctx, rc, J.err);
}

int ingest_file_host(PolishJob &J, int i, pp_sam_counts &c) {
    pp_ctx *const ctx = J.ctx;
    pp_ingest *gi = J.g;
    if (J.per_file) {
        if (int rc = pp_ingest_create(J.a, J.opt->max_errors, J.opt->careful, &gi)) return rc;
        J.gs.push_back(gi);
    }
    int rc = J.pass ? pp_ingest_sam_filtered(gi, J.sams[i], J.pass[i], J.n_pass[i], &c, J.err, sizeof J.err)
                    : pp_ingest_sam(gi, J.sams[i], &c, J.err, sizeof J.err);
    if (rc) {
        set_err(ctx, rc, J.err);
        return replay_records_before_defect(J, i, gi, rc);
    }
    if (!J.stream_adds) return PP_OK;
    if ((rc = J.wait_pending())) return rc;  // the upload of the file before
    const bool first = !J.begun;
    J.begun = true;
    // room for all files at once: this file's batch scaled by the files' sizes on disk
    double scale = 1.0, all_bytes = 0;
    for (uint64_t b : J.sam_bytes) all_bytes += (double)b;
    if (first && J.n_sams > 1 && J.sam_bytes[(size_t)i] > 0) scale = std::min(64.0, all_bytes / (double)J.sam_bytes[(size_t)i] * 1.02);
    J.pending.push_back(std::async(std::launch::async, [ctx, gi, first, scale, nc = J.nc, off = J.off, a = J.a, prm = J.prm]() {
        int r = first ? pp_polish_begin(ctx, nc, off, pp_assembly_bases(a), PP_MEM_HOST, &prm) : PP_OK;
        pp_aln_batch bi;
        pp_ingest_batch(gi, &bi);
        if (r == PP_OK && first && scale > 1.0)
            r = pp_polish_reserve(ctx, (uint64_t)((double)bi.n_aln * scale) + 1024, (uint64_t)((double)bi.seq_bytes * scale) + 4096,
                                  (uint64_t)((double)bi.n_cig_total * scale) + 1024);
        if (r == PP_OK) r = pp_polish_add(ctx, &bi, PP_MEM_HOST);
        return r;
    }));
    return PP_OK;
}

// ---- BAM: the record chain on the device (pp_bam_files.h -> pp_batch_gate -> pp_polish_add), file by file ----
// The error pp_polish_finish left about a job record, said about the BAM record it came from: the path and the 1-based number
// counting all records of the file; a good alignment on a reference the assembly lacks in the reference's own words.
int bam_polish_error(PolishJob &J, int rc) {
    pp_ctx *const ctx = J.ctx;
    uint64_t record = 0;
    uint32_t kind = 0;
    if ((rc != PP_ERR_QUIT && rc != PP_ERR_PANIC) || !pp_polish_error_record(ctx, &record, &kind)) return rc;
    const std::string said = pp_last_error(ctx);
    for (const BamAdded &A : J.added) {
        if (record < A.base || record - A.base >= A.n) continue;
        pp_aln_batch b;
        const uint32_t *orig = nullptr;
        pp_gated_batch(A.g, &b, &orig);
        uint32_t o = 0, contig = 0;
        if (pp_ctx_download(ctx, &o, orig + (record - A.base), 4) != PP_OK || pp_ctx_download(ctx, &contig, b.contig + (record - A.base), 4) != PP_OK) break;
        if (kind == KIND_BAD_CONTIG)
            return ppb::fail(ctx, rc, "query name %s in SAM but not in assembly: \"%s\" (record %llu)", ppb::name_of(J.rnames, contig).c_str(),
                             J.sams[A.file], (unsigned long long)o + 1);
        return ppb::fail(ctx, rc, "%s: \"%s\" (record %llu)", said.c_str(), J.sams[A.file], (unsigned long long)o + 1);
    }
    return set_err(ctx, rc, said.c_str());
}

int bam_add_gated(PolishJob &J, int i, const pp_gated *g) {
    pp_aln_batch b;
    pp_gated_batch(g, &b, nullptr);
    if (!b.n_aln) return PP_OK;
    const uint64_t base = J.added.empty() ? 0 : J.added.back().base + J.added.back().n;
    if (J.added.size() == 1) {
        // The second batch makes the job gather its batches into arrays of its own: room for all of them at once -- the two that are
        // known, scaled by the files' sizes on disk for the files still to come -- instead of arrays that grow with every file
        // (an allocation and a copy of what the files before filled, per array).
        pp_aln_batch first;
        pp_gated_batch(J.added[0].g, &first, nullptr);
        double known = 0, all = 0;
        for (int f = 0; f < J.n_sams; f++) {
            all += (double)J.sam_bytes[(size_t)f];
            if (f <= i) known += (double)J.sam_bytes[(size_t)f];
        }
        const double scale = known > 0 && all > known ? std::min(64.0, all / known * 1.02) : 1.0;
        if (int rc = pp_polish_reserve(J.ctx, (uint64_t)((double)(first.n_aln + b.n_aln) * scale) + 1024,
                                       (uint64_t)((double)(first.seq_bytes + b.seq_bytes) * scale) + 4096,
                                       (uint64_t)((double)(first.n_cig_total + b.n_cig_total) * scale) + 1024))
            return rc;
    }
    J.added.push_back(BamAdded{i, base, b.n_aln, g});
    if (J.bam_prepare) {  // the direct path (pp_batch_prepare); off by default: DESIGN.md sections 2 and 3 have what it costs and saves
        pp_prepared *p = nullptr;
        if (int rc = pp_batch_prepare(J.ctx, J.nc, J.off, &b, PP_MEM_DEVICE, &p)) return rc;
        J.prepared.push_back(p);
        pp_prepared_batch(p, &b);
    }
    return pp_polish_add(J.ctx, &b, PP_MEM_DEVICE);
}

// One BAM file: front end -> pp_batch_gate(pass = the ZP:Z:fail bytes, ANDed with the filter's verdicts where the caller brings them) ->
// pp_polish_add.  The reference streams, so when the decode or the gate refuses record N (QUIT / PANIC) the records in front of N are
// decoded, the group still pending there dropped -- the trailing run of aligned records with the last aligned record's QNAME --, the
// rest gated and polished together with the earlier files' batches (what replay_records_before_defect does for text): an error
// found on the way stands, otherwise N's.
int ingest_file_bam(PolishJob &J, int i, pp_sam_counts &c) {
    pp_ctx *const ctx = J.ctx;
    ppb::BamFile *B = nullptr;
    if (J.given) B = J.given->fronts[i];
    else {
        J.fronts.emplace_back(new ppb::BamFile);
        B = J.fronts.back().get();
        if (int rc = B->open(ctx, J.sams[i], J.kinds[(size_t)i], J.rnames, &J.lap)) return rc;
    }
    int standing = PP_OK;  // the refusal at N
    std::string standing_msg;
    auto stand = [&](int rc) { standing = rc; standing_msg = pp_last_error(ctx); };
    auto defect = [](int rc) { return rc == PP_ERR_QUIT || rc == PP_ERR_PANIC; };
    std::vector<uint16_t> flag;
    std::vector<uint64_t> rid;
    bool have_groups = false;
    auto groups = [&]() {
        if (have_groups) return (int)PP_OK;
        have_groups = true;
        return ppb::download_groups(*B, B->n_decoded, flag, rid);
    };
    uint64_t limit = B->n_rec;
    if (!B->rec) {
        uint64_t bad = 0;
        int rc = B->decode(limit, J.qnames, &bad);
        if (defect(rc)) {
            stand(rc);
            if ((rc = B->decode(bad, J.qnames, nullptr))) return rc;
            if ((rc = groups())) return rc;
            uint64_t last = bad;  // one past the last aligned record in front of N
            while (last > 0 && (flag[last - 1] & 4)) last--;
            limit = last ? last - 1 : bad;
            for (uint64_t q = limit; last && q-- > 0;) {
                if (flag[q] & 4) continue;
                if (rid[q] != rid[last - 1]) break;
                limit = q;
            }
        } else if (rc) return rc;
        if (J.lap.on) J.lap(("decoded " + B->path).c_str());
    }
    pp_raw_batch raw;
    pp_bam_raw(B->rec, &raw);
    const uint8_t *pass = nullptr;
    uint64_t n_aligned = 0;
    pp_bam_pass(B->rec, &pass, &n_aligned);
    std::vector<uint8_t> both;  // the filter's verdicts (the fused command) ANDed with the ZP:Z:fail bytes the file came with
    if (J.pass && J.n_pass[i] >= n_aligned && (standing || J.n_pass[i] == n_aligned)) {
        both.resize(n_aligned ? n_aligned : 1);
        for (uint64_t q = 0; q < n_aligned; q++) both[q] = pass[q] && J.pass[i][q];
        pass = both.data();
    } else if (J.pass) {  // verdicts for another number of records: the gate says so
        pass = J.pass[i];
        n_aligned = J.n_pass[i];
    }
    pp_gated *g = nullptr;
    for (int round = 0;; round++) {
        uint64_t n_pass = n_aligned;
        if (limit < B->n_decoded) {
            if (int rc = groups()) return rc;
            n_pass = 0;
            for (uint64_t q = 0; q < limit; q++) n_pass += !(flag[q] & 4);
        }
        raw.n_rec = limit;
        uint64_t at = 0;
        const int rc = pp_batch_gate(ctx, &raw, PP_MEM_DEVICE, J.opt->max_errors, J.opt->careful, pass, n_pass, &g, &at);
        if (rc == PP_OK) break;
        if (!defect(rc) || round > 1) return rc;
        if (int rg = groups()) return rg;
        const std::string qname = ppb::name_of(J.qnames, rid[at]);
        if (rc == PP_ERR_QUIT)
            ppb::fail(ctx, rc, "no alignments for read %s contain sequence: \"%s\" (record %llu)", qname.c_str(), J.sams[i], (unsigned long long)at + 1);
        else
            ppb::fail(ctx, rc, "aligned record of read %s has an empty CIGAR: \"%s\" (record %llu)", qname.c_str(), J.sams[i], (unsigned long long)at + 1);
        stand(rc);
        limit = at;
    }
    J.gated.push_back(g);
    pp_gated_counts(g, &c);
    B->drop_records();  // the gate's output is its own
    if (standing) {
        int rc = bam_add_gated(J, i, g);
        if (rc == PP_OK) rc = pp_polish_finish(ctx);
        if (defect(rc)) return bam_polish_error(J, rc);  // the device's message stands
        return set_err(ctx, standing, standing_msg.c_str());
    }
    if (c.alignments == 0) return ppb::fail(ctx, PP_ERR_QUIT, "no alignments in \"%s\"", J.sams[i]);
    return bam_add_gated(J, i, g);
}

// load_alignments, polish.rs:109-134.  A device tokenizer that meets a defect in the text (or bytes outside ASCII, which the
// host parsers must judge) only says so: which defect the reference reports FIRST also depends on what its CIGAR walk makes of
// the records before it, and the host ingest works that out (replay_records_before_defect): HAND_BACK, at J.handed_back_at.
int load_alignments(PolishJob &J) {
    J.log("Loading alignments\n");
    if (int rc = create_ingests(J)) return rc;
    for (int i = 0; i < J.n_sams; i++) {
        pp_sam_counts c{0, 0, 0};
        if (i == J.resume_log_at) J.log.quiet = J.opt->quiet != 0;
        const int rc = J.bam       ? ingest_file_bam(J, i, c)
                       : J.sharded ? ingest_file_sharded(J, i, c)
                       : J.dev_ingest ? ingest_file_device(J, i, c)
                                      : ingest_file_host(J, i, c);
        if (rc == HAND_BACK) J.handed_back_at = i;
        if (rc) return rc;
        J.log("%s: %s alignments from %s reads\n", J.sams[i], commas(c.alignments).c_str(), commas(c.reads).c_str());
        if (J.lap.on) { char what[64]; snprintf(what, sizeof what, "file %d ingested", i + 1); J.lap(what); }
        J.alignment_total += c.alignments;
        J.used_total += c.used;
    }
    if (int rc = J.wait_pending()) return rc;
    J.log("\nFiltering for high-quality end-to-end alignments%s:\n  %s alignments kept\n  %s alignments discarded\n\n",
          J.opt->careful ? " from reads with only one alignment" : "", commas(J.used_total).c_str(),
          commas(J.alignment_total - J.used_total).c_str());
    J.lap("alignments ingested");
    return PP_OK;
}

// create_debug_file, polish.rs:230-245: the file is created (and the header written) before polishing
int create_debug_file(PolishJob &J) {
    if (J.opt->debug_path) {
        J.dbg = fopen(J.opt->debug_path, "wb");
        if (!J.dbg) {
            snprintf(J.err, sizeof J.err, "unable to create \"%s\"", J.opt->debug_path);
            return set_err(J.ctx, PP_ERR_QUIT, J.err);
        }
        fputs("name\tpos\tbase\tdepth\tinvalid\tvalid\tpileup\tstatus\tnew_base\n", J.dbg);
    }
    J.debug_set = true;
    for (int d = 0; d < J.n_ctx; d++) pp_polish_set_debug(J.ctxs[d], J.dbg ? 1 : 0);
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

int polish_on_one_context(PolishJob &J) {
    pp_ctx *const ctx = J.ctx;
    int rc = PP_OK;
    if (!J.begun) {  // one batch (device tokenizer), or no SAM files at all
        pp_aln_batch batch{};
        if (J.dev_ingest) pp_dev_ingest_batch(J.dg, &batch); else if (J.g) pp_ingest_batch(J.g, &batch);
        rc = pp_polish_begin(ctx, J.nc, J.off, pp_assembly_bases(J.a), PP_MEM_HOST, &J.prm);
        if (rc == PP_OK && (J.dev_ingest || J.g)) rc = pp_polish_add(ctx, &batch, J.dev_ingest ? PP_MEM_DEVICE : PP_MEM_HOST);
    }
    if (rc == PP_OK) rc = pp_polish_finish(ctx);
    if (rc && J.bam) rc = bam_polish_error(J, rc);
    J.lap("uploaded + polished on device");
    if (rc == PP_OK && J.dbg) {
        rc = write_debug_tsv(ctx, J.dbg, J.names, 0, J.off[J.nc]);
        J.lap("--debug file written");
    }
    rc = close_debug_file(J, rc, false);
    if (rc == PP_OK) rc = pp_polish_result_size(ctx, &J.total);
    // offsets and statistics now; the bytes go straight into the FASTA buffer below (contig by contig) when that is a
    // handful of copies, else through one copy of everything
    J.direct_fetch = rc == PP_OK && J.out && J.nc <= 256 && J.header_bytes + J.total + J.nc <= J.fasta_cap;
    if (!J.direct_fetch) J.polished.resize(J.total ? J.total : 1);
    if (rc == PP_OK) rc = pp_polish_result(ctx, J.direct_fetch ? nullptr : J.polished.data(), PP_MEM_HOST, J.out_off.data(), J.stats.data());
    return rc;
}

// ---- the plan, from the alignment counts per contig ----
// source batches in file order: sharded -> (file, slice) pieces living on the contexts' GPUs; host ingest -> files
int collect_sources(PolishJob &J, std::vector<uint64_t> &per_contig) {
    uint64_t base = 0;
    if (!J.sharded) {
        for (pp_ingest *gi : J.gs) {
            pp_aln_batch v;
            pp_ingest_batch(gi, &v);
            J.srcs.push_back(Src{v, -1, base, 0u, {}});
            base += v.n_aln;
            pp_shard_count(nullptr, &v, PP_MEM_HOST, J.nc, per_contig.data());
        }
        return PP_OK;
    }
    std::vector<pp_aln_batch> whole((size_t)J.n_ctx);
    for (int d = 0; d < J.n_ctx; d++) pp_dev_ingest_batch(J.dgs[(size_t)d], &whole[(size_t)d]);
    for (size_t f = 0; f < J.slice_end.size(); f++)
        for (int sidx = 0; sidx < J.n_ctx; sidx++) {
            const uint64_t lo = f ? J.slice_end[f - 1][(size_t)sidx] : 0, hi = J.slice_end[f][(size_t)sidx];
            const pp_aln_batch &wb = whole[(size_t)sidx];
            pp_aln_batch v = wb;  // seq / cigar: the whole arrays (seq_off / cig_off are absolute)
            v.n_aln = hi - lo;
            v.contig += lo; v.ref_start += lo; v.k += lo; v.seq_off += lo; v.seq_len += lo; v.cig_off += lo; v.n_cig += lo;
            if (v.wo) v.wo += lo;  // (a slice's entries of the window-order mirror are its own stretch; they count from lo)
            // the slice's runs: the whole batch's, cut to [lo, hi) and counted from lo (the tokenizer ends a run with every
            // file: one run, the slice itself) -- with them a part of the slice takes the direct path like any other
            std::vector<uint64_t> runs;
            for (uint32_t r = 0; v.wo && wb.wo_run_end && r < wb.wo_n_runs; r++) {
                const uint64_t e = std::min(std::max(wb.wo_run_end[r], lo), hi) - lo;
                if (e > (runs.empty() ? 0 : runs.back())) runs.push_back(e);
            }
            if (runs.empty() || runs.back() != hi - lo) runs.clear();  // (not known: the bucketing path)
            J.srcs.push_back(Src{v, sidx, base, (uint32_t)lo, std::move(runs)});
            Src &s = J.srcs.back();
            s.view.wo_n_runs = (uint32_t)s.runs.size();
            s.view.wo_run_end = s.runs.empty() ? nullptr : s.runs.data();
            base += hi - lo;
        }
    // (one context after the other: a histogram kernel each, they add into the same host array)
    for (int d = 0; d < J.n_ctx; d++)
        if (int rc = pp_shard_count(J.ctxs[d], &whole[(size_t)d], PP_MEM_DEVICE, J.nc, per_contig.data())) {
            if (d) set_err(J.ctx, rc, pp_last_error(J.ctxs[d]));
            return rc;
        }
    return PP_OK;
}

// ---- every source batch is split once per destination (on the GPU that holds it, or on the host) ----
int plan_and_split(PolishJob &J) {
    std::vector<uint64_t> per_contig(J.nc, 0);  // alignment records per contig (the planner's weights)
    int rc = collect_sources(J, per_contig);
    if (rc == PP_OK) rc = pp_shard_plan_create(J.nc, J.off, per_contig.data(), (uint32_t)J.n_ctx, 0, &J.plan);
    const size_t nq = J.srcs.size();
    J.pieces.assign((size_t)J.n_ctx, std::vector<Piece>(nq, Piece{nullptr, 0, 0, 0}));
    for (auto &v : J.pieces)
        for (size_t q = 0; q < nq; q++) { v[q].src = J.srcs[q].owner; v[q].base = J.srcs[q].base; }
    if (rc == PP_OK && J.sharded)
        rc = on_all(J, [&](int sidx) {  // a context splits the pieces it holds, for every destination
            for (size_t q = 0; q < nq; q++)
                for (int d = 0; J.srcs[q].owner == sidx && d < J.n_ctx; d++)
                    if (int r = pp_shard_split_view_(J.ctxs[sidx], J.plan, (uint32_t)d, &J.srcs[q].view, PP_MEM_DEVICE,
                                                     J.srcs[q].wo_base, &J.pieces[(size_t)d][q].part))
                        return r;
            return (int)PP_OK;
        });
    else if (rc == PP_OK)
        rc = on_all(J, [&](int d) {
            for (size_t q = 0; q < nq; q++)
                if (int r = pp_shard_split(nullptr, J.plan, (uint32_t)d, &J.srcs[q].view, PP_MEM_HOST, &J.pieces[(size_t)d][q].part)) {
                    set_err(J.ctxs[d], r, "splitting the records failed");
                    return r;
                }
            return (int)PP_OK;
        });
    for (auto &v : J.pieces)
        for (Piece &pc : v)
            if (pc.part) {
                pp_aln_batch b;
                pp_shard_part_batch(pc.part, &b, nullptr);
                pc.n = b.n_aln;
            }
    // the tokenizers' batches (and their text buffers) are not needed once every part has been cut out of them
    for (pp_dev_ingest *&x : J.dgs) { pp_dev_ingest_free(x); x = nullptr; }
    J.lap("records split");
    return rc;
}

// ---- how the polished bytes will reach the host: one RCCL gather to the first context's GPU, or every device by itself ----
// The RCCL route is OPT-IN (PP_GATHER=rccl) in this one-process driver: it has only ever run with world = 1 -- the boxes
// this was built on have one GPU, and RCCL refuses two ranks on one device -- and a rank that fails inside
// ncclCommInitRank leaves the other threads waiting there.  The default is the route every test runs: each device
// copies its share out and the FASTA is assembled on the host.  (One process per GPU -- python -m
// polypolish_amd.distributed, bench.py --gpus N -- gathers over RCCL, behind a watchdog.)
void choose_gather_route(PolishJob &J, int rc) {
    bool use_rccl = getenv("PP_GATHER") && !strcmp(getenv("PP_GATHER"), "rccl");
    for (int d = 0; d < J.n_ctx && use_rccl && !getenv("PP_RCCL_LIB"); d++)  // (a stand-in library, tests: it takes several ranks on one device)
        for (int e = 0; e < d; e++)
            if (pp_ctx_device_(J.ctxs[d]) == pp_ctx_device_(J.ctxs[e])) use_rccl = false;  // RCCL refuses two ranks on one device
    if (use_rccl && rc == PP_OK) {
        uint8_t id[PP_COMM_ID_BYTES];
        if (pp_comm_unique_id(id) != PP_OK) use_rccl = false;  // librccl not loadable
        else {
            J.comms = true;
            if (on_all(J, [&](int d) { return pp_comm_init(J.ctxs[d], d, J.n_ctx, id); }) != PP_OK) {
                for (int d = 0; d < J.n_ctx; d++) pp_comm_destroy(J.ctxs[d]);
                J.comms = use_rccl = false;
            }
        }
    }
    J.use_rccl = use_rccl;
    if (J.lap.on)
        fprintf(stderr, "[timing] polished bytes -> host: %s\n",
                use_rccl ? "ONE RCCL gather (ncclSend/ncclRecv over xGMI) to the first GPU + one D2H"
                         : "every device copies its share out, assembled on the host (the default; PP_GATHER=rccl asks for "
                           "the RCCL gather -- not with two contexts on one device or without librccl)");
}

// one context: its records, the ranges of its units, finish, its own bytes to the host
int polish_rank(PolishJob &J, int d) {
    pp_ctx *cd = J.ctxs[d];
    RankResult &R = J.ranks[(size_t)d];
    int r = pp_polish_begin(cd, J.nc, J.off, pp_assembly_bases(J.a), PP_MEM_HOST, &J.prm);
    uint64_t tn = 0, ts = 0, tc = 0;
    for (const Piece &pc : J.pieces[(size_t)d]) {
        pp_aln_batch v;
        pp_shard_part_batch(pc.part, &v, nullptr);  // (every part exists: the split went through)
        tn += v.n_aln; ts += v.seq_bytes; tc += v.n_cig_total;
    }
    if (r == PP_OK) r = pp_polish_reserve(cd, tn + 16, ts + 64, tc + 16);
    bool first = true;
    for (const Piece &pc : J.pieces[(size_t)d]) {
        if (r) break;
        pp_aln_batch v;
        pp_shard_part_batch(pc.part, &v, nullptr);
        if (v.n_aln == 0) continue;
        // (a part on this context's own GPU is device memory; the FIRST batch of a job would be used in place,
        // which is fine -- the parts live until every context has finished)
        const int pm = pp_shard_part_mem(pc.part);
        r = pp_polish_add(cd, &v, pm == PP_MEM_HOST ? PP_MEM_HOST : (pc.src == d && !first ? PP_MEM_DEVICE : PP_MEM_PEER));
        first = false;
    }
    std::vector<uint64_t> lo(J.nc), hi(J.nc);
    if (r == PP_OK) r = pp_shard_emit_ranges(J.plan, (uint32_t)d, lo.data(), hi.data());
    if (r == PP_OK) r = pp_polish_set_emit(cd, lo.data(), hi.data());
    if (r == PP_OK) r = pp_polish_finish(cd);
    if (r == PP_OK) r = pp_polish_result_size(cd, &R.total);
    // offsets and statistics now; the bytes follow over RCCL, or (host route) with this very call
    if (r == PP_OK && !J.use_rccl) R.bytes.resize(R.total ? R.total : 1);
    if (r == PP_OK) r = pp_polish_result(cd, J.use_rccl ? nullptr : R.bytes.data(), PP_MEM_HOST, R.off.data(), R.stats.data());
    return R.rc = r;
}

// the one exchange of the job: every context's bytes to the first context's GPU, then one copy to the host
int gather_over_rccl(PolishJob &J) {
    uint64_t sum = 0;
    for (const RankResult &R : J.ranks) sum += R.total;
    J.gathered.resize(sum ? sum : 1);
    std::vector<uint64_t> lens((size_t)J.n_ctx, 0);
    const auto tg = std::chrono::steady_clock::now();
    int rc = on_all(J, [&](int d) {
        return pp_polish_gather_to_host_(J.ctxs[d], d == 0 ? J.gathered.data() : nullptr, d == 0 ? sum : 0,
                                         d == 0 ? lens.data() : nullptr, nullptr);
    });
    if (J.lap.on) fprintf(stderr, "[timing] RCCL gather of %llu bytes from %d contexts + one D2H: %.3f ms\n", (unsigned long long)sum, J.n_ctx,
                          1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - tg).count());
    for (int d = 0; rc == PP_OK && d < J.n_ctx; d++)
        if (lens[(size_t)d] != J.ranks[(size_t)d].total) rc = set_err(J.ctx, PP_ERR_HIP, "the RCCL gather delivered a rank's bytes short");
    return rc;
}

// The job's error is the one about its FIRST bad record in file order (the reference streams,
// src/alignment.rs:238-303): a context numbers the records it was sent, the parts know where those came from.
int first_error_of_job(PolishJob &J, int rc) {
    uint64_t best = ~0ull;
    int best_d = -1;
    uint32_t best_kind = 0;
    for (int d = 0; d < J.n_ctx; d++) {
        if (J.ranks[(size_t)d].rc == PP_OK) continue;
        uint32_t kind = 0;
        const uint64_t jr = job_record_of(J.ctxs[d], J.ctxs, J.pieces[(size_t)d], &kind);
        if (best_d < 0 || jr < best) { best = jr; best_d = d; best_kind = kind; }
    }
    if (best_d < 0) return rc;
    if (best != ~0ull) return pp_polish_error_text(J.ctx, best_kind, best);
    rc = J.ranks[(size_t)best_d].rc;
    if (best_d) set_err(J.ctx, rc, pp_last_error(J.ctxs[best_d]));
    return rc;
}

// every context polishes its share, side by side
int polish_on_all_contexts(PolishJob &J) {
    J.ranks.assign((size_t)J.n_ctx, RankResult{});
    for (RankResult &R : J.ranks) { R.off.assign(J.nc + 1, 0); R.stats.resize(J.nc); }
    (void)on_all(J, [&](int d) { return polish_rank(J, d); });
    bool all_ok = true;
    for (const RankResult &R : J.ranks) all_ok = all_ok && R.rc == PP_OK;
    return first_error_of_job(J, all_ok && J.use_rccl ? gather_over_rccl(J) : PP_OK);
}

// --debug: the plan's units in order (contig by contig, a tiled contig's windows in position order), each formatted by
// the context that emits it -- neighbouring units of one context in one go
int write_debug_by_units(PolishJob &J) {
    const pp_shard_plan *plan = J.plan;
    const uint64_t *off = J.off;
    int rc = PP_OK;
    for (uint32_t u = 0; rc == PP_OK && u < plan->n_units;) {
        const uint32_t r = plan->rank[u];
        const uint64_t lo = off[plan->contig[u]] + plan->lo[u];
        uint64_t hi = off[plan->contig[u]] + plan->hi[u];
        for (u++; u < plan->n_units && plan->rank[u] == r && off[plan->contig[u]] + plan->lo[u] == hi; u++) hi = off[plan->contig[u]] + plan->hi[u];
        if (r >= (uint32_t)J.n_ctx) return set_err(J.ctx, PP_ERR_HIP, "a unit of the plan names no context");
        rc = write_debug_tsv(J.ctxs[r], J.dbg, J.names, lo, hi);
        if (rc && r) set_err(J.ctx, rc, pp_last_error(J.ctxs[r]));
    }
    return rc;
}

int assemble_from_ranks(PolishJob &J) {
    std::vector<const uint8_t *> bp((size_t)J.n_ctx);
    std::vector<const uint64_t *> op((size_t)J.n_ctx);
    uint64_t at = 0;
    for (int d = 0; d < J.n_ctx; d++) {
        const RankResult &R = J.ranks[(size_t)d];
        bp[(size_t)d] = J.use_rccl ? J.gathered.data() + at : R.bytes.data();
        at += R.total;
        op[(size_t)d] = R.off.data();
    }
    int rc = pp_shard_assemble(J.plan, bp.data(), op.data(), nullptr, J.out_off.data());
    J.total = J.out_off[J.nc];
    J.polished.resize(J.total ? J.total : 1);
    if (rc == PP_OK) rc = pp_shard_assemble(J.plan, bp.data(), op.data(), J.polished.data(), J.out_off.data());
    for (uint32_t c = 0; c < J.nc; c++) {  // a position is counted by the rank that emits it
        J.stats[c] = pp_contig_stats{J.out_off[c + 1] - J.out_off[c], 0, 0, 0.0};
        for (const RankResult &R : J.ranks) {
            J.stats[c].changed += R.stats[c].changed;
            J.stats[c].zero_depth += R.stats[c].zero_depth;
            J.stats[c].depth_sum += R.stats[c].depth_sum;
        }
    }
    return rc;
}

int polish_on_several_contexts(PolishJob &J) {
    int rc = plan_and_split(J);
    choose_gather_route(J, rc);
    if (rc == PP_OK) rc = polish_on_all_contexts(J);
    J.lap("uploaded + polished on the devices");
    if (J.dbg && rc == PP_OK) rc = write_debug_by_units(J);
    rc = close_debug_file(J, rc, true);
    if (rc == PP_OK) rc = assemble_from_ranks(J);
    J.release_exchange();
    return rc;
}

// print_seq_to_stdout (polish.rs:196-203), one contig after the other in FASTA order, with print_polishing_info's lines
int write_fasta_and_log(PolishJob &J, pp_bytes *fasta) {
    const uint32_t nc = J.nc;
    const uint64_t *off = J.off, *out_off = J.out_off.data();
    if (J.out_toucher.joinable()) J.out_toucher.join();
    if (!J.out || J.header_bytes + J.total + nc > J.fasta_cap) {  // (a job whose polished bytes outgrow the bound: a buffer of the exact size)
        free(J.out);
        J.out = (uint8_t *)malloc(J.header_bytes + J.total + nc + 1);
        if (!J.out) return set_err(J.ctx, PP_ERR_HIP, "out of host memory for the FASTA");
    }
    uint8_t *out = J.out;
    const uint8_t *d_polished = J.direct_fetch ? pp_polish_result_device(J.ctx) : nullptr;
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
        // print_polishing_info, polish.rs:206-227
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
    fasta->data = out;
    fasta->len = w;
    J.out = nullptr;  // the caller's now (pp_bytes_free)
    J.lap("FASTA assembled");
    return PP_OK;
}

// finished_message, polish.rs:76-90
void log_finished(const PolishJob &J) {
    J.log("Finished!\nPolished sequence (to stdout):\n");
    for (uint32_t c = 0; c < J.nc; c++) J.log("  %s_polypolish (%s bp)\n", J.names[c], commas(J.stats[c].polished_len).c_str());
    J.log("\nTime to run: %s\n\n", format_duration(J.lap.seconds()).c_str());
}

// polish::polish (src/polish.rs:26-38) for one look at the input.  HAND_BACK: nothing was polished, the host ingest is to
// take the input, its log resuming at file J.handed_back_at.
int polish_once(PolishJob &J, pp_bytes *fasta) {
    if (int rc = check_options_and_inputs(J)) return rc;
    log_banner(J);
    J.lap("driver entered");
    if (int rc = load_assembly(J)) return rc;
    J.lap("assembly loaded");
    reserve_fasta(J);
    if (int rc = load_alignments(J)) return rc;
    // polish_sequences, polish.rs:137-154 -- on the device
    J.log("Polishing assembly sequences\n");
    if (int rc = create_debug_file(J)) return rc;
    if (int rc = J.multi ? polish_on_several_contexts(J) : polish_on_one_context(J)) return rc;
    J.lap(J.direct_fetch ? "result: offsets fetched" : "result fetched");
    if (int rc = write_fasta_and_log(J, fasta)) return rc;
    log_finished(J);
    J.release();
    J.lap("device and host buffers released");
    return PP_OK;
}

}  // namespace

// (tests) where the multi-GPU driver would cut `text` at or after `from`
extern "C" uint64_t pp_sam_group_cut_(const char *text, uint64_t size, uint64_t from) { return group_cut(text, (size_t)size, (size_t)from); }

static int polish_files_impl(pp_ctx *const *ctxs, int n_ctx, const char *assembly, const char *const *sams, int n_sams,
                             const pp_polish_options *opt, pp_bytes *fasta, const uint8_t *const *pass, const uint64_t *n_pass,
                             const BamGiven *given = nullptr) {
    if (!ctxs[0] || !assembly || !opt || !fasta || (n_sams > 0 && !sams)) return PP_ERR_ARG;
    fasta->data = nullptr;
    fasta->len = 0;
    // The second look, if the device tokenizer hands a file back: a job of its own on the host ingest, after everything of
    // the first has been released.
    for (int resume_log_at = -1;;) {
        PolishJob job{ctxs, n_ctx, assembly, sams, n_sams, opt, pass, n_pass, resume_log_at, given};
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

int ppb::polish_bam_fronts(pp_ctx *ctx, const char *assembly, pp_assembly *a, ppb::BamFile *const *fronts, pp_names *rnames, pp_names *qnames,
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
