// pp_driver.h -- the `polish` command's job, shared by pp_driver.cpp (common stages, one-context polish, entry points) and the
// input routes: pp_driver_text.cpp (SAM text on one context), pp_driver_multi.cpp (several contexts), pp_driver_bam.cpp (BAM).
// PolishJob keeps what every route needs; what one route makes lives in that route's struct, whose reset() gives it back.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <future>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "polypolish_hip.h"
#include "pp_host.h"
#include "pp_bam_files.h"

namespace ppd __attribute__((visibility("hidden"))) {

// The input route of a job: chosen once, in check_options_and_inputs, when the files' kinds are known.
// Several contexts: every GPU uploads and tokenizes its own slice of each file (SHARDED), so a byte of text crosses PCIe once; the
// host ingest (PP_DEVICE_INGEST=0, or a file the tokenizer handed back) parses once and sends every context the records that reach
// its units (MULTI_HOST).  Host ingest on one context: one ingest object per SAM file, and the batch of file i goes to the device
// (pp_polish_begin + pp_polish_add on a helper thread) while file i+1 is parsed (HOST_STREAMED) -- the reference streams its files
// one after the other as well (alignment.rs:238-265) --, or all files in one object (HOST_ONE, PP_STREAM_ADDS=0).
// TEXT_CHAIN (pp_ctx_set_text_chain): SAM text, plain or bgzipped, on the BAM route's code behind a text front (ppb::TextFile).
enum class Route { TOKENIZER, HOST_ONE, HOST_STREAMED, SHARDED, MULTI_HOST, BAM, TEXT_CHAIN };
inline bool chained(Route r) { return r == Route::BAM || r == Route::TEXT_CHAIN; }
inline bool tokenizes(Route r) { return r == Route::TOKENIZER || r == Route::SHARDED; }
inline bool several_contexts(Route r) { return r == Route::SHARDED || r == Route::MULTI_HOST; }

// what an ingest_file_* returns for a file the host ingest must look at again (not a PP_ERR_* code); the caller decides
constexpr int HAND_BACK = -1;
inline int hand_back_if_text_defect(int rc) { return rc == PP_ERR_QUIT || rc == PP_ERR_PANIC || rc == PP_ERR_NOT_ASCII ? HAND_BACK : rc; }

// A stretch of the records a context was sent, in the order it was sent them: its record `at` is record base + orig[at] of
// `source` (BAM: a file, base 0; several contexts: a source batch, base = where that one starts in the job).  `orig` is memory of
// kind `mem`, held by `holder`.  A device error names a context's record; the stretches turn it back into the source's.
struct Stretch { uint64_t n; const uint32_t *orig; int mem; pp_ctx *holder; uint64_t base; int source; };
struct Origin { const Stretch *s; uint64_t at, record; };
bool origin_of(const std::vector<Stretch> &sent, uint64_t local, Origin *o);

// SAM text on one context; the host ingest's objects per file are also what MULTI_HOST plans over
struct TextRoute {
    pp_ingest *g = nullptr;                 // host ingest, all files in one ...
    std::vector<pp_ingest *> gs;            // ... or one per file
    pp_dev_ingest *dg = nullptr;
    std::vector<std::future<int>> pending;  // the upload of the file before
    bool begun = false;                     // pp_polish_begin has run on the context
    int wait_pending();
    void reset();
    ~TextRoute() { reset(); }
};

// a part of a source batch cut out for a destination context, and the context that holds the source (-1: the host)
struct Piece { pp_shard_part *part; int src; };
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
struct MultiRoute {
    std::vector<pp_dev_ingest *> dgs;  // sharded ingest: one per context
    // sharded: the records of file i's slice on context s are records [slice_end[i-1][s], slice_end[i][s]) of its batch
    std::vector<std::vector<uint64_t>> slice_end;
    std::vector<Src> srcs;
    pp_shard_plan *plan = nullptr;
    std::vector<std::vector<Piece>> pieces;  // [context][source]: the parts (owned here from the split on) in file order
    std::vector<std::vector<Stretch>> sent;  // [context]: where its records came from
    bool use_rccl = false;                   // the gather route
    std::vector<pp_ctx *> comms;             // the contexts whose communicators exist
    std::vector<RankResult> ranks;
    std::vector<uint8_t> gathered;
    // the communicators, the plan and what the contexts brought back: not needed once the FASTA's bytes are in `polished`
    void release_exchange();
    void reset();
    ~MultiRoute() { reset(); }
};

// Files that pp_filter_polish_files has opened and decoded already, with the assembly and the tables behind them
struct BamGiven { pp_assembly *a; ppb::Front *const *fronts; pp_names *rnames, *qnames; };
// BAM input, or SAM text on the chain (all files of a command are of one kind): the record chain on the device, file by file
// (ingest_file_bam).  The gated batches (and the prepared ones, PP_BAM_PREPARE=1) live until pp_polish_finish has returned.
struct BamRoute {
    std::vector<int> kinds;  // pp_aln_file_kind(_text) of every file
    std::vector<ppb::Front *> fronts;                   // [file], as the files are opened -- or all of them, borrowed
    std::vector<std::unique_ptr<ppb::Front>> opened;    // the ones this job opened
    pp_names *rnames = nullptr, *qnames = nullptr;      // RNAME -> contig index (seeded with the assembly's names); QNAME -> read_id
    bool borrowed = false;                              // fronts and tables are the fused command's: PolishJob::borrow
    std::vector<pp_gated *> gated;                      // [file]
    std::vector<pp_regrouped *> regrouped;              // [file] with pp_ctx_set_regroup, else empty: kept for perm (view record -> file record)
    std::vector<pp_prepared *> prepared;
    std::vector<Stretch> added;  // the gated batches that went into the job
    bool prepare = getenv("PP_BAM_PREPARE") && atoi(getenv("PP_BAM_PREPARE")) != 0;
    void reset();
    ~BamRoute() { reset(); }
};

// The FASTA that will be returned (reserve_fasta): its buffer, touched by a helper thread while the alignments are loaded
struct FastaOut {
    uint8_t *buf = nullptr;
    size_t cap = 0, header_bytes = 0;
    std::thread toucher;
    void join() { if (toucher.joinable()) toucher.join(); }
    void reset() { join(); free(buf); buf = nullptr; }  // the toucher is joined before its buffer is freed
    ~FastaOut() { reset(); }
};

// Everything one `polish` command allocates, opens or starts.  release() gives all of it back and the destructor calls it: every
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
    int handed_back_at = -1;  // the file at which this look ended with HAND_BACK
    pp_ctx *ctx = ctxs[0];    // carries the error text
    Route route = Route::TOKENIZER;
    pph::Log log{opt->quiet != 0 || resume_log_at >= 0};
    pph::Lap lap{"", 36, true};  // "[timing] <stage>  <seconds since the driver was entered>  (process <seconds>)"
    pp_params prm{opt->min_depth, opt->fraction_valid, opt->fraction_invalid};
    char err[1024] = "";
    pp_assembly *a = nullptr;
    bool a_borrowed = false;
    uint32_t nc = 0;
    const uint64_t *off = nullptr;
    std::vector<const char *> names;
    std::vector<uint64_t> sam_bytes;  // the SAM files' sizes on disk (0: not a regular file)
    FastaOut fasta;
    TextRoute text;
    MultiRoute multi;
    BamRoute bam;
    FILE *dbg = nullptr;
    bool debug_set = false;  // pp_polish_set_debug was called on the contexts
    uint64_t total = 0;
    bool direct_fetch = false;
    bool form_on = false;  // pp_ctx_set_fasta_form: the FASTA is made by pp_fasta_text (write_fasta_form_and_log), at this width ...
    int64_t form_width = -1;
    int form_bgzf = 0;     // ... and compressed by pp_bgzf_deflate
    // pp_ctx_set_bed / pp_ctx_set_soft_mask (one context): the job keeps its per-position status; the BED is made and the masked bytes
    // are taken before the records are closed (polish_on_one_context), the FASTA's sequence bytes then come from `masked`
    bool bed_on = false;
    uint32_t bed_mask = 0, soft_mask = 0;
    int bed_bgzf = 0;
    pp_masked *masked = nullptr;
    std::vector<uint8_t> bed_file;  // the BED of this run (make_bed), the context's once the run has succeeded
    // pp_ctx_set_depth (one context): the job keeps its per-position depth; the track is made next to the BED (make_depth)
    bool depth_on = false;
    uint32_t depth_bin = 0;
    int depth_bgzf = 0;
    std::vector<uint8_t> depth_file;  // the depth track of this run, the context's once the run has succeeded
    // pp_ctx_set_tbi (one context): the .tbi of the bgzipped VCF | BED | depth track (PP_TBI_*), made where the track is made (make_tbi)
    bool tbi_on[3] = {false, false, false};
    std::vector<uint8_t> tbi_file[3];  // the indexes of this run, the context's once the run has succeeded
    bool wants_status() const { return bed_on || soft_mask != 0 || depth_on; }
    std::vector<uint8_t> polished = std::vector<uint8_t>(1);
    std::vector<uint64_t> out_off;
    std::vector<pp_contig_stats> stats;

    // the one place where the fused command's objects are taken: none of them is freed here
    void borrow(const BamGiven &G) {
        a = G.a;
        bam.fronts.assign(G.fronts, G.fronts + n_sams);
        bam.rnames = G.rnames;
        bam.qnames = G.qnames;
        a_borrowed = bam.borrowed = true;
    }
    // (an input that is handed back keeps its pre-faulted mappings: the host ingest of the second look takes them)
    ~PolishJob() {
        release();
        if (handed_back_at < 0) pph::prefetch_drop_all(ctx);
    }
    // In this order: uploads in flight are joined before the batches they read are freed (text.reset), the contexts stop keeping
    // per-position records, the exchange and the parts go before the ingests the parts were cut from, and the FASTA buffer's
    // toucher is joined before the buffer is freed (fasta.reset).
    void release() {
        (void)text.wait_pending();
        if (dbg) fclose(dbg);
        dbg = nullptr;
        pp_masked_free(masked);
        masked = nullptr;
        for (int d = 0; debug_set && d < n_ctx; d++) pp_polish_set_debug(ctxs[d], 0);
        debug_set = false;
        multi.reset();
        text.reset();
        bam.reset();
        if (!a_borrowed) pp_assembly_free(a);
        a = nullptr;
        fasta.reset();
    }
};

inline int set_err(pp_ctx *ctx, int code, const char *msg) { return pp_ctx_set_error_(ctx, code, msg); }
// run f(d) for every context on its own thread; the first failure (lowest d) is returned, its text put on ctxs[0]
int on_all(PolishJob &J, const std::function<int(int)> &f);
// (an assembly loaded through the device link, PP_DEVICE_FASTA=1 and one context: its bases are in that context's device memory)
inline int begin_job(PolishJob &J, pp_ctx *ctx) {
    const uint8_t *dev = J.n_ctx == 1 ? pp_assembly_bases_device(J.a) : nullptr;
    return pp_polish_begin(ctx, J.nc, J.off, dev ? dev : pp_assembly_bases(J.a), dev ? PP_MEM_DEVICE : PP_MEM_HOST, &J.prm);
}
// Room in the job for all files at once, from the batches that are known: their sizes times `scale` = what all files take on disk
// over what the known ones take, 2 % over and 64 at the most (scale_to_all_files); the caller decides when that is worth asking.
double bytes_on_disk(const PolishJob &J, int n_files);
inline double scale_to_all_files(double all, double known) { return std::min(64.0, all / known * 1.02); }
int reserve_scaled(pp_ctx *ctx, uint64_t n_aln, uint64_t seq_bytes, uint64_t n_cig_total, double scale);
// The end of a replay of the records in front of a refusal (the reference streams: they had gone through add_alignment already):
// an error the device found among them stands, otherwise the refusal.
int replayed_or_refusal(pp_ctx *ctx, int replayed, int refusal, const char *refusal_msg);
int write_debug_tsv(pp_ctx *ctx, FILE *f, const std::vector<const char *> &names, uint64_t lo, uint64_t hi);
int close_debug_file(PolishJob &J, int rc, bool say);

// a route offers: create, ingest one file, hand its batches to the polish, name a job record's origin (dispatch: pp_driver.cpp)
int tokenizer_create(PolishJob &J);
int ingest_file_device(PolishJob &J, int i, pp_sam_counts &c);
int ingest_file_host(PolishJob &J, int i, pp_sam_counts &c);
int text_hand_over(PolishJob &J);
int sharded_create(PolishJob &J);
int ingest_file_sharded(PolishJob &J, int i, pp_sam_counts &c);
int polish_on_several_contexts(PolishJob &J);
int bam_create(PolishJob &J);
int ingest_file_bam(PolishJob &J, int i, pp_sam_counts &c);
int bam_polish_error(PolishJob &J, int rc);

}  // namespace ppd
