// pp_driver_multi.cpp -- the polish driver on several contexts: where a SAM file may be cut, the sharded ingest, the plan over the
// source batches and their split, the contexts polishing side by side, the gather route, the assembly of what they bring back.
#include <chrono>

#include "pp_driver.h"

namespace ppd {

void MultiRoute::release_exchange() {
    for (pp_ctx *c : comms) pp_comm_destroy(c);
    comms.clear();
    pp_shard_plan_free(plan);
    plan = nullptr;
    ranks = {};
    gathered = {};
}

void MultiRoute::reset() {
    release_exchange();
    for (auto &v : pieces)
        for (Piece &pc : v) pp_shard_part_free(pc.part);
    for (pp_dev_ingest *x : dgs) pp_dev_ingest_free(x);
    pieces.clear();
    sent.clear();
    dgs.clear();
}

// ---- several GPUs, ONE copy of the text: every GPU uploads and tokenizes a slice of each SAM file ---------------------
// Where may a file be cut?  At the start of a line that opens a read group (src/alignment.rs:255-263: an aligned record
// joins the group of the aligned record before it when that one's QNAME is empty or equal; header, empty and unaligned
// lines neither join nor close anything).  Returns the first such line start at or after `from`, or `size`.
struct LineView { const char *q; size_t qlen; bool aligned; };
static LineView look_at_line(const char *text, size_t ls, size_t le) {
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
static size_t group_cut(const char *text, size_t size, size_t from) {
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

int sharded_create(PolishJob &J) {
    J.multi.dgs.assign((size_t)J.n_ctx, nullptr);
    return on_all(J, [&](int d) { return pp_dev_ingest_create(J.ctxs[d], J.a, J.opt->max_errors, J.opt->careful, &J.multi.dgs[(size_t)d]); });
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
        return pp_dev_ingest_slice_(J.multi.dgs[s], J.sams[i], F.text + cut[s], cut[s + 1] - cut[s], &cs[s]);
    });
    for (auto &x : cs) { c.alignments += x.alignments; c.used += x.used; c.reads += x.reads; }
    if (rs == PP_OK && c.alignments == 0) rs = PP_ERR_PANIC;  // a file without aligned records: the host path has the message
    if (rs) return hand_back_if_text_defect(rs);  // as for one context
    std::vector<uint64_t> ends(n);
    for (size_t d = 0; d < n; d++) {
        pp_aln_batch bd;
        pp_dev_ingest_batch(J.multi.dgs[d], &bd);
        ends[d] = bd.n_aln;
    }
    J.multi.slice_end.push_back(ends);
    return PP_OK;
}

// ---- the plan, from the alignment counts per contig ----
// source batches in file order: sharded -> (file, slice) pieces living on the contexts' GPUs; host ingest -> files
static int collect_sources(PolishJob &J, std::vector<uint64_t> &per_contig) {
    uint64_t base = 0;
    if (J.route != Route::SHARDED) {
        for (pp_ingest *gi : J.text.gs) {
            pp_aln_batch v;
            pp_ingest_batch(gi, &v);
            J.multi.srcs.push_back(Src{v, -1, base, 0u, {}});
            base += v.n_aln;
            pp_shard_count(nullptr, &v, PP_MEM_HOST, J.nc, per_contig.data());
        }
        return PP_OK;
    }
    std::vector<pp_aln_batch> whole((size_t)J.n_ctx);
    for (int d = 0; d < J.n_ctx; d++) pp_dev_ingest_batch(J.multi.dgs[(size_t)d], &whole[(size_t)d]);
    for (size_t f = 0; f < J.multi.slice_end.size(); f++)
        for (int sidx = 0; sidx < J.n_ctx; sidx++) {
            const uint64_t lo = f ? J.multi.slice_end[f - 1][(size_t)sidx] : 0, hi = J.multi.slice_end[f][(size_t)sidx];
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
            J.multi.srcs.push_back(Src{v, sidx, base, (uint32_t)lo, std::move(runs)});
            Src &s = J.multi.srcs.back();
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
static int plan_and_split(PolishJob &J) {
    std::vector<uint64_t> per_contig(J.nc, 0);  // alignment records per contig (the planner's weights)
    int rc = collect_sources(J, per_contig);
    if (rc == PP_OK) rc = pp_shard_plan_create(J.nc, J.off, per_contig.data(), (uint32_t)J.n_ctx, 0, &J.multi.plan);
    const size_t nq = J.multi.srcs.size();
    J.multi.pieces.assign((size_t)J.n_ctx, std::vector<Piece>(nq, Piece{nullptr, 0}));
    for (auto &v : J.multi.pieces)
        for (size_t q = 0; q < nq; q++) v[q].src = J.multi.srcs[q].owner;
    if (rc == PP_OK && J.route == Route::SHARDED)
        rc = on_all(J, [&](int sidx) {  // a context splits the pieces it holds, for every destination
            for (size_t q = 0; q < nq; q++)
                for (int d = 0; J.multi.srcs[q].owner == sidx && d < J.n_ctx; d++)
                    if (int r = pp_shard_split_view_(J.ctxs[sidx], J.multi.plan, (uint32_t)d, &J.multi.srcs[q].view, PP_MEM_DEVICE,
                                                     J.multi.srcs[q].wo_base, &J.multi.pieces[(size_t)d][q].part))
                        return r;
            return (int)PP_OK;
        });
    else if (rc == PP_OK)
        rc = on_all(J, [&](int d) {
            for (size_t q = 0; q < nq; q++)
                if (int r = pp_shard_split(nullptr, J.multi.plan, (uint32_t)d, &J.multi.srcs[q].view, PP_MEM_HOST, &J.multi.pieces[(size_t)d][q].part)) {
                    set_err(J.ctxs[d], r, "splitting the records failed");
                    return r;
                }
            return (int)PP_OK;
        });
    // where every context's records will have come from (a context numbers the records it is sent)
    J.multi.sent.assign((size_t)J.n_ctx, {});
    for (int d = 0; rc == PP_OK && d < J.n_ctx; d++)
        for (size_t q = 0; q < nq; q++) {
            const Piece &pc = J.multi.pieces[(size_t)d][q];
            pp_aln_batch b;
            const uint32_t *orig = nullptr;
            pp_shard_part_batch(pc.part, &b, &orig);
            J.multi.sent[(size_t)d].push_back(Stretch{b.n_aln, orig, pp_shard_part_mem(pc.part), pc.src < 0 ? nullptr : J.ctxs[pc.src], J.multi.srcs[q].base, (int)q});
        }
    // the tokenizers' batches (and their text buffers) are not needed once every part has been cut out of them
    for (pp_dev_ingest *&x : J.multi.dgs) { pp_dev_ingest_free(x); x = nullptr; }
    J.lap("records split");
    return rc;
}

// ---- how the polished bytes will reach the host: one RCCL gather to the first context's GPU, or every device by itself ----
// The RCCL route is OPT-IN (PP_GATHER=rccl) in this one-process driver: it has only ever run with world = 1 -- the boxes
// this was built on have one GPU, and RCCL refuses two ranks on one device -- and a rank that fails inside
// ncclCommInitRank leaves the other threads waiting there.  The default is the route every test runs: each device
// copies its share out and the FASTA is assembled on the host.  (One process per GPU -- python -m
// polypolish_amd.distributed, bench.py --gpus N -- gathers over RCCL, behind a watchdog.)
static void choose_gather_route(PolishJob &J, int rc) {
    bool use_rccl = getenv("PP_GATHER") && !strcmp(getenv("PP_GATHER"), "rccl");
    for (int d = 0; d < J.n_ctx && use_rccl && !getenv("PP_RCCL_LIB"); d++)  // (a stand-in library, tests: it takes several ranks on one device)
        for (int e = 0; e < d; e++)
            if (pp_ctx_device_(J.ctxs[d]) == pp_ctx_device_(J.ctxs[e])) use_rccl = false;  // RCCL refuses two ranks on one device
    if (use_rccl && rc == PP_OK) {
        uint8_t id[PP_COMM_ID_BYTES];
        if (pp_comm_unique_id(id) != PP_OK) use_rccl = false;  // librccl not loadable
        else {
            J.multi.comms = std::vector<pp_ctx *>(J.ctxs, J.ctxs + J.n_ctx);
            if (on_all(J, [&](int d) { return pp_comm_init(J.ctxs[d], d, J.n_ctx, id); }) != PP_OK) {
                for (int d = 0; d < J.n_ctx; d++) pp_comm_destroy(J.ctxs[d]);
                J.multi.comms.clear();
                use_rccl = false;
            }
        }
    }
    J.multi.use_rccl = use_rccl;
    if (J.lap.on)
        fprintf(stderr, "[timing] polished bytes -> host: %s\n",
                use_rccl ? "ONE RCCL gather (ncclSend/ncclRecv over xGMI) to the first GPU + one D2H"
                         : "every device copies its share out, assembled on the host (the default; PP_GATHER=rccl asks for "
                           "the RCCL gather -- not with two contexts on one device or without librccl)");
}

// one context: its records, the ranges of its units, finish, its own bytes to the host
static int polish_rank(PolishJob &J, int d) {
    pp_ctx *cd = J.ctxs[d];
    RankResult &R = J.multi.ranks[(size_t)d];
    int r = begin_job(J, cd);
    uint64_t tn = 0, ts = 0, tc = 0;
    for (const Piece &pc : J.multi.pieces[(size_t)d]) {
        pp_aln_batch v;
        pp_shard_part_batch(pc.part, &v, nullptr);  // (every part exists: the split went through)
        tn += v.n_aln; ts += v.seq_bytes; tc += v.n_cig_total;
    }
    if (r == PP_OK) r = pp_polish_reserve(cd, tn + 16, ts + 64, tc + 16);
    bool first = true;
    for (const Piece &pc : J.multi.pieces[(size_t)d]) {
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
    if (r == PP_OK) r = pp_shard_emit_ranges(J.multi.plan, (uint32_t)d, lo.data(), hi.data());
    if (r == PP_OK) r = pp_polish_set_emit(cd, lo.data(), hi.data());
    if (r == PP_OK) r = pp_polish_finish(cd);
    if (r == PP_OK) r = pp_polish_result_size(cd, &R.total);
    // offsets and statistics now; the bytes follow over RCCL, or (host route) with this very call
    if (r == PP_OK && !J.multi.use_rccl) R.bytes.resize(R.total ? R.total : 1);
    if (r == PP_OK) r = pp_polish_result(cd, J.multi.use_rccl ? nullptr : R.bytes.data(), PP_MEM_HOST, R.off.data(), R.stats.data());
    return R.rc = r;
}

// the one exchange of the job: every context's bytes to the first context's GPU, then one copy to the host
static int gather_over_rccl(PolishJob &J) {
    uint64_t sum = 0;
    for (const RankResult &R : J.multi.ranks) sum += R.total;
    J.multi.gathered.resize(sum ? sum : 1);
    std::vector<uint64_t> lens((size_t)J.n_ctx, 0);
    const auto tg = std::chrono::steady_clock::now();
    int rc = on_all(J, [&](int d) {
        return pp_polish_gather_to_host_(J.ctxs[d], d == 0 ? J.multi.gathered.data() : nullptr, d == 0 ? sum : 0,
                                         d == 0 ? lens.data() : nullptr, nullptr);
    });
    if (J.lap.on) fprintf(stderr, "[timing] RCCL gather of %llu bytes from %d contexts + one D2H: %.3f ms\n", (unsigned long long)sum, J.n_ctx,
                          1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - tg).count());
    for (int d = 0; rc == PP_OK && d < J.n_ctx; d++)
        if (lens[(size_t)d] != J.multi.ranks[(size_t)d].total) rc = set_err(J.ctx, PP_ERR_HIP, "the RCCL gather delivered a rank's bytes short");
    return rc;
}

// The job's error is the one about its FIRST bad record in file order (the reference streams,
// src/alignment.rs:238-303): a context numbers the records it was sent, the parts know where those came from.
static int first_error_of_job(PolishJob &J, int rc) {
    uint64_t best = ~0ull;
    int best_d = -1;
    uint32_t best_kind = 0;
    for (int d = 0; d < J.n_ctx; d++) {
        if (J.multi.ranks[(size_t)d].rc == PP_OK) continue;
        uint32_t kind = 0;
        uint64_t local = 0, jr = ~0ull;  // the job-wide number of the record the context's error is about, or ~0 (not a record-level error)
        Origin o;
        if (pp_polish_error_record(J.ctxs[d], &local, &kind) && origin_of(J.multi.sent[(size_t)d], local, &o)) jr = o.record;
        if (best_d < 0 || jr < best) { best = jr; best_d = d; best_kind = kind; }
    }
    if (best_d < 0) return rc;
    if (best != ~0ull) return pp_polish_error_text(J.ctx, best_kind, best);
    rc = J.multi.ranks[(size_t)best_d].rc;
    if (best_d) set_err(J.ctx, rc, pp_last_error(J.ctxs[best_d]));
    return rc;
}

// every context polishes its share, side by side
static int polish_on_all_contexts(PolishJob &J) {
    J.multi.ranks.assign((size_t)J.n_ctx, RankResult{});
    for (RankResult &R : J.multi.ranks) { R.off.assign(J.nc + 1, 0); R.stats.resize(J.nc); }
    (void)on_all(J, [&](int d) { return polish_rank(J, d); });
    bool all_ok = true;
    for (const RankResult &R : J.multi.ranks) all_ok = all_ok && R.rc == PP_OK;
    return first_error_of_job(J, all_ok && J.multi.use_rccl ? gather_over_rccl(J) : PP_OK);
}

// --debug: the plan's units in order (contig by contig, a tiled contig's windows in position order), each formatted by
// the context that emits it -- neighbouring units of one context in one go
static int write_debug_by_units(PolishJob &J) {
    const pp_shard_plan *plan = J.multi.plan;
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

static int assemble_from_ranks(PolishJob &J) {
    std::vector<const uint8_t *> bp((size_t)J.n_ctx);
    std::vector<const uint64_t *> op((size_t)J.n_ctx);
    uint64_t at = 0;
    for (int d = 0; d < J.n_ctx; d++) {
        const RankResult &R = J.multi.ranks[(size_t)d];
        bp[(size_t)d] = J.multi.use_rccl ? J.multi.gathered.data() + at : R.bytes.data();
        at += R.total;
        op[(size_t)d] = R.off.data();
    }
    int rc = pp_shard_assemble(J.multi.plan, bp.data(), op.data(), nullptr, J.out_off.data());
    J.total = J.out_off[J.nc];
    J.polished.resize(J.total ? J.total : 1);
    if (rc == PP_OK) rc = pp_shard_assemble(J.multi.plan, bp.data(), op.data(), J.polished.data(), J.out_off.data());
    for (uint32_t c = 0; c < J.nc; c++) {  // a position is counted by the rank that emits it
        J.stats[c] = pp_contig_stats{J.out_off[c + 1] - J.out_off[c], 0, 0, 0.0};
        for (const RankResult &R : J.multi.ranks) {
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
    J.multi.release_exchange();
    return rc;
}

}  // namespace ppd

// (tests) where the multi-GPU driver would cut `text` at or after `from`
extern "C" uint64_t pp_sam_group_cut_(const char *text, uint64_t size, uint64_t from) { return ppd::group_cut(text, (size_t)size, (size_t)from); }
