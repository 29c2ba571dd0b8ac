// pp_driver_bam.cpp -- the polish driver's BAM route: the record chain on the device (pp_bam_files.h -> pp_batch_gate ->
// pp_polish_add), file by file, on one context; with pp_ctx_set_regroup, pp_batch_regroup stands in front of the gate.  SAM text on
// the chain (Route::TEXT_CHAIN) is the same code behind ppb::TextFile: a front says "record N" or "line N" for itself.  The fronts
// and the name tables are the job's own, or the fused command's (PolishJob::borrow), which has decoded the files for its filter
// already.
#include "pp_driver.h"

namespace ppd {

constexpr uint32_t KIND_BAD_CONTIG = 4;  // DE_BAD_CONTIG (pp_internal.h), as pp_polish_error_record reports it

void BamRoute::reset() {
    for (pp_prepared *x : prepared) pp_prepared_free(x);
    for (pp_gated *x : gated) pp_gated_free(x);
    for (pp_regrouped *x : regrouped) pp_regrouped_free(x);  // (before the fronts: an object never outlives the file it was made of)
    prepared.clear();
    gated.clear();
    regrouped.clear();
    added.clear();
    fronts.clear();
    opened.clear();
    if (!borrowed) {
        pp_names_free(qnames);
        pp_names_free(rnames);
    }
    qnames = rnames = nullptr;
}

// no ingest object: the two name tables of the record chain, and the job the gated batches are added to
int bam_create(PolishJob &J) {
    BamRoute &R = J.bam;
    int rc = PP_OK;
    if (!R.borrowed) {
        rc = pp_names_create(J.ctx, J.nc, &R.rnames);
        if (rc == PP_OK) rc = ppb::seed_names(R.rnames, J.a);
        if (rc == PP_OK) rc = pp_names_create(J.ctx, 0, &R.qnames);
    }
    if (rc == PP_OK) rc = begin_job(J, J.ctx);
    J.lap("device ready, polish job open");
    return rc;
}

// the file's own index of record `*at` of a regrouped view
static int file_record(pp_ctx *ctx, const pp_regrouped *g, uint64_t *at) {
    uint32_t p = 0;
    if (int rc = pp_ctx_download(ctx, &p, pp_regrouped_perm(g) + *at, 4)) return rc;
    *at = p;
    return PP_OK;
}

// The error pp_polish_finish left about a job record, said about the BAM record it came from: the path and the 1-based number
// counting all records of the file; a good alignment on a reference the assembly lacks in the reference's own words.
int bam_polish_error(PolishJob &J, int rc) {
    pp_ctx *const ctx = J.ctx;
    uint64_t record = 0;
    uint32_t kind = 0;
    if ((rc != PP_ERR_QUIT && rc != PP_ERR_PANIC) || !pp_polish_error_record(ctx, &record, &kind)) return rc;
    const std::string said = pp_last_error(ctx);
    Origin o;
    pp_aln_batch b;
    uint32_t contig = 0;
    if (!origin_of(J.bam.added, record, &o)) return set_err(ctx, rc, said.c_str());
    pp_gated_batch(J.bam.gated[(size_t)o.s->source], &b, nullptr);
    if (pp_ctx_download(ctx, &contig, b.contig + o.at, 4) != PP_OK) return set_err(ctx, rc, said.c_str());
    if (!J.bam.regrouped.empty() && file_record(ctx, J.bam.regrouped[(size_t)o.s->source], &o.record) != PP_OK) return set_err(ctx, rc, said.c_str());
    if (kind == KIND_BAD_CONTIG)
        return ppb::fail(ctx, rc, "query name %s in SAM but not in assembly: \"%s\" (%s)", ppb::name_of(J.bam.rnames, contig).c_str(),
                         J.sams[o.s->source], J.bam.fronts[(size_t)o.s->source]->where(o.record).c_str());
    return ppb::fail(ctx, rc, "%s: \"%s\" (%s)", said.c_str(), J.sams[o.s->source], J.bam.fronts[(size_t)o.s->source]->where(o.record).c_str());
}

static int bam_add_gated(PolishJob &J, int i, const pp_gated *g) {
    BamRoute &R = J.bam;
    pp_aln_batch b;
    const uint32_t *orig = nullptr;
    pp_gated_batch(g, &b, &orig);
    if (!b.n_aln) return PP_OK;
    if (R.added.size() == 1) {
        // The second batch makes the job gather its batches into arrays of its own: room for all of them at once -- the two that are
        // known, scaled by the files' sizes on disk for the files still to come -- instead of arrays that grow with every file
        // (an allocation and a copy of what the files before filled, per array).
        pp_aln_batch first;
        pp_gated_batch(R.gated[(size_t)R.added[0].source], &first, nullptr);
        const double known = bytes_on_disk(J, i + 1), all = bytes_on_disk(J, J.n_sams);
        const double scale = known > 0 && all > known ? scale_to_all_files(all, known) : 1.0;
        if (int rc = reserve_scaled(J.ctx, first.n_aln + b.n_aln, first.seq_bytes + b.seq_bytes, first.n_cig_total + b.n_cig_total, scale)) return rc;
    }
    R.added.push_back(Stretch{b.n_aln, orig, PP_MEM_DEVICE, J.ctx, 0, i});
    if (R.prepare) {  // the direct path (pp_batch_prepare); off by default: DESIGN.md sections 2 and 3 have what it costs and saves
        pp_prepared *p = nullptr;
        if (int rc = pp_batch_prepare(J.ctx, J.nc, J.off, &b, PP_MEM_DEVICE, &p)) return rc;
        R.prepared.push_back(p);
        pp_prepared_batch(p, &b);
    }
    return pp_polish_add(J.ctx, &b, PP_MEM_DEVICE);
}

// A text on the chain that holds a byte >= 0x80: whether its lines are valid UTF-8 is the host parsers' to say.  Plain text files
// without regrouping go on where they would go without pp_ctx_set_text_chain -- the host ingest, the log resuming at this file as
// after a tokenizer's hand-back; a bgzipped file, or regrouping, has no such route: refused, naming the path.
static int text_outside_ascii(PolishJob &J, int i, int rc) {
    bool plain = !J.bam.borrowed && !pp_ctx_regroup_(J.ctx);
    for (int k : J.bam.kinds) plain = plain && k == PP_ALN_SAM;
    if (!plain) return set_err(J.ctx, PP_ERR_QUIT, std::string(pp_last_error(J.ctx)).c_str());  // (the front's sentence names the path)
    if (J.lap.on) J.lap((std::string("text chain: bytes outside ASCII in ") + J.sams[i] + ", continuing on the host ingest").c_str());
    return HAND_BACK;
}

// One BAM file: front end -> pp_batch_gate(pass = the ZP:Z:fail bytes, ANDed with the filter's verdicts where the caller brings them) ->
// pp_polish_add.  The reference streams, so when the decode or the gate refuses record N (QUIT / PANIC) the records in front of N are
// decoded, the group still pending there dropped -- the trailing run of aligned records with the last aligned record's QNAME --, the
// rest gated and polished together with the earlier files' batches (what replay_records_before_defect does for text): an error
// found on the way stands, otherwise N's.
// With regrouping on, pp_batch_regroup stands between the decode and the gate: the gate sees the regrouped view, the verdicts go
// through pp_regrouped_pass, and "in front of N" means in front of N in the REGROUPED sequence -- the reference's streaming order on
// the file as a name-grouped one would have it.  The decode's own refusal is reported at once (no replay: what lies in front of a
// record has no cheap meaning once records move), and every record a message names goes through perm back to the file's numbering.
int ingest_file_bam(PolishJob &J, int i, pp_sam_counts &c) {
    pp_ctx *const ctx = J.ctx;
    BamRoute &R = J.bam;
    if (!R.borrowed && J.route == Route::TEXT_CHAIN) {
        ppb::TextFile *T = new ppb::TextFile;
        R.opened.emplace_back(T);
        R.fronts.push_back(T);
        if (int rc = T->open(ctx, J.sams[i], R.kinds[(size_t)i], R.rnames, &J.lap)) return rc;
    } else if (!R.borrowed) {
        ppb::BamFile *F = new ppb::BamFile;
        R.opened.emplace_back(F);
        R.fronts.push_back(F);
        if (int rc = F->open(ctx, J.sams[i], R.kinds[(size_t)i], R.rnames, &J.lap)) return rc;
    }
    ppb::Front *const B = R.fronts[(size_t)i];
    const bool regroup = pp_ctx_regroup_(ctx) != 0;
    pp_raw_batch raw{};
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
        if (!regroup) return ppb::download_groups(*B, B->n_decoded, flag, rid);
        const uint64_t n = raw.n_rec;  // the regrouped view's: what the gate numbers
        flag.assign(n ? n : 1, 0);
        rid.assign(n ? n : 1, 0);
        if (!n) return (int)PP_OK;
        if (int rc = pp_ctx_download(ctx, flag.data(), raw.flag, n * 2)) return rc;
        return pp_ctx_download(ctx, rid.data(), raw.read_id, n * 8);
    };
    uint64_t limit = ~0ull;  // in records; ~0: all that are decoded
    if (!B->decoded()) {
        uint64_t bad = 0;
        int rc = B->decode(B->all_units(), R.qnames, &bad);
        if (rc == PP_ERR_NOT_ASCII) return text_outside_ascii(J, i, rc);
        if (defect(rc) && regroup) return rc;
        if (defect(rc)) {
            stand(rc);
            if ((rc = B->decode(bad, R.qnames, nullptr)) || (rc = B->group_reads())) return rc;
            if ((rc = groups())) return rc;
            const uint64_t front = B->n_decoded;  // the records in front of N
            uint64_t last = front;                // one past the last aligned record among them
            while (last > 0 && (flag[last - 1] & 4)) last--;
            limit = last ? last - 1 : front;
            for (uint64_t q = limit; last && q-- > 0;) {
                if (flag[q] & 4) continue;
                if (rid[q] != rid[last - 1]) break;
                limit = q;
            }
        } else if (rc) return rc;
        if (J.lap.on) J.lap(("decoded " + B->path).c_str());
    }
    if (int rc = B->group_reads()) return rc;  // (behind the filter, where the fused command has run one; before anybody reads read_id here)
    B->raw(&raw);
    limit = std::min(limit, B->n_decoded);
    const uint8_t *pass = nullptr;
    uint64_t n_aligned = 0;
    B->pass(&pass, &n_aligned);
    std::vector<uint8_t> both;  // the filter's verdicts (the fused command) ANDed with the ZP:Z:fail bytes the file came with
    if (J.pass && J.n_pass[i] >= n_aligned && (standing || J.n_pass[i] == n_aligned)) {
        both.resize(n_aligned ? n_aligned : 1);
        for (uint64_t q = 0; q < n_aligned; q++) both[q] = pass[q] && J.pass[i][q];
        pass = both.data();
    } else if (J.pass) {  // verdicts for another number of records: the gate says so
        pass = J.pass[i];
        n_aligned = J.n_pass[i];
    }
    std::vector<uint8_t> carried;  // the verdicts in the regrouped numbering
    const pp_regrouped *grouped = nullptr;
    if (regroup) {
        pp_regrouped *made = nullptr;
        if (int rc = pp_batch_regroup(ctx, &raw, PP_MEM_DEVICE, &made)) return rc;
        R.regrouped.push_back(made);
        grouped = made;
        pp_regrouped_raw(grouped, &raw);
        if (pass) {
            carried.resize(n_aligned ? n_aligned : 1);
            if (int rc = pp_regrouped_pass(grouped, pass, n_aligned, carried.data())) return rc;
            pass = carried.data();
        }
        if (J.lap.on) J.lap(("regrouped " + B->path).c_str());
    }
    const uint64_t n_view = raw.n_rec;
    pp_gated *g = nullptr;
    for (int round = 0;; round++) {
        uint64_t n_pass = n_aligned;
        if (limit < n_view) {
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
        const std::string qname = ppb::name_of(R.qnames, rid[at]);
        uint64_t said_at = at;  // the file's own record
        if (grouped)
            if (int rp = file_record(ctx, grouped, &said_at)) return rp;
        if (rc == PP_ERR_QUIT)
            ppb::fail(ctx, rc, "no alignments for read %s contain sequence: \"%s\" (%s)", qname.c_str(), J.sams[i], B->where(said_at).c_str());
        else
            ppb::fail(ctx, rc, "aligned record of read %s has an empty CIGAR: \"%s\" (%s)", qname.c_str(), J.sams[i], B->where(said_at).c_str());
        stand(rc);
        limit = at;
    }
    R.gated.push_back(g);
    pp_gated_counts(g, &c);
    // the gate's output is its own.  (A regrouped view borrowed the records' seq and cigar: from here on nothing is read through it;
    // the object stays for its perm, which it owns and which the messages about the job's records need.)
    B->drop_records();
    if (standing) {
        int rc = bam_add_gated(J, i, g);
        if (rc == PP_OK) rc = pp_polish_finish(ctx);
        return replayed_or_refusal(ctx, bam_polish_error(J, rc), standing, standing_msg.c_str());
    }
    if (c.alignments == 0) return ppb::fail(ctx, PP_ERR_QUIT, "no alignments in \"%s\"", J.sams[i]);
    return bam_add_gated(J, i, g);
}

}  // namespace ppd
