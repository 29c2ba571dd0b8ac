// pp_bam_files.h -- the front ends of the command drivers for ONE alignment file (pp_bam_files.cpp): host code over the C ABI of
// include/polypolish_hip.h only.  BamFile joins the links of the record chain that the drivers share,
//   file -> pp_bgzf_inflate -> pp_bam_header -> pp_names (ref_map) -> pp_bgzf_bam_walk -> pp_bam_records -> pp_names_ids (read_id),
// and owns their objects.  pp_driver_bam.cpp takes the records on through pp_batch_gate into the polish, pp_filter_host.cpp through
// pp_filter_records into pp_bam_tagged / pp_bam_out_deflate.  From the compressed file on no alignment byte is decoded on the host.
#pragma once
#include <string>
#include <vector>

#include "polypolish_hip.h"
#include "pp_host.h"

namespace ppb {

// pp_ctx_set_error_ with a format
int fail(pp_ctx *ctx, int code, const char *fmt, ...) __attribute__((format(printf, 3, 4)));

// What the drivers' replay, regroup, gate and error code (pp_driver_bam.cpp) asks of ONE input file, whatever it holds: BamFile below
// decodes BAM records, TextFile the lines of SAM text.  A "unit" is what the decode counts and refuses: a record of a BAM file, a line
// of a text (header and empty lines included).
struct Front {
    pp_ctx *ctx = nullptr;
    std::string path;
    int kind = PP_ALN_SAM;              // pp_aln_file_kind_text's answer once open
    uint64_t n_decoded = 0;             // how many RECORDS the decoded object holds (a prefix, when the file has a defect)
    virtual ~Front() {}
    virtual uint64_t all_units() const = 0;  // a limit that takes the whole file
    // the first `limit` units decoded, contig and read_id filled in (QNAMEs through `qnames`).  A unit the decode refuses: the code,
    // the message (path and 1-based unit), *bad = its index, no records.
    virtual int decode(uint64_t limit, pp_names *qnames, uint64_t *bad) = 0;
    virtual bool decoded() const = 0;
    // read_id as the GATE wants it, once the filter (which keys its reads by name alone) is done with the records: a text applies the
    // reference's rule for the record behind an empty QNAME (pp_sam_empty_qname_rule_); BAM has no empty QNAME to apply it to
    virtual int group_reads() { return PP_OK; }
    virtual void raw(pp_raw_batch *out) const = 0;                            // the decoded records (DEVICE)
    virtual void pass(const uint8_t **zp, uint64_t *n_aligned) const = 0;     // HOST: the ZP:Z:fail bytes the file came with
    virtual std::string where(uint64_t record) const = 0;                     // "record 12" / "line 40": 1-based, as a message names it
    // the records and the bytes they borrow: when the next link's output (the gate's, the written file) is all that is needed.
    // (where() still answers behind it.)
    virtual void drop_records() = 0;
};

struct BamFile : Front {
    pph::FileText file;                 // BGZF: unmapped as soon as pp_bgzf_inflate has returned; raw BAM: the bytes themselves
    pp_bgzf *z = nullptr;               // BGZF: the inflated bytes and, behind walk, the record offsets (DEVICE)
    std::vector<uint64_t> host_off;     // raw BAM: the record offsets (HOST, as the bytes are)
    // what pp_bam_records / pp_bam_tagged take: bytes and rec_off in `mem` (borrowed from z, or from file / host_off)
    const uint8_t *bytes = nullptr;
    uint64_t n_bytes = 0;
    const uint64_t *rec_off = nullptr;
    uint64_t n_rec = 0;
    int mem = PP_MEM_DEVICE;
    uint64_t records_at = 0;            // where the header ends
    uint32_t n_ref = 0;
    std::vector<uint32_t> ref_map;      // n_ref + 1 entries; empty = identity (no assembly: `filter`)
    pp_bam *rec = nullptr;              // the decoded records; borrows `bytes` until it is freed

    BamFile() = default;
    BamFile(const BamFile &) = delete;
    BamFile &operator=(const BamFile &) = delete;
    ~BamFile() override { drop_records(); }
    uint64_t all_units() const override { return n_rec; }
    bool decoded() const override { return rec != nullptr; }
    void raw(pp_raw_batch *out) const override { pp_bam_raw(rec, out); }
    void pass(const uint8_t **zp, uint64_t *n_aligned) const override { pp_bam_pass(rec, zp, n_aligned); }
    std::string where(uint64_t record) const override { return "record " + std::to_string(record + 1); }

    // Steps 1-5: map the file; inflate (BGZF) or take the bytes (raw); the header from a prefix of the inflated bytes, doubling from
    // 64 KiB; ref_map from `rnames` -- a table seeded with the assembly's names in FASTA order, asked for the header's names plus "*"
    // (NULL: identity) --; the block_size chain.  Every failure leaves its message, which names the path and the block or the record
    // (1-based), on the context and returns the library's code.  `lap` (may be NULL) times the steps.
    int open(pp_ctx *ctx, const char *path, int kind, pp_names *rnames, const pph::Lap *lap);
    // Steps 6-8: pp_bam_records over the first `limit` records, their QNAMEs through `qnames` into read_id.  A record the decode
    // refuses: the code, *bad = its index, no records.
    int decode(uint64_t limit, pp_names *qnames, uint64_t *bad) override;
    void drop_records() override;
};

// The text front (pp_ctx_set_text_chain): one file of SAM text, plain or bgzipped, through
//   file -> (pp_bgzf_inflate) -> pp_sam_records(_lines) -> pp_names_ids twice (RNAME -> contig, QNAME -> read_id).
// The decoded object owns the only device copy of the text: the mapping (or the inflated bytes) goes when the decode has returned,
// and comes back for a replay.
struct TextFile : Front {
    pph::FileText file;                 // plain text: mapped while it is decoded
    pp_bgzf *z = nullptr;               // bgzipped text: the inflated bytes (DEVICE) while they are decoded
    pp_names *rnames = nullptr;         // RNAME -> contig (borrowed: seeded with the assembly's names, or the filter's own)
    pp_sam *rec = nullptr;              // the decoded lines
    std::vector<uint32_t> line_of;      // HOST: the 0-based line of every decoded record, kept behind drop_records for where()
    const pph::Lap *lap = nullptr;

    TextFile() = default;
    TextFile(const TextFile &) = delete;
    TextFile &operator=(const TextFile &) = delete;
    ~TextFile() override { drop_records(); }
    // the path, the kind (PP_ALN_SAM or PP_ALN_SAM_BGZF) and the RNAME table; the bytes are read by decode -- and read AGAIN by the
    // replay's decode, so a path that is no regular file (a pipe, a process substitution) is refused here, by name
    int open(pp_ctx *ctx, const char *path, int kind, pp_names *rnames, const pph::Lap *lap);
    uint64_t all_units() const override { return ~0ull; }
    int decode(uint64_t limit, pp_names *qnames, uint64_t *bad) override;
    bool decoded() const override { return rec != nullptr; }
    int group_reads() override { return rec ? pp_sam_empty_qname_rule_(rec) : (int)PP_OK; }
    void raw(pp_raw_batch *out) const override { pp_sam_raw(rec, out); }
    void pass(const uint8_t **zp, uint64_t *n_aligned) const override { pp_sam_pass(rec, zp, n_aligned); }
    std::string where(uint64_t record) const override {
        return record < line_of.size() ? "line " + std::to_string((uint64_t)line_of[(size_t)record] + 1) : std::string("line ?");
    }
    void drop_records() override;
};

// pp_bgzf_inflate of a whole mapped file for a front: a BGZF defect names the path and the 1-based block
int inflate_file(pp_ctx *ctx, const char *path, const pph::FileText &file, pp_bgzf **z);
// flag / read_id of the first n decoded records, downloaded (the error paths' look at the read groups)
int download_groups(const Front &B, uint64_t n, std::vector<uint16_t> &flag, std::vector<uint64_t> &read_id);
// pp_aln_file_kind for a driver (pp_aln_file_kind_text with pp_ctx_set_text_chain): a refusal goes onto the context; a path that
// cannot be read is left to the text route, which says so in its own order
int file_kind(pp_ctx *ctx, const char *path, int *kind);
inline bool is_text(int kind) { return kind == PP_ALN_SAM || kind == PP_ALN_SAM_BGZF; }
// the assembly's contig names into an empty table, in FASTA order: their ids are the contig indices
int seed_names(pp_names *t, const pp_assembly *a);
// the name behind an id of `t`, for a message
std::string name_of(const pp_names *t, uint64_t id);
// The commands' loader of the assembly.  PP_DEVICE_FASTA=1 in the environment and one context: pp_assembly_load_device, the bases stay
// in device memory (begin_job of pp_driver.h hands them to pp_polish_begin as PP_MEM_DEVICE); otherwise pp_assembly_load.  Off by
// default, like PP_DEVICE_FILTER and PP_BAM_PREPARE; the codes and the messages are the same either way.
inline int load_assembly_file(pp_ctx *ctx, int n_ctx, const char *path, pp_assembly **out, char *err, size_t errlen) {
    const char *e = getenv("PP_DEVICE_FASTA");
    if (e && atoi(e) != 0 && n_ctx == 1) return pp_assembly_load_device(ctx, path, out, err, errlen);
    return pp_assembly_load(path, out, err, errlen);
}

// polish::polish over files (BAM, or SAM text on the chain) that a caller has opened and decoded already (pp_filter_polish_files decodes once): fronts[i] for
// paths[i], pass[i] the filter's own verdicts for its aligned records (the driver ANDs them with pp_bam_pass), `a` the loaded assembly, rnames / qnames
// the tables behind the fronts' contig and read_id.  Everything is borrowed; the records are dropped as the gate has taken them.
int polish_bam_fronts(pp_ctx *ctx, const char *assembly, pp_assembly *a, Front *const *fronts, pp_names *rnames, pp_names *qnames,
                      const char *const *paths, int n, const pp_polish_options *opt, pp_bytes *fasta, const uint8_t *const *pass,
                      const uint64_t *n_pass);

}  // namespace ppb
