// pp_bam_files.h -- the front end of the command drivers for ONE BAM file (pp_bam_files.cpp): host code over the C ABI of
// include/polypolish_hip.h only.  It joins the links of the record chain that the drivers share,
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

struct BamFile {
    pp_ctx *ctx = nullptr;
    std::string path;
    int kind = PP_ALN_SAM;              // PP_ALN_BAM or PP_ALN_BAM_RAW once open
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
    uint64_t n_decoded = 0;             // how many of the n_rec records `rec` holds (a prefix, when the file has a defect)

    BamFile() = default;
    BamFile(const BamFile &) = delete;
    BamFile &operator=(const BamFile &) = delete;
    ~BamFile() { drop_records(); }

    // Steps 1-5: map the file; inflate (BGZF) or take the bytes (raw); the header from a prefix of the inflated bytes, doubling from
    // 64 KiB; ref_map from `rnames` -- a table seeded with the assembly's names in FASTA order, asked for the header's names plus "*"
    // (NULL: identity) --; the block_size chain.  Every failure leaves its message, which names the path and the block or the record
    // (1-based), on the context and returns the library's code.  `lap` (may be NULL) times the steps.
    int open(pp_ctx *ctx, const char *path, int kind, pp_names *rnames, const pph::Lap *lap);
    // Steps 6-8: pp_bam_records over the first `limit` records, their QNAMEs through `qnames` into read_id.  A record the decode
    // refuses: the code, *bad = its index, no records.
    int decode(uint64_t limit, pp_names *qnames, uint64_t *bad);
    // the records and the bytes they borrow: when the next link's output (the gate's, the written file) is all that is needed
    void drop_records();
};

// flag / read_id of the first n decoded records, downloaded (the error paths' look at the read groups)
int download_groups(const BamFile &B, uint64_t n, std::vector<uint16_t> &flag, std::vector<uint64_t> &read_id);
// pp_aln_file_kind for a driver: a refusal goes onto the context; a path that cannot be read is left to the text route, which says
// so in its own order
int file_kind(pp_ctx *ctx, const char *path, int *kind);
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

// polish::polish over BAM files that a caller has opened and decoded already (pp_filter_polish_files decodes once): fronts[i] for
// paths[i], pass[i] the filter's own verdicts for its aligned records (the driver ANDs them with pp_bam_pass), `a` the loaded assembly, rnames / qnames
// the tables behind the fronts' contig and read_id.  Everything is borrowed; the records are dropped as the gate has taken them.
int polish_bam_fronts(pp_ctx *ctx, const char *assembly, pp_assembly *a, BamFile *const *fronts, pp_names *rnames, pp_names *qnames,
                      const char *const *paths, int n, const pp_polish_options *opt, pp_bytes *fasta, const uint8_t *const *pass,
                      const uint64_t *n_pass);

}  // namespace ppb
