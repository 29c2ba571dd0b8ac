/*
 * polypolish_hip.h -- C ABI of libpolypolish_hip.so, the MI355X (gfx950) implementation of
 * Polypolish's alignment-filter + per-base pileup/vote hot path.
 *
 * The reference (rrwick/Polypolish v0.6.1, Rust) has no FFI of its own; these entry points sit
 * at the two seams where its drivers call into the hot path, and take exactly what those calls
 * take, as structure-of-arrays in SAM file order (citations are file:line into the reference):
 *
 *   seam B (polish): process_one_read -> pileup.add_alignment(a, depth_contribution)
 *                    (src/alignment.rs:297-303) and polish_one_sequence -> get_polished_seq
 *                    (src/polish.rs:170-187)              => pp_polish_begin / _add / _finish
 *   seam A (filter): filter_sam -> alignment_pass_qc (src/filter.rs:334) and the sampling loop of
 *                    get_insert_size_thresholds (src/filter.rs:155-167)
 *                                                         => pp_filter_samples / pp_filter_thresholds / pp_filter_pairs
 *
 * plus the ingest either side of them (FASTA/SAM text -> the SoA above; src/misc.rs:38-167,
 * src/alignment.rs:49-128,225-322, src/filter.rs:91-145,309-349) that the `polypolish` CLI and any
 * binding share: as multi-threaded host code (pp_ingest_*, pp_filter_load / pp_filter_write) and as
 * device tokenizers over the uploaded text (pp_dev_ingest_*, pp_filter_load_device), and the whole
 * commands (pp_polish_files, pp_filter_files, pp_filter_polish_files).  A caller who holds alignment
 * RECORDS, not SAM text, has the record chain, every link on the device: pp_bam_records (uncompressed
 * BAM bytes -> raw records, the chain's front end) -> pp_names -> pp_filter_records -> (pp_batch_regroup, for
 * a file whose reads do not stand together ->) pp_batch_gate -> pp_batch_prepare -> pp_polish_*.  pp_sam_records
 * is the chain's second front end: SAM text -> the same raw records, for a caller who wants a link of the chain
 * (or a step of their own) between the text and the gate.  The chain writes the filter's verdicts back in
 * either form: pp_bam_tagged as a BAM file, pp_sam_tagged as SAM text; pp_bgzf_deflate compresses both.
 *
 * Conventions: plain pointers and sizes, no C++/torch types.  Every function returns PP_OK or a
 * PP_ERR_* code and never exits the process; pp_last_error() holds the message the reference
 * would have printed after "Error: ".  A pp_ctx is bound to one HIP device and one stream and is
 * not thread-safe; distinct contexts are independent.  There is no CPU fallback: without a
 * usable gfx950 device pp_ctx_create fails with PP_ERR_HIP.
 */
#ifndef POLYPOLISH_HIP_H
#define POLYPOLISH_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------------------------- */
#define PP_OK 0
#define PP_ERR_QUIT 1    /* the reference would quit_with_error (src/misc.rs:29-33): exit code 1 */
#define PP_ERR_HIP 3     /* HIP runtime failure, or no usable device                             */
#define PP_ERR_ARG 4     /* the caller broke this header's contract                               */
#define PP_ERR_LIMIT 5   /* input exceeds a documented implementation limit                       */
#define PP_ERR_NOT_ASCII 6 /* device text front ends (pp_dev_ingest_sam*, pp_filter_load_device) only: the file holds
                              bytes outside ASCII.  Whether all of its lines are valid UTF-8 -- the reference refuses
                              the others (BufRead::lines) -- is decided by the host parsers: load it with those.  The
                              file drivers (pp_polish_files, pp_filter_files, ...) do that by themselves           */
#define PP_ERR_PANIC 101 /* the reference would panic (unwrap / index out of bounds): exit 101    */

#define PP_MEM_HOST 0   /* pointer is host memory: the library copies it to the device             */
#define PP_MEM_DEVICE 1 /* pointer is device memory on the context's device: borrowed, not copied  */
#define PP_MEM_PEER 2   /* pp_polish_add only: device memory of ANOTHER GPU of this process (a pp_shard_part made on that
                           GPU's context): copied over the fabric, the source may be released when the call returns   */

/* CIGAR runs are packed (length << 4) | op with these op codes (SAM order). */
enum { PP_OP_M = 0, PP_OP_I = 1, PP_OP_D = 2, PP_OP_N = 3, PP_OP_S = 4, PP_OP_H = 5, PP_OP_P = 6,
       PP_OP_EQ = 7, PP_OP_X = 8 };
/* Filter input only: a run with this op code marks an alignment whose CIGAR holds a length that does not fit 64 bits.
   The reference parses run lengths when it needs an alignment's end (get_ref_end, src/alignment.rs:138-149, called from
   get_insert_size / get_orientation, src/filter.rs:189-218) and panics there, so such an alignment is only fatal if it
   takes part in a pair comparison: its ref_end is PP_REF_END_UNPARSEABLE and pp_filter_samples / pp_filter_pairs
   return PP_ERR_PANIC if they have to evaluate it (a precomputed ref_end array uses the same value). */
#define PP_OP_UNPARSEABLE 15
#define PP_REF_END_UNPARSEABLE 0xFFFFFFFFFFFFFFFFull

/* BaseStatus (src/pileup.rs:18-25) in the order of its debug strings (src/pileup.rs:156-163). */
enum { PP_ST_KEPT = 0, PP_ST_CHANGED = 1, PP_ST_LOW_DEPTH = 2, PP_ST_NONE = 3, PP_ST_MULTIPLE = 4,
       PP_ST_TOO_CLOSE = 5 };

typedef struct pp_ctx pp_ctx;

/* ---- context ------------------------------------------------------------------------------ */
int pp_device_count(void);             /* usable HIP devices (0 if there is none); initialises the HIP runtime */
int pp_ctx_create(int device, pp_ctx **out);
/* Same, but the HIP runtime / device initialisation (a few 100 ms in a fresh process) runs on a helper
 * thread so that host-side work (pp_assembly_load, pp_ingest_sam, the host half of pp_polish_files /
 * pp_filter_files) overlaps it.  Every entry point that needs the device waits for it first;
 * pp_ctx_wait() waits explicitly and returns PP_OK or PP_ERR_HIP / PP_ERR_ARG (no usable device). */
int pp_ctx_create_async(int device, pp_ctx **out);
int pp_ctx_wait(pp_ctx *ctx);
void pp_ctx_destroy(pp_ctx *ctx);
const char *pp_last_error(const pp_ctx *ctx);
int pp_ctx_sync(pp_ctx *ctx);          /* hipStreamSynchronize on the context's stream          */
void *pp_ctx_stream(pp_ctx *ctx);      /* the hipStream_t every kernel of this context runs on  */
/* device -> host copy on the context's stream, synchronous (for bindings that have no HIP of their own) */
int pp_ctx_download(pp_ctx *ctx, void *host_dst, const void *dev_src, uint64_t bytes);
const char *pp_version(void);          /* "polypolish-mi355x <ver> (parity target v0.6.1)"       */

/* Three strings of the run log that the reference pins with unit tests, exported so that those vectors can be
 * checked against the product's own text: PP_TEXT_QSCORE (qscore, src/polish.rs:290-300; value = identity in %),
 * PP_TEXT_DURATION (format_duration, src/misc.rs:195-201; value = microseconds), PP_TEXT_PERCENTILE_NAME
 * (get_percentile_name, src/filter.rs:262-270).  PP_OK and a NUL-terminated string in out, or PP_ERR_ARG (unknown `what`, text does not fit). */
enum { PP_TEXT_QSCORE = 0, PP_TEXT_DURATION = 1, PP_TEXT_PERCENTILE_NAME = 2 };
int pp_log_text(int what, double value, char *out, size_t cap);

/* ---- seam B: pileup accumulate + per-position vote ------------------------------------------ */
typedef struct {
    uint32_t min_depth;      /* -d, src/main.rs:97-99   */
    double fraction_valid;   /* -v, src/main.rs:89-91   */
    double fraction_invalid; /* -i, src/main.rs:85-87   */
} pp_params;

/* One batch of GOOD alignments (the gates of process_one_read, src/alignment.rs:282-287, already
 * applied; SEQ "*" already filled, src/alignment.rs:290-295), in global SAM order: array index i
 * is the order in which the reference would call add_alignment.  Contract per record:
 *   contig     index into the assembly's contigs (FASTA order)
 *   ref_start  0-based leftmost reference position (POS-1; src/alignment.rs:58-61)
 *   k          number of good alignments of the read (depth contribution is 1.0/k, :288), >= 1
 *   seq        SEQ bytes after to_ascii_uppercase (src/alignment.rs:94), seq_len[i] of them at
 *              seq + seq_off[i]
 *   cigar      n_cig[i] packed runs at cigar + cig_off[i]; every run length >= 1; first and last
 *              run M or '=' (starts_and_ends_with_match, src/alignment.rs:155-159)
 * The device validates all of it (runs other than M,=,X,I,D; CIGAR/SEQ length mismatch; reads
 * running past the contig end) and reports the FIRST offending record in file order, as the
 * reference would. */
typedef struct {
    uint64_t n_aln;
    const uint32_t *contig;
    const uint32_t *ref_start;
    const uint32_t *k;
    const uint64_t *seq_off;
    const uint32_t *seq_len;
    const uint64_t *cig_off;
    const uint32_t *n_cig;
    const uint8_t *seq;
    uint64_t seq_bytes;
    const uint32_t *cigar;
    uint64_t n_cig_total;
    /* Optional (NULL = none): a 4-bit mirror of seq, two bases per byte -- base seq[i] in bits 4*(i&1).. of seq4[i >> 1]
     * (the mirror is a function of the whole seq ARRAY, position by position, not of the records), (seq_bytes + 1) / 2
     * bytes followed by at least 32 readable bytes; codes PP_SEQ4_*.  With it the pileup kernel fetches the reads without
     * indels at half the bytes, one lane per read.  The library's own producers bring one (pp_dev_ingest_batch,
     * device parts of pp_shard_split); pp_polish_add copies it along, and packs one on the device for a batch that comes
     * without (host batches: the host ingest's, anybody's) whenever the batch is copied into the library's arrays anyway --
     * only a foreign PP_MEM_DEVICE batch that is polished in place (the only batch of its job) runs without.  Every result
     * is the same with and without it.  seq must be there all the same: everything that needs a byte as it was delivered
     * (string-keyed tallies, trims through bytes other than A/C/G/T/N/-) reads seq. */
    const uint8_t *seq4;
    /* Optional (NULL = none): the records once more, in WINDOW ORDER -- n_aln entries of 32 bytes, a permutation of the batch's
     * records in which the records that start in one 2048-position window of the assembly are adjacent (per SAM file, as the
     * SEQ bytes of PP_SEQ_WINDOW_GROUPED; inside a window in any order).  Like seq4 it is a mirror, a function of the arrays
     * above, and a hint: every result is the same with and without it.  The polish reads the records through it when it
     * is there: a workgroup's records then fall into a handful of windows and its work items are written next to each
     * other, where the file order scatters them over the whole assembly (the bucketing kernels take 0.15 instead of 0.25 ms
     * on the 5 Mbp / 200x job).  The library's ingests bring one; pp_polish_add carries it along while every batch of the
     * job has one.
     * The hint is ENFORCED (round 6): a mirror that is not one of the library's own (pp_ingest_batch, pp_dev_ingest_batch, the
     * parts of pp_shard_split, or a part of one of those) is compared with the arrays on the device before anything reads the
     * records through it -- every entry a record of the batch, none twice, contig / ref_start / k / seq_off / seq_len / first
     * run the record's -- and one that does not stand the comparison is left aside: the job runs without it and gives the
     * same bytes.  The comparison is a scattered read of the arrays (about 1 ms per 6.7 M records): a caller who has no cheap
     * mirror of its own hands the batch to pp_batch_prepare (below) instead, whose result is one of the library's own. */
    const struct pp_wo_rec *wo;
    /* Optional with wo (0 / NULL = not known): the mirror as RUNS.  wo_n_runs stretches of entries, one behind the other
     * (one per SAM file, as the library's ingests write it), each of them window-grouped IN ASCENDING WINDOW ORDER;
     * wo_run_end[r] = the index one past the last entry of run r (ascending; the last one = n_aln).  HOST memory whatever
     * the batch's `mem` (a handful of numbers; copied by pp_polish_add).  With it -- a sharded job (pp_polish_set_emit)
     * included: pp_shard_split restricts the table along with the mirror -- the pileup kernel takes the records that are one short M run inside their contig STRAIGHT from
     * the mirror, window by window (round 5: no bucketing pass, no work items for them); one streaming pass over the
     * mirror validates every record as before, finds where each window's entries start in every run and cuts work items
     * only for the others (indels, long reads) and for the reads that reach into the next window.  A hint like the
     * mirror itself: where the entries turn out not to be in that order (any permutation is still a valid mirror) the
     * job silently takes the bucketing path; every result is the same. */
    uint32_t wo_n_runs;
    const uint64_t *wo_run_end;
} pp_aln_batch;
#define PP_WO_MAX_RUNS 16  /* more runs than this: the bucketing path */
/* one record of pp_aln_batch.wo: the fields the bucketing reads, file_idx = the record's index in the batch's arrays (its
 * place in file order), op0 = its only CIGAR run (packed as in `cigar`) or PP_WO_MULTI_RUN for a record of several runs
 * (those are read from n_cig / cig_off / cigar by file_idx) */
typedef struct pp_wo_rec {
    uint32_t contig, ref_start, k, seq_len;
    uint64_t seq_off;
    uint32_t op0, file_idx;
} pp_wo_rec;
#define PP_WO_MULTI_RUN 0xFFFFFFFFu
/* The library's own producers of batches (pp_ingest_*, pp_dev_ingest_*, pp_shard_split) start every record's SEQ on a multiple
 * of PP_SEQ_ALIGN bytes of the seq array, the bytes in between zero, and lay the SEQ bytes of a SAM file out WINDOW-GROUPED
 * (PP_SEQ_WINDOW_GROUPED below: the default since round 4): the pileup kernel waits for the 128-byte lines a read touches,
 * and fetches a window's reads from one stretch of memory.  A batch from elsewhere may place its SEQ bytes anywhere (seq_off). */
#define PP_SEQ_ALIGN 32
/* codes of seq4: the four bases as their counter rows, N, '-' (the deletion key, src/pileup.rs:194-197), anything else */
#define PP_SEQ4_A 0
#define PP_SEQ4_C 1
#define PP_SEQ4_T 2
#define PP_SEQ4_G 3
#define PP_SEQ4_N 4
#define PP_SEQ4_DASH 5
#define PP_SEQ4_OTHER 15

/* ANY valid batch laid out as the library's ingests lay theirs out, on the device: the way to the direct path
 * (pp_polish_took_direct_path) for a caller who holds alignments but no SAM text -- a binding that parses SAM or BAM itself,
 * anything that edits or filters records.  The result is a batch of the library's own (pp_prepared_batch: DEVICE memory of the
 * context's device, owned by the object, valid until pp_prepared_free): the records in the SAME order as in `batch` (file
 * order: it fixes the f64 depth and the "first offending record"); contig / ref_start / k / seq_len / cig_off / n_cig / cigar
 * copied as they are; every record's SEQ bytes in a room of its own of (seq_len + 31) & ~31 bytes -- the rooms tile the new
 * seq array, WINDOW-GROUPED (PP_SEQ_WINDOW_GROUPED), zeros behind a read up to the boundary -- and seq_off rewritten; seq4 = the
 * 4-bit mirror of the new seq array with the slack it needs; wo = the window-order mirror as ONE run (wo_n_runs = 1, wo_run_end =
 * {n_aln}: the windows ascend over the whole batch, inside a window in any order -- the kernels order a position's alignments
 * by the file index the entries carry, so the records of several SAM files need no runs of their own).  A record whose contig
 * index is out of range goes with the last window.  pp_polish_add takes the mirror unchecked; a prepared batch that is its
 * job's only batch is polished in place, job after job.
 *   contig_off   HOST, n_contigs + 1, as for pp_polish_begin (the windows are those of this assembly)
 *   mem          PP_MEM_HOST or PP_MEM_DEVICE (where `batch` lives); its seq4 / wo / wo_run_end are ignored: the result is a
 *                function of the nine arrays alone.  The source may be released when the call returns (the context's stream
 *                has been synchronised).
 * Nothing is validated that the polish reports later; the call is memory-safe for any contents of the arrays: a record whose
 * [seq_off, seq_off + seq_len) does not lie inside the source's seq array is not read, gets no bytes and keeps a seq_off outside
 * the prepared array, so pp_polish_finish names the same record with the same message as on `batch` itself.
 * PP_ERR_ARG: null arguments, n_contigs == 0, descending contig_off, PP_MEM_PEER, a null array in a non-empty batch;
 * PP_ERR_LIMIT: the limits of pp_polish_begin / pp_polish_add (assembly < 2^32-4096 bp, < 2^32-1 records, < 2^40 SEQ bytes --
 * of rooms, too) and 2^24 records that start in one window.  An empty batch prepares to an empty batch. */
typedef struct pp_prepared pp_prepared;
int pp_batch_prepare(pp_ctx *ctx, uint32_t n_contigs, const uint64_t *contig_off, const pp_aln_batch *batch, int mem,
                     pp_prepared **out);
void pp_prepared_batch(const pp_prepared *p, pp_aln_batch *out); /* borrowed view, DEVICE memory */
/* HIP-event time of the prepare's kernels (placement + copy; not the upload of a host batch); PP_ERR_ARG unless the context
 * had profiling on (pp_ctx_set_profiling) when the batch was prepared */
int pp_prepared_kernel_ms(const pp_prepared *p, float *ms);
void pp_prepared_free(pp_prepared *p);

/* The step in front of it for a caller who holds RAW records: process_one_read (src/alignment.rs:275-322) over the alignment
 * records of ONE SAM file as Alignment::new leaves them, on the device -- what pp_ingest_sam / pp_dev_ingest_sam do behind the
 * SAM text.  With it the record chain filter -> gate -> prepare -> polish needs nothing but this header.
 *   flag       SAM FLAG; bit 4: the record takes part in nothing (alignment.rs:250), bit 16: the strand
 *   read_id    QNAME as a number: adjacent ALIGNED records are one read <=> equal ids (alignment.rs:255; an unaligned record
 *              between two of them does not part them)
 *   contig, ref_start   as pp_aln_batch (copied, not looked at);  nm = NM:i
 *   seq        seq_len[r] ASCII bytes, any case, at seq + seq_off[r], packed anywhere; seq_len 0 = SEQ "*" (BAM's l_seq 0)
 *   cigar      n_cig[r] packed runs at cigar + cig_off[r]: any of the nine ops, every length >= 1 */
typedef struct {
    uint64_t n_rec;
    const uint16_t *flag;
    const uint64_t *read_id;
    const uint32_t *contig, *ref_start, *nm;
    const uint64_t *seq_off;
    const uint32_t *seq_len;
    const uint64_t *cig_off;
    const uint32_t *n_cig;
    const uint8_t *seq;
    uint64_t seq_bytes;
    const uint32_t *cigar;
    uint64_t n_cig_total;
} pp_raw_batch;
/* A read group is a maximal run of adjacent aligned records with equal read_id.  With `careful` a group of more than one
 * record is left out whole, unlooked at.  Every other group needs a source -- its first record with seq_len > 0 -- or the
 * call ends with PP_ERR_QUIT ("no alignments for read record N contain sequence"), and none of its records may have
 * n_cig == 0 (PP_ERR_PANIC, as the reference).  A record is GOOD when its first and its last run are each M or '=',
 * nm <= max_errors and pass[a] != 0 (HOST memory whatever `mem`), a = its index among the ALIGNED records (the numbering of pp_filter_file and of
 * pp_ingest_sam_filtered; pass == NULL: no verdicts, n_pass is not looked at; a line that carries ZP:Z:fail is a 0 there).
 * The result holds the good records in file order: contig / ref_start / CIGAR runs as they came (the runs packed densely,
 * cig_off rewritten), k = the good records of the group, the SEQ bytes ASCII-upper-cased in a room of (seq_len + 31) & ~31
 * bytes each, rooms in record order (PP_SEQ_FILE_ORDER), zeros behind the read; a good record with seq_len == 0 takes its
 * group's source, reverse-complemented (src/misc.rs:170-182) when bit 16 of the two flags differs.  No seq4, no wo: hand the
 * batch to pp_polish_add, or to pp_batch_prepare (mem = PP_MEM_DEVICE) for the direct path.  orig[i] = the index of good
 * record i in `raw`.  Byte for byte the batch pp_ingest_sam makes of the equivalent text in file order.
 * Of several defects the one of the first group in file order is reported; *bad_record (may be NULL) = the index in `raw`
 * of that group's first record.  n_pass other than the number of aligned records: PP_ERR_ARG, once the records have been
 * found free of those defects.  One call per SAM file: groups never span files.
 * PP_ERR_ARG: null arguments, PP_MEM_PEER, a null array in a non-empty batch, and a record of a group that is looked at
 * whose SEQ or CIGAR range does not lie inside the arrays (found on the device before anything is read through it;
 * *bad_record = that record).  PP_ERR_LIMIT: as pp_polish_add.  A batch without aligned records gates to an empty batch
 * with counts {0, 0, 0}: "no alignments in file" is the caller's sentence.  A contig index out of range travels on and is
 * reported by pp_polish_finish.  The context's stream has been synchronised when the call returns: `raw` may be released. */
typedef struct {
    uint64_t alignments; /* aligned records seen            (src/alignment.rs:252) */
    uint64_t used;       /* good alignments kept            (src/alignment.rs:304) */
    uint64_t reads;      /* read groups                     (src/alignment.rs:260,266) */
} pp_sam_counts;  /* (what the ingests further down count, too) */
typedef struct pp_gated pp_gated;
int pp_batch_gate(pp_ctx *ctx, const pp_raw_batch *raw, int mem, uint32_t max_errors, int careful, const uint8_t *pass,
                  uint64_t n_pass, pp_gated **out, uint64_t *bad_record);
void pp_gated_batch(const pp_gated *g, pp_aln_batch *out, const uint32_t **orig); /* borrowed views, DEVICE memory */
void pp_gated_counts(const pp_gated *g, pp_sam_counts *out); /* as add_to_pileup counts them (src/alignment.rs:252-266,304) */
/* HIP-event time of the gate's kernels (not the upload of a host batch); PP_ERR_ARG unless the context had profiling on */
int pp_gated_kernel_ms(const pp_gated *g, float *ms);
void pp_gated_free(pp_gated *g);

/* The step in front of the gate for a file whose reads do NOT stand together: a coordinate-sorted file (samtools sort) scatters a
 * read's records, and the gate, like the reference, takes every run of adjacent aligned records with one read_id for a read of its
 * own.  pp_batch_regroup brings the records of ONE file (one call per file, like the gate) together again, on the device:
 *   order      output record j is raw record perm[j].  perm is the stable order of the records by the index of the first record
 *              that carries the same read_id: groups stand in the order of their first record, inside a group the records keep
 *              file order.  All records count, aligned or not: `flag` plays no part in the order.  Equality is equality of the
 *              64-bit ids, no value is reserved.  A name-grouped file regroups to itself (n_moved, the number of j with
 *              perm[j] != j, is 0), and regrouping is idempotent.  The order depends on the records alone.
 *   the view   pp_regrouped_raw: the nine per-record arrays (flag, read_id, contig, ref_start, nm, seq_off, seq_len, cig_off,
 *              n_cig) gathered through perm; seq and cigar are not moved (seq_off and cig_off are indirections already, and the
 *              gate copies what it keeps).  PP_MEM_DEVICE: seq and cigar stay BORROWED from `raw`, which must outlive the
 *              object; with n_moved == 0 the view is raw's own arrays and nothing is copied.  PP_MEM_HOST: everything is
 *              uploaded and owned by the object.  What pp_batch_gate(..., PP_MEM_DEVICE, ...) makes of the view is, byte for
 *              byte, what it makes of the same records laid out in that order by the caller; its orig[] and *bad_record are
 *              indices into the VIEW: perm turns them back into raw's.
 *   verdicts   pp_regrouped_pass carries a pass array (HOST, one byte per ALIGNED record of `raw`: the numbering of
 *              pp_filter_records and pp_bam_pass) into the numbering of the regrouped batch: out[a'] = pass[a], where the
 *              regrouped record with aligned rank a' is the raw record with aligned rank a (out may be pass only when
 *              n_moved == 0).  n_pass other than the number of aligned records: PP_ERR_ARG.
 *   counts     n_groups = the distinct read_ids.
 * PP_ERR_ARG: null arguments, PP_MEM_PEER, a null per-record array in a non-empty batch (PP_MEM_HOST: seq / cigar, too).
 * PP_ERR_LIMIT: n_rec >= 2^32-1.  Nothing in the records can be refused: offsets and lengths are copied, never followed, so the
 * call is memory-safe for any contents.  n_rec == 0 gives an empty object.  The context's stream has been synchronised when the
 * call returns.  pp_regrouped_kernel_ms: as pp_gated_kernel_ms.  The object belongs to its context and is freed before it. */
typedef struct pp_regrouped pp_regrouped;
int pp_batch_regroup(pp_ctx *ctx, const pp_raw_batch *raw, int mem, pp_regrouped **out);
void pp_regrouped_raw(const pp_regrouped *g, pp_raw_batch *out); /* borrowed view, DEVICE memory */
const uint32_t *pp_regrouped_perm(const pp_regrouped *g); /* DEVICE, n_rec entries */
void pp_regrouped_counts(const pp_regrouped *g, uint64_t *n_groups, uint64_t *n_moved);
int pp_regrouped_pass(const pp_regrouped *g, const uint8_t *pass, uint64_t n_pass, uint8_t *out); /* HOST arrays */
int pp_regrouped_kernel_ms(const pp_regrouped *g, float *ms);
void pp_regrouped_free(pp_regrouped *g);

/* The step in front of the record chain for a caller who holds NAMES: pp_raw_batch.read_id is the QNAME and .contig the RNAME as
 * a number, equal names <=> equal ids, exactly (a hash value is no id: two names that collide would be one read).  A pp_names is
 * a set of byte strings with dense ids that lives on the device (the reference's HashMap<String, ..>), so that no host hash map
 * is needed: one table seeded with the assembly's contig names gives `contig`, one table shared by both SAM files `read_id`.
 *   pp_names_ids   name i = the len[i] bytes at bytes + off[i], compared as BYTES: NUL and bytes >= 0x80 are ordinary, a name of
 *                  len 0 is a name like any other; ranges may overlap or repeat.  mem = PP_MEM_HOST or PP_MEM_DEVICE holds for
 *                  bytes, off, len, id64 and id32; id64 or id32 may be NULL (not both), they carry the same values.
 *   ids            dense and deterministic: a name's id = the number of distinct names in front of its first occurrence, over all
 *                  calls on the object in call order and, inside a call, in index order.  So a first call with the contig names
 *                  in FASTA order gives 0..n_contigs-1, and every RNAME met later that is not among them a DISTINCT id >=
 *                  n_contigs (what pp_filter_records asks of such records); a name that comes twice in a call has the id of its
 *                  first occurrence; file 2's QNAMEs get file 1's ids.  The ids depend neither on `expect`, nor on `mem`, nor
 *                  on how the names are cut into calls, nor on how often the table grew.
 *   ownership      the table keeps a copy of every distinct name's bytes; the context's stream has been synchronised when the
 *                  call returns: the caller's arrays may be released or overwritten.
 *   memory safety  a name's range is tested on the device before anything is read through it (without a sum that could wrap),
 *                  and no byte outside [0, n_bytes) is ever loaded, by a wide load either: a PP_MEM_DEVICE array may end where
 *                  its allocation ends.
 * PP_ERR_ARG: null arguments, PP_MEM_PEER, a null array with n > 0, a name (len > 0) whose [off, off + len) does not lie inside
 * [0, n_bytes): *bad (may be NULL) = the first such index, and the table is unchanged.  PP_ERR_LIMIT: 2^32-1 or more distinct
 * names (the table keeps the names of the call that came before that one), n >= 2^32-1 in one call.  n == 0 succeeds and changes
 * nothing.  `expect` sizes the first table (distinct names to come; a guess, 0 is fine): the table doubles when a call's names
 * that are not yet in it, each counted as new, would take it past half its slots.
 * pp_names_name copies a name to HOST memory (for messages): *len = its length; PP_ERR_ARG for an id the table does not have
 * and for cap < *len (*len is set then, too).  pp_names_kernel_ms: HIP-event time of the kernels of the last pp_names_ids (not the
 * upload of host arrays); PP_ERR_ARG unless the context had profiling on.  A table belongs to its context and is freed before it. */
typedef struct pp_names pp_names;
int pp_names_create(pp_ctx *ctx, uint64_t expect, pp_names **out);
int pp_names_ids(pp_names *t, const uint8_t *bytes, uint64_t n_bytes, const uint64_t *off, const uint32_t *len, uint64_t n, int mem,
                 uint64_t *id64, uint32_t *id32, uint64_t *bad);
uint64_t pp_names_count(const pp_names *t); /* distinct names held */
int pp_names_name(const pp_names *t, uint64_t id, uint8_t *out, uint32_t cap, uint32_t *len);
int pp_names_kernel_ms(const pp_names *t, float *ms);
void pp_names_free(pp_names *t);

/* IN FRONT of the BAM front end: the BGZF blocks of a file inflated on the device, so that a caller uploads a BAM file as it is on
 * disk and every later byte is produced and consumed in device memory.  A BGZF block is a gzip member of at most 64 KiB on either
 * side: 1f 8b 08, a FLG with FEXTRA, XLEN, extra subfields among which BC (SLEN 2) holds BSIZE = the block's size - 1, one raw DEFLATE
 * stream with no dictionary from the block in front, CRC32 and ISIZE.
 *   pp_bgzf_walk      HOST, no context: the twin of pp_bam_walk.  Follows the BSIZE chain from `from`: blk_off[b] = the block's offset,
 *                     out_off[b] = the sum of the ISIZEs in front of it, *end = the first byte not consumed.  blk_off has `cap`
 *                     entries, out_off (may be NULL) cap + 1: one more entry, the sum of all, follows the last block written.  The
 *                     walk stops cleanly at n_bytes -- and, with an array to fill, after `cap` blocks.  blk_off == NULL or cap == 0 only
 *                     counts, to the end.  Per block it checks 1f 8b 08 and FEXTRA; XLEN against the bytes; the subfields against
 *                     XLEN, walking them for BC (it need not be the first); BSIZE + 1 >= header + 8; the block against n_bytes; ISIZE
 *                     <= 65536.  The 28-byte EOF block (ISIZE 0) is an ordinary block.  Memory-safe for any bytes, no sum that could
 *                     wrap.  A block that fails: PP_ERR_ARG, *n_blk = the blocks in front of it, *end = its offset, the message in
 *                     pp_bam_last_error().
 *   pp_bgzf_inflate   inflates the blocks at blk_off[0 .. n_blk) into one dense DEVICE array, in index order; they need not be
 *                     adjacent, ordered or distinct (a region subset works).  mem = PP_MEM_HOST or PP_MEM_DEVICE holds for `bytes`
 *                     and `blk_off`; with PP_MEM_HOST and blk_off == NULL the library runs pp_bgzf_walk from offset 0 itself (n_blk
 *                     is ignored then).  The compressed device copy of host bytes is released before the call returns: the object
 *                     owns the inflated bytes only.  Everything is validated on the device before anything is read through it,
 *                     without sums that could wrap, and no byte outside [0, n_bytes) is ever loaded, by a wide load either: a
 *                     PP_MEM_DEVICE array may end where its allocation ends.  Stored, fixed and dynamic DEFLATE blocks, any number
 *                     per BGZF block; each block's produced length is checked against ISIZE and its CRC32 against the footer, on the
 *                     device.  A malformed stream ends with an error, never with a write outside the block's own room.
 *                     PP_ERR_ARG with *bad_block (may be NULL) = the first such block in index order, and no object: a blk_off or
 *                     block outside the array, a header pp_bgzf_walk would refuse; block type 3; LEN != ~NLEN; code lengths that are
 *                     over-subscribed, incomplete where zlib refuses that, overrun HLIT + HDIST, repeat a length that is not there or
 *                     leave out the end-of-block code; a code that stands for nothing, length symbol 286 / 287, distance symbol 30 /
 *                     31; a distance beyond the bytes produced so far; output longer or shorter than ISIZE; a stream that runs past
 *                     the payload; a CRC32 that is not the footer's.  Also PP_ERR_ARG: null arguments, PP_MEM_PEER, blk_off == NULL
 *                     with PP_MEM_DEVICE, a chain that pp_bgzf_walk refuses (*bad_block = the blocks in front).  PP_ERR_LIMIT: 2^32-1
 *                     or more blocks.  n_blk == 0 inflates to an empty object.  The context's stream has been synchronised when
 *                     the call returns: host inputs may be released.
 *   pp_bgzf_bytes     the inflated bytes (DEVICE, borrowed until pp_bgzf_free): what pp_bam_records(..., PP_MEM_DEVICE, ...) takes.
 *                     The BAM header is read with pp_ctx_download of a prefix plus pp_bam_header.
 *   pp_bgzf_bam_walk  the block_size chain of the inflated bytes from `from`, for a caller with no HIP of its own: the record
 *                     offsets end up in DEVICE memory owned by the object (pp_bgzf_rec_off: *n_rec entries, valid until the next
 *                     pp_bgzf_bam_walk on the object or pp_bgzf_free).  It is pp_bam_walk_device (below) over the inflated bytes: no
 *                     byte leaves device memory.  Its failure contract is pp_bam_walk's: PP_ERR_ARG, *n_rec = the records in
 *                     front, *end = the offending offset, the message in pp_bam_last_error() (and pp_last_error).
 *   pp_bgzf_kernel_ms HIP-event time of the object's stages so far: the headers, the scan and the inflate | the CRC32 | the kernels of
 *                     pp_bgzf_bam_walk; PP_ERR_ARG unless the context had profiling on at pp_bgzf_inflate.
 * The object belongs to its context and is freed before it. */
int pp_bgzf_walk(const uint8_t *bytes, uint64_t n_bytes, uint64_t from, uint64_t *blk_off, uint64_t *out_off, uint64_t cap, uint64_t *n_blk,
                 uint64_t *end); /* HOST, no context */
typedef struct pp_bgzf pp_bgzf;
int pp_bgzf_inflate(pp_ctx *ctx, const uint8_t *bytes, uint64_t n_bytes, const uint64_t *blk_off, uint64_t n_blk, int mem, pp_bgzf **out,
                    uint64_t *bad_block);
void pp_bgzf_bytes(const pp_bgzf *z, const uint8_t **dev, uint64_t *n_bytes); /* borrowed view, DEVICE memory */
int pp_bgzf_bam_walk(pp_bgzf *z, uint64_t from, uint64_t *n_rec, uint64_t *end); /* the block_size chain of the inflated bytes */
const uint64_t *pp_bgzf_rec_off(const pp_bgzf *z);                               /* DEVICE, n_rec entries */
int pp_bgzf_kernel_ms(const pp_bgzf *z, float *ms);
void pp_bgzf_free(pp_bgzf *z);

/* The FRONT END of the record chain for a caller who holds BAM: the alignment records of UNCOMPRESSED BAM bytes as a pp_raw_batch,
 * decoded on the device.  A file's BGZF blocks are inflated by pp_bgzf_inflate above, whose bytes go in here as PP_MEM_DEVICE; the
 * commands read BAM files through exactly these calls (pp_aln_file_kind below; the reference reads SAM text only).  A BAM CIGAR word is len << 4 | op with MIDNSHP=X -> 0..8, bit for bit pp_raw_batch.cigar; l_seq 0 is
 * SEQ "*"; a record's read_name is an (off, len) range into the bytes, which is what pp_names_ids(..., PP_MEM_DEVICE) takes.
 *
 * Two HOST helpers need no device.  Both are memory-safe for any bytes, never read outside [0, n_bytes) and form no sum that could
 * wrap; a failing one returns PP_ERR_ARG and leaves its message in pp_bam_last_error() (per thread; they have no context).
 *   pp_bam_header  magic BAM\1, l_text, the text, n_ref, then l_name, name, l_ref per reference: name_off[i] / name_len[i] = the
 *                  name's range in `bytes` (the length without its NUL), ref_len[i] = l_ref, *records_at = the offset of the first
 *                  alignment record.  The arrays have `cap` entries; n_ref > cap: *n_ref is set all the same, the first cap entries are
 *                  written and the call returns PP_ERR_ARG.  A truncated or inconsistent header (a length that runs past the bytes,
 *                  l_name 0, a name without its NUL): PP_ERR_ARG.
 *   pp_bam_walk    follows the block_size chain from `from`: rec_off[r] = the offset of record r's block_size word, *end = the first
 *                  byte not consumed.  The walk stops cleanly at n_bytes -- and, with an array to fill, after `cap` records (*end
 *                  is then where the next call goes on).  rec_off == NULL or cap == 0 only counts, to the end.  A block_size < 32, or
 *                  a record (its block_size word, too) that runs past n_bytes: PP_ERR_ARG, *n_rec = the records in front of it, *end
 *                  = its offset.  The chain is serial by the format, so it is walked on the host: a caller who inflates blocks meets
 *                  every block_size anyway.
 *
 * pp_bam_walk_device is the same walk ON THE DEVICE, to the end, for bytes that are (or belong) in device memory: *n_rec, *end and
 * the offsets (pp_bam_offs_dev: DEVICE, *n_rec entries, what pp_bam_records(..., PP_MEM_DEVICE, ...) takes as rec_off) are exactly
 * what pp_bam_walk yields on the same bytes from the same `from`.  The chain is serial only along the true chain: chunks of the bytes
 * are walked from every offset at once, and the chunks are chained through a small entry zone each.
 *   memory       mem = PP_MEM_HOST: the bytes are uploaded and the copy is released before the call returns; PP_MEM_DEVICE: they are
 *                borrowed for the call only.  The object owns nothing but the offsets (16 bytes for no records).  The context's
 *                stream has been synchronised when the call returns.
 *   a break      a chain that pp_bam_walk refuses: PP_ERR_ARG, no object, *n_rec = the records in front of the break, *end = the
 *                offending offset, pp_bam_last_error() = the very string pp_bam_walk leaves on these bytes (the bytes end inside a
 *                block_size, block_size < 32, a record runs past the end, the start lies behind the bytes), and pp_last_error(ctx)
 *                the same string behind "pp_bam_walk_device: ".
 *   also         PP_ERR_ARG: null arguments, PP_MEM_PEER, null bytes with n_bytes > 0.  PP_ERR_LIMIT: 2^32-1 or more records (as
 *                pp_bam_records), n_bytes >= 2^40.  from == n_bytes: no records, PP_OK.
 *   safety       every length is compared with what is left, no sum can wrap, and no byte outside [0, n_bytes) is loaded, by a wide
 *                load either: a device array may end where its allocation ends.  Bytes in front of `from` and bytes off the chain
 *                are arbitrary: they are read as data only and can neither fault nor change the result.  Every loop is bounded by
 *                n_bytes whatever the bytes hold.
 * pp_bam_offs_kernel_ms: as pp_gated_kernel_ms.  The object belongs to its context and is freed before it.
 *
 * pp_bam_records decodes the records at rec_off[0 .. n_rec) -- they need not be adjacent, ordered or distinct (a region subset
 * works); output record r is input record r.
 *   memory       mem = PP_MEM_HOST or PP_MEM_DEVICE holds for `bytes` and `rec_off`; rec_off is required with PP_MEM_DEVICE; with
 *                PP_MEM_HOST and rec_off == NULL the library runs pp_bam_walk from offset 0 itself (n_rec is ignored then).  Host
 *                bytes are uploaded and the device copy lives until pp_bam_free (the name ranges point into it); device bytes are
 *                borrowed until pp_bam_free.  ref_map is HOST memory whatever `mem`.
 *   flag         the record's flag;  ref_start = pos < 0 ? 0 : pos (the reference's POS 0, src/alignment.rs:58-61);  seq_len = l_seq
 *   contig       ref_map[refID]; ref_map has n_ref + 1 entries, entry n_ref answers refID -1 (the "*"); ref_map == NULL: identity,
 *                and 0xFFFFFFFF for -1.  A pp_names seeded with the FASTA names and asked for the header's names plus "*" yields
 *                exactly such a map, with the distinct ids per unknown name that pp_filter_records asks for.
 *   n_cig/cigar  the record's words copied as they are, packed densely in record order
 *   seq          the nibbles expanded through =ACMGRSVTWYHKDBN, high nibble first; every record in a room of (seq_len + 31) & ~31
 *                bytes, rooms in record order, zeros behind the read: seq_off is a multiple of PP_SEQ_ALIGN, l_seq 0 takes no room
 *   read_id      zero until the caller fills it (pp_bam_read_id: DEVICE, n_rec entries), e.g. pp_names_ids over pp_bam_names with
 *                PP_MEM_DEVICE and id64 = that array
 *   nm           restates Alignment::new (src/alignment.rs:65-78): it starts at 0xFFFFFFFF; every aux field with tag NM and type
 *                c C s S i I sets it, the last one wins; NM of any other type is ignored (as NM:Z: is in the text); a negative value
 *                is PP_ERR_PANIC (the reference's parse::<u32>().unwrap()); behind the walk an ALIGNED record whose nm is still
 *                0xFFFFFFFF is PP_ERR_QUIT "missing NM tag" -- a type-I value of 4294967295 included, as in the reference
 *   ZP:Z:fail    tag bytes ZP ignoring ASCII case, type exactly Z, value exactly the four bytes "fail" ignoring case (src/alignment.rs:72)
 *                clears the pass byte of that aligned record (pp_bam_pass: HOST, one byte per ALIGNED record, what pp_batch_gate
 *                takes as `pass`, to be ANDed with the filter's verdicts)
 *   aux walk     understands A c C s S i I f Z H and B with the sub-types c C s S i I f
 *   ignored      mapq, bin, the mate fields, tlen, QUAL.  LIMIT: a CG:B:I long CIGAR is not interpreted; its placeholder CIGAR starts
 *                with S, so the gate drops the record.
 * Everything is validated on the device before anything is read through it, without sums that could wrap, and no byte outside
 * [0, n_bytes) is ever loaded, by a wide load either: a PP_MEM_DEVICE array may end where its allocation ends.  PP_ERR_ARG with
 * *bad_record (may be NULL) = the first such record in index order, and no object: a rec_off or record outside the array; block_size
 * < 32 + l_read_name + 4 * n_cigar_op + (l_seq + 1) / 2 + l_seq; l_read_name == 0 or a name without its NUL; a CIGAR op above 8; a
 * refID outside [-1, n_ref) (ref_map == NULL: below -1); an aux field that is cut, of unknown type, a Z / H without NUL inside the
 * record, a B whose count runs past the record.  Only when no record has such a defect is the first QUIT / PANIC record in index order
 * reported (*bad_record = it).  The reference streams: to get ITS order against the gate's own errors, gate the records in front of
 * bad_record first.  Also PP_ERR_ARG: null arguments, PP_MEM_PEER, rec_off == NULL with PP_MEM_DEVICE, a chain that pp_bam_walk
 * refuses (*bad_record = the records in front).  PP_ERR_LIMIT as for pp_polish_add (< 2^32-1 records, < 2^40 SEQ bytes of rooms).
 * n_rec == 0 decodes to an empty batch.  The context's stream has been synchronised when the call returns: host inputs may be
 * released.  pp_bam_kernel_ms: as pp_gated_kernel_ms.  The object belongs to its context and is freed before it. */
typedef struct pp_bam pp_bam;
int pp_bam_header(const uint8_t *bytes, uint64_t n_bytes, uint32_t cap, uint32_t *n_ref, uint64_t *name_off, uint32_t *name_len,
                  uint32_t *ref_len, uint64_t *records_at);
int pp_bam_walk(const uint8_t *bytes, uint64_t n_bytes, uint64_t from, uint64_t *rec_off, uint64_t cap, uint64_t *n_rec, uint64_t *end);
const char *pp_bam_last_error(void);
typedef struct pp_bam_offs pp_bam_offs;
int pp_bam_walk_device(pp_ctx *ctx, const uint8_t *bytes, uint64_t n_bytes, uint64_t from, int mem, pp_bam_offs **out, uint64_t *n_rec,
                       uint64_t *end);
const uint64_t *pp_bam_offs_dev(const pp_bam_offs *o); /* DEVICE, n_rec entries: what pp_bam_records(..., PP_MEM_DEVICE, ...) takes */
uint64_t pp_bam_offs_count(const pp_bam_offs *o);
int pp_bam_offs_kernel_ms(const pp_bam_offs *o, float *ms);
void pp_bam_offs_free(pp_bam_offs *o);
int pp_bam_records(pp_ctx *ctx, const uint8_t *bytes, uint64_t n_bytes, const uint64_t *rec_off, uint64_t n_rec, int mem,
                   const uint32_t *ref_map, uint32_t n_ref, pp_bam **out, uint64_t *bad_record);
void pp_bam_raw(const pp_bam *b, pp_raw_batch *out); /* borrowed view, DEVICE memory; out->read_id = the array below */
uint64_t *pp_bam_read_id(pp_bam *b);                 /* DEVICE, n_rec entries: zero until the caller fills it */
void pp_bam_names(const pp_bam *b, const uint8_t **bytes_dev, uint64_t *n_bytes, const uint64_t **off, const uint32_t **len); /* DEVICE: what pp_names_ids takes */
void pp_bam_pass(const pp_bam *b, const uint8_t **zp, uint64_t *n_aligned); /* HOST: one byte per ALIGNED record, 0 = carries ZP:Z:fail */
int pp_bam_kernel_ms(const pp_bam *b, float *ms);
void pp_bam_free(pp_bam *b);

/* The SECOND front end of the record chain, for a caller who holds SAM TEXT (what `bwa mem` writes, the only format the reference
 * reads): the lines of the text as a pp_raw_batch, decoded on the device -- the text twin of pp_bam_records.  The commands use
 * it with pp_ctx_set_text_chain (their --text_chain); without it their text routes are the fused ones (pp_dev_ingest_sam,
 * pp_filter_load_device), which leave no raw records behind.
 *   records      every line that is neither empty nor begins with '@' is a record, aligned or not, in file order.  Line ends are
 *                "\n" or "\r\n"; a missing final newline is fine.  What a line is, Alignment::new decides (src/alignment.rs:49-98),
 *                exactly as the two ingests follow it.
 *   flag         the FLAG column;  ref_start = POS, less 1 when POS > 0
 *   nm           starts at 0xFFFFFFFF; every field that begins with the bytes "NM:i:" sets it (case-sensitive, parse::<u32>: a
 *                leading '+' is fine), the last one wins; still 0xFFFFFFFF behind the walk is legal on an unaligned line only
 *   n_cig/cigar  get_expanded_cigar (src/alignment.rs:325-346) kept as runs len << 4 | op, packed densely in record order: "*" gives
 *                no runs, a zero-length run vanishes, a run above 2^28-1 is cut into pieces of at most that
 *   seq          is NOT copied.  The object owns one device copy of the text; raw.seq is that copy, raw.seq_off[r] the offset of
 *                record r's SEQ column in it, raw.seq_bytes = n_bytes: no rooms, any case (the gate copies and upper-cases what it
 *                keeps).  seq_len = the column's length, 0 for "*".  The name ranges point into the same copy.  So the caller's
 *                `text` may be released when the call returns, with either `mem`; no byte outside [0, n_bytes) of the caller's array
 *                is ever loaded; no byte behind n_bytes can change a result.  With PP_MEM_DEVICE the copy is one device-to-device copy.
 *   read_id      zero until the caller fills it (pp_sam_read_id: DEVICE, n_rec entries): pp_names_ids over pp_sam_names with
 *                PP_MEM_DEVICE and id64 = that array.  A record joins the read in front of it also when THAT record's QNAME is empty
 *                (src/alignment.rs:255): a caller who interns names has to know.
 *   contig       zero until the caller fills it (pp_sam_contig: DEVICE, n_rec entries): pp_names_ids over pp_sam_rnames with id32 =
 *                that array, on a table seeded with the FASTA names (see pp_names)
 *   lines        pp_sam_lines: DEVICE, n_rec entries, the 0-based line of record r -- what a later link's bad_record (through
 *                pp_regrouped_perm where there is a regroup) turns into the file's own line
 *   ZP:Z:fail    a field of exactly nine bytes, ZP:Z:fail ignoring ASCII case as the tokenizer matches it, clears the pass byte of that
 *                aligned record (pp_sam_pass: HOST, one byte per ALIGNED record, what pp_batch_gate takes as `pass`)
 *   refusals     the first refused line in file order wins, whatever its kind; *bad_line (may be NULL) = its 0-based index among all
 *                lines; no object.  PP_ERR_QUIT (too few columns, missing NM tag on an aligned line, invalid CIGAR) and PP_ERR_PANIC
 *                (FLAG, POS, an NM:i: value, a CIGAR run that overflows u32) with the sentence pp_ingest_sam has for that line, the
 *                path "text" and the line numbered from 1: the device decides which line, the host parser then runs on that one line
 *                (downloaded when the text is device memory).  PP_ERR_LIMIT, naming the line, for a line the reference takes but a raw
 *                batch cannot hold: FLAG above 65535, POS above 2^32-1, an aligned line whose SEQ column is empty (not "*": seq_len 0
 *                would turn it into one).  PP_ERR_LIMIT also for 2^32-1 or more lines and n_bytes >= 2^40.  PP_ERR_NOT_ASCII for a byte
 *                >= 0x80 anywhere in the text, as pp_dev_ingest_sam answers it (no bad_line: which lines are valid UTF-8 is the host
 *                parsers' to say).  PP_ERR_ARG: null arguments, PP_MEM_PEER, null text with n_bytes > 0.  n_bytes == 0, or a text of
 *                header lines only, gives an empty object.
 *   order        the reference streams: to get ITS order against the gate's own errors, gate the records in front of bad_line first.
 *                `filter`'s new_quick never looks at NM; this decode does (as for the BAM route).
 * The context's stream has been synchronised when the call returns.  pp_sam_kernel_ms: as pp_gated_kernel_ms (the kernels; the copy of
 * the text is not among them).  The object belongs to its context and is freed before it. */
typedef struct pp_sam pp_sam;
int pp_sam_records(pp_ctx *ctx, const uint8_t *text, uint64_t n_bytes, int mem, pp_sam **out, uint64_t *bad_line);
/* pp_sam_records over the first n_lines lines of the text only -- the text twin of a BAM decode with a record limit: what a driver
 * replays when line N = n_lines is refused and the reference, which streams, has taken the lines in front of it already.  The whole
 * text is still copied (uploaded, for host memory) and its newlines indexed -- that finds where line n_lines starts, and it is the
 * cost of the call whatever n_lines is --; from there on the object's copy is set to zeros, so no such byte is loaded by the scan, the
 * placing or the CIGAR pass, and none of them -- a byte >= 0x80 or a malformed line included -- changes a result or a refusal.
 * Refusals speak as pp_sam_records_lines.  The object is the one pp_sam_records makes of the prefix: n_bytes and
 * raw.seq_bytes are the prefix's length.  n_lines at or beyond the text's line count: pp_sam_records.  n_lines == 0: an empty object. */
int pp_sam_records_lines(pp_ctx *ctx, const uint8_t *text, uint64_t n_bytes, int mem, uint64_t n_lines, pp_sam **out, uint64_t *bad_line);
void pp_sam_raw(const pp_sam *s, pp_raw_batch *out);      /* borrowed view, DEVICE; read_id / contig = the two arrays below */
uint64_t *pp_sam_read_id(pp_sam *s);                      /* DEVICE, n_rec entries, zero until the caller fills it */
uint32_t *pp_sam_contig(pp_sam *s);                       /* DEVICE, n_rec entries, zero until the caller fills it */
void pp_sam_names(const pp_sam *s, const uint8_t **bytes_dev, uint64_t *n_bytes, const uint64_t **off, const uint32_t **len);  /* QNAME ranges: what pp_names_ids takes, id64 = pp_sam_read_id */
void pp_sam_rnames(const pp_sam *s, const uint8_t **bytes_dev, uint64_t *n_bytes, const uint64_t **off, const uint32_t **len); /* RNAME ranges, id32 = pp_sam_contig */
const uint32_t *pp_sam_lines(const pp_sam *s);            /* DEVICE, n_rec entries: 0-based line of record r, for messages of later links */
void pp_sam_pass(const pp_sam *s, const uint8_t **zp, uint64_t *n_aligned); /* HOST, as pp_bam_pass */
/* 1 and *line (may be NULL) = the 0-based line of the first EMPTY line of the decoded text -- no bytes, or "\r" only --, 0 when it has
 * none (or s is NULL).  The decode skips such a line as polish::polish does; filter::filter quits on it (src/filter.rs:126-130), so the
 * filter drivers ask.  Taken by the scan that classifies every line: no pass of its own. */
int pp_sam_first_empty_line(const pp_sam *s, uint64_t *line);
int pp_sam_kernel_ms(const pp_sam *s, float *ms);
void pp_sam_free(pp_sam *s);

/* The WRITE side of the record chain for a caller who holds BAM: the filter's verdicts written back as a BAM file, on the device --
 * what `polypolish filter` does with SAM text (filter_sam, src/filter.rs:296-343: every line again, ZP:Z:fail appended to the aligned
 * ones that failed), for records.  The files it makes go back through pp_bgzf_inflate ... pp_bam_records into polish: the reference's
 * two-command workflow.  `filter` on BAM input writes its outputs with this call and pp_bam_out_deflate.
 *   inputs       bytes[0, n_bytes): uncompressed BAM; records_at: where its header ends (pp_bam_header); rec_off[0, n_rec): the records,
 *                as for pp_bam_records not necessarily adjacent, ordered or distinct; pass[0, n_pass): HOST memory whatever `mem`, one
 *                byte per ALIGNED record (flag & 4 == 0) in index order -- the numbering of pp_filter_records' pass1 / pass2.
 *   the stream   U' = bytes[0, records_at), then per record r in index order its 4 + block_size bytes as they are; an aligned record
 *                whose verdict is 0 has block_size + 8 in its first word and the eight bytes 5A 50 5A 66 61 69 6C 00 (ZP, type Z,
 *                "fail", NUL) behind its last byte.  An unaligned record is copied and takes no verdict (filter_sam's !a.is_aligned()
 *                branch).  A failing record that already carries ZP:Z:fail gets a second one: the reference pushes the field without
 *                looking.  `pass` is the FILTER'S OWN verdict, NOT ANDed with pp_bam_pass: a record that came with the tag and passes
 *                keeps its one tag, exactly as its SAM line would.
 *   the file     U' cut every 65,280 bytes (0xff00, htslib's payload size; the last piece is shorter, an empty U' has none), each piece
 *                one BGZF block around one STORED DEFLATE block: the 18-byte header 1f 8b 08 04 00000000 00 ff 0600 42 43 0200 BSIZE
 *                with BSIZE = len + 30, then 01 LEN ~LEN, the bytes, CRC32, ISIZE -- len + 31 bytes, so block b starts at b * 65,311 --
 *                and the 28-byte EOF block behind the last one.  Level-0 BGZF, which every BAM reader takes; no compression.
 *   memory       mem = PP_MEM_HOST or PP_MEM_DEVICE holds for `bytes` and `rec_off`.  Host bytes are uploaded and the copy is released
 *                before the call returns; device bytes are borrowed for the call only.  The object owns the output only.
 *   validation   on the device before anything is read through a record, with no sum that could wrap; no byte outside [0, n_bytes) is
 *                loaded, by a wide load either: a PP_MEM_DEVICE array may end where its allocation ends.  PP_ERR_ARG with *bad_record
 *                (may be NULL) = the first such record in index order, and no object: a rec_off outside the array or the array ending
 *                inside the block_size word; block_size < 32; a record running past n_bytes (pp_bam_walk's three verdicts).  Also
 *                PP_ERR_ARG: records_at > n_bytes, null arguments, PP_MEM_PEER, pass == NULL with aligned records present, n_pass other
 *                than the number of aligned records -- reported only once the records are free of the defects above, as pp_batch_gate
 *                does.  PP_ERR_LIMIT: 2^32-1 or more records, n_bytes >= 2^40, a block_size above 0xFFFFFFF7 (*bad_record = it).
 *   edge cases   n_rec == 0 yields the framed header alone; n_rec == 0 with records_at == 0 the EOF block alone.
 * The context's stream has been synchronised when the call returns: host inputs may be released.
 *   pp_bam_out_bytes      the file (DEVICE, borrowed until pp_bam_out_free): pp_bgzf_inflate(..., blk_off[b] = b * 65,311, PP_MEM_DEVICE)
 *                         reads it back
 *   pp_bam_out_counts     aligned records that passed, that failed, and the blocks without the EOF block
 *   pp_bam_out_write      downloads the file in slices and writes it to `path`; a path that cannot be created or written: PP_ERR_QUIT
 *                         "unable to write alignments to ..." in pp_last_error(ctx), the code and the words of pp_filter_write
 *   pp_bam_out_kernel_ms  as pp_gated_kernel_ms
 * The object belongs to its context and is freed before it. */
typedef struct pp_bam_out pp_bam_out;
int pp_bam_tagged(pp_ctx *ctx, const uint8_t *bytes, uint64_t n_bytes, uint64_t records_at, const uint64_t *rec_off, uint64_t n_rec,
                  int mem, const uint8_t *pass, uint64_t n_pass, pp_bam_out **out, uint64_t *bad_record);
/* pp_bam_tagged with a header of the caller's: the stream starts with head[0, n_head) (HOST memory whatever `mem`; n_head == 0: with
 * the first record) instead of bytes[0, records_at).  Everything else -- the records, the verdicts, the file, the validation, the
 * refusals with records_at > n_bytes among them, the edge cases -- is pp_bam_tagged's contract word for word; also PP_ERR_ARG: head ==
 * NULL with n_head > 0; PP_ERR_LIMIT: n_head >= 2^40.  With rec_off = pp_bam_sorted_rec_off, pass = what pp_bam_sorted_pass gives and
 * head = pp_bam_sorted_head this call and pp_bam_out_deflate write the coordinate-sorted file without another pass over the records. */
int pp_bam_tagged_head(pp_ctx *ctx, const uint8_t *bytes, uint64_t n_bytes, uint64_t records_at, const uint64_t *rec_off, uint64_t n_rec,
                       int mem, const uint8_t *pass, uint64_t n_pass, const uint8_t *head, uint64_t n_head, pp_bam_out **out,
                       uint64_t *bad_record);
void pp_bam_out_bytes(const pp_bam_out *o, const uint8_t **dev, uint64_t *n_bytes); /* DEVICE, borrowed until pp_bam_out_free */
void pp_bam_out_counts(const pp_bam_out *o, uint64_t *pass_count, uint64_t *fail_count, uint64_t *n_blocks); /* n_blocks without the EOF block */
int pp_bam_out_write(const pp_bam_out *o, const char *path); /* download in slices, write the file */
int pp_bam_out_kernel_ms(const pp_bam_out *o, float *ms);
void pp_bam_out_free(pp_bam_out *o);

/* The COORDINATE ORDER of BAM records, on the device: what a caller needs to write pp_bam_tagged's file sorted (pp_bam_tagged_head).
 *   inputs       bytes, n_bytes, records_at, rec_off, n_rec, mem: as pp_bam_tagged takes them; the records need not be adjacent, ordered
 *                or distinct.  bytes[0, records_at) must be a BAM header (pp_bam_header) that ends at records_at; with PP_MEM_DEVICE
 *                the library downloads it.
 *   the key      64 bits per record.  High word: ref_id where it is >= 0, else 0xFFFFFFFF: unplaced records come last.  Low word:
 *                (uint32_t)(pos + 1) << 1 | ((flag >> 4) & 1), in 32 bits: pos == 2^31 - 1 loses its top bit and sorts in front of
 *                its reference (no reference is that long; it is not refused).  perm is the STABLE order of the indices by that key:
 *                reference id, position, reverse strand, input order -- this library's reading of `samtools sort`'s coordinate
 *                order, not compared with samtools.  pp_bam_sorted_perm[j] = the input record at place j; pp_bam_sorted_rec_off[j] =
 *                rec_off[perm[j]].  Two calls give identical bytes, and sorting what is sorted moves nothing.
 *   the header   pp_bam_sorted_head: bytes[0, records_at) with the first line of its text made to say SO:coordinate.  The text is
 *                what stands in front of its trailing NULs.  A first line "@HD" (alone, or followed by a tab) has its first SO: field
 *                replaced, or "\tSO:coordinate" appended where it has none; any other first line, and no text, gets
 *                "@HD\tVN:1.6\tSO:coordinate\n" in front.  l_text is adjusted; the trailing NULs and the reference table are
 *                kept byte for byte.  HOST memory of the object.
 *   validation   the header first: what pp_bam_header refuses is refused with its code and words, a header that ends elsewhere than at
 *                records_at with PP_ERR_ARG, a text that would pass 2^31 - 1 bytes with PP_ERR_LIMIT.  Then the records, on the
 *                device before a field is read and with no sum that could wrap; no byte outside [0, n_bytes) is loaded, by a wide
 *                load either.  PP_ERR_ARG with *bad_record (may be NULL) = the first such record in index order, and no object:
 *                pp_bam_walk's three verdicts as pp_bam_tagged has them; pos < -1; ref_id < -1 or >= the header's n_ref.  Also
 *                PP_ERR_ARG: records_at > n_bytes, null arguments, PP_MEM_PEER.  PP_ERR_LIMIT: 2^32-1 or more records, n_bytes >= 2^40.
 *   edge cases   n_rec == 0 yields an empty permutation and the rewritten header.
 *   pp_bam_sorted_counts     the places j with perm[j] != j, and the records with ref_id == -1
 *   pp_bam_sorted_pass       as pp_regrouped_pass: pass (HOST, one byte per ALIGNED record of the input in index order) -> out (HOST,
 *                            n_pass bytes, may be `pass` only where nothing moved), the same verdicts in the numbering of the
 *                            sorted records; n_pass other than the number of aligned records: PP_ERR_ARG
 *   pp_bam_sorted_kernel_ms  as pp_gated_kernel_ms
 * The context's stream has been synchronised when the call returns.  The object belongs to its context and is freed before it. */
typedef struct pp_bam_sorted pp_bam_sorted;
int pp_bam_sort(pp_ctx *ctx, const uint8_t *bytes, uint64_t n_bytes, uint64_t records_at, const uint64_t *rec_off, uint64_t n_rec,
                int mem, pp_bam_sorted **out, uint64_t *bad_record);
const uint32_t *pp_bam_sorted_perm(const pp_bam_sorted *s); /* DEVICE, n_rec entries */
const uint64_t *pp_bam_sorted_rec_off(const pp_bam_sorted *s); /* DEVICE, n_rec entries: rec_off[perm[j]] */
void pp_bam_sorted_head(const pp_bam_sorted *s, const uint8_t **head, uint64_t *n_head); /* HOST, borrowed until pp_bam_sorted_free */
void pp_bam_sorted_counts(const pp_bam_sorted *s, uint64_t *n_moved, uint64_t *n_unplaced);
int pp_bam_sorted_pass(const pp_bam_sorted *s, const uint8_t *pass, uint64_t n_pass, uint8_t *out); /* HOST arrays */
int pp_bam_sorted_kernel_ms(const pp_bam_sorted *s, float *ms);
void pp_bam_sorted_free(pp_bam_sorted *s);

/* The COMPRESSOR of the record chain: bytes in device memory compressed into BGZF blocks, on the device.  pp_bam_tagged's level-0 file
 * is 4.6 times the size of the BAM file that came in; pp_bam_out_deflate makes the same file compressed.  pp_bam_tagged's own bytes
 * stay what they are.
 *   the pieces   the bytes cut every 65,280 (0xff00; the last piece is shorter, no bytes give no piece), each piece one BGZF block
 *                around ONE DEFLATE block with BFINAL = 1: the 18-byte header of pp_bam_tagged with the real BSIZE, the stream,
 *                CRC32, ISIZE.  The blocks are dense, at any byte alignment, the 28-byte EOF block behind the last; an empty input
 *                gives the EOF block alone.
 *   the stream   defined byte for byte by a plain model (tests/bgzf_deflate_model.py) as a function of the piece's bytes alone: two
 *                calls give identical bytes.  Match candidates come from a hash table of 2^13 entries over the piece's 4-byte groups,
 *                read in strips of 256 positions (a candidate lies in an earlier strip of the same piece, never in another piece);
 *                matches of 4 .. 258 bytes at distances up to 32,768; a greedy parse; length-limited Huffman codes (15 bits, 7 for the
 *                code-length code), always complete; the exact bit costs of the stored, the fixed and the dynamic form decide, a tie
 *                goes to the earlier of the three.  A block is therefore never longer than its piece + 31 bytes and the file never
 *                longer than pp_bam_tagged's.  Every BGZF or gzip reader takes it.
 *   memory       pp_bgzf_deflate: mem = PP_MEM_HOST or PP_MEM_DEVICE holds for `bytes`; host bytes are uploaded and the copy is
 *                released before the call returns, device bytes are borrowed for the call only.  pp_bam_out_deflate reads the
 *                payloads of the level-0 file where they lie (block b's at b * 65,311 + 23); the pp_bam_out stays valid and is the
 *                caller's to free.  No byte outside [0, n_bytes) is loaded, by a wide load either.  The object owns the output only;
 *                during the call the library holds one 65,344-byte slot per piece and the tokens of at most 1,024 pieces.
 *   errors       PP_ERR_ARG: null arguments (bytes == NULL with n_bytes > 0, out == NULL, o == NULL), PP_MEM_PEER.  PP_ERR_LIMIT:
 *                n_bytes >= 2^40.  There is nothing in the bytes themselves that could be refused.
 * The context's stream has been synchronised when either call returns: host inputs may be released.
 *   pp_bgzf_out_bytes      the file (DEVICE, borrowed until pp_bgzf_out_free)
 *   pp_bgzf_out_blk_off    the blocks' offsets in the file (DEVICE, borrowed): *n_blk + 1 entries, the EOF block's offset last --
 *                          exactly what pp_bgzf_inflate(file, n_bytes, blk_off, n_blk, PP_MEM_DEVICE, ...) takes to read the file back
 *   pp_bgzf_out_counts     the blocks by form: stored, fixed, dynamic (the EOF block is not counted)
 *   pp_bgzf_out_write      as pp_bam_out_write: downloads the file in slices and writes it to `path`; PP_ERR_QUIT "unable to write
 *                          alignments to ..." for a path that cannot be created or written
 *   pp_bgzf_out_kernel_ms  as pp_gated_kernel_ms
 * The object belongs to its context and is freed before it. */
typedef struct pp_bgzf_out pp_bgzf_out;
int pp_bgzf_deflate(pp_ctx *ctx, const uint8_t *bytes, uint64_t n_bytes, int mem, pp_bgzf_out **out); /* any bytes, cut every 65,280 */
int pp_bam_out_deflate(pp_ctx *ctx, const pp_bam_out *o, pp_bgzf_out **out);                          /* the tagged file, compressed */
void pp_bgzf_out_bytes(const pp_bgzf_out *o, const uint8_t **dev, uint64_t *n_bytes); /* DEVICE, borrowed until pp_bgzf_out_free */
const uint64_t *pp_bgzf_out_blk_off(const pp_bgzf_out *o, uint64_t *n_blk); /* DEVICE, n_blk + 1 entries: the EOF block's offset last */
void pp_bgzf_out_counts(const pp_bgzf_out *o, uint64_t *stored, uint64_t *fixed, uint64_t *dynamic);
int pp_bgzf_out_write(const pp_bgzf_out *o, const char *path); /* download in slices, write the file */
int pp_bgzf_out_kernel_ms(const pp_bgzf_out *o, float *ms);
void pp_bgzf_out_free(pp_bgzf_out *o);

/* The WRITE side of the record chain for a caller who holds SAM TEXT: the filter's verdicts written back as text, on the device -- the
 * text twin of pp_bam_tagged.  The output is, byte for byte and for every text and every `pass`, what pp_filter_write_text writes
 * (filter_sam, src/filter.rs:309-349); that host routine is the definition, and it needs the whole text in host memory.
 *   lines        are cut at '\n'; one trailing '\r' is dropped from a line's content.  Every output line ends in '\n': also a last
 *                line without a newline, and one that ends in a bare '\r'.  An empty line stays an empty line; an empty text gives an
 *                empty output.
 *   aligned      a line is an ALIGNED RECORD when it is not empty, does not begin with '@', has a tab, and its second column parses
 *                as parse::<u32> (a leading '+' is fine, 4294967296 is not) with bit 2 clear.  Nothing else about the line is looked
 *                at: this is NOT the eleven-column predicate of pp_sam_records, and a line that decode would refuse is copied like any
 *                other.  On any text pp_sam_records accepts the two agree.
 *   pass         pass[0, n_pass): HOST memory whatever `mem`, one byte per aligned record in file order -- the numbering of pp_sam_pass
 *                and of pp_filter_records' pass1 / pass2.  An aligned record whose byte is 0 gets the ten bytes "\tZP:Z:fail" between
 *                its content and its '\n'; one that already carries the tag gets a second one (the reference pushes the field without
 *                looking).  `pass` is the FILTER'S OWN verdict, not ANDed with pp_sam_pass.
 *   the rest     header lines, unaligned lines, lines that are no records and bytes >= 0x80 are copied as they are.  There is nothing
 *                in the bytes that could be refused.
 *   memory       mem = PP_MEM_HOST or PP_MEM_DEVICE holds for `text`.  Host text is uploaded and the copy is released before the call
 *                returns; device text is borrowed for the call only and read where it lies, at any alignment.  No byte outside
 *                [0, n_bytes) is loaded, by a wide load either: a PP_MEM_DEVICE text may end where its allocation ends, and no byte
 *                behind n_bytes can change a result.  pp_sam_tagged_records reads the pp_sam's own device copy of the text: no second
 *                upload; the pp_sam stays valid and is the caller's to free.  The object owns the output only.
 *   errors       PP_ERR_ARG: null arguments, PP_MEM_PEER, text == NULL with n_bytes > 0, pass == NULL with aligned records present,
 *                n_pass other than the number of aligned records ("N verdicts for M aligned records", pp_filter_write_text's
 *                sentence, in pp_last_error).  PP_ERR_LIMIT: n_bytes >= 2^40, 2^32-1 or more lines.  After a refusal there is no
 *                object, and the context serves the next call.
 *   geometry     pass A takes 1,024 lines per workgroup; pass B, the copy, gives every workgroup a tile of 16,384 OUTPUT bytes and
 *                writes it with 16-byte stores aligned on the output (the allocation is rounded up to 16; spare bytes are zeros).  A
 *                line longer than a tile spans workgroups; a tile in which more than 2,048 lines start takes a second, slower way
 *                to the same bytes.
 * The context's stream has been synchronised when either call returns: host inputs may be released.  Two calls on the same input give
 * identical bytes.
 *   pp_sam_out_bytes      the text (DEVICE, borrowed until pp_sam_out_free).  There is no compressor call of its own:
 *                         pp_bgzf_deflate(ctx, dev, n_bytes, PP_MEM_DEVICE, ...) on these bytes makes the bgzipped file, and
 *                         pp_bgzf_inflate with pp_bgzf_out_blk_off reads it back
 *   pp_sam_out_counts     aligned records that passed, that failed, and the lines
 *   pp_sam_out_write      as pp_bam_out_write: downloads the text in slices and writes it to `path`; PP_ERR_QUIT "unable to write
 *                         alignments to ..." for a path that cannot be created or written, the code and the words of pp_filter_write
 *   pp_sam_out_kernel_ms  as pp_gated_kernel_ms
 * The object belongs to its context and is freed before it. */
typedef struct pp_sam_out pp_sam_out;
int pp_sam_tagged(pp_ctx *ctx, const uint8_t *text, uint64_t n_bytes, int mem, const uint8_t *pass, uint64_t n_pass, pp_sam_out **out);
int pp_sam_tagged_records(pp_ctx *ctx, const pp_sam *s, const uint8_t *pass, uint64_t n_pass, pp_sam_out **out); /* the object's own device copy of the text */
void pp_sam_out_bytes(const pp_sam_out *o, const uint8_t **dev, uint64_t *n_bytes); /* DEVICE, borrowed until pp_sam_out_free */
void pp_sam_out_counts(const pp_sam_out *o, uint64_t *pass_count, uint64_t *fail_count, uint64_t *n_lines);
int pp_sam_out_write(const pp_sam_out *o, const char *path); /* download in slices, write the file */
int pp_sam_out_kernel_ms(const pp_sam_out *o, float *ms);
void pp_sam_out_free(pp_sam_out *o);

/* The link BETWEEN the two formats: SAM TEXT encoded as uncompressed BAM, on the device.  The output -- the bytes, records_at and
 * rec_off, all DEVICE memory -- is exactly what pp_bam_records, pp_bam_walk_device and pp_bam_tagged take with PP_MEM_DEVICE, so this
 * call needs no tagging, framing or compressor of its own: pp_bam_tagged(pass) -> pp_bam_out_deflate -> pp_bgzf_out_write finish a
 * compressed BAM file from text.  The bytes are restated by a plain model, tests/sam_bam_model.py.  The reference has no counterpart.
 *
 * pp_sam_header is the text twin of pp_bam_header: a HOST helper that needs no context and no device.  Lines are cut at '\n', one
 * trailing '\r' is not content.  The header is the leading run of lines that begin with '@'; *header_end = the offset of the first
 * line that is no header line (n_bytes when there is none).  Per line whose first column is exactly "@SQ", in file order: name_off[i] /
 * name_len[i] = the range in `text` of the value of its first SN: field, ref_len[i] = the value of its first LN: field.  The arrays
 * have `cap` entries; n_ref > cap: *n_ref is set all the same, the first cap entries are written and the call returns PP_ERR_ARG (as
 * do null arguments).  PP_ERR_QUIT with the sentence in pp_bam_last_error() (per thread), naming the 1-based line: an @SQ line without
 * SN: or with an empty one; without LN:, or with one that is not digits in 1 .. 2^31-1; a second @SQ line with the same name.  It is
 * memory-safe for any bytes: it never reads outside [0, n_bytes), and a text cut at any byte is answered without a fault.
 *
 * pp_sam_bam:
 *   memory       mem = PP_MEM_HOST or PP_MEM_DEVICE holds for `text`.  Host text is uploaded and the copy is released before the call
 *                returns; device text is borrowed for the call only and read where it lies, at any alignment.  No byte outside
 *                [0, n_bytes) is loaded, by a wide load either, and no byte behind n_bytes changes a result.  pp_sam_bam_records reads
 *                the pp_sam's own device copy of the text: no second upload.  The object owns the output only (the bytes in an
 *                allocation rounded up to 16, spare bytes zeros, and n_rec + 1 offsets).  The context's stream has been synchronised
 *                when the call returns.  Two calls on the same text give the same bytes.
 *   the header   BAM\1, l_text and the text's header lines, each ended by "\n" (a "\r" in front of it is dropped); n_ref and per @SQ
 *                line in order l_name, the name, NUL, l_ref.  An empty text gives the 12-byte header; a text of header lines only the
 *                header and no records.  *records_at = the header's length.
 *   records      every line behind the header that is neither empty nor begins with '@' is a record, in file order; rec_off[r] = the
 *                offset of record r's block_size word.  The columns are the eleven of SAM, split at tabs; every further column is an
 *                aux field.  block_size | refID pos l_read_name mapq bin n_cigar_op flag l_seq next_refID next_pos tlen | name NUL |
 *                CIGAR words | SEQ nibbles | QUAL | aux.
 *   refID        RNAME / RNEXT "*" is -1, RNEXT "=" is the record's refID, any other name its index among the @SQ lines: pp_names_ids
 *                over the two columns' ranges on a table seeded with the SN names in header order.
 *   numbers      FLAG, POS, MAPQ, PNEXT: [+]digits; pos = POS - 1 and next_pos = PNEXT - 1 from a value in 0 .. 2^31, mapq 0 .. 255,
 *                flag 0 .. 65535.  TLEN: [+-]digits in 32 signed bits.
 *   bin          reg2bin(pos, end): end = pos + the CIGAR's reference length (M D N = X) when FLAG & 4 is clear and that length is
 *                above 0, else pos + 1.  --end; for (shift, base) in (14, 4681) (17, 585) (20, 73) (23, 9) (26, 1): base + (pos >>
 *                shift) at the first shift where pos >> shift == end >> shift, else 0; arithmetic shifts on signed values, so
 *                (-1, 0) is 4680.
 *   CIGAR        "*" is no word, else len << 4 | op per run of digits and one of MIDNSHP=X (0 .. 8).
 *   SEQ, QUAL    SEQ "*" (or empty) is l_seq 0; else either case through =ACMGRSVTWYHKDBN, high nibble first, the spare low nibble
 *                behind an odd length 0.  QUAL "*" is l_seq bytes 0xFF, else byte - 33.
 *   aux          TAG:TYPE:VALUE in the line's order.  A: one byte.  i: [+-]digits, in the smallest type of C c S s I i that holds the
 *                value.  Z: the bytes and a NUL.  H: as Z, an even number of hex digits.  f: a float32.  B: a sub-type of c C s S i I
 *                f, a 32-bit count, the values ("B:c" alone is count 0).
 *   a float      [+-]digits[.digits][(e|E)[+-]digits]: w = the digits without the point and without leading zeros as one integer,
 *                e10 = the exponent less the digits behind the point; the value is (double)w * 10^e10 or (double)w / 10^-e10 in ONE
 *                IEEE double operation, then rounded to float; a zero of any form is +-0.0.  That is C's strtod-then-float whenever w
 *                has at most 15 digits and |e10| <= 22; beyond that the line is refused.
 *   refusals     no object; the first refused line in file order wins, whatever its kind; *bad_line (may be NULL) = its 0-based index
 *                among all lines; pp_last_error names the path "text", the 1-based line and the column or the aux tag.  Inside one
 *                line the checks run in this order: the columns' number, QNAME, FLAG, POS, MAPQ, CIGAR (run by run, then the number
 *                of runs), PNEXT, TLEN, SEQ, QUAL, the bin, the aux fields left to right, then RNAME and RNEXT.
 *                PP_ERR_QUIT: fewer than 11 columns; a FLAG, POS, MAPQ, PNEXT or TLEN that is no number; a CIGAR that is not runs of
 *                digits and an op; QUAL present with SEQ "*", of another length than SEQ, or with a byte below 33; an aux field that is
 *                not XX:T:... (an empty field behind a trailing tab included), of unknown type, an A of other than one byte, an i that
 *                is no number, an H of odd length or with a byte that is no hex digit, a B with an unknown sub-type, an empty element or
 *                a value outside its sub-type; an RNAME or RNEXT that no @SQ line names; a line that begins with '@' behind the first
 *                record (one in front of it is skipped).
 *                PP_ERR_LIMIT, a valid line this encoder does not hold: a value beyond its field (FLAG, POS, MAPQ, PNEXT, TLEN, an i
 *                outside -2^31 .. 2^32-1); a QNAME that is empty or longer than 254 bytes; more than 65,535 CIGAR runs, a run of 2^28
 *                or more, a run of length 0 (the text's expansion drops it, a BAM word would keep it); a SEQ byte outside the table;
 *                the bin's `end` above 2^29 (the bin has 16 bits); a float outside the rule above, inf
 *                and nan included; a line of 2^31 or more bytes; 2^32-1 or more lines; n_bytes >= 2^40; an output of 2^40 bytes or more.
 *                PP_ERR_NOT_ASCII for a byte >= 0x80 anywhere in the text, as pp_sam_records (no bad_line).  PP_ERR_ARG: null
 *                arguments, PP_MEM_PEER, null text with n_bytes > 0.  A refusal of pp_sam_header comes through with its own code and
 *                sentence.  After a refusal the context serves the next call.
 *   NM           is not looked at: an aligned line without NM encodes like any other (`filter`'s new_quick never reads NM).  On any
 *                text that both this call and pp_sam_records accept, record r of one is record r of the other.
 *   geometry     pass B gives every workgroup a tile of 16,384 OUTPUT bytes, built in LDS and written with 16-byte stores aligned on
 *                the output; a record longer than a tile spans workgroups.
 * pp_bam_enc_bytes / pp_bam_enc_rec_off: borrowed until pp_bam_enc_free.  pp_bam_enc_kernel_ms: as pp_gated_kernel_ms, the
 * pp_names_ids kernels included.  The object belongs to its context and is freed before it. */
int pp_sam_header(const uint8_t *text, uint64_t n_bytes, uint32_t cap, uint32_t *n_ref, uint64_t *name_off, uint32_t *name_len,
                  uint32_t *ref_len, uint64_t *header_end);
typedef struct pp_bam_enc pp_bam_enc;
int pp_sam_bam(pp_ctx *ctx, const uint8_t *text, uint64_t n_bytes, int mem, pp_bam_enc **out, uint64_t *bad_line);
int pp_sam_bam_records(pp_ctx *ctx, const pp_sam *s, pp_bam_enc **out, uint64_t *bad_line); /* the pp_sam's own device copy, no second upload */
void pp_bam_enc_bytes(const pp_bam_enc *e, const uint8_t **dev, uint64_t *n_bytes, uint64_t *records_at); /* DEVICE: uncompressed BAM */
const uint64_t *pp_bam_enc_rec_off(const pp_bam_enc *e, uint64_t *n_rec);                                /* DEVICE, n_rec entries */
int pp_bam_enc_kernel_ms(const pp_bam_enc *e, float *ms);
void pp_bam_enc_free(pp_bam_enc *e);

/* The opposite direction: uncompressed BAM decoded to SAM TEXT, on the device.  The result is a pp_sam_out, the object pp_sam_tagged
 * makes: pp_sam_out_bytes / _counts / _write / _kernel_ms / _free and pp_bgzf_deflate on its bytes work on it unchanged.  The bytes are
 * defined by a plain model, tests/bam_sam_model.py; they were not compared with `samtools view`.  For every CANONICAL text T -- plain
 * decimals, upper-case SEQ, RNEXT "=" for a repeated name, floats in the "%g" form of a float32, no "\r", no empty line, a final
 * "\n" -- pp_bam_sam(pp_sam_bam(T)) == T byte for byte.  The reference has no counterpart.
 *   arguments    bytes[0, n_bytes), records_at, rec_off[0, n_rec): as pp_bam_tagged; mem = PP_MEM_HOST or PP_MEM_DEVICE holds for
 *                `bytes` and `rec_off`.  Device bytes are borrowed for the call only; no byte outside [0, n_bytes) is loaded, by a wide
 *                load either.  pp_bam_sam_encoded reads a pp_bam_enc's own device memory.  pass[0, n_pass): HOST memory, one byte per
 *                ALIGNED record (flag & 4 == 0) in index order, pp_bam_tagged's numbering; pass == NULL with n_pass == 0: no verdicts,
 *                nothing is appended.  The context's stream has been synchronised when the call returns; two calls on the same input
 *                give identical bytes.
 *   the header   bytes[0, records_at) must be a BAM header (pp_bam_header) that ends at records_at; with PP_MEM_DEVICE the library
 *                downloads it.  The text starts as the l_text bytes of header text without trailing NULs, a "\n" appended where it is
 *                not empty and does not end in one.  Where no line's first column is exactly "@SQ" and n_ref > 0, one line
 *                "@SQ\tSN:<name>\tLN:<l_ref>" per reference follows, in order (htslib does the same): pp_sam_header of the output
 *                gives back the BAM's reference table.
 *   a record     one line QNAME FLAG RNAME POS MAPQ CIGAR RNEXT PNEXT TLEN SEQ QUAL and the aux fields, joined by tabs, ended by
 *                "\n", in index order.  Numbers are plain decimals.  RNAME "*" for refID -1, else the name; RNEXT "*" for -1, "=" where
 *                it equals a refID >= 0, else the name; POS = pos + 1, PNEXT = next_pos + 1.  CIGAR "*" for no word, else len and one
 *                of MIDNSHP=X per word (a CG:B:I aux field is printed as the aux field it is).  SEQ "*" for l_seq 0, else the
 *                nibbles through =ACMGRSVTWYHKDBN.  QUAL "*" where l_seq is 0 or its first byte is 0xFF, else byte + 33.
 *   aux          in the record's order: A one byte; c C s S i I as TAG:i:<decimal>; Z and H their bytes; B as TAG:B:<sub> and
 *                ",<value>" per element; f (also inside B) as C's printf("%g") of the float widened to double, exact over all of
 *                float32.
 *   verdicts     an aligned record whose byte is 0 gets the ten bytes "\tZP:Z:fail" in front of its "\n", also behind a tag that is
 *                already there; unaligned records take no verdict.  NM is not looked at.
 *   refusals     no object; the first refused record in index order wins, *bad_record (may be NULL) = its index; inside one record a
 *                PP_ERR_ARG defect goes in front of a PP_ERR_LIMIT.
 *                PP_ERR_ARG: pp_bam_tagged's three (a rec_off outside the array or ending inside the block_size word, block_size <
 *                32, a record past n_bytes); pp_bam_records' inner defects (block_size below the sum of its parts, l_read_name == 0 or
 *                a name without its NUL, a CIGAR op above 8, a refID or next_refID outside [-1, n_ref), an aux field that is cut or of
 *                unknown type, a Z / H without NUL inside the record, a B of unknown sub-type or whose count runs past the record);
 *                pos or next_pos below -1; bytes[0, records_at) that is no BAM header ending there; null arguments, PP_MEM_PEER.
 *                Another number of verdicts than aligned records is PP_ERR_ARG too, reported only once the records are free of
 *                defects.
 *                PP_ERR_LIMIT, a valid record that has no SAM line: an empty QNAME, one that begins with '@' or holds a byte outside
 *                0x21..0x7E; a used reference name that is empty, "*", "=" or holds a byte outside 0x21..0x7E; an A value outside
 *                0x21..0x7E; a Z byte outside 0x20..0x7E; an H that is not an even number of hex digits; a tag that is not
 *                [A-Za-z][A-Za-z0-9]; a QUAL byte above 93 where the first byte is not 0xFF; a float that is inf or nan; a reference
 *                whose @SQ line would have to be written and cannot be (such a name, or l_ref outside 1 .. 2^31-1; no bad_record);
 *                2^32-1 or more records; n_bytes >= 2^40; an output of 2^40 bytes or more.
 *                Every line written is a line pp_sam_bam parses; pp_sam_bam's own capacity limits (a CIGAR run of length 0, an end
 *                above 2^29, a float beyond 10^+-22) stay its own.  After a refusal the context serves the next call.
 *   geometry     pass A takes 1,024 records per workgroup; pass B gives every workgroup a tile of 16,384 OUTPUT bytes, built in LDS
 *                and written with 16-byte stores aligned on the output; a record longer than a tile spans workgroups. */
int pp_bam_sam(pp_ctx *ctx, const uint8_t *bytes, uint64_t n_bytes, uint64_t records_at, const uint64_t *rec_off, uint64_t n_rec,
               int mem, const uint8_t *pass, uint64_t n_pass, pp_sam_out **out, uint64_t *bad_record);
int pp_bam_sam_encoded(pp_ctx *ctx, const pp_bam_enc *e, const uint8_t *pass, uint64_t n_pass, pp_sam_out **out, uint64_t *bad_record);

/* What an alignment file holds, told by its CONTENT: the commands (pp_polish_files, pp_filter_files, pp_filter_polish_files) take SAM
 * text as before and BAM through the record chain above, and ask this.  HOST, no context; reads only the head of the file.
 *   PP_ALN_SAM      anything that is neither of the two below, an empty file included: the text routes keep their own errors.  A
 *                   path that is no regular file (a pipe, a process substitution) is not opened: it is text
 *   PP_ALN_BAM      BGZF -- 1f 8b 08, FEXTRA, a BC subfield of SLEN 2 among the extra subfields (it need not be the first) -- whose
 *                   inflated bytes start with BAM\1; the first block(s) are inflated on the host for those four bytes, no more
 *   PP_ALN_BAM_RAW  the file itself starts with BAM\1: uncompressed BAM
 * PP_ERR_QUIT with the message in pp_bam_last_error(): a gzip member without BC ("... is gzip-compressed but not BGZF"); BGZF whose
 * content is not BAM, a bgzipped SAM ("... is BGZF-compressed but does not hold BAM"); a file that begins 1f 8b and ends before a whole
 * gzip header; a path that cannot be read ("unable to load alignments from ...", the drivers' words).  PP_ERR_ARG: null arguments.
 * Neither 0x1f nor 0x01 occurs in a valid SAM line: no SAM input changes its route. */
enum { PP_ALN_SAM = 0, PP_ALN_BAM = 1, PP_ALN_BAM_RAW = 2 };
int pp_aln_file_kind(const char *path, int *kind);
enum { PP_ALN_SAM_BGZF = 3 }; /* pp_aln_file_kind_text only */
/* pp_aln_file_kind for a caller who reads bgzipped SAM text as well (the commands with pp_ctx_set_text_chain): the same answers and
 * refusals, except that BGZF whose inflated head is not BAM\1 -- fewer than four bytes of content included -- is PP_ALN_SAM_BGZF
 * instead of a refusal.  gzip that is not BGZF stays refused. */
int pp_aln_file_kind_text(const char *path, int *kind);

/* Per-contig figures the reference prints to stderr (src/polish.rs:206-227). */
typedef struct {
    uint64_t polished_len;     /* bytes of the polished sequence                      */
    uint64_t changed;          /* positions with status Changed                       */
    uint64_t zero_depth;       /* positions with depth == 0.0                         */
    double depth_sum;          /* sum of per-position depth (cosmetic: the "mean read depth" line of the log, polish.rs:206-227).
                                * Exact where every depth share 1/k is a power of two; a position with other shares adds its depth
                                * rounded to 2^-10 (its VOTE is exact -- interval test or ordered replay -- its contribution to this
                                * sum is not replayed): |depth_sum - reference| <= polished_len * 2^-11 + 1e-6 * depth_sum, i.e. the
                                * mean depth printed to one decimal can differ in that digit only when it lies within 0.0005 of a
                                * rounding boundary (tests/test_gpu_parity.py compares the sums under this bound). */
} pp_contig_stats;

/* Optional, between pp_polish_begin and pp_polish_finish: restrict what contig c EMITS to its positions
 * [emit_lo[c], emit_hi[c]) (0-based, relative to the contig; arrays of n_contigs, host memory).  Positions outside
 * the range contribute no polished bytes and no statistics, records that do not reach the range are validated and
 * then dropped, windows outside it are not worked on.  This is how one rank of a sharded job (SURVEY 8e, configs
 * C4 / C5) polishes its contigs or its window of a large contig: it is given the records that reach its ranges
 * (pp_shard_split -- or simply all records) and emits only what it owns; an owned position sees all of its
 * alignments in file order either way, so the order-dependent f64 depth is exact.  NULL, NULL = everything. */
int pp_polish_set_emit(pp_ctx *ctx, const uint64_t *emit_lo, const uint64_t *emit_hi);

/* Start a polish job.  contig_off is a HOST array of n_contigs+1 offsets into `bases` (the
 * concatenated, ASCII-uppercased assembly, src/misc.rs:114,129; total length < 2^32-4096). */
int pp_polish_begin(pp_ctx *ctx, uint32_t n_contigs, const uint64_t *contig_off,
                    const uint8_t *bases, int bases_mem, const pp_params *params);
/* Provide alignments, one batch after the other as the reference streams its SAM files (src/alignment.rs:238-265):
 * every record of a later batch follows the records of the earlier ones in file order; seq_off / cig_off are
 * relative to the batch's own seq / cigar arrays.  `mem` applies to every pointer in the batch.  Host batches are
 * copied before the call returns; PP_MEM_DEVICE batches must stay valid and unchanged until pp_polish_finish returns
 * (a job's ONLY batch is used in place; with more than one batch everything is gathered into library-owned arrays
 * with device-to-device copies on the context's stream).  Limits per job: < 2^32-1 records, < 2^40 SEQ bytes. */
int pp_polish_add(pp_ctx *ctx, const pp_aln_batch *batch, int mem);
/* Optional, after pp_polish_begin: room for everything the job's batches will hold together (a guess is fine). */
int pp_polish_reserve(pp_ctx *ctx, uint64_t n_aln, uint64_t seq_bytes, uint64_t n_cig_total);
/* Run the kernels: CIGAR walk + homopolymer trim (src/alignment.rs:175-201,364-378), pileup
 * accumulation (src/pileup.rs:56-65,189-200), vote (src/pileup.rs:67-134), '-' removal and
 * concatenation (src/polish.rs:185-188).  Results stay on the device until fetched. */
int pp_polish_finish(pp_ctx *ctx);
/* Total polished bytes over all contigs (no headers, no newlines). */
int pp_polish_result_size(pp_ctx *ctx, uint64_t *total_bytes);
/* Copy the polished bytes to `out` (host or device, >= result_size bytes); contig c occupies
 * [contig_out_off[c], contig_out_off[c+1]).  contig_out_off (HOST, n_contigs+1) and stats (HOST,
 * n_contigs) may be NULL. */
int pp_polish_result(pp_ctx *ctx, uint8_t *out, int out_mem, uint64_t *contig_out_off,
                     pp_contig_stats *stats);
/* Device pointer to the polished bytes (valid until the next pp_polish_begin); the context's stream is idle when this returns
 * (pp_polish_finish itself may return a few microseconds before its last kernel's end has been signalled: it has the job's
 * results from that kernel's last workgroup -- readers on other streams come through here). */
const uint8_t *pp_polish_result_device(pp_ctx *ctx);

/* Optional per-position record (what the --debug TSV is made of, src/pileup.rs:150-166):
 * enable before pp_polish_finish, fetch after.  Arrays are HOST, one element per assembly
 * position in concatenated order; any pointer may be NULL. */
typedef struct {
    double *depth;
    uint32_t *count_a, *count_c, *count_g, *count_t;
    uint32_t *count_other;  /* sum over the string-keyed table, deletions ("-") included */
    uint32_t *valid_thr, *invalid_thr;
    uint8_t *status;        /* PP_ST_* */
} pp_positions;
int pp_polish_set_debug(pp_ctx *ctx, int enable);
int pp_polish_positions(pp_ctx *ctx, const pp_positions *out);

/* The rest of a --debug line (src/pileup.rs:137-166): the string-keyed tallies and the winning
 * sequence of every position.  Valid after pp_polish_finish with debug enabled; the arrays are
 * malloc'd by the library (release with pp_debug_extra_free).
 *   emit[p]      0 = nothing is emitted (a deletion won, or the assembly byte is '-'), 1..127 = that
 *                byte, >= 128 = a multi-byte winner listed in multi_* (raw bytes at seq + multi_off)
 *   key_*        one record per (position, distinct key other than A/C/G/T): the key is the len bytes
 *                at seq + off (the batch's seq array); len 0 = the deletion key "-"            */
typedef struct {
    uint8_t *emit;         /* one per assembly position */
    uint64_t n_multi;
    uint32_t *multi_pos, *multi_len;
    uint64_t *multi_off;
    uint64_t n_keys;
    uint32_t *key_pos, *key_len, *key_count;
    uint64_t *key_off;
} pp_debug_extra;
int pp_polish_debug_extra(pp_ctx *ctx, pp_debug_extra *out);
void pp_debug_extra_free(pp_debug_extra *d);

/* The --debug TSV itself (src/polish.rs:257-266, without its header line), formatted on the device: the lines of the
 * positions [pos_lo, pos_hi) (concatenated assembly coordinates) in position order, into `out` (PP_MEM_HOST or
 * PP_MEM_DEVICE, cap bytes).  Valid after pp_polish_finish with pp_polish_set_debug(ctx, 1); a context with
 * pp_polish_set_emit writes the lines of the positions it emits and skips the others.  contig_names: one NUL-terminated
 * name per contig (read on the first call after a job).  Writes whole lines only: *len = bytes written, *pos_next = the
 * first position not written (pos_hi when the range is done; call again from there).  PP_ERR_ARG, and nothing written,
 * when cap is smaller than the first line.  Device memory: 4 bytes per assembly position and a bounded staging area,
 * whatever the TSV's size. */
int pp_polish_debug_tsv(pp_ctx *ctx, const char *const *contig_names, uint64_t pos_lo, uint64_t pos_hi, uint8_t *out,
                        int out_mem, uint64_t cap, uint64_t *len, uint64_t *pos_next);

/* ---- the polish's edits as VCF text on the device (pp_k_vcf.h; not in the reference) ----------
 * pp_polish_vcf writes where the finished job changed the assembly, and to what, as VCF 4.2 text in device memory: a post-pass over
 * what every job leaves on the context -- the assembly bases, the emit codes, the multi-byte winners' list and the polished bytes.
 * Valid after a successful pp_polish_finish and until the next pp_polish_begin, with or without pp_polish_set_debug, whichever path
 * the job took; the bytes depend on neither.  The batch's seq array is NOT read (the caller may have released it): ALT bytes come from
 * the polished output.  tests/vcf_model.py defines the text:
 *   header     "##fileformat=VCFv4.2\n", "##source=" pp_version() "\n", per contig in assembly order "##contig=<ID=name,length=L>\n",
 *              then "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
 *   edited     position p emits e(p), its bytes in the polished output (the winner without its '-': it may be empty); p is edited
 *              iff e(p) is not exactly the one byte bases[p]
 *   records    each maximal run [a, b) of edited positions inside ONE contig (runs never join across a contig boundary) is one line
 *              name \t POS \t . \t REF \t ALT \t . \t . \t . \n, with R = bases[a..b), A = e(a)...e(b-1), positions local and 0-based:
 *                  A not empty                        POS a+1   REF R                ALT A
 *                  A empty, a > 0                     POS a     REF bases[a-1] R     ALT bases[a-1]   (the anchor is unedited)
 *                  A empty, a == 0, b < L             POS 1     REF R bases[b]       ALT bases[b]
 *                  A empty, the run is the contig     POS 1     REF R                ALT <DEL>
 *              in assembly order.  Bytes are written as they are: nothing is re-cased, trimmed or normalised, and a name or an
 *              assembly byte that VCF does not allow is written all the same.
 * contig_names: one NUL-terminated name per contig.  Refusals, all but the last decided on the host before anything is launched:
 * PP_ERR_ARG for a null argument, a context without a finished job (a job that ended in an error leaves none), a context with
 * pp_polish_set_emit ranges (a rank's share has no defined runs at its edges), a name that holds a tab or a newline; PP_ERR_LIMIT
 * for a text of 2^40 bytes or more (the header's share on the host; the records' once the device has scanned their lengths, before
 * the text is allocated).  A job without an edit gives the header alone and *n_records == 0.  Returns with the context's stream
 * synchronised.  The object belongs to its context (free it before the context); device memory beyond the text: 2 bytes per
 * assembly position during the call (6 with multi-byte winners) and 40 per record.
 *   pp_vcf_out_bytes      the text (DEVICE, borrowed until pp_vcf_out_free): pp_bgzf_deflate(ctx, dev, n_bytes, PP_MEM_DEVICE, ...)
 *                         makes the bgzipped file
 *   pp_vcf_out_write      as pp_fasta_out_write: downloads the text in slices and writes it to `path`
 *   pp_vcf_out_kernel_ms  as pp_fasta_out_kernel_ms: the HIP-event spans of the call's stages on the stream (the host's read-backs and
 *                         allocations between their launches lie inside them) */
typedef struct pp_vcf_out pp_vcf_out;
int pp_polish_vcf(pp_ctx *ctx, const char *const *contig_names, pp_vcf_out **out);
void pp_vcf_out_bytes(const pp_vcf_out *o, const uint8_t **dev, uint64_t *n_bytes, uint64_t *n_records); /* DEVICE, borrowed */
int pp_vcf_out_write(const pp_vcf_out *o, const char *path);                                             /* download in slices, write */
int pp_vcf_out_kernel_ms(const pp_vcf_out *o, float *ms);
void pp_vcf_out_free(pp_vcf_out *o);

/* ---- undecided regions: the per-position outcome as BED text and as a soft mask, on the device (pp_k_bed.h; not in the reference) ----
 * A polish decides one of six outcomes per assembly position (PP_ST_*, src/pileup.rs:111-129).  pp_status_bed writes the runs of equal
 * status as BED text in device memory; pp_polish_bed does so for the finished job's own status plane; pp_polish_masked gives a copy of
 * the job's polished bytes in which the bytes of selected positions are in lower case (FASTA soft-masking).  tests/bed_model.py
 * defines the bytes:
 *   text       no header line.  Per record, in assembly order:  name \t start \t end \t word \n  -- start and end 0-based, half-open and
 *              local to the contig; word is the reference's own: kept, changed, low_depth, none, multiple, too_close
 *   record     a maximal run of consecutive positions of ONE contig (runs never join across a contig boundary) that share one status
 *              whose bit (1 << PP_ST_x) is set in status_mask.  Two different selected statuses side by side are two records.
 *              Names are written verbatim
 *   masked     position p emits e(p) bytes of the polished output (the scan of the emitted lengths gives where); every byte 'A'..'Z'
 *              emitted by a position whose status is selected becomes lower case, a multi-byte winner whole; a position that emits
 *              nothing changes nothing; every other byte is the job's.  The job's own polished bytes stay as they are
 * pp_status_bed: `status` holds G = contig_off[n_contigs] bytes (PP_MEM_HOST: uploaded; PP_MEM_DEVICE: read in place, at any
 * alignment, and no byte outside [0, G) is loaded, by a wide load either: the array may end where its allocation ends); contig_off
 * (HOST, n_contigs + 1 entries from 0 on) and contig_names (one NUL-terminated name per contig) as for pp_polish_vcf.  pp_polish_bed
 * and pp_polish_masked are valid after a successful pp_polish_finish of a job that ran with pp_polish_set_debug(ctx, 1), and until the
 * next pp_polish_begin, whichever path the job took.
 * Refusals, decided on the host before anything is launched except the last two: PP_ERR_ARG for a null argument, PP_MEM_PEER, a mask of
 * 0 or one with a bit above 5, contig_off[0] != 0, offsets that decrease, G >= 2^32, a name that holds a tab or a newline; for the two
 * pp_polish_* calls a context without a finished job (a job that ended in an error leaves none), a job finished without
 * pp_polish_set_debug(ctx, 1) (it kept no status), a context with pp_polish_set_emit ranges (a rank's share has no defined runs at its
 * edges); a status byte above 5, *bad_pos = the first such position (a device check; bad_pos may be NULL); PP_ERR_LIMIT for a text of
 * 2^40 bytes or more (known once the device has scanned the lines' lengths, before the text is allocated).  n_contigs == 0, or no
 * selected position, gives an empty text and *n_records == 0.  Both calls return with the context's stream synchronised.  The objects
 * belong to their context (free them before the context).  Device memory beyond the results: 24 bytes per record during pp_status_bed
 * (G bytes more for a PP_MEM_HOST array); 4 bytes per position during pp_polish_masked when the job has multi-byte winners.
 *   pp_bed_out_bytes      the text (DEVICE, borrowed until pp_bed_out_free): pp_bgzf_deflate(ctx, dev, n_bytes, PP_MEM_DEVICE, ...) makes
 *                         the bgzipped file
 *   pp_bed_out_counts     positions[s] = the positions of status s inside the records (their summed lengths)
 *   pp_bed_out_write      as pp_vcf_out_write
 *   pp_bed_out_kernel_ms  as pp_vcf_out_kernel_ms: the HIP-event spans of the call's stages (the context had pp_ctx_set_profiling on)
 *   pp_masked_bytes       the bytes (DEVICE, borrowed until pp_masked_free), n_bytes = pp_polish_result_size: laid out as the job's own,
 *                         pp_polish_result's contig_out_off holds for them */
#define PP_BED_UNDECIDED ((1u << PP_ST_LOW_DEPTH) | (1u << PP_ST_NONE) | (1u << PP_ST_MULTIPLE) | (1u << PP_ST_TOO_CLOSE))
typedef struct pp_bed_out pp_bed_out;
int pp_status_bed(pp_ctx *ctx, const uint8_t *status, int mem, uint32_t n_contigs, const uint64_t *contig_off /*HOST*/,
                  const char *const *contig_names, uint32_t status_mask, pp_bed_out **out, uint64_t *bad_pos);
int pp_polish_bed(pp_ctx *ctx, const char *const *contig_names, uint32_t status_mask, pp_bed_out **out);
void pp_bed_out_bytes(const pp_bed_out *o, const uint8_t **dev, uint64_t *n_bytes, uint64_t *n_records); /* DEVICE, borrowed */
void pp_bed_out_counts(const pp_bed_out *o, uint64_t positions[6]);
int pp_bed_out_write(const pp_bed_out *o, const char *path);
int pp_bed_out_kernel_ms(const pp_bed_out *o, float *ms);
void pp_bed_out_free(pp_bed_out *o);

typedef struct pp_masked pp_masked;
int pp_polish_masked(pp_ctx *ctx, uint32_t status_mask, pp_masked **out);
void pp_masked_bytes(const pp_masked *o, const uint8_t **dev, uint64_t *n_bytes); /* DEVICE, borrowed */
int pp_masked_kernel_ms(const pp_masked *o, float *ms);
void pp_masked_free(pp_masked *o);

/* ---- read depth: the per-position depth as bedGraph text, on the device (pp_k_depth.h; not in the reference) ----
 * A polish computes a read depth for every assembly position: the double that PileupBase::add_seq accumulates from the reads' 1/k
 * shares (src/pileup.rs:56-65).  pp_depth_bedgraph writes a caller's array of such depths as bedGraph text in device memory -- the
 * format of `bedtools genomecov -bga` --, pp_polish_depth does so for the finished job's own depth plane.  tests/depth_model.py
 * defines the bytes:
 *   tenths(x)  the integer 10 x rounded from x's exact binary value, ties to even: what format!("{:.1}") and the --debug TSV print,
 *              without the point (0 <= x < 2^32)
 *   text       no header or track line.  Per record, in assembly order:  name \t start \t end \t value \n  -- start and end 0-based,
 *              half-open and local to the contig; names are written verbatim
 *   bin == 0   (runs) a record is a maximal run of consecutive positions of ONE contig (runs never join across a contig boundary)
 *              that share one tenths value -- two doubles that print alike are one run, zero-depth runs are written like any other;
 *              value = tenths / 10 '.' tenths % 10
 *   bin == W   (bins, 1 <= W <= 2^24) per contig of length L one record per bin [kW, min((k+1)W, L)), k = 0 .. ceil(L/W) - 1, equal
 *              neighbours not merged; value = the mean of the bin's depths as printed, to two decimals, in integer arithmetic: with
 *              S the sum of the bin's tenths and n its length, q = 10 S / n rounded, ties to even, written q / 100 '.' and the two
 *              digits of q % 100 -- exact and free of the order of the sum
 *   summary    zero_positions: the positions whose tenths are 0; max_tenths; sum_tenths: over all positions
 * pp_depth_bedgraph: `depth` holds G = contig_off[n_contigs] doubles (PP_MEM_HOST: uploaded; PP_MEM_DEVICE: read in place -- aligned
 * to 8 bytes, and no byte outside [0, 8 G) is loaded, by a wide load either: the array may end where its allocation ends); contig_off
 * and contig_names as for pp_status_bed.  pp_polish_depth is valid after a successful pp_polish_finish of a job that ran with
 * pp_polish_set_debug(ctx, 1), and until the next pp_polish_begin, whichever path the job took.
 * Refusals, decided on the host before anything is launched except the last two: PP_ERR_ARG for a null argument, PP_MEM_PEER,
 * bin > 2^24, a device array that is not aligned to 8 bytes, contig_off[0] != 0, offsets that decrease, G >= 2^32, a name that holds a
 * tab or a newline; for pp_polish_depth a context without a finished job (a job that ended in an error leaves none), a job finished
 * without pp_polish_set_debug(ctx, 1) (it kept no depth), a context with pp_polish_set_emit ranges; a depth whose sign bit is set
 * (-0.0 too), that is not a number, or is 2^32 or more, *bad_pos = the first such position (a device check; bad_pos may be NULL);
 * PP_ERR_LIMIT for a text of 2^40 bytes or more (known once the device has scanned the lines' lengths, before the text is allocated).
 * n_contigs == 0 gives an empty text, a contig of length 0 no record.  Both calls return with the context's stream synchronised.  The
 * object belongs to its context (free it before the context).  Device memory beyond the result: no plane per position (the tenths
 * are made again where a pass needs them), 8 bytes per workgroup of 2048 positions in the runs form, 8 bytes per bin in the bins
 * form; per record 24 bytes for its row and 8 for its place in the text (8 G bytes more for a PP_MEM_HOST array).
 *   pp_depth_out_bytes      the text (DEVICE, borrowed until pp_depth_out_free): pp_bgzf_deflate(ctx, dev, n_bytes, PP_MEM_DEVICE, ...)
 *                           makes the bgzipped file
 *   pp_depth_out_summary    the three numbers above (any of the pointers may be NULL)
 *   pp_depth_out_write      as pp_vcf_out_write
 *   pp_depth_out_kernel_ms  as pp_vcf_out_kernel_ms: the HIP-event spans of the call's stages (the context had pp_ctx_set_profiling on) */
typedef struct pp_depth_out pp_depth_out;
int pp_depth_bedgraph(pp_ctx *ctx, const double *depth, int mem, uint32_t n_contigs, const uint64_t *contig_off /*HOST*/,
                      const char *const *contig_names, uint32_t bin, pp_depth_out **out, uint64_t *bad_pos);
int pp_polish_depth(pp_ctx *ctx, const char *const *contig_names, uint32_t bin, pp_depth_out **out);
void pp_depth_out_bytes(const pp_depth_out *o, const uint8_t **dev, uint64_t *n_bytes, uint64_t *n_records); /* DEVICE, borrowed */
void pp_depth_out_summary(const pp_depth_out *o, uint64_t *zero_positions, uint64_t *max_tenths, uint64_t *sum_tenths);
int pp_depth_out_write(const pp_depth_out *o, const char *path);
int pp_depth_out_kernel_ms(const pp_depth_out *o, float *ms);
void pp_depth_out_free(pp_depth_out *o);

/* Per-kernel device time of the last pp_polish_finish, measured with HIP events on the context's
 * stream when profiling is enabled.  names[i] are static strings. */
#define PP_MAX_KERNELS 16
typedef struct {
    int n;
    const char *name[PP_MAX_KERNELS];
    float ms[PP_MAX_KERNELS];
    uint64_t n_entries;   /* (alignment, window) work items the tile kernel consumed */
    uint64_t n_flagged;   /* positions resolved by the exact (string-keyed, ordered-f64) kernel */
    uint64_t n_passes;    /* passes over the pipeline: 1, or more when a device buffer had to grow (first job) */
} pp_kernel_times;
int pp_ctx_set_profiling(pp_ctx *ctx, int enable); /* 0 off, 1 every kernel group, 2 only the dominant kernel ("tile") */
int pp_polish_kernel_times(pp_ctx *ctx, pp_kernel_times *out);
/* Which way the last pp_polish_finish of this context went: 1 = the direct path (the window-order mirror and its run table:
 * pp_aln_batch.wo_run_end -- a rank of a sharded job included: pp_shard_split restricts the table with the mirror), 0 = the
 * bucketing path (no mirror, no run table, more than PP_WO_MAX_RUNS runs -- one per SAM file, or per file and device in the
 * one-process multi-GPU driver --, a
 * mirror that turned out not to be in run order or not to mirror its records, a window that needs more room for its extras
 * than the windows can be given).  The results are the same either way; for reports (bench.py names the kernel it timed). */
int pp_polish_took_direct_path(const pp_ctx *ctx);

/* ---- multi-GPU: contigs (and windows of a large contig) shard across ranks -----------------------------------------
 * The reference is one thread on one CPU; the partition is SURVEY.md 8(e) / BASELINE.json configs[3], [4].
 * A rank polishes the records that reach its units (pp_shard_split picks them out of a batch; giving a rank every
 * record is allowed too) with pp_polish_set_emit(the ranges of its units): the device works on its windows only, and
 * every owned position sees all of its alignments in file order.  The only exchange of the polish itself is
 * pp_polish_gather.
 *   plan    whole contigs by longest-processing-time on their alignment counts; a contig with more than one rank's
 *           share of the alignments is cut into up to `world` windows on 2048-bp boundaries (>= min_window bp each,
 *           0 = 65536), one per rank.  Units are listed contig by contig, windows in position order. */
typedef struct {
    uint32_t n_units, world, n_contigs;
    uint32_t *contig;      /* per unit */
    uint64_t *lo, *hi;     /* [lo, hi) of the contig */
    uint32_t *rank;        /* the rank that polishes it */
} pp_shard_plan;
int pp_shard_plan_create(uint32_t n_contigs, const uint64_t *contig_off, const uint64_t *aln_per_contig, uint32_t world,
                         uint64_t min_window, pp_shard_plan **out);
void pp_shard_plan_free(pp_shard_plan *plan);
/* the ranges one rank emits, as pp_polish_set_emit takes them (arrays of n_contigs; empty range = not its contig) */
int pp_shard_emit_ranges(const pp_shard_plan *plan, uint32_t rank, uint64_t *emit_lo, uint64_t *emit_hi);
/* The ranks' polished bytes back in assembly order (HOST memory): rank_bytes[r] / rank_contig_off[r] are what rank
 * r's pp_polish_result returned (out, contig_out_off); out may be NULL to get the offsets only. */
int pp_shard_assemble(const pp_shard_plan *plan, const uint8_t *const *rank_bytes, const uint64_t *const *rank_contig_off,
                      uint8_t *out, uint64_t *contig_out_off);
/* The records of `batch` (file order) that rank `dest` needs under `plan`: a record goes to the rank of every unit its
 * reference span [ref_start, ref_start + sum of its M/=/X/D/N run lengths) touches -- its contig's owner, or, on a tiled
 * contig, every window it overlaps (src/alignment.rs:297-303, src/pileup.rs:189-200: an alignment only ever touches
 * its own contig's positions ref_start + j).  A record that touches no unit (bad contig index, start beyond the
 * contig's end) goes to one fixed rank, which reports it.  mem = where `batch` lives: PP_MEM_HOST -> the part is host
 * memory (ctx may be NULL), PP_MEM_DEVICE -> the part is made by kernels on ctx's stream and lives on ctx's GPU.
 * The part is a pp_aln_batch of its own (offsets relative to its own seq / cigar arrays); orig[i] is the index of its
 * record i in `batch` (same memory kind as the part): a record number reported by a rank's pp_polish_finish is
 * rank-local, orig turns it back into the job's, and the job's first bad record is the minimum over the ranks.
 * The part's seq array: every record in a room of its SEQ bytes up to the next multiple of PP_SEQ_ALIGN, the rooms one behind
 * the other, zeros behind the read.  The rooms follow the order of `batch`'s seq array, slot by slot of PP_SEQ_ALIGN bytes (a
 * window-grouped batch gives window-grouped parts), when every selected record that has SEQ bytes starts on a slot of its own
 * inside that array -- as in every batch of the library's own producers --, otherwise the order of the records; host and
 * device parts alike.  A record without SEQ bytes takes no room and claims no slot: its seq_off is that of the room of the
 * record that starts in its slot (or, without one, of the next room).
 * The part's window-order mirror is `batch`'s, restricted (with its run table); it counts as one of the library's own only
 * when `batch`'s does: the restriction of a caller's mirror is compared with the arrays by pp_polish_add like the caller's. */
typedef struct pp_shard_part pp_shard_part;
int pp_shard_split(pp_ctx *ctx, const pp_shard_plan *plan, uint32_t dest, const pp_aln_batch *batch, int mem,
                   pp_shard_part **out);
void pp_shard_part_batch(const pp_shard_part *part, pp_aln_batch *out, const uint32_t **orig); /* borrowed views */
int pp_shard_part_mem(const pp_shard_part *part);
void pp_shard_part_free(pp_shard_part *part);
/* Alignment records per contig -- the planner's weights -- ADDED to aln_per_contig (HOST, n_contigs). */
int pp_shard_count(pp_ctx *ctx, const pp_aln_batch *batch, int mem, uint32_t n_contigs, uint64_t *aln_per_contig);
/* The record and the kind of the device error pp_polish_finish last returned on this context (PP_ERR_QUIT / PP_ERR_PANIC
 * from the CIGAR walk): *record = its index over the batches added to THIS context; returns 0 when there was none.
 * pp_polish_error_text writes the message for that kind with another record number (the job-wide one). */
int pp_polish_error_record(const pp_ctx *ctx, uint64_t *record, uint32_t *kind);
int pp_polish_error_text(pp_ctx *ctx, uint32_t kind, uint64_t record);

/* RCCL communicator of one rank (librccl is loaded at run time; the process's own copy is used if it has one):
 * rank 0 calls pp_comm_unique_id, the launcher hands the PP_COMM_ID_BYTES to every rank, every rank calls
 * pp_comm_init on the context of its GPU. */
#define PP_COMM_ID_BYTES 128
int pp_comm_unique_id(void *id);
int pp_comm_init(pp_ctx *ctx, int rank, int world, const void *id);
void pp_comm_destroy(pp_ctx *ctx);
/* After pp_polish_finish, on every rank: the polished bytes of all ranks go to rank 0 (ncclAllGather of the byte
 * counts and per-contig output offsets, then one group of ncclSend / ncclRecv into exclusive-scan offsets).
 * gathered: DEVICE buffer on rank 0 (>= the sum of the counts, `cap` bytes; NULL elsewhere), filled rank by rank;
 * rank_len (world) and rank_contig_off (world x (n_contigs + 1)): HOST, filled on every rank, either may be NULL. */
int pp_polish_gather(pp_ctx *ctx, uint8_t *gathered, uint64_t cap, uint64_t *rank_len, uint64_t *rank_contig_off);

/* ---- seam A: paired-read insert-size filter --------------------------------------------------
 * Alignments of both SAM files as SoA in file order (Alignment::new_quick, src/alignment.rs:
 * 102-128), plus the read-name grouping the reference builds in its HashMap (src/filter.rs:
 * 91-145): reads are numbered 0..n_reads-1; for file f, the alignments of read r are
 * grp_idx[f][grp_off[f][r] .. grp_off[f][r+1]) (indices into file f's arrays, file order). */
typedef struct {
    uint64_t n_aln;
    const uint32_t *ref_id;     /* RNAME interned to an integer (equal names <=> equal ids) */
    const uint32_t *ref_start;  /* POS-1 */
    const uint32_t *flags;      /* FLAG */
    const uint64_t *cig_off;
    const uint32_t *n_cig;
    const uint32_t *cigar;      /* packed runs; ops outside MIDNSHP=X never appear (regex) */
    uint64_t n_cig_total;
    const uint32_t *read;       /* read number of each alignment */
    const uint32_t *grp_off;    /* n_reads+1 */
    const uint32_t *grp_idx;    /* n_aln */
    const uint64_t *ref_end;    /* optional: precomputed get_ref_end per alignment; then cig_off / n_cig / cigar are not read */
} pp_filter_file;

typedef struct {
    uint32_t n_reads;
    pp_filter_file file[2];
} pp_filter_input;

/* Upload (or adopt) the input and compute ref_end for every alignment on the device
 * (Alignment::get_ref_end, src/alignment.rs:138-149). */
int pp_filter_begin(pp_ctx *ctx, const pp_filter_input *in, int mem);
/* For every read with exactly one alignment in each file on the same reference
 * (src/filter.rs:155-167): orientation (0 fr, 1 rf, 2 ff, 3 rr; get_orientation,
 * src/filter.rs:189-209) and insert size (src/filter.rs:212-218).  orient[r] = 255 for reads that
 * are not sampled.  HOST arrays of n_reads. */
int pp_filter_samples(pp_ctx *ctx, uint8_t *orient, uint32_t *insert);
/* alignment_pass_qc (src/filter.rs:352-377) for every alignment of both files; pass1/pass2 are
 * HOST arrays (1 = pass, 0 = append ZP:Z:fail). */
int pp_filter_pairs(pp_ctx *ctx, uint32_t low, uint32_t high, uint8_t orientation,
                    uint8_t *pass1, uint8_t *pass2);
int pp_filter_kernel_times(pp_ctx *ctx, pp_kernel_times *out);

/* Host half of the filter (no device needed): both SAM files -> the pp_filter_input above, and the
 * re-emission of a file with "\tZP:Z:fail" appended where pass == 0.  Multi-threaded; the result does
 * not depend on the thread count.
 *   pp_filter_load    load_alignments, src/filter.rs:91-145 (Alignment::new_quick, src/alignment.rs:102-128):
 *                     file 1 then file 2; counts[f].loaded tells which files were read completely when
 *                     an error is returned ("unable to load", "too few columns ... (line N)", ...)
 *   pp_filter_write   filter_sam, src/filter.rs:309-349: header and unaligned lines verbatim, every line
 *                     ends in "\n"; pass = HOST array over the alignments of file f (0/1) */
typedef struct pp_filter_loaded pp_filter_loaded;
typedef struct {
    uint64_t alignments; /* aligned records in the file        (filter.rs:105) */
    uint64_t reads;      /* distinct QNAMEs among them                          */
    int loaded;
} pp_filter_file_counts;
int pp_filter_load(const char *in1, const char *in2, pp_filter_loaded **out, pp_filter_file_counts counts[2],
                   char *err, size_t errlen);
void pp_filter_loaded_input(const pp_filter_loaded *loaded, pp_filter_input *in); /* borrows from `loaded` */
int pp_filter_write(const pp_filter_loaded *loaded, int file, const uint8_t *pass, const char *out_path,
                    uint64_t *pass_count, uint64_t *fail_count, char *err, size_t errlen);
void pp_filter_loaded_free(pp_filter_loaded *loaded);

/* The same load on the DEVICE: both texts are uploaded; quick parse, get_ref_end, QNAME / RNAME interning
 * (device hash tables) and the per-file group index run as kernels.  pp_filter_dev_input gives the
 * pp_filter_input view in DEVICE memory (ref_end filled in, no CIGAR arrays) for pp_filter_begin(..., PP_MEM_DEVICE);
 * it equals pp_filter_load's result except that RNAME ids are arbitrary.  The host mappings of the two files
 * stay open inside the object (pp_filter_dev_text) for pp_filter_write_text. */
typedef struct pp_filter_dev pp_filter_dev;
int pp_filter_load_device(pp_ctx *ctx, const char *in1, const char *in2, pp_filter_dev **out,
                          pp_filter_file_counts counts[2]);
void pp_filter_dev_input(const pp_filter_dev *loaded, pp_filter_input *in);
const char *pp_filter_dev_text(const pp_filter_dev *loaded, int file, uint64_t *size);
void pp_filter_dev_free(pp_filter_dev *loaded);
/* filter_sam (src/filter.rs:309-349) straight from a SAM text in memory: pass = HOST array over its aligned
 * records (lines that are neither headers nor FLAG & 4), in file order. */
int pp_filter_write_text(const char *text, uint64_t size, const uint8_t *pass, uint64_t n_pass, const char *out_path,
                         uint64_t *pass_count, uint64_t *fail_count, char *err, size_t errlen);

/* ---- host ingest (text -> SoA) -------------------------------------------------------------- */
typedef struct pp_assembly pp_assembly;
/* load_fasta + check_load_fasta (src/misc.rs:38-75): plain or gzip, uppercased. */
int pp_assembly_load(const char *path, pp_assembly **out, char *err, size_t errlen);
void pp_assembly_free(pp_assembly *a);
uint32_t pp_assembly_n_contigs(const pp_assembly *a);
const char *pp_assembly_name(const pp_assembly *a, uint32_t i);
const char *pp_assembly_description(const pp_assembly *a, uint32_t i);
const uint64_t *pp_assembly_offsets(const pp_assembly *a); /* n_contigs+1 */
const uint8_t *pp_assembly_bases(const pp_assembly *a);

/* ---- FASTA text -> contig bases on the device (pp_fasta.hip) ----------------------------------
 * pp_fasta_records is load_fasta_not_gzipped + check_load_fasta (src/misc.rs:102-133, 56-75) exactly as pp_assembly_load restates
 * them, this project's deviations included, for a caller who holds FASTA bytes: text[0, n_bytes) in host memory (PP_MEM_HOST: one
 * staging copy) or in memory of the context's device (PP_MEM_DEVICE: read where it is, at any alignment).  The text is read once;
 * the object owns its output only.  No byte outside [0, n_bytes) is loaded, by a wide load either: a device text may end where its
 * allocation ends, and nothing behind n_bytes can change a result.
 *   lines       end at "\n"; a "\r" directly in front of it is dropped, and so is one that is the text's last byte (as the host
 *               loader's line reader does); any other "\r" is a byte of its line.  A missing final newline is fine; lines that are
 *               empty after that are skipped.
 *   headers     a line whose first byte is '>': name = what lies between '>' and the first Unicode White_Space character (multi-byte
 *               forms included), description = everything behind that one character.  A header with an empty name opens no contig
 *               and is dropped silently when a header or the end of the text follows.
 *   sequence    every other line: its bytes are appended to the open contig, ASCII letters upper-cased, nothing stripped.
 *   refusals    the first offending line in file order wins, whatever its kind; *bad_line (may be NULL) = its 0-based index among all
 *               lines, ~0 where no line is to blame.  PP_ERR_QUIT "... is not correctly formatted": a sequence line with no named
 *               header open.  PP_ERR_QUIT "unable to load ...": a header, or an offending sequence line, that is not valid UTF-8.
 *               PP_ERR_LIMIT: a byte >= 0x80 in a sequence line that is valid UTF-8.  Behind the walk, in this order, PP_ERR_QUIT
 *               "contains no sequences", "has an empty sequence", "has a duplicated name".  The path in every message is `text`.
 *               The device decides which line is refused; the host loader's code then runs on that one line.
 *   arguments   PP_ERR_ARG: null arguments, PP_MEM_PEER, a null text with n_bytes > 0.  PP_ERR_LIMIT: n_bytes >= 2^40.  (The limit of
 *               2^32 - 4096 bases stays with pp_polish_begin.)
 * The device does what is proportional to the text (line ends, line kinds, the bases compacted and upper-cased, the bases in front of
 * every header, the header lines' ranges, the first offending byte); the host what is proportional to the headers.  The context's
 * stream has been synchronised when the call returns.
 *   pp_fasta_bases        the bases of all contigs, one behind the other (DEVICE, borrowed until pp_fasta_free): what
 *                         pp_polish_begin(..., PP_MEM_DEVICE, ...) takes
 *   pp_fasta_offsets      HOST, n_contigs + 1: contig i is bases[off[i], off[i + 1])
 *   pp_fasta_kernel_ms    HIP-event time of the kernels (not of a host text's staging copy); PP_ERR_ARG unless the context had
 *                         profiling on at pp_fasta_records
 * The object belongs to its context and is freed before it. */
typedef struct pp_fasta pp_fasta;
int pp_fasta_records(pp_ctx *ctx, const uint8_t *text, uint64_t n_bytes, int mem, pp_fasta **out, uint64_t *bad_line);
void pp_fasta_bases(const pp_fasta *f, const uint8_t **dev, uint64_t *n_bases); /* DEVICE, borrowed */
uint32_t pp_fasta_n_contigs(const pp_fasta *f);
const uint64_t *pp_fasta_offsets(const pp_fasta *f); /* HOST, n_contigs + 1 */
const char *pp_fasta_name(const pp_fasta *f, uint32_t i);
const char *pp_fasta_description(const pp_fasta *f, uint32_t i);
int pp_fasta_kernel_ms(const pp_fasta *f, float *ms);
void pp_fasta_free(pp_fasta *f);

/* pp_assembly_load through pp_fasta_records: the same pp_assembly (names, descriptions, offsets, index), its bases in device memory.
 * A plain file is mapped and parsed as PP_MEM_HOST; a BGZF file (bgzip) is inflated by pp_bgzf_inflate and parsed from device memory;
 * a gzip file that is not BGZF goes to pp_assembly_load unchanged.  The codes and messages are those of pp_assembly_load on the same
 * file, byte for byte; a HIP failure is PP_ERR_HIP with the context's message.  The object belongs to the context and is freed before
 * it.  pp_assembly_bases_device: the bases in DEVICE memory, NULL for an assembly whose bases are in host memory (pp_assembly_load,
 * the gzip case); pp_assembly_bases on such an object downloads them once, on first use (not from two threads at once). */
int pp_assembly_load_device(pp_ctx *ctx, const char *path, pp_assembly **out, char *err, size_t errlen);
const uint8_t *pp_assembly_bases_device(const pp_assembly *a);

typedef struct pp_ingest pp_ingest;
int pp_ingest_create(const pp_assembly *a, uint32_t max_errors, int careful, pp_ingest **out);
/* add_to_pileup's streaming half (src/alignment.rs:225-272): parse, group adjacent QNAMEs, apply
 * process_one_read's gates, append the good alignments to the batch.  Files in argv order. */
int pp_ingest_sam(pp_ingest *g, const char *path, pp_sam_counts *counts, char *err, size_t errlen);
/* Same, with the filter's verdicts handed over in memory instead of as "ZP:Z:fail" tags in a rewritten
 * file (fused filter -> polish): pass[i] == 0 fails the i-th ALIGNED record of the file (file order, the
 * numbering of pp_filter_file), exactly as if the tag had been appended to its line (src/alignment.rs:72-74).
 * pass == NULL: no verdicts (n_pass is not looked at).  Otherwise n_pass must equal the number of aligned records -- zero
 * verdicts for a file with aligned records included --, or the call ends with PP_ERR_ARG once the text has been found free of
 * defects.  pp_dev_ingest_sam_filtered follows the same rule. */
int pp_ingest_sam_filtered(pp_ingest *g, const char *path, const uint8_t *pass, uint64_t n_pass,
                           pp_sam_counts *counts, char *err, size_t errlen);
void pp_ingest_batch(const pp_ingest *g, pp_aln_batch *out); /* borrowed view, host memory */
/* QNAME of batch record i (for error messages). */
const char *pp_ingest_read_name(const pp_ingest *g, uint64_t i);
void pp_ingest_free(pp_ingest *g);

/* ---- whole-command drivers (what bin/polypolish calls) --------------------------------------- */
typedef struct {
    double fraction_invalid; /* default 0.2  */
    double fraction_valid;   /* default 0.5  */
    uint32_t max_errors;     /* default 10   */
    uint32_t min_depth;      /* default 5    */
    int careful;
    const char *debug_path;  /* NULL = no --debug file */
    int quiet;               /* suppress the stderr log */
} pp_polish_options;

typedef struct {
    uint8_t *data; /* malloc'd by the library, release with pp_bytes_free */
    uint64_t len;
} pp_bytes;
void pp_bytes_free(pp_bytes *b);

/* ---- contig bases -> FASTA text on the device (pp_fasta_out.hip) ------------------------------
 * pp_fasta_text is the mirror of pp_fasta_records and the link in front of pp_bgzf_deflate: the contigs' bytes, where they lie in
 * device memory, as FASTA text at a chosen line width (not in the reference, which prints one line per contig).
 * tests/fasta_text_model.py defines the bytes.
 *   arguments   bases: the contigs' bytes one behind the other, contig c = bases[contig_off[c], contig_off[c + 1]) -- contig_off (HOST,
 *               n_contigs + 1) is what pp_polish_result fills.  mem = PP_MEM_DEVICE: read where they lie, at any alignment (what
 *               pp_polish_result_device returns); PP_MEM_HOST: one staging copy, released before the call returns.  Header c is
 *               headers[header_off[c], header_off[c + 1]) (both HOST): the line without its '>' and without its newline.
 *   the text    for each contig in order '>', the header, "\n", then the body.  width == 0: the contig's bytes and one "\n" (a contig
 *               of no bytes gives an empty line): byte for byte what pp_polish_files returns.  width == W > 0: a contig of L bytes
 *               gives ceil(L / W) lines of W bytes, the last one shorter, each ended by "\n"; L == 0 gives no body line at all.  The
 *               bytes are copied as they are: nothing is upper-cased or checked.
 *   memory      no byte outside bases[contig_off[0], contig_off[n_contigs]) and outside the header bytes is loaded, by a wide load
 *               either: a device array may end where its allocation ends.
 *   errors      all decided on the host before anything is uploaded.  PP_ERR_ARG: null arguments, PP_MEM_PEER, null bases with bytes
 *               to copy, offsets that decrease, a header that holds "\n".  PP_ERR_LIMIT: a text of 2^40 bytes or more, width above
 *               2^31 - 1.  n_contigs == 0 gives an empty text.
 * The host does what is proportional to the contigs (the checks, a table per contig, the .fai rows), the device what is proportional
 * to the text.  The context's stream has been synchronised when the call returns.
 *   pp_fasta_out_bytes      the text (DEVICE, borrowed until pp_fasta_out_free): pp_bgzf_deflate(ctx, dev, n_bytes, PP_MEM_DEVICE, ...)
 *                           makes the bgzipped file, pp_fasta_records reads it back
 *   pp_fasta_out_fai        the text's .fai index (HOST, release with pp_bytes_free): per contig name \t L \t offset \t linebases \t
 *                           linewidth \n -- name = the header up to its first space or tab, offset = the text offset of the contig's
 *                           first base, linebases = min(L, W) (L with W == 0), linewidth = linebases + 1; "0 0" for L == 0
 *   pp_fasta_out_write      as pp_bgzf_out_write: downloads the text in slices and writes it to `path`
 *   pp_fasta_out_kernel_ms  as pp_fasta_kernel_ms
 *   pp_bgzf_out_gzi         the .gzi index of ANY pp_bgzf_out (HOST, release with pp_bytes_free), little-endian: a uint64 count, then
 *                           per block except the first its offset in the file and the uncompressed bytes in front of it (b * 65,280);
 *                           no pair for the EOF block
 * Both indexes follow the published formats (samtools faidx, bgzip -i) as this project reads them; they were not compared with
 * htslib's own files.  The object belongs to its context and is freed before it. */
typedef struct pp_fasta_out pp_fasta_out;
int pp_fasta_text(pp_ctx *ctx, const uint8_t *bases, int mem, uint32_t n_contigs, const uint64_t *contig_off /* HOST, n+1 */,
                  const uint8_t *headers /* HOST */, const uint64_t *header_off /* HOST, n+1 */, uint32_t width, pp_fasta_out **out);
void pp_fasta_out_bytes(const pp_fasta_out *o, const uint8_t **dev, uint64_t *n_bytes); /* DEVICE, borrowed */
int pp_fasta_out_fai(const pp_fasta_out *o, pp_bytes *fai);                             /* the .fai text, HOST */
int pp_fasta_out_write(const pp_fasta_out *o, const char *path);                        /* download in slices, write */
int pp_fasta_out_kernel_ms(const pp_fasta_out *o, float *ms);
void pp_fasta_out_free(pp_fasta_out *o);
int pp_bgzf_out_gzi(const pp_bgzf_out *z, pp_bytes *gzi); /* the .gzi of any pp_bgzf_out, HOST */

/* The .bai of the file that pp_bam_tagged_head (or pp_bam_tagged, with n_head = records_at) makes of the same bytes, rec_off, mem and
 * pass, made on the device; the records must stand in coordinate order (pp_bam_sorted_rec_off, pp_bam_sorted_pass).
 *   offsets      record r starts in the stream at n_head + the sum over q < r of 4 + block_size_q + 8 fail_q; a stream offset u is the
 *                virtual offset blk_off[u / 65,280] << 16 | u % 65,280.  blk_off[0, n_blk] (n_blk + 1 entries, HOST or DEVICE by
 *                blk_mem): pp_bgzf_out_blk_off for the compressed file, b * 65,311 for the level-0 file; n_blk must be the stream's
 *                number of blocks.  A record's end at a multiple of 65,280 is the start of the next block, offset 0: a reader's tell.
 *   per record   beg = pos, end = pos + the lengths of its M D N = X runs, pos + 1 where that is 0 or the record is unmapped but
 *                placed; bin = reg2bin(beg, end) of the SAM specification, section 5.3.
 *   chunks       one per maximal run of consecutive records with one (ref_id, bin), from its first record's start to its last
 *                record's end; a bin's chunks in file order, a reference's bins in ascending number.  No merging of small bins into
 *                parents or of neighbouring chunks: a valid BAI, not `samtools index`'s bytes.
 *   linear       ioffset[w] = the smallest start of a record overlapping window w (16,384 bases); n_intv = the last touched window
 *                + 1; an untouched window takes the value of the next touched one.
 *   pseudo-bin   37450 for every reference with records: {first record's start, last record's end}, {mapped, unmapped}; a
 *                reference without records has n_bin = 0, n_intv = 0.  The trailing n_no_coor counts the records with ref_id == -1.
 *   refusals     PP_ERR_ARG with *bad_record = the first such record in index order: pp_bam_tagged's three; a CIGAR that runs past
 *                its block_size; then (n_pass first, as pp_bam_tagged) ref_id outside [-1, n_ref), ref_id >= 0 with pos < 0, a
 *                record in front of its predecessor by (unsigned ref_id, pos; unplaced records are in order whatever their pos).
 *                PP_ERR_LIMIT: end > 2^29 (*bad_record; BAI holds positions below 2^29, CSI is not written), a blk_off >= 2^48,
 *                pp_bam_tagged's limits, more than 2^24 references, more than 2^27 windows in the linear index.  Also PP_ERR_ARG:
 *                null arguments, PP_MEM_PEER, n_blk other than the stream's blocks.
 * *bai is HOST memory: release with pp_bytes_free.  tests/bam_sort_model.py defines the bytes. */
int pp_bam_index(pp_ctx *ctx, const uint8_t *bytes, uint64_t n_bytes, uint64_t n_head, const uint64_t *rec_off, uint64_t n_rec,
                 int mem, const uint8_t *pass, uint64_t n_pass, uint32_t n_ref,
                 const uint64_t *blk_off, uint64_t n_blk, int blk_mem, pp_bytes *bai, uint64_t *bad_record);

/* ---- the .tbi of a bgzipped, position-sorted, tab-separated text, made on the device (pp_tabix.hip) ----------------------------
 * pp_tabix_index indexes the file that pp_bgzf_deflate makes of `text`, so that tabix, bcftools, IGV and JBrowse can fetch a region
 * from it: the polish's VCF, BED and bedGraph (pp_vcf_out_bytes, pp_bed_out_bytes, pp_depth_out_bytes), or any caller's own text.
 * tests/tabix_model.py is the executable form of what follows.
 *   arguments    text[0, n_bytes): the UNCOMPRESSED text.  mem = PP_MEM_HOST: uploaded; PP_MEM_DEVICE: read in place, at any alignment,
 *                and no byte outside [0, n_bytes) is loaded, by a wide load either: the text may end where its allocation ends.
 *                blk_off[0, n_blk] (HOST or DEVICE by blk_mem): pp_bgzf_out_blk_off of the file pp_bgzf_deflate makes of the same
 *                text (b * 65,311 for a level-0 file); n_blk must be ceil(n_bytes / 65,280).
 *   lines        the text is cut at every '\n'; last bytes without a '\n' are a line too.  A line whose first byte is '#' is a meta
 *                line: skipped, not counted.  Every other line is a data line.  *bad_line is a 0-based line number of the text that
 *                counts every line, meta lines included.
 *   columns      column 1, up to the first tab, is the name: at least one byte, taken verbatim.  PP_TBX_BED: columns 2 and 3 are beg
 *                and end, each 1 to 10 decimal digits; column 3 ends at a tab or at the line's end.  PP_TBX_VCF: column 2 is POS (1 to
 *                10 digits, at least 1), beg = POS - 1, end = beg + the byte length of column 4 (REF), which is at least 1 and must be
 *                closed by a tab.  INFO/END= is NOT read (pp_polish_vcf always writes '.' there): for a foreign VCF with END= this
 *                differs from tabix, which takes the record's end from it.  In both presets end == beg counts as [beg, beg + 1), as
 *                pp_bam_index does for a record without a span.
 *   names        the distinct names in the order of their first line are the name list, each closed by a NUL; l_nm is the sum of
 *                their lengths with the NULs.  A contig without a line is not listed, as in tabix.  The lines of one name must be
 *                consecutive, and beg must not decrease inside a name.
 *   offsets      a line starts at its first byte's stream offset and ends behind its '\n' (at n_bytes without one).  A stream offset
 *                u is the virtual offset blk_off[u / 65,280] << 16 | u % 65,280, as in pp_bam_index: an end at a multiple of 65,280
 *                is the next block's offset 0, and blk_off[n_blk] is the EOF block's.
 *   tables       pp_bam_index's, with the name's index as the reference id: bin = reg2bin(beg, end); one chunk per maximal run of
 *                consecutive lines with one (name, bin) -- a meta line between two data lines ends the run -- from its first line's
 *                start to its last line's end; a bin's chunks in file order, a name's bins in ascending number, nothing merged; the
 *                linear index over 16,384-base windows holds the smallest start of an overlapping line, an untouched window the next
 *                touched one's; the pseudo-bin 37450 is {first line's start, last line's end}, {lines, 0}; the trailing n_no_coor
 *                is 0.  The result is a valid .tbi, not tabix's bytes (tabix merges small bins and neighbouring chunks), the choice
 *                pp_bam_index made for the .bai.
 *   *raw         "TBI\1", then the int32 fields n_ref, format, col_seq, col_beg, col_end, meta = 35, skip = 0, l_nm and the names;
 *                per name n_bin, the bins {bin, n_chunk, chunks}, n_intv, ioff[]; then the uint64 n_no_coor.  PP_TBX_VCF: format 2,
 *                col_seq 1, col_beg 2, col_end 0; PP_TBX_BED: format 0x10000, col_seq 1, col_beg 2, col_end 3.  A text without a data
 *                line has n_ref = 0 and l_nm = 0.  raw may be NULL.
 *   *tbi         the same index as a BGZF file -- pp_bgzf_deflate of the raw bytes, EOF block included: the bytes of "<file>.tbi".
 *   refusals     *bad_line = the first offender in line order.  PP_ERR_ARG: a null argument, PP_MEM_PEER, an unknown preset, n_blk
 *                other than the stream's blocks; an empty data line, an empty name, a missing column, a number that is empty, holds
 *                a non-digit or has more than 10 digits, POS 0, an empty REF, end < beg, beg below the beg of the line before it in
 *                the same name, a name that comes back after another name (at the line where it comes back).  PP_ERR_LIMIT:
 *                end > 2^29 (*bad_line; CSI is not written), a blk_off >= 2^48, n_bytes >= 2^40, more than 2^32 - 2 lines (meta
 *                lines counted), more than 2^24 names, l_nm >= 2^31, more than 2^27 windows in the linear index.
 * One lane parses a line whose columns are closed inside its first PP_TBX_LANE_BYTES bytes; a line with a longer name, ID or REF is
 * parsed by a workgroup.  The bytes do not depend on which of the two took a line.  *tbi and *raw are HOST memory: release with
 * pp_bytes_free.  The context's stream has been synchronised when the call returns. */
#define PP_TBX_VCF 0 /* format 2,       col_seq 1, col_beg 2, col_end 0, meta '#', skip 0 */
#define PP_TBX_BED 1 /* format 0x10000, col_seq 1, col_beg 2, col_end 3, meta '#', skip 0 (bedGraph too) */
#define PP_TBX_LANE_BYTES 64
int pp_tabix_index(pp_ctx *ctx, const uint8_t *text, uint64_t n_bytes, int mem, int preset, const uint64_t *blk_off, uint64_t n_blk,
                   int blk_mem, pp_bytes *tbi, pp_bytes *raw /* may be NULL */, uint64_t *bad_line);

/* Coordinate-sorted BAM for the file drivers below (the commands' --regroup): with `on` != 0, pp_polish_files and the polish half of
 * pp_filter_polish_files put pp_batch_regroup between the decode and the gate of every BAM file, so that a read's records count as
 * one read wherever they lie in the file (the filter joins them already, and writes in file order).  The state lives on the
 * context, like pp_ctx_set_profiling's; off when the context is made.  Messages still name the file's own 1-based record.  With it
 * on, SAM text is refused (PP_ERR_QUIT, "--regroup takes BAM input"), and a QUIT or PANIC of the decode (missing or negative NM) is
 * reported at once, without the replay of the records in front.  Without it every command behaves as
 * before: there is no switch on an @HD SO:coordinate header. */
int pp_ctx_set_regroup(pp_ctx *ctx, int on);

/* Compressed BAM outputs from SAM text for the filter drivers below (the commands' --out_bam; not in the reference): with `on` != 0,
 * pp_filter_files and pp_filter_polish_files with outputs named write, for two SAM TEXT inputs, every line again as a BAM record
 * instead of as text: per file pp_sam_bam on the text the run holds in host memory, pp_bam_tagged with the filter's own verdicts,
 * pp_bam_out_deflate, pp_bgzf_out_write.  Both files are encoded before either output is created: a line pp_sam_bam refuses ends the
 * call with PP_ERR_QUIT (also where pp_sam_bam says PP_ERR_LIMIT or PP_ERR_NOT_ASCII) and leaves nothing behind; the message names the
 * input's path, the 1-based line and --out_bam.  The counts, the log and the FASTA are what they are without it.  It changes nothing
 * for BAM inputs (they write BAM already) and for pp_filter_polish_files without outputs.  The state lives on the context, like
 * pp_ctx_set_regroup's; off when the context is made. */
int pp_ctx_set_out_bam(pp_ctx *ctx, int on);

/* Its mirror, SAM text outputs from BAM for the same drivers (the commands' --out_sam; not in the reference): with `on` != 0,
 * pp_filter_files and pp_filter_polish_files with outputs named write, for two BAM inputs, every record as a line of SAM text instead
 * of as a BAM record: per file pp_bam_sam on the bytes the run holds with the filter's own verdicts, then pp_sam_out_write.  Both
 * files are decoded before either output is created: a record pp_bam_sam refuses ends the call with PP_ERR_QUIT and leaves nothing
 * behind; the message names the input's path, the 1-based record and --out_sam.  The counts, the log and the FASTA are what they are
 * without it.  It changes nothing for SAM text inputs (they write text already) and for pp_filter_polish_files without outputs; with
 * pp_ctx_set_out_bam on as well, each flag speaks to its own kind of input.  Off when the context is made. */
int pp_ctx_set_out_sam(pp_ctx *ctx, int on);

/* SAM text through the record chain for the file drivers below (the commands' --text_chain; not in the reference): with `on` != 0,
 * SAM text inputs of pp_polish_files, pp_filter_files and pp_filter_polish_files take the route BAM takes, file by file on one
 * context: (pp_bgzf_inflate, for bgzipped text ->) pp_sam_records -> pp_names_ids twice (RNAME on the table seeded with the FASTA
 * names, QNAME) -> (pp_filter_records) -> (pp_batch_regroup, with pp_ctx_set_regroup) -> pp_batch_gate(pass = pp_sam_pass, ANDed with
 * the filter's verdicts in the fused command) -> (pp_batch_prepare, PP_BAM_PREPARE=1) -> pp_polish_add.  The raw records exist on this
 * route, so pp_ctx_set_regroup is accepted on text (coordinate-sorted SAM), bgzipped text is read (pp_aln_file_kind_text; the filter's
 * outputs are then bgzipped text as well: pp_sam_tagged_records -> pp_bgzf_deflate) and pp_ctx_set_out_bam encodes from the decoded
 * object (pp_sam_bam_records: no second upload).  The log, the counts and the FASTA are those of the run without it on any text that
 * run accepts.  Messages name the input's path and the file's own 1-based line, "<path>" (line N), counting all lines; their order is
 * the BAM route's (the replay of the lines in front of a refused one; under regrouping the decode's refusal
 * at once).  Refused by name with PP_ERR_QUIT: more than one context, a mix of text and BAM, gzip that is not BGZF, an empty line for
 * the filter, and a byte >= 0x80 in a bgzipped file or under regrouping -- a plain text file without regrouping continues on the
 * fused route (PP_TIMING=1 says so).  pp_sam_records' limits stand (PP_ERR_LIMIT), and the filter looks at NM as on the BAM route.
 * Off when the context is made and off by default in the commands: the fused routes are the measured default, and what they refuse
 * is pinned by tests. */
int pp_ctx_set_text_chain(pp_ctx *ctx, int on);

/* Sorted, indexed BAM from the filter drivers below (the commands' --sort_out and --out_bai): with `on` != 0 every BAM output of
 * pp_filter_files and pp_filter_polish_files -- BAM inputs, or SAM text inputs with pp_ctx_set_out_bam -- is written in coordinate
 * order behind the header that says SO:coordinate (pp_bam_sort -> pp_bam_sorted_pass -> pp_bam_tagged_head -> pp_bam_out_deflate), and
 * with `index` != 0 "<output>.bai" (pp_bam_index) next to each.  Both files and both indexes are complete before any output is
 * created: a record that the sort or the index refuses ("--sort_out: ..." with the input's path and the record, PP_ERR_QUIT) leaves
 * nothing behind.  That holds for refusals only: the four files are then written one after the other, and a write that fails
 * (PP_ERR_QUIT "unable to write alignments to ...") leaves the files written before it on disk.  The log and, for pp_filter_polish_files, the FASTA are the plain run's: the polish half takes the records it holds,
 * whatever the order of the outputs.  Outputs that are SAM text -- the text routes without pp_ctx_set_out_bam, BAM inputs with
 * pp_ctx_set_out_sam -- are refused by name (PP_ERR_QUIT) before an input is read.  index != 0 with on == 0: PP_ERR_ARG.  Off by
 * default: without it the drivers run the code they ran. */
int pp_ctx_set_sort_out(pp_ctx *ctx, int on, int index);

/* The form of the polished FASTA that the file drivers below return (the commands' --wrap, --out_bgzf, --out, --index; not in the
 * reference): with width >= 0 the pp_bytes of pp_polish_files, pp_polish_files_multi and pp_filter_polish_files are made by
 * pp_fasta_text at that line width (0: one line per contig, today's bytes), and with bgzf != 0 they are that text compressed by
 * pp_bgzf_deflate on the device bytes.  On one context the source is the polished bytes in device memory; on several contexts it is the
 * host bytes the ranks' results were assembled into (PP_MEM_HOST), so no route is refused.  width < 0 switches the form off: the
 * drivers then run exactly the code they ran before (bgzf is ignored).  PP_ERR_LIMIT: a width above 2^31 - 1.  The log does not
 * change.  The state lives on the context, like pp_ctx_set_out_bam's; off when the context is made.
 * pp_ctx_fasta_index: the indexes of the last text a driver made on this context with the form set -- the .fai of pp_fasta_out_fai,
 * and with bgzf the .gzi of pp_bgzf_out_gzi (else empty); either argument may be NULL; release with pp_bytes_free.  PP_ERR_ARG when
 * no such text was made. */
int pp_ctx_set_fasta_form(pp_ctx *ctx, int64_t width, int bgzf);
int pp_ctx_fasta_index(pp_ctx *ctx, pp_bytes *fai, pp_bytes *gzi);

/* The polish's edits as a VCF file next to the FASTA (the commands' --vcf, --vcf_bgzf; not in the reference): with on != 0
 * pp_polish_files, pp_filter_polish_files and pp_polish_files_multi on ONE context run pp_polish_vcf behind their polish, on every
 * input route, and with bgzf != 0 pass the device text through pp_bgzf_deflate.  The file's bytes stay with the context:
 * pp_ctx_vcf returns the file of the last such run that succeeded (HOST, release with pp_bytes_free; PP_ERR_ARG when there is none --
 * a run that begins drops the file of the run before, a run that fails leaves none).  Several contexts are refused by name
 * (PP_ERR_QUIT "--vcf runs on one GPU ...") before any input is looked at.  The FASTA, the log and every other output are the plain
 * run's, byte for byte.  The state lives on the context, like pp_ctx_set_fasta_form's; off when the context is made. */
int pp_ctx_set_vcf(pp_ctx *ctx, int on, int bgzf);
int pp_ctx_vcf(pp_ctx *ctx, pp_bytes *vcf);

/* The undecided regions as a BED file next to the FASTA, and the FASTA soft-masked (the commands' --bed, --bed_bgzf, --soft_mask,
 * --bed_status; not in the reference).  With pp_ctx_set_bed(on != 0) pp_polish_files, pp_filter_polish_files and
 * pp_polish_files_multi on ONE context keep the job's per-position status (as for a --debug file; no TSV is written unless the
 * options ask for one), run pp_polish_bed with status_mask behind their polish, on every input route, and with bgzf != 0 pass the
 * device text through pp_bgzf_deflate; pp_ctx_bed returns the file of the last such run that succeeded (HOST, release with
 * pp_bytes_free; PP_ERR_ARG when there is none -- a run that begins drops the file of the run before, a run that fails leaves none).
 * With pp_ctx_set_soft_mask(status_mask != 0) the FASTA's sequence bytes come from pp_polish_masked in every form (plain, wrapped,
 * bgzipped, indexed); headers, the log and a VCF of the same run are the plain run's, byte for byte; 0 switches it off.  Several
 * contexts are refused by name (PP_ERR_QUIT "--bed runs on one GPU ...", "--soft_mask runs on one GPU ...") before any input is
 * looked at.  PP_ERR_ARG: a mask of 0 with on != 0, a mask with a bit above 5.  The state lives on the context; off when it is made. */
int pp_ctx_set_bed(pp_ctx *ctx, int on, uint32_t status_mask, int bgzf);
int pp_ctx_bed(pp_ctx *ctx, pp_bytes *bed);
int pp_ctx_set_soft_mask(pp_ctx *ctx, uint32_t status_mask);   /* 0 = off */

/* The read depth as a bedGraph file next to the FASTA (the commands' --depth, --depth_bin, --depth_bgzf; not in the reference).  With
 * pp_ctx_set_depth(on != 0) pp_polish_files, pp_filter_polish_files and pp_polish_files_multi on ONE context keep the job's
 * per-position records (as for a --debug file; no TSV is written unless the options ask for one), run pp_polish_depth with `bin`
 * behind their polish, on every input route, and with bgzf != 0 pass the device text through pp_bgzf_deflate; pp_ctx_depth returns the
 * file of the last such run that succeeded (HOST, release with pp_bytes_free; PP_ERR_ARG when there is none -- a run that begins drops
 * the file of the run before, a run that fails leaves none).  The FASTA, the log and every other output are the plain run's, byte for
 * byte.  Several contexts are refused by name (PP_ERR_QUIT "--depth runs on one GPU ...") before any input is looked at.  PP_ERR_ARG:
 * bin > 2^24 with on != 0.  The state lives on the context; off when it is made. */
int pp_ctx_set_depth(pp_ctx *ctx, int on, uint32_t bin, int bgzf);
int pp_ctx_depth(pp_ctx *ctx, pp_bytes *depth);

/* The .tbi next to the bgzipped tracks (the commands' --vcf_tbi, --bed_tbi, --depth_tbi; not in the reference).  With
 * pp_ctx_set_tbi(vcf, bed, depth) the file drivers above run pp_tabix_index behind pp_bgzf_deflate on the device text of each track
 * whose flag is not 0, with the text and the block table where they lie in device memory; pp_ctx_tbi(which) returns the index of the
 * last such run that succeeded (HOST, release with pp_bytes_free; PP_ERR_ARG when there is none, or for an unknown `which` -- a run
 * that begins drops the indexes of the run before, a run that fails leaves none).  An index is made of a bgzipped track: a run with
 * an index on whose track is off or not compressed (pp_ctx_set_vcf / _bed / _depth with bgzf != 0) is refused with PP_ERR_ARG before
 * any input is looked at; several contexts are refused by the track's own name.  The tracks, the FASTA and the log's text are the
 * run's without it.  The state lives on the context; off when it is made. */
#define PP_TBI_VCF 0
#define PP_TBI_BED 1
#define PP_TBI_DEPTH 2
int pp_ctx_set_tbi(pp_ctx *ctx, int vcf, int bed, int depth);
int pp_ctx_tbi(pp_ctx *ctx, int which, pp_bytes *tbi);

/* polish::polish (src/polish.rs:26-38): FASTA text exactly as the reference prints to stdout.
 * `sams` are SAM text files or -- all of them -- BAM files (pp_aln_file_kind; a mix is PP_ERR_QUIT).  BAM goes through the record
 * chain on the device, file by file: pp_bgzf_inflate -> pp_bam_header -> pp_bgzf_bam_walk -> pp_bam_records -> pp_names ->
 * (pp_batch_regroup, with pp_ctx_set_regroup ->) pp_batch_gate(pass = pp_bam_pass) -> pp_polish_add; pp_batch_prepare in between
 * with PP_BAM_PREPARE=1 in the environment.  SAM text takes the fused routes, or with pp_ctx_set_text_chain the same chain behind
 * pp_sam_records (messages then name the path and the 1-based line).
 * Messages about a BAM file name its path and the block or the record (1-based, counting all records); "no alignments in <path>"
 * for a file without aligned records.  Order of errors: INTEGRATION.md section 6. */
int pp_polish_files(pp_ctx *ctx, const char *assembly, const char *const *sams, int n_sams,
                    const pp_polish_options *opt, pp_bytes *fasta);

/* polish::polish on SEVERAL GPUs from one process: the host ingest runs once, every context (one per device, see
 * pp_ctx_create) gets the full batches and the emit ranges of its units (pp_shard_plan_create), the contexts polish
 * side by side and the FASTA is assembled on the host.  Same bytes as pp_polish_files; --debug is not available.
 * The error text is on ctxs[0].  BAM input runs on one GPU: with n_ctx > 1 it is refused (PP_ERR_QUIT). */
int pp_polish_files_multi(pp_ctx *const *ctxs, int n_ctx, const char *assembly, const char *const *sams, int n_sams,
                          const pp_polish_options *opt, pp_bytes *fasta);

/* The same ingest on the DEVICE: the raw SAM text is uploaded and tokenized by kernels
 * (newline index, field split, number / CIGAR / tag validation, contig lookup, read groups, gates, 1/k,
 * "*" fill, upper-casing, CIGAR packing).  The batch is bit-identical to pp_ingest_sam's and lives in HBM:
 * hand it to pp_polish_add with PP_MEM_DEVICE and keep the object alive until pp_polish_finish.  Errors
 * (same codes and messages as the host ingest) are reported through pp_last_error(ctx). */
typedef struct pp_dev_ingest pp_dev_ingest;
int pp_dev_ingest_create(pp_ctx *ctx, const pp_assembly *a, uint32_t max_errors, int careful, pp_dev_ingest **out);
int pp_dev_ingest_sam(pp_dev_ingest *g, const char *path, pp_sam_counts *counts);
/* with the filter's verdicts, as pp_ingest_sam_filtered (pass: HOST array over the file's aligned records) */
int pp_dev_ingest_sam_filtered(pp_dev_ingest *g, const char *path, const uint8_t *pass, uint64_t n_pass,
                               pp_sam_counts *counts);
/* How the batch's SEQ bytes are laid out (seq_off may point anywhere, so this is the producer's choice, not a format):
 * PP_SEQ_WINDOW_GROUPED (the default since round 4) = the reads that start in one 2048-position window of the assembly are
 * adjacent (per SAM file; inside a window in no particular order) -- the pileup kernel then fetches a window's reads from
 * one stretch of memory instead of all over the array; PP_SEQ_FILE_ORDER = in the order of the records.  The window layout
 * costs the tokenizer a count / scan / placement pass over eight bytes per record (no second look at the text or the parse
 * records).  Every other array, the order of the records and every result are the same.  Set before the first
 * pp_dev_ingest_sam* / pp_ingest_sam*; `PP_SEQ_LAYOUT=file` in the environment selects file order for the file drivers.
 * Both ingests write the same layout (the host ingest in file order inside a window); the device tokenizer's batch also
 * brings the 4-bit mirror of its seq array (pp_aln_batch.seq4; `PP_SEQ4=0`: none). */
#define PP_SEQ_FILE_ORDER 0
#define PP_SEQ_WINDOW_GROUPED 1
int pp_dev_ingest_set_seq_layout(pp_dev_ingest *g, int layout);
int pp_ingest_set_seq_layout(pp_ingest *g, int layout);
/* Optional hint, before the first file: the bytes of SAM text of ALL the files that will be handed to this ingest.  The
 * batch's arrays are then sized once, for all of them, off the first file (without it the second file makes every array
 * grow: a device allocation and a copy of what the first one filled -- 6 ms on a 2 x 1.2 GB pair). */
int pp_dev_ingest_expect(pp_dev_ingest *g, uint64_t total_text_bytes);
void pp_dev_ingest_batch(const pp_dev_ingest *g, pp_aln_batch *out); /* borrowed view, DEVICE memory */
void pp_dev_ingest_free(pp_dev_ingest *g);

typedef struct {
    uint64_t before_count, after_count;
    uint32_t low_threshold, high_threshold;
    int orientation; /* 0 fr 1 rf 2 ff 3 rr */
    uint64_t orientation_counts[4];
} pp_filter_report;
/* After pp_filter_begin: the rest of get_insert_size_thresholds (src/filter.rs:168-186, 221-259) on the samples the pass over
 * the reads left in device memory -- pp_filter_samples's arrays never travel.  Runs that pass if it has not run yet (as
 * pp_filter_pairs does), then, on the device: the four orientation counts; the correct orientation -- "auto": the unique
 * maximum, any other string is looked up in fr / rf / ff / rr (an unknown one has no sizes, as in the reference) --; the two
 * nearest-rank percentiles (rank = max(ceil(p / 100 * n) as usize, 1), computed on the host in double) of the insert sizes of
 * that orientation, by an exact selection over all 32 bits.  Fills orientation_counts, orientation, low_threshold,
 * high_threshold and before_count (the two files' n_aln); after_count stays 0.  Hand low_threshold / high_threshold /
 * orientation to pp_filter_pairs.  Errors, in the reference's order: PP_ERR_QUIT "--low must be greater than 0 and less
 * than 50" / "--high must be greater than 50 and less than 100"; PP_ERR_PANIC where the sampling loop needs an end that cannot
 * be parsed (as pp_filter_samples); PP_ERR_QUIT "no one-alignment-per-read pairs available to determine orientation and insert
 * size thresholds", "could not automatically determine read pair orientation" (a tie), "no read pairs available to determine
 * insert size thresholds".  The counts known so far are in `report` when one of the last three is returned.
 * pp_filter_kernel_times names its kernels "thr_count" and "thr_select". */
int pp_filter_thresholds(pp_ctx *ctx, const char *orientation, double low, double high, pp_filter_report *report);

/* filter::filter (src/filter.rs:26-37) between loading and writing, over the RAW records of the two SAM files: the first link
 * of the record chain filter -> gate -> prepare -> polish.  raw[f] is the pp_raw_batch that pp_batch_gate takes next (the caller
 * builds its arrays once); read here: flag, read_id, contig, ref_start, cig_off, n_cig, cigar -- nm and seq* are not looked at
 * and may be NULL.  mem = PP_MEM_HOST or PP_MEM_DEVICE (both batches).
 *   aligned records   a record with flag & 4 takes part in nothing; the others are numbered in file order -- the numbering of
 *                     pp_filter_file and of pass[] in pp_batch_gate / pp_ingest_sam_filtered.  pass1 / pass2: HOST arrays over
 *                     the aligned records of file 1 / file 2 (1 = pass), exactly what pp_batch_gate takes (may be NULL for a
 *                     file without aligned records)
 *   reads             ALL aligned records of the two files with equal read_id are one read, adjacent or not (the reference's
 *                     HashMap; the gate joins adjacent records only); a read's records keep file order.  Any 64-bit value is an
 *                     id: none is reserved
 *   contig            the RNAME as an id, compared for EQUALITY only and not range-checked.  This differs from the gate's use:
 *                     records whose RNAME is not in the assembly must carry DISTINCT ids per name (a BAM refID, or any value
 *                     >= n_contigs) -- not one shared "no contig" value, or two unknown references compare equal where the
 *                     reference compares their names
 *   CIGAR             a record with a run of op PP_OP_UNPARSEABLE has the end PP_REF_END_UNPARSEABLE: fatal (PP_ERR_PANIC) only
 *                     when a pair comparison needs it, as in pp_filter_file.  n_cig == 0: ref_end = ref_start
 *   counts[f]         the aligned records of file f and the distinct ids among them (may be NULL): the context never sees a
 *                     path, so the "N alignments from M reads" line is the caller's to print
 *   report            complete (may be NULL); after_count = the 1s of the two pass arrays
 * PP_ERR_ARG: null arguments, PP_MEM_PEER, a null array in a non-empty batch, a CIGAR range of an aligned record outside the cigar
 * array (found on the device before anything is read through it).  PP_ERR_LIMIT: 2^32-1 or more records in a file, or aligned
 * records in the two files together.  PP_ERR_QUIT "no alignments found in file 1": file 1 has no aligned record (the reference
 * names the path; the caller has it).  Everything after that comes from pp_filter_thresholds and pp_filter_pairs.  The
 * context's stream is synchronised on return: `raw` may be released; the context's filter job is closed (pp_filter_begin
 * starts the next).  pp_filter_kernel_times also names the grouping kernels: "rec_compact", "rec_intern", "rec_groups". */
int pp_filter_records(pp_ctx *ctx, const pp_raw_batch raw[2], int mem, const char *orientation, double low, double high,
                      uint8_t *pass1, uint8_t *pass2, pp_filter_file_counts counts[2], pp_filter_report *report);

/* filter::filter (src/filter.rs:26-37).  in1 / in2 are both SAM text or both BAM (pp_aln_file_kind; one of each is PP_ERR_QUIT).
 * BAM in, compressed BAM out: two front ends, one QNAME table for both files, pp_filter_records, then per file pp_bam_tagged(pass =
 * the filter's own verdict) -> pp_bam_out_deflate -> pp_bgzf_out_write.  The log is the text route's.  An aligned BAM record without
 * NM is refused here too, because pp_bam_records refuses it (the text route never looks at NM). */
int pp_filter_files(pp_ctx *ctx, const char *in1, const char *in2, const char *out1,
                    const char *out2, const char *orientation, double low, double high, int quiet,
                    pp_filter_report *report);

/* filter + polish in one process: the filter's verdicts go straight into the polish ingest,
 * the tagged SAMs are written only if out1/out2 are given (both or neither).  The FASTA is byte-identical
 * to `filter` followed by `polish` on its outputs.  Two BAM inputs are decoded once: the filter's verdicts ANDed with pp_bam_pass go
 * into pp_batch_gate, and out1 / out2 are BAM files, those of pp_filter_files. */
int pp_filter_polish_files(pp_ctx *ctx, const char *assembly, const char *in1, const char *in2,
                           const char *out1, const char *out2, const char *orientation, double low, double high,
                           const pp_polish_options *opt, pp_filter_report *report, pp_bytes *fasta);

#ifdef __cplusplus
}
#endif
#endif
