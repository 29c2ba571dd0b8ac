"""The C ABI of libpolypolish_hip.so as ctypes sees it: the structures of include/polypolish_hip.h and the ONE place a symbol's
signature is written -- SIGNATURES (every symbol the header declares, in its order) and HOOKS (the internal `pp_*_` hooks the
Python side uses).  polypolish_amd.lib() applies both tables; tests/test_binding_cpu.py holds SIGNATURES against the header."""
import ctypes as C


class Params(C.Structure):
    _fields_ = [("min_depth", C.c_uint32), ("fraction_valid", C.c_double), ("fraction_invalid", C.c_double)]


class AlnBatch(C.Structure):
    _fields_ = [("n_aln", C.c_uint64), ("contig", C.c_void_p), ("ref_start", C.c_void_p), ("k", C.c_void_p),
                ("seq_off", C.c_void_p), ("seq_len", C.c_void_p), ("cig_off", C.c_void_p), ("n_cig", C.c_void_p),
                ("seq", C.c_void_p), ("seq_bytes", C.c_uint64), ("cigar", C.c_void_p), ("n_cig_total", C.c_uint64),
                ("seq4", C.c_void_p),  # optional 4-bit mirror of seq (include/polypolish_hip.h); None = none
                ("wo", C.c_void_p),    # optional window-order mirror of the records (pp_wo_rec[n_aln]); None = none
                ("wo_n_runs", C.c_uint32), ("wo_run_end", C.c_void_p)]  # optional: the mirror's runs (HOST array of u64 ends)


class RawBatch(C.Structure):
    """pp_raw_batch: the alignment records of one SAM file as Alignment::new leaves them (include/polypolish_hip.h)"""
    _fields_ = [("n_rec", C.c_uint64), ("flag", C.c_void_p), ("read_id", C.c_void_p), ("contig", C.c_void_p),
                ("ref_start", C.c_void_p), ("nm", C.c_void_p), ("seq_off", C.c_void_p), ("seq_len", C.c_void_p),
                ("cig_off", C.c_void_p), ("n_cig", C.c_void_p), ("seq", C.c_void_p), ("seq_bytes", C.c_uint64),
                ("cigar", C.c_void_p), ("n_cig_total", C.c_uint64)]


class ContigStats(C.Structure):
    _fields_ = [("polished_len", C.c_uint64), ("changed", C.c_uint64), ("zero_depth", C.c_uint64),
                ("depth_sum", C.c_double)]


class PositionsOut(C.Structure):
    _fields_ = [("depth", C.c_void_p), ("count_a", C.c_void_p), ("count_c", C.c_void_p), ("count_g", C.c_void_p),
                ("count_t", C.c_void_p), ("count_other", C.c_void_p), ("valid_thr", C.c_void_p),
                ("invalid_thr", C.c_void_p), ("status", C.c_void_p)]


PP_MAX_KERNELS = 16


class KernelTimes(C.Structure):
    _fields_ = [("n", C.c_int), ("name", C.c_char_p * PP_MAX_KERNELS), ("ms", C.c_float * PP_MAX_KERNELS),
                ("n_entries", C.c_uint64), ("n_flagged", C.c_uint64), ("n_passes", C.c_uint64)]

    def as_dict(self):
        d = {self.name[i].decode(): float(self.ms[i]) for i in range(self.n)}
        return {"ms": d, "n_entries": int(self.n_entries), "n_flagged": int(self.n_flagged),
                "n_passes": int(self.n_passes)}


class SamCounts(C.Structure):
    _fields_ = [("alignments", C.c_uint64), ("used", C.c_uint64), ("reads", C.c_uint64)]


class PolishOptions(C.Structure):
    _fields_ = [("fraction_invalid", C.c_double), ("fraction_valid", C.c_double), ("max_errors", C.c_uint32),
                ("min_depth", C.c_uint32), ("careful", C.c_int), ("debug_path", C.c_char_p), ("quiet", C.c_int)]


class Bytes(C.Structure):
    _fields_ = [("data", C.c_void_p), ("len", C.c_uint64)]


class FilterReport(C.Structure):
    _fields_ = [("before_count", C.c_uint64), ("after_count", C.c_uint64), ("low_threshold", C.c_uint32),
                ("high_threshold", C.c_uint32), ("orientation", C.c_int), ("orientation_counts", C.c_uint64 * 4)]


class FilterFile(C.Structure):
    _fields_ = [("n_aln", C.c_uint64), ("ref_id", C.c_void_p), ("ref_start", C.c_void_p), ("flags", C.c_void_p),
                ("cig_off", C.c_void_p), ("n_cig", C.c_void_p), ("cigar", C.c_void_p), ("n_cig_total", C.c_uint64),
                ("read", C.c_void_p), ("grp_off", C.c_void_p), ("grp_idx", C.c_void_p), ("ref_end", C.c_void_p)]


class FilterInput(C.Structure):
    _fields_ = [("n_reads", C.c_uint32), ("file", FilterFile * 2)]


class ShardPlan(C.Structure):
    _fields_ = [("n_units", C.c_uint32), ("world", C.c_uint32), ("n_contigs", C.c_uint32), ("contig", C.POINTER(C.c_uint32)),
                ("lo", C.POINTER(C.c_uint64)), ("hi", C.POINTER(C.c_uint64)), ("rank", C.POINTER(C.c_uint32))]


COMM_ID_BYTES = 128


class FilterFileCounts(C.Structure):
    _fields_ = [("alignments", C.c_uint64), ("reads", C.c_uint64), ("loaded", C.c_int)]


# ---- the signatures --------------------------------------------------------------------------------------------------
# name -> (restype, argtypes).  Opaque objects, arrays and device addresses go as c_void_p: callers pass integers or None.
_i, _vp, _str, _sz = C.c_int, C.c_void_p, C.c_char_p, C.c_size_t
_u8, _u32, _u64, _f64 = C.c_uint8, C.c_uint32, C.c_uint64, C.c_double
_P = C.POINTER
_pvp, _pu32, _pu64, _pf32 = _P(_vp), _P(_u32), _P(_u64), _P(C.c_float)

SIGNATURES = {
    "pp_device_count": (_i, []),
    "pp_ctx_create": (_i, [_i, _pvp]),
    "pp_ctx_create_async": (_i, [_i, _pvp]),
    "pp_ctx_wait": (_i, [_vp]),
    "pp_ctx_destroy": (None, [_vp]),
    "pp_last_error": (_str, [_vp]),
    "pp_ctx_sync": (_i, [_vp]),
    "pp_ctx_stream": (_vp, [_vp]),
    "pp_ctx_download": (_i, [_vp, _vp, _vp, _u64]),
    "pp_version": (_str, []),
    "pp_log_text": (_i, [_i, _f64, _str, _sz]),
    "pp_batch_prepare": (_i, [_vp, _u32, _vp, _P(AlnBatch), _i, _pvp]),
    "pp_prepared_batch": (None, [_vp, _P(AlnBatch)]),
    "pp_prepared_kernel_ms": (_i, [_vp, _pf32]),
    "pp_prepared_free": (None, [_vp]),
    "pp_batch_gate": (_i, [_vp, _P(RawBatch), _i, _u32, _i, _vp, _u64, _pvp, _pu64]),
    "pp_gated_batch": (None, [_vp, _P(AlnBatch), _pvp]),
    "pp_gated_counts": (None, [_vp, _P(SamCounts)]),
    "pp_gated_kernel_ms": (_i, [_vp, _pf32]),
    "pp_gated_free": (None, [_vp]),
    "pp_batch_regroup": (_i, [_vp, _P(RawBatch), _i, _pvp]),
    "pp_regrouped_raw": (None, [_vp, _P(RawBatch)]),
    "pp_regrouped_perm": (_vp, [_vp]),
    "pp_regrouped_counts": (None, [_vp, _pu64, _pu64]),
    "pp_regrouped_pass": (_i, [_vp, _vp, _u64, _vp]),
    "pp_regrouped_kernel_ms": (_i, [_vp, _pf32]),
    "pp_regrouped_free": (None, [_vp]),
    "pp_names_create": (_i, [_vp, _u64, _pvp]),
    "pp_names_ids": (_i, [_vp, _vp, _u64, _vp, _vp, _u64, _i, _vp, _vp, _pu64]),
    "pp_names_count": (_u64, [_vp]),
    "pp_names_name": (_i, [_vp, _u64, _vp, _u32, _pu32]),
    "pp_names_kernel_ms": (_i, [_vp, _pf32]),
    "pp_names_free": (None, [_vp]),
    "pp_bgzf_walk": (_i, [_vp, _u64, _u64, _vp, _vp, _u64, _pu64, _pu64]),
    "pp_bgzf_inflate": (_i, [_vp, _vp, _u64, _vp, _u64, _i, _pvp, _pu64]),
    "pp_bgzf_bytes": (None, [_vp, _pvp, _pu64]),
    "pp_bgzf_bam_walk": (_i, [_vp, _u64, _pu64, _pu64]),
    "pp_bgzf_rec_off": (_vp, [_vp]),
    "pp_bgzf_kernel_ms": (_i, [_vp, _pf32]),
    "pp_bgzf_free": (None, [_vp]),
    "pp_bam_header": (_i, [_vp, _u64, _u32, _pu32, _vp, _vp, _vp, _pu64]),
    "pp_bam_walk": (_i, [_vp, _u64, _u64, _vp, _u64, _pu64, _pu64]),
    "pp_bam_last_error": (_str, []),
    "pp_bam_walk_device": (_i, [_vp, _vp, _u64, _u64, _i, _pvp, _pu64, _pu64]),
    "pp_bam_offs_dev": (_vp, [_vp]),
    "pp_bam_offs_count": (_u64, [_vp]),
    "pp_bam_offs_kernel_ms": (_i, [_vp, _pf32]),
    "pp_bam_offs_free": (None, [_vp]),
    "pp_bam_records": (_i, [_vp, _vp, _u64, _vp, _u64, _i, _vp, _u32, _pvp, _pu64]),
    "pp_bam_raw": (None, [_vp, _P(RawBatch)]),
    "pp_bam_read_id": (_vp, [_vp]),
    "pp_bam_names": (None, [_vp, _pvp, _pu64, _pvp, _pvp]),
    "pp_bam_pass": (None, [_vp, _pvp, _pu64]),
    "pp_bam_kernel_ms": (_i, [_vp, _pf32]),
    "pp_bam_free": (None, [_vp]),
    "pp_sam_records": (_i, [_vp, _vp, _u64, _i, _pvp, _pu64]),
    "pp_sam_records_lines": (_i, [_vp, _vp, _u64, _i, _u64, _pvp, _pu64]),
    "pp_sam_raw": (None, [_vp, _P(RawBatch)]),
    "pp_sam_read_id": (_vp, [_vp]),
    "pp_sam_contig": (_vp, [_vp]),
    "pp_sam_names": (None, [_vp, _pvp, _pu64, _pvp, _pvp]),
    "pp_sam_rnames": (None, [_vp, _pvp, _pu64, _pvp, _pvp]),
    "pp_sam_lines": (_vp, [_vp]),
    "pp_sam_pass": (None, [_vp, _pvp, _pu64]),
    "pp_sam_first_empty_line": (_i, [_vp, _pu64]),
    "pp_sam_kernel_ms": (_i, [_vp, _pf32]),
    "pp_sam_free": (None, [_vp]),
        "pp_bam_tagged": (_i, [_vp, _vp, _u64, _u64, _vp, _u64, _i, _vp, _u64, _pvp, _pu64]),
    "pp_bam_tagged_head": (_i, [_vp, _vp, _u64, _u64, _vp, _u64, _i, _vp, _u64, _vp, _u64, _pvp, _pu64]),
    "pp_bam_out_bytes": (None, [_vp, _pvp, _pu64]),
    "pp_bam_out_counts": (None, [_vp, _pu64, _pu64, _pu64]),
    "pp_bam_out_write": (_i, [_vp, _str]),
    "pp_bam_out_kernel_ms": (_i, [_vp, _pf32]),
    "pp_bam_out_free": (None, [_vp]),
    "pp_bam_sort": (_i, [_vp, _vp, _u64, _u64, _vp, _u64, _i, _pvp, _pu64]),
    "pp_bam_sorted_perm": (_vp, [_vp]),
    "pp_bam_sorted_rec_off": (_vp, [_vp]),
    "pp_bam_sorted_head": (None, [_vp, _pvp, _pu64]),
    "pp_bam_sorted_counts": (None, [_vp, _pu64, _pu64]),
    "pp_bam_sorted_pass": (_i, [_vp, _vp, _u64, _vp]),
    "pp_bam_sorted_kernel_ms": (_i, [_vp, _pf32]),
    "pp_bam_sorted_free": (None, [_vp]),
    "pp_bgzf_deflate": (_i, [_vp, _vp, _u64, _i, _pvp]),
    "pp_bam_out_deflate": (_i, [_vp, _vp, _pvp]),
    "pp_bgzf_out_bytes": (None, [_vp, _pvp, _pu64]),
    "pp_bgzf_out_blk_off": (_vp, [_vp, _pu64]),
    "pp_bgzf_out_counts": (None, [_vp, _pu64, _pu64, _pu64]),
    "pp_bgzf_out_write": (_i, [_vp, _str]),
    "pp_bgzf_out_kernel_ms": (_i, [_vp, _pf32]),
    "pp_bgzf_out_free": (None, [_vp]),
    "pp_sam_tagged": (_i, [_vp, _vp, _u64, _i, _vp, _u64, _pvp]),
    "pp_sam_tagged_records": (_i, [_vp, _vp, _vp, _u64, _pvp]),
    "pp_sam_out_bytes": (None, [_vp, _pvp, _pu64]),
    "pp_sam_out_counts": (None, [_vp, _pu64, _pu64, _pu64]),
    "pp_sam_out_write": (_i, [_vp, _str]),
    "pp_sam_out_kernel_ms": (_i, [_vp, _pf32]),
    "pp_sam_out_free": (None, [_vp]),
    "pp_sam_header": (_i, [_vp, _u64, _u32, _pu32, _vp, _vp, _vp, _pu64]),
    "pp_sam_bam": (_i, [_vp, _vp, _u64, _i, _pvp, _pu64]),
    "pp_sam_bam_records": (_i, [_vp, _vp, _pvp, _pu64]),
    "pp_bam_enc_bytes": (None, [_vp, _pvp, _pu64, _pu64]),
    "pp_bam_enc_rec_off": (_vp, [_vp, _pu64]),
    "pp_bam_enc_kernel_ms": (_i, [_vp, _pf32]),
    "pp_bam_enc_free": (None, [_vp]),
    "pp_bam_sam": (_i, [_vp, _vp, _u64, _u64, _vp, _u64, _i, _vp, _u64, _pvp, _pu64]),
    "pp_bam_sam_encoded": (_i, [_vp, _vp, _vp, _u64, _pvp, _pu64]),
    "pp_aln_file_kind": (_i, [_str, _P(_i)]),
    "pp_aln_file_kind_text": (_i, [_str, _P(_i)]),
    "pp_polish_set_emit": (_i, [_vp, _vp, _vp]),
    "pp_polish_begin": (_i, [_vp, _u32, _vp, _vp, _i, _P(Params)]),
    "pp_polish_add": (_i, [_vp, _P(AlnBatch), _i]),
    "pp_polish_reserve": (_i, [_vp, _u64, _u64, _u64]),
    "pp_polish_finish": (_i, [_vp]),
    "pp_polish_result_size": (_i, [_vp, _pu64]),
    "pp_polish_result": (_i, [_vp, _vp, _i, _vp, _vp]),
    "pp_polish_result_device": (_vp, [_vp]),
    "pp_polish_set_debug": (_i, [_vp, _i]),
    "pp_polish_positions": (_i, [_vp, _P(PositionsOut)]),
    "pp_polish_debug_extra": (_i, [_vp, _vp]),
    "pp_debug_extra_free": (None, [_vp]),
    "pp_polish_debug_tsv": (_i, [_vp, _vp, _u64, _u64, _vp, _i, _u64, _pu64, _pu64]),
    "pp_polish_vcf": (_i, [_vp, _vp, _pvp]),
    "pp_vcf_out_bytes": (None, [_vp, _pvp, _pu64, _pu64]),
    "pp_vcf_out_write": (_i, [_vp, _str]),
    "pp_vcf_out_kernel_ms": (_i, [_vp, _pf32]),
    "pp_vcf_out_free": (None, [_vp]),
    "pp_status_bed": (_i, [_vp, _vp, _i, _u32, _vp, _vp, _u32, _pvp, _pu64]),
    "pp_polish_bed": (_i, [_vp, _vp, _u32, _pvp]),
    "pp_bed_out_bytes": (None, [_vp, _pvp, _pu64, _pu64]),
    "pp_bed_out_counts": (None, [_vp, _pu64]),
    "pp_bed_out_write": (_i, [_vp, _str]),
    "pp_bed_out_kernel_ms": (_i, [_vp, _pf32]),
    "pp_bed_out_free": (None, [_vp]),
    "pp_polish_masked": (_i, [_vp, _u32, _pvp]),
    "pp_masked_bytes": (None, [_vp, _pvp, _pu64]),
    "pp_masked_kernel_ms": (_i, [_vp, _pf32]),
    "pp_masked_free": (None, [_vp]),
    "pp_depth_bedgraph": (_i, [_vp, _vp, _i, _u32, _vp, _vp, _u32, _pvp, _pu64]),
    "pp_polish_depth": (_i, [_vp, _vp, _u32, _pvp]),
    "pp_depth_out_bytes": (None, [_vp, _pvp, _pu64, _pu64]),
    "pp_depth_out_summary": (None, [_vp, _pu64, _pu64, _pu64]),
    "pp_depth_out_write": (_i, [_vp, _str]),
    "pp_depth_out_kernel_ms": (_i, [_vp, _pf32]),
    "pp_depth_out_free": (None, [_vp]),
    "pp_ctx_set_profiling": (_i, [_vp, _i]),
    "pp_polish_kernel_times": (_i, [_vp, _P(KernelTimes)]),
    "pp_polish_took_direct_path": (_i, [_vp]),
    "pp_shard_plan_create": (_i, [_u32, _vp, _vp, _u32, _u64, _P(_P(ShardPlan))]),
    "pp_shard_plan_free": (None, [_P(ShardPlan)]),
    "pp_shard_emit_ranges": (_i, [_P(ShardPlan), _u32, _vp, _vp]),
    "pp_shard_assemble": (_i, [_P(ShardPlan), _vp, _vp, _vp, _vp]),
    "pp_shard_split": (_i, [_vp, _P(ShardPlan), _u32, _P(AlnBatch), _i, _pvp]),
    "pp_shard_part_batch": (None, [_vp, _P(AlnBatch), _pvp]),
    "pp_shard_part_mem": (_i, [_vp]),
    "pp_shard_part_free": (None, [_vp]),
    "pp_shard_count": (_i, [_vp, _P(AlnBatch), _i, _u32, _vp]),
    "pp_polish_error_record": (_i, [_vp, _pu64, _pu32]),
    "pp_polish_error_text": (_i, [_vp, _u32, _u64]),
    "pp_comm_unique_id": (_i, [_vp]),
    "pp_comm_init": (_i, [_vp, _i, _i, _vp]),
    "pp_comm_destroy": (None, [_vp]),
    "pp_polish_gather": (_i, [_vp, _vp, _u64, _vp, _vp]),
    "pp_filter_begin": (_i, [_vp, _P(FilterInput), _i]),
    "pp_filter_samples": (_i, [_vp, _vp, _vp]),
    "pp_filter_pairs": (_i, [_vp, _u32, _u32, _u8, _vp, _vp]),
    "pp_filter_kernel_times": (_i, [_vp, _P(KernelTimes)]),
    "pp_filter_load": (_i, [_str, _str, _pvp, _P(FilterFileCounts), _str, _sz]),
    "pp_filter_loaded_input": (None, [_vp, _P(FilterInput)]),
    "pp_filter_write": (_i, [_vp, _i, _vp, _str, _pu64, _pu64, _str, _sz]),
    "pp_filter_loaded_free": (None, [_vp]),
    "pp_filter_load_device": (_i, [_vp, _str, _str, _pvp, _P(FilterFileCounts)]),
    "pp_filter_dev_input": (None, [_vp, _P(FilterInput)]),
    "pp_filter_dev_text": (_vp, [_vp, _i, _pu64]),
    "pp_filter_dev_free": (None, [_vp]),
    "pp_filter_write_text": (_i, [_vp, _u64, _vp, _u64, _str, _pu64, _pu64, _str, _sz]),
    "pp_assembly_load": (_i, [_str, _pvp, _str, _sz]),
    "pp_assembly_free": (None, [_vp]),
    "pp_assembly_n_contigs": (_u32, [_vp]),
    "pp_assembly_name": (_str, [_vp, _u32]),
    "pp_assembly_description": (_str, [_vp, _u32]),
    "pp_assembly_offsets": (_pu64, [_vp]),
    "pp_assembly_bases": (_P(_u8), [_vp]),
    "pp_fasta_records": (_i, [_vp, _vp, _u64, _i, _pvp, _pu64]),
    "pp_fasta_bases": (None, [_vp, _pvp, _pu64]),
    "pp_fasta_n_contigs": (_u32, [_vp]),
    "pp_fasta_offsets": (_vp, [_vp]),
    "pp_fasta_name": (_str, [_vp, _u32]),
    "pp_fasta_description": (_str, [_vp, _u32]),
    "pp_fasta_kernel_ms": (_i, [_vp, _pf32]),
    "pp_fasta_free": (None, [_vp]),
    "pp_assembly_load_device": (_i, [_vp, _str, _pvp, _str, _sz]),
    "pp_assembly_bases_device": (_vp, [_vp]),
    "pp_ingest_create": (_i, [_vp, _u32, _i, _pvp]),
    "pp_ingest_sam": (_i, [_vp, _str, _P(SamCounts), _str, _sz]),
    "pp_ingest_sam_filtered": (_i, [_vp, _str, _vp, _u64, _P(SamCounts), _str, _sz]),
    "pp_ingest_batch": (None, [_vp, _P(AlnBatch)]),
    "pp_ingest_read_name": (_str, [_vp, _u64]),
    "pp_ingest_free": (None, [_vp]),
    "pp_bytes_free": (None, [_P(Bytes)]),
    "pp_fasta_text": (_i, [_vp, _vp, _i, _u32, _vp, _vp, _vp, _u32, _pvp]),
    "pp_fasta_out_bytes": (None, [_vp, _pvp, _pu64]),
    "pp_fasta_out_fai": (_i, [_vp, _P(Bytes)]),
    "pp_fasta_out_write": (_i, [_vp, _str]),
    "pp_fasta_out_kernel_ms": (_i, [_vp, _pf32]),
    "pp_fasta_out_free": (None, [_vp]),
    "pp_bgzf_out_gzi": (_i, [_vp, _P(Bytes)]),
    "pp_bam_index": (_i, [_vp, _vp, _u64, _u64, _vp, _u64, _i, _vp, _u64, _u32, _vp, _u64, _i, _P(Bytes), _pu64]),
    "pp_tabix_index": (_i, [_vp, _vp, _u64, _i, _i, _vp, _u64, _i, _P(Bytes), _P(Bytes), _pu64]),
    "pp_ctx_set_regroup": (_i, [_vp, _i]),
    "pp_ctx_set_out_bam": (_i, [_vp, _i]),
    "pp_ctx_set_out_sam": (_i, [_vp, _i]),
    "pp_ctx_set_text_chain": (_i, [_vp, _i]),
    "pp_ctx_set_sort_out": (_i, [_vp, _i, _i]),
    "pp_ctx_set_fasta_form": (_i, [_vp, C.c_int64, _i]),
    "pp_ctx_fasta_index": (_i, [_vp, _P(Bytes), _P(Bytes)]),
    "pp_ctx_set_vcf": (_i, [_vp, _i, _i]),
    "pp_ctx_vcf": (_i, [_vp, _P(Bytes)]),
    "pp_ctx_set_bed": (_i, [_vp, _i, _u32, _i]),
    "pp_ctx_bed": (_i, [_vp, _P(Bytes)]),
    "pp_ctx_set_soft_mask": (_i, [_vp, _u32]),
    "pp_ctx_set_depth": (_i, [_vp, _i, _u32, _i]),
    "pp_ctx_depth": (_i, [_vp, _P(Bytes)]),
    "pp_ctx_set_tbi": (_i, [_vp, _i, _i, _i]),
    "pp_ctx_tbi": (_i, [_vp, _i, _P(Bytes)]),
    "pp_polish_files": (_i, [_vp, _str, _P(_str), _i, _P(PolishOptions), _P(Bytes)]),
    "pp_polish_files_multi": (_i, [_pvp, _i, _str, _P(_str), _i, _P(PolishOptions), _P(Bytes)]),
    "pp_dev_ingest_create": (_i, [_vp, _vp, _u32, _i, _pvp]),
    "pp_dev_ingest_sam": (_i, [_vp, _str, _P(SamCounts)]),
    "pp_dev_ingest_sam_filtered": (_i, [_vp, _str, _vp, _u64, _P(SamCounts)]),
    "pp_dev_ingest_set_seq_layout": (_i, [_vp, _i]),
    "pp_ingest_set_seq_layout": (_i, [_vp, _i]),
    "pp_dev_ingest_expect": (_i, [_vp, _u64]),
    "pp_dev_ingest_batch": (None, [_vp, _P(AlnBatch)]),
    "pp_dev_ingest_free": (None, [_vp]),
    "pp_filter_thresholds": (_i, [_vp, _str, _f64, _f64, _P(FilterReport)]),
    "pp_filter_records": (_i, [_vp, _P(RawBatch), _i, _str, _f64, _f64, _vp, _vp, _P(FilterFileCounts), _P(FilterReport)]),
    "pp_filter_files": (_i, [_vp] + [_str] * 5 + [_f64, _f64, _i, _P(FilterReport)]),
    "pp_filter_polish_files": (_i, [_vp] + [_str] * 6 + [_f64, _f64, _P(PolishOptions), _P(FilterReport), _P(Bytes)]),
}

# the internal hooks (not in the header) the binding, tools/ and tests/ call; one missing from a PP_LIB_PATH variant is skipped
HOOKS = {
    "pp_ctx_trust_mirrors_": (_i, [_vp, _i]),
    "pp_ctx_regroup_": (_i, [_vp]),
    "pp_ctx_text_chain_": (_i, [_vp]),
    "pp_gated_stage_ms_": (_i, [_vp, _pf32]),       # float[3]
    "pp_regrouped_stage_ms_": (_i, [_vp, _pf32]),   # float[3]
    "pp_regroup_geometry_": (None, [_pu32]),
    "pp_names_stage_ms_": (_i, [_vp, _pf32]),       # float[5]
    "pp_bgzf_stage_ms_": (_i, [_vp, _pf32]),        # float[3]
    "pp_bam_stage_ms_": (_i, [_vp, _pf32]),         # float[3]
    "pp_sam_stage_ms_": (_i, [_vp, _pf32]),         # float[5]
    "pp_fasta_stage_ms_": (_i, [_vp, _pf32]),       # float[4]
    "pp_fasta_geometry_": (None, [_pu32] * 3),
    "pp_fasta_out_stage_ms_": (_i, [_vp, _pf32]),   # float[2]
    "pp_fasta_out_geometry_": (None, [_pu32] * 2),
    "pp_vcf_out_stage_ms_": (_i, [_vp, _pf32]),     # float[4]
    "pp_vcf_geometry_": (None, [_pu32] * 4),
    "pp_bed_out_stage_ms_": (_i, [_vp, _pf32]),     # float[3]
    "pp_bed_geometry_": (None, [_pu32] * 4),
    "pp_depth_out_stage_ms_": (_i, [_vp, _pf32]),   # float[4]
    "pp_depth_geometry_": (None, [_pu32] * 4),
    "pp_ctx_fasta_form_": (_i, [_vp, _P(C.c_int64), _P(_i)]),
    "pp_ctx_set_fasta_out_name_": (_i, [_vp, _str]),
    "pp_bam_out_stage_ms_": (_i, [_vp, _pf32]),     # float[3]
    "pp_bam_sorted_stage_ms_": (_i, [_vp, _pf32]),  # float[3]
    "pp_bam_index_stage_ms_": (_i, [_vp, _pf32]),   # float[4]
    "pp_tabix_stage_ms_": (_i, [_vp, _pf32]),       # float[5]
    "pp_bgzf_out_stage_ms_": (_i, [_vp, _pf32]),    # float[3]
    "pp_sam_out_stage_ms_": (_i, [_vp, _pf32]),     # float[4]
    "pp_sam_out_geometry_": (None, [_pu32] * 3),
    "pp_bam_enc_stage_ms_": (_i, [_vp, _pf32]),     # float[5]
    "pp_sam_bam_geometry_": (None, [_pu32] * 3),
    "pp_bam_sam_geometry_": (None, [_pu32] * 5),
    "pp_bam_offs_stage_ms_": (_i, [_vp, _pf32]),    # float[3]
    "pp_bam_offs_stats_": (_i, [_vp, _pu64]),       # uint64[4]
    "pp_bam_walk_geometry_": (None, [_pu32] * 3),
    "pp_sam_group_cut_": (_u64, [_str, _u64, _u64]),
    "pp_shard_split_view_": (_i, [_vp, _P(ShardPlan), _u32, _P(AlnBatch), _i, _u32, _pvp]),  # pp_shard_split + wo_idx_base
}
