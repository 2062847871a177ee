"""ctypes binding of include/strelka_amd.h (plumbing for tests and bench.py; the product is the C-ABI library).

There is deliberately no fallback: if libstrelka_amd.so is missing this module raises, and if no gfx950 device is present
`init()` raises with the library's own error text.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libstrelka_amd.so")

c_void_p = C.c_void_p


class ScoreOp(C.Structure):
    _fields_ = [("length", C.c_uint16), ("kind", C.c_uint8), ("flags", C.c_uint8), ("src", C.c_int32)]


SCORE_OP_DTYPE = np.dtype([("length", "<u2"), ("kind", "u1"), ("flags", "u1"), ("src", "<i4")])
OP_BASES, OP_SOFT_CLIP, OP_NOBASE = 0, 1, 2
OPFLAG_PENALTY = 1


class AlignBatch(C.Structure):
    _fields_ = [("n_reads", C.c_int32), ("n_cals", C.c_int32), ("n_ops", C.c_int64),
                ("read_off", c_void_p), ("read_code", c_void_p), ("read_qual", c_void_p),
                ("hap_off", c_void_p), ("hap_code", c_void_p), ("cal_off", c_void_p), ("op_off", c_void_p),
                ("ops", c_void_p), ("max_read_len", C.c_int32), ("max_hap_len", C.c_int32),
                ("entries", c_void_p), ("evmask", c_void_p), ("evmask_words", C.c_int32),
                ("colmat", c_void_p), ("colmat_off", c_void_p), ("addmask", c_void_p)]


class PathSeg(C.Structure):
    _fields_ = [("type", C.c_uint32), ("length", C.c_uint32)]


class IndelKey(C.Structure):
    _fields_ = [("pos", C.c_int32), ("type", C.c_int32), ("del_len", C.c_uint32), ("ins_len", C.c_uint32),
                ("ins_seq", C.c_char_p), ("is_candidate", C.c_int32)]


class CandidateAlignment(C.Structure):
    _fields_ = [("pos", C.c_int32), ("n_seg", C.c_int32), ("path", C.POINTER(PathSeg)), ("n_indels", C.c_int32),
                ("indels", C.POINTER(IndelKey)), ("leading", IndelKey), ("trailing", IndelKey)]


MAX_SAMPLES = 8
SEG = dict(NONE=0, MATCH=1, INSERT=2, DELETE=3, SKIP=4, SOFT_CLIP=5, HARD_CLIP=6, PAD=7, SEQ_MATCH=8, SEQ_MISMATCH=9)
CIGAR_CHARS = "?MIDNSHP=X"
INDEL = dict(NONE=0, INDEL=1, MISMATCH=2, BP_LEFT=3, BP_RIGHT=4)
MAPLEVEL = dict(UNKNOWN=0, TIER1=1, TIER2=2, SUB=3, UNMAPPED=4)


class RealignOptions(C.Structure):
    _fields_ = [("max_read_indel_toggle", C.c_int32), ("max_candidate_indel_density", C.c_double),
                ("max_realignment_candidates", C.c_uint32), ("max_indel_size", C.c_uint32),
                ("is_smoothed_alignments", C.c_int32), ("smoothed_lnp_range", C.c_double),
                ("upstream_oligo_size", C.c_uint32), ("is_haplotyping_enabled", C.c_int32),
                ("min_read_bp_flank", C.c_int32), ("sample_count", C.c_int32), ("host_threads", C.c_int32),
                ("enumeration", C.c_int32)]


class IndelInfo(C.Structure):
    _fields_ = [("key", IndelKey), ("ref_to_indel_log_prob", C.c_double), ("indel_to_ref_log_prob", C.c_double),
                ("active_region_id", C.c_int32), ("haplotype_id", C.c_int8 * MAX_SAMPLES),
                ("is_haplotyping_bypassed", C.c_uint8 * MAX_SAMPLES), ("is_forced_output", C.c_uint8),
                ("not_discovered_from_reads", C.c_uint8)]


class ReadInput(C.Structure):
    _fields_ = [("read_code", c_void_p), ("read_qual", c_void_p), ("read_len", C.c_int32), ("pos", C.c_int32),
                ("n_seg", C.c_int32), ("path", C.POINTER(PathSeg)), ("is_fwd_strand", C.c_int32),
                ("map_level", C.c_int32), ("sample_index", C.c_int32), ("realign_begin", C.c_int32),
                ("realign_end", C.c_int32), ("n_observed", C.c_int32), ("observed", C.POINTER(C.c_int32))]


class ReadPathScores(C.Structure):
    _fields_ = [("indel", C.c_int32), ("ref_lnp", C.c_float), ("indel_lnp", C.c_float), ("non_ambig", C.c_uint16),
                ("read_length", C.c_uint16), ("is_tier1_read", C.c_uint8), ("is_fwd_strand", C.c_uint8),
                ("read_pos", C.c_int16), ("distance_from_closest_read_edge", C.c_int16), ("n_alt", C.c_int32),
                ("alt_indel", C.c_int32 * 2), ("alt_lnp", C.c_float * 2)]


class ReadResult(C.Structure):
    _fields_ = [("n_candidate_alignments", C.c_int32), ("is_realigned", C.c_int32), ("realign_pos", C.c_int32),
                ("realign_n_seg", C.c_int32), ("realign_path", C.POINTER(PathSeg)), ("max_score", C.c_double),
                ("n_scores", C.c_int32), ("scores", C.POINTER(ReadPathScores)), ("n_suboverlap", C.c_int32),
                ("suboverlap", C.POINTER(C.c_int32)), ("warn_origin_skip", C.c_int32),
                ("warn_max_toggle_depth", C.c_int32)]


class AlignScores(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("match", "mismatch", "open", "extend", "off_edge", "insert_delete",
                                         "is_allow_edge_insertion", "is_require_edge_deletion")]


class GlobalAlignBatch(C.Structure):
    _fields_ = [("n", C.c_int32), ("query_off", c_void_p), ("query", c_void_p), ("ref_off", c_void_p), ("ref", c_void_p)]


class IntakeOptions(C.Structure):
    _fields_ = [("max_indel_size", C.c_uint32), ("min_alt_allele_fraction", C.c_float)]


class PileupOptions(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("min_basecall_qscore", "mismatch_density_flank_size", "mismatch_density_max_count",
                                         "use_tier2_evidence", "tier2_mismatch_density_max_count", "is_mapq_adjust",
                                         "min_distance_from_read_edge", "largest_total_indel_ref_span_per_read",
                                         "report_begin", "report_end")]


class ReadBatchStruct(C.Structure):
    _fields_ = [("n_reads", C.c_int32), ("read_off", c_void_p), ("read_code", c_void_p), ("read_qual", c_void_p),
                ("path_off", c_void_p), ("path", c_void_p), ("pos", c_void_p), ("is_fwd", c_void_p), ("mapq", c_void_p),
                ("map_level", c_void_p), ("ref_seq", c_void_p), ("ref_offset", C.c_int32), ("ref_len", C.c_int32),
                ("cand_snv_mask", c_void_p)]


class PileupColumns(C.Structure):
    _fields_ = [("n_loci", C.c_int32), ("capacity", C.c_int64), ("call_off", c_void_p), ("calls", c_void_p),
                ("spandel_count", c_void_p), ("submapped_count", c_void_p)]


PILEUP_RAW_TIER1, PILEUP_RAW_TIER2, PILEUP_CLEAN_TIER1, PILEUP_CLEAN_TIER2 = 0, 1, 2, 3


GVCF_SITE_SUMMARY_DTYPE = np.dtype([("flags", np.uint32), ("gqx", np.int32), ("ref_fwd", np.uint32), ("ref_rev", np.uint32)])


GVCF_RUN_DTYPE = np.dtype([("len", np.int32), ("filter_key", np.uint32), ("gqx_min", np.int32), ("gqx_max", np.int32), ("dpu_min", np.uint32),
                           ("dpu_max", np.uint32), ("dpf_min", np.uint32), ("dpf_max", np.uint32)])
assert GVCF_RUN_DTYPE.itemsize == 32


class GvcfBlockOptions(C.Structure):
    _fields_ = [("min_passed_call_depth", C.c_uint32), ("is_min_homref_gqx", C.c_int32), ("min_homref_gqx", C.c_double), ("is_max_depth", C.c_int32),
                ("is_max_base_filt", C.c_int32), ("max_chrom_depth", C.c_double), ("max_base_filt", C.c_double), ("block_percent_tol", C.c_uint32),
                ("block_abs_tol", C.c_uint32)]


def gvcf_block_options(**kw):
    """the reference's defaults (gvcf_options.hh:57-77); max depth filter off unless max_chrom_depth is given"""
    o = GvcfBlockOptions(3, 1, 30.0, 0, 1, 0.0, 0.4, 30, 3)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


class PileupWindow(C.Structure):
    _fields_ = [("begin", C.c_int32), ("end", C.c_int32), ("tier1_off", c_void_p), ("tier1_calls", c_void_p),
                ("tier2_off", c_void_p), ("tier2_calls", c_void_p), ("spandel_count", c_void_p), ("submapped_count", c_void_p),
                ("mapq_count", c_void_p), ("mapq_zero_count", c_void_p), ("mapq_sum_square", c_void_p),
                ("clean_count", c_void_p), ("genotype", c_void_p), ("evs_off", c_void_p), ("evs_words", c_void_p),
                ("site_summary", c_void_p), ("gvcf_runs", c_void_p)]


class SomaticPileupWindow(C.Structure):
    _fields_ = [("normal", PileupWindow), ("tumor", PileupWindow), ("normal_clean_tier2_count", c_void_p),
                ("tumor_clean_tier2_count", c_void_p), ("tumor_tier1_read_pos", c_void_p), ("genotype", c_void_p)]


class PileupBatch(C.Structure):
    _fields_ = [("n_loci", C.c_int32), ("call_off", c_void_p), ("calls", c_void_p), ("de", c_void_p),
                ("ref_base", c_void_p), ("ploidy", c_void_p)]


class GermlineOptions(C.Structure):
    _fields_ = [("bsnp_diploid_theta", C.c_double), ("bsnp_ssd_no_mismatch", C.c_double),
                ("bsnp_ssd_one_mismatch", C.c_double), ("is_min_vexp", C.c_int32), ("min_vexp", C.c_double)]


class SomaticSnvOptions(C.Structure):
    _fields_ = [("bsnp_diploid_theta", C.c_double), ("somatic_snv_rate", C.c_double),
                ("shared_site_error_rate", C.c_double), ("shared_site_error_strand_bias_fraction", C.c_double),
                ("ssnv_contam_tolerance", C.c_double)]


class IndelOptions(C.Structure):
    _fields_ = [("min_read_bp_flank", C.c_int32), ("random_base_match_prob", C.c_double),
                ("tier2_random_base_match_prob", C.c_double), ("read_confident_support_threshold", C.c_double),
                ("is_use_alt_indel", C.c_int32), ("fast_form", C.c_int32)]


class SomaticIndelOptions(C.Structure):
    _fields_ = [("bindel_diploid_theta", C.c_double), ("somatic_indel_rate", C.c_double),
                ("shared_indel_error_factor", C.c_double), ("indel_contam_tolerance", C.c_double)]


class ReadScoreBatch(C.Structure):
    _fields_ = [("n_indels", C.c_int32), ("read_off", c_void_p), ("ref_lnp", c_void_p), ("indel_lnp", c_void_p),
                ("alt_lnp", c_void_p), ("non_ambig", c_void_p), ("read_length", c_void_p), ("read_flags", c_void_p),
                ("del_len", c_void_p), ("ins_len", c_void_p), ("is_breakpoint", c_void_p)]


class AlleleGroupBatch(C.Structure):
    _fields_ = [("n_groups", C.c_int32), ("read_off", c_void_p), ("n_alt", c_void_p), ("ploidy", c_void_p),
                ("del_len", c_void_p), ("ins_len", c_void_p), ("ref_lnp", c_void_p), ("allele_lnp", c_void_p),
                ("non_ambig", c_void_p), ("read_length", c_void_p), ("read_flags", c_void_p)]


MAX_ALT, MAX_INDEL_GT = 3, 10
SOMATIC_INDEL_CALL_DTYPE = np.dtype([("normal_lhood", "<f8", (21,)), ("tumor_lhood", "<f8", (21,)), ("max_gt", "<u4"),
                                     ("qphred", "<i4"), ("from_ntype_qphred", "<i4"), ("ntype", "<u4")])
ALLELE_GROUP_CALL_DTYPE = np.dtype([("lhood", "<f8", (MAX_INDEL_GT,)), ("counts", "<u4", (2, MAX_ALT + 2)),
                                    ("n_genotypes", "<u4"), ("n_reads_used", "<u4")])
assert SOMATIC_INDEL_CALL_DTYPE.itemsize == 352 and ALLELE_GROUP_CALL_DTYPE.itemsize == 128
# multi-sample allele groups (up to ploidy x sample_count alternate alleles): sk_allele_group_call_wide
MAX_ALT_WIDE, MAX_INDEL_GT_WIDE = 8, 45
ALLELE_GROUP_CALL_WIDE_DTYPE = np.dtype([("lhood", "<f8", (MAX_INDEL_GT_WIDE,)), ("counts", "<u4", (2, MAX_ALT_WIDE + 2)),
                                         ("n_genotypes", "<u4"), ("n_reads_used", "<u4")])
assert ALLELE_GROUP_CALL_WIDE_DTYPE.itemsize == 448
# ... of runs of up to eight samples: sk_allele_group_call_xwide
MAX_ALT_XWIDE, MAX_INDEL_GT_XWIDE = 16, 153
ALLELE_GROUP_CALL_XWIDE_DTYPE = np.dtype([("lhood", "<f8", (MAX_INDEL_GT_XWIDE,)), ("counts", "<u4", (2, MAX_ALT_XWIDE + 2)),
                                          ("n_genotypes", "<u4"), ("n_reads_used", "<u4")])
assert ALLELE_GROUP_CALL_XWIDE_DTYPE.itemsize == 1376

DIGT_RS_DTYPE = np.dtype([("ref_pprob", "<f8"), ("max_gt", "<u4"), ("snp_qphred", "<i4"), ("max_gt_qphred", "<i4"),
                          ("_pad", "<i4")])
DIGT_CALL_DTYPE = np.dtype([("lhood", "<f4", (10,)), ("phredLoghood", "<u4", (10,)), ("genome", DIGT_RS_DTYPE),
                            ("poly", DIGT_RS_DTYPE), ("strand_bias", "<f8"), ("ref_gt", "<u4"), ("is_called", "<u4")])
SOMATIC_CALL_DTYPE = np.dtype([("normal_lhood", "<f4", (30,)), ("tumor_lhood", "<f4", (30,)), ("max_gt", "<u4"),
                               ("qphred", "<i4"), ("from_ntype_qphred", "<i4"), ("ntype", "<u4"),
                               ("strand_bias", "<f4"), ("is_called", "<u4"), ("normal_alt_id", "<u4"),
                               ("tumor_alt_id", "<u4")])
assert DIGT_CALL_DTYPE.itemsize == 144 and SOMATIC_CALL_DTYPE.itemsize == 272

# every symbol include/strelka_amd.h declares (tests check the library exports all of them)
EXPORTS = [
    "sk_device_count", "sk_host_alloc", "sk_host_free", "sk_init", "sk_init_strict", "sk_check_device_errors", "sk_debug_force_device_libm", "sk_debug_libm_eval", "sk_debug_grown_bytes", "sk_debug_set_g3_variant", "sk_debug_g3_global_pass_count", "sk_shutdown", "sk_last_error", "sk_version", "sk_is_initialized", "sk_sync_mode", "sk_libm_restated", "sk_broker_client", "sk_broker_enable", "sk_broker_serve", "sk_broker_selftest", "sk_get_qscore_tables",
    "sk_score_alignments", "sk_score_alignments_dev", "sk_align_evmask_words", "sk_align_prepare", "sk_align_colmat_words", "sk_align_prepare_cols",
    "sk_bgzf_scan", "sk_bgzf_inflate", "sk_bgzf_inflate_prefixed", "sk_bgzf_inflate_dev", "sk_bgzf_deflate_bound", "sk_bgzf_deflate", "sk_bgzf_deflate_dev", "sk_bam_header_end", "sk_bam_scan_records", "sk_bam_decode", "sk_bam_decode_kept", "sk_bam_decode_dev", "sk_normalize_alignments", "sk_normalize_alignments_dev",
    "sk_intake_options_default", "sk_read_intake_obs_bound", "sk_read_intake", "sk_read_intake_dev", "sk_read_intake_scratch_bytes",
    "sk_ar_state_initial", "sk_ref_anchors", "sk_ref_anchors_dev", "sk_active_regions_bound", "sk_active_regions", "sk_active_regions_dev",
    "sk_sync_state_initial", "sk_sync_regions_bound", "sk_sync_active_regions", "sk_sync_active_regions_dev", "sk_sync_region_params", "sk_sync_region_params_dev",
    "sk_region_haplotypes_params", "sk_region_haplotypes_params_dev",
    "sk_region_haplotypes_seq_bound", "sk_region_haplotypes_support_bound", "sk_region_haplotypes_scratch_bytes", "sk_region_haplotypes", "sk_region_haplotypes_dev",
    "sk_region_alleles_allele_bound", "sk_region_alleles_insert_bound", "sk_region_alleles_scratch_bytes", "sk_region_alleles", "sk_region_alleles_dev", "sk_debug_region_alleles",
    "sk_indel_table_key_bound", "sk_indel_table_id_bound", "sk_indel_table_insert_bound", "sk_indel_table_scratch_bytes", "sk_indel_table", "sk_indel_table_dev",
    "sk_indel_candidate_options_default", "sk_read_depth_scratch_bytes", "sk_read_depth", "sk_read_depth_dev", "sk_indel_candidates_scratch_bytes", "sk_indel_candidates", "sk_indel_candidates_dev",
    "sk_realign_gate_observed_bound", "sk_realign_gate_scratch_bytes", "sk_realign_gate", "sk_realign_gate_dev",
    "sk_realign_preamble_scratch_bytes", "sk_realign_preamble", "sk_realign_preamble_dev", "sk_debug_realign_preamble_host", "sk_realign_job_add_reads_prepared",
    "sk_debug_realign_job_prepared",
    "sk_align_builder_create", "sk_align_builder_destroy", "sk_align_builder_clear", "sk_align_builder_append", "sk_align_builder_add_read",
    "sk_align_builder_finish", "sk_align_builder_error", "sk_align_builder_set_host_threads",
    "sk_align_scores_default", "sk_global_align",
    "sk_pileup_options_default", "sk_pileup_reads", "sk_pileup_reads_dev", "sk_pileup_scratch_bytes",
    "sk_pileup_stream_create", "sk_pileup_stream_destroy", "sk_pileup_stream_begin_region", "sk_pileup_stream_push", "sk_pileup_stream_push_begin", "sk_pileup_stream_push_finish", "sk_pileup_stream_enable_evs_words", "sk_gvcf_site_summaries", "sk_gvcf_site_summaries_dev", "sk_gvcf_plain_runs_dev", "sk_gvcf_plain_runs", "sk_pileup_stream_set_gvcf_block_options",
    "sk_somatic_pileup_stream_create", "sk_somatic_pileup_stream_destroy", "sk_somatic_pileup_stream_begin_region", "sk_somatic_pileup_stream_push", "sk_somatic_pileup_stream_push_begin", "sk_somatic_pileup_stream_push_finish",
    "sk_realign_options_default", "sk_realign_job_create", "sk_realign_job_destroy", "sk_realign_job_error",
    "sk_realign_job_set_reference", "sk_realign_job_set_indels", "sk_realign_job_add_read", "sk_realign_job_add_reads", "sk_realign_job_get_batch",
    "sk_realign_job_finish", "sk_realign_job_run", "sk_realign_job_n_reads", "sk_realign_job_read_result",
    "sk_realign_job_clear_reads", "sk_realign_job_rescore", "sk_realign_job_indels_consulted", "sk_realign_job_enumeration_counts", "sk_realign_device_job_counts", "sk_debug_f5_tail_order", "sk_debug_f5_tail_launches", "sk_debug_f5_shared_rounds", "sk_debug_f5_late_turn_downs", "sk_realign_reference_reads_outside", "sk_realign_job_stage3_counts", "sk_make_start_pos_alignment", "sk_get_end_pin_start_pos",
    "sk_germline_options_default", "sk_dependent_eprob", "sk_dependent_eprob_dev", "sk_site_digt_call",
    "sk_site_digt_call_dev", "sk_site_digt_call_fused", "sk_site_digt_call_fused_dev",
    "sk_somatic_snv_options_default", "sk_somatic_snv_call_batch", "sk_somatic_snv_call_batch_dev",
    "sk_somatic_snv_call_tiers", "sk_somatic_snv_call_tiers_dev", "sk_somatic_snv_tiers_scratch_bytes",
    "sk_indel_options_default", "sk_somatic_indel_options_default", "sk_indel_grid_lhood", "sk_indel_grid_lhood_dev",
    "sk_somatic_indel_call_batch", "sk_somatic_indel_call_tiers", "sk_allele_group_genotype_lhoods", "sk_allele_group_genotype_lhoods_dev",
    "sk_allele_group_genotype_lhoods_wide", "sk_allele_group_genotype_lhoods_wide_dev",
    "sk_allele_group_genotype_lhoods_xwide", "sk_allele_group_genotype_lhoods_xwide_dev",
    "sk_discover_indels_and_mismatches", "sk_global_align_scratch_bytes", "sk_global_align_dev", "sk_bai_query", "sk_bam_region_filter", "sk_gvcf_block_sites", "sk_gvcf_block_sites_dev",
]

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("strelka_amd: %s is missing -- run `python -m strelka_amd.build` (there is no CPU fallback)"
                               % LIB_PATH)
        try:
            # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64 (same soname as /opt/rocm's).  When
            # torch is going to be used in this process (bench.py, device.py) it must be loaded FIRST so that this
            # library binds to the runtime torch initialises; loading /opt/rocm's copy first leaves torch without GPUs.
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        L.sk_last_error.restype = C.c_char_p
        L.sk_debug_grown_bytes.argtypes = [c_void_p, c_void_p]
        L.sk_debug_grown_bytes.restype = None
        L.sk_debug_libm_eval.argtypes = [C.c_int, C.c_int, C.c_int64, c_void_p, c_void_p, c_void_p, c_void_p]
        L.sk_align_builder_create.restype = c_void_p
        L.sk_align_builder_error.restype = C.c_char_p
        L.sk_align_builder_error.argtypes = [c_void_p]
        L.sk_align_builder_destroy.argtypes = [c_void_p]
        L.sk_align_builder_clear.argtypes = [c_void_p]
        L.sk_align_builder_add_read.argtypes = [c_void_p, c_void_p, c_void_p, C.c_int32, C.c_char_p, C.c_int32,
                                                C.c_int32, C.POINTER(CandidateAlignment), C.c_int32]
        L.sk_align_builder_finish.argtypes = [c_void_p, C.POINTER(AlignBatch)]
        L.sk_align_scores_default.argtypes = [C.POINTER(AlignScores)]
        L.sk_global_align.argtypes = [C.POINTER(GlobalAlignBatch), C.POINTER(AlignScores), c_void_p, c_void_p, c_void_p, c_void_p]
        L.sk_pileup_options_default.argtypes = [C.POINTER(PileupOptions)]
        L.sk_pileup_reads.argtypes = [C.POINTER(ReadBatchStruct), C.POINTER(PileupOptions), C.c_int, C.POINTER(PileupColumns)]
        L.sk_pileup_scratch_bytes.restype = C.c_int64
        L.sk_pileup_scratch_bytes.argtypes = [C.c_int32, C.c_int64, C.c_int32]
        L.sk_pileup_reads_dev.argtypes = [C.POINTER(ReadBatchStruct), C.c_int64, C.POINTER(PileupOptions), C.c_int,
                                          C.POINTER(PileupColumns), c_void_p, c_void_p]
        L.sk_realign_options_default.argtypes = [C.POINTER(RealignOptions)]
        L.sk_realign_job_create.restype = c_void_p
        L.sk_realign_job_create.argtypes = [C.POINTER(RealignOptions)]
        L.sk_realign_job_destroy.argtypes = [c_void_p]
        L.sk_realign_job_enumeration_counts.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p]
        L.sk_realign_device_job_counts.argtypes = [c_void_p, c_void_p, c_void_p]
        L.sk_realign_device_job_counts.restype = None
        L.sk_debug_f5_tail_order.argtypes = [c_void_p, C.c_int32, C.c_int32, C.c_int32, c_void_p, c_void_p, c_void_p]
        L.sk_debug_f5_tail_launches.argtypes = []
        L.sk_debug_f5_tail_launches.restype = C.c_int64
        L.sk_debug_f5_shared_rounds.argtypes = []
        L.sk_debug_f5_shared_rounds.restype = C.c_int64
        L.sk_debug_f5_late_turn_downs.argtypes = []
        L.sk_debug_f5_late_turn_downs.restype = C.c_int64
        L.sk_realign_reference_reads_outside.argtypes = []
        L.sk_realign_reference_reads_outside.restype = C.c_int64
        L.sk_realign_job_stage3_counts.argtypes = [c_void_p, c_void_p, c_void_p]
        L.sk_realign_job_indels_consulted.argtypes = [c_void_p, c_void_p, C.c_int32]
        L.sk_realign_job_error.restype = C.c_char_p
        L.sk_realign_job_error.argtypes = [c_void_p]
        L.sk_realign_job_set_reference.argtypes = [c_void_p, C.c_char_p, C.c_int32, C.c_int32]
        L.sk_realign_job_set_indels.argtypes = [c_void_p, C.POINTER(IndelInfo), C.c_int32]
        L.sk_realign_job_add_read.argtypes = [c_void_p, C.POINTER(ReadInput)]
        L.sk_realign_job_add_reads.argtypes = [c_void_p, C.POINTER(ReadInput), C.c_int32]
        L.sk_realign_job_get_batch.argtypes = [c_void_p, C.POINTER(AlignBatch)]
        L.sk_realign_job_finish.argtypes = [c_void_p, c_void_p]
        L.sk_realign_job_run.argtypes = [c_void_p]
        L.sk_realign_job_n_reads.argtypes = [c_void_p]
        L.sk_realign_job_read_result.argtypes = [c_void_p, C.c_int32, C.POINTER(ReadResult)]
        L.sk_realign_job_clear_reads.argtypes = [c_void_p]
        L.sk_make_start_pos_alignment.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.POINTER(IndelKey),
                                                  C.c_int32, C.POINTER(C.c_int32), C.POINTER(PathSeg), C.c_int32,
                                                  C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.sk_get_end_pin_start_pos.argtypes = [C.POINTER(IndelKey), C.c_int32, C.c_uint32, C.c_int32, C.c_int32,
                                               C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.sk_score_alignments.argtypes = [C.POINTER(AlignBatch), c_void_p]
        L.sk_align_evmask_words.argtypes = [C.c_int32]
        L.sk_bgzf_scan.restype = C.c_int64
        L.sk_bgzf_scan.argtypes = [c_void_p, C.c_int64, c_void_p, c_void_p, C.c_int32]
        L.sk_bgzf_inflate.argtypes = [c_void_p, c_void_p, c_void_p, C.c_int32, c_void_p]
        L.sk_bgzf_inflate_dev.argtypes = [c_void_p, c_void_p, c_void_p, C.c_int32, c_void_p, c_void_p, c_void_p]
        L.sk_bgzf_deflate_bound.restype = C.c_int64
        L.sk_bgzf_deflate_bound.argtypes = [C.c_int64, C.c_int]
        L.sk_bgzf_deflate.argtypes = [c_void_p, C.c_int64, C.c_int, C.c_int, c_void_p, C.c_int64, c_void_p]
        L.sk_bgzf_deflate_dev.argtypes = [c_void_p, C.c_int64, C.c_int, C.c_int, c_void_p, C.c_int64, c_void_p, c_void_p]
        L.sk_bam_header_end.restype = C.c_int64
        L.sk_bam_header_end.argtypes = [c_void_p, C.c_int64]
        L.sk_bam_scan_records.restype = C.c_int64
        L.sk_bam_scan_records.argtypes = [c_void_p, C.c_int64, C.c_int64, c_void_p, c_void_p, c_void_p, C.c_int32]
        L.sk_bam_decode.argtypes = [c_void_p, C.c_int64, c_void_p, C.c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
        L.sk_bam_decode_dev.argtypes = [c_void_p, c_void_p, C.c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
        L.sk_normalize_alignments.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.c_int32] + [c_void_p] * 7
        L.sk_normalize_alignments_dev.argtypes = [c_void_p, C.c_int32, C.c_int32, C.c_int32] + [c_void_p] * 8
        L.sk_intake_options_default.argtypes = [C.POINTER(IntakeOptions)]
        L.sk_intake_options_default.restype = None
        L.sk_read_intake_obs_bound.restype = C.c_int64
        L.sk_read_intake_obs_bound.argtypes = [C.c_int64]
        L.sk_read_intake_scratch_bytes.restype = C.c_size_t
        L.sk_read_intake_scratch_bytes.argtypes = [C.c_int32, C.c_int64, C.c_int32]
        L.sk_read_intake.argtypes = [c_void_p, C.c_int32, C.c_int32, C.c_int32] + [c_void_p] * 7 + [C.POINTER(IntakeOptions), C.c_int32, C.c_int32,
                                     c_void_p, c_void_p, c_void_p, C.c_int64, c_void_p, c_void_p]
        L.sk_read_intake_dev.argtypes = [c_void_p, C.c_int32, C.c_int32, C.c_int32] + [c_void_p] * 7 + [C.POINTER(IntakeOptions), C.c_int32, C.c_int32,
                                         c_void_p, c_void_p, c_void_p, C.c_int64, c_void_p, c_void_p, c_void_p, C.c_size_t, c_void_p]
        L.sk_ar_state_initial.argtypes = [c_void_p]
        L.sk_ar_state_initial.restype = None
        L.sk_active_regions_bound.restype = C.c_int64
        L.sk_active_regions_bound.argtypes = [C.c_int32]
        L.sk_ref_anchors.argtypes = [c_void_p, C.c_int32, C.c_int32, C.c_int32, c_void_p, C.c_int32, C.c_int32, c_void_p, C.c_int32, c_void_p, c_void_p]
        L.sk_ref_anchors_dev.argtypes = L.sk_ref_anchors.argtypes + [c_void_p]
        L.sk_active_regions.argtypes = [C.c_int32, C.c_int32] + [c_void_p] * 6 + [C.c_int64, c_void_p]
        L.sk_active_regions_dev.argtypes = L.sk_active_regions.argtypes + [c_void_p]
        L.sk_sync_state_initial.argtypes = [c_void_p]
        L.sk_sync_state_initial.restype = None
        L.sk_sync_regions_bound.restype = C.c_int64
        L.sk_sync_regions_bound.argtypes = [C.c_int32]
        L.sk_sync_active_regions.argtypes = [C.c_int32, C.c_int32, C.c_int32] + [c_void_p] * 5 + [C.c_int32, c_void_p, c_void_p, C.c_int32, c_void_p, c_void_p, c_void_p,
                                             C.c_int64, c_void_p, c_void_p]
        L.sk_sync_active_regions_dev.argtypes = L.sk_sync_active_regions.argtypes + [c_void_p]
        L.sk_sync_region_params.argtypes = [c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, c_void_p, c_void_p]
        L.sk_sync_region_params_dev.argtypes = [c_void_p, c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, c_void_p, c_void_p, c_void_p]
        L.sk_region_haplotypes_seq_bound.restype = C.c_int64
        L.sk_region_haplotypes_seq_bound.argtypes = [C.c_int64]
        L.sk_region_haplotypes_support_bound.restype = C.c_int64
        L.sk_region_haplotypes_support_bound.argtypes = [C.c_int32, C.c_int64]
        L.sk_region_haplotypes_scratch_bytes.restype = C.c_size_t
        L.sk_region_haplotypes_scratch_bytes.argtypes = [C.c_int32, C.c_int64, C.c_int64, C.c_int64]
        L.sk_region_haplotypes.argtypes = [c_void_p, C.c_int32, C.c_int32, C.c_int32] + [c_void_p] * 10 + [C.c_uint32, C.c_int32, C.c_int32, C.c_int32, c_void_p, C.c_int32,
                                           c_void_p, c_void_p, C.c_int64, c_void_p, C.c_int64, c_void_p, c_void_p]
        L.sk_region_haplotypes_dev.argtypes = [c_void_p, C.c_int32, C.c_int32, C.c_int32] + [c_void_p] * 10 + [C.c_uint32, C.c_int32, C.c_int32, C.c_int32, c_void_p, c_void_p,
                                               C.c_int64, c_void_p, c_void_p, C.c_int64, c_void_p, C.c_int64, c_void_p, c_void_p, c_void_p, C.c_size_t, c_void_p]
        L.sk_region_haplotypes_params.argtypes = [c_void_p, C.c_int32, C.c_int32, C.c_int32] + [c_void_p] * 10 + [C.c_uint32, c_void_p, c_void_p, C.c_int32,
                                                  c_void_p, c_void_p, C.c_int64, c_void_p, C.c_int64, c_void_p, c_void_p]
        L.sk_region_haplotypes_params_dev.argtypes = [c_void_p, C.c_int32, C.c_int32, C.c_int32] + [c_void_p] * 10 + [C.c_uint32, c_void_p, c_void_p, c_void_p,
                                                      C.c_int64, c_void_p, c_void_p, C.c_int64, c_void_p, C.c_int64, c_void_p, c_void_p, c_void_p, C.c_size_t, c_void_p]
        L.sk_region_alleles_allele_bound.restype = C.c_int64
        L.sk_region_alleles_allele_bound.argtypes = [C.c_int64, C.c_int32]
        L.sk_region_alleles_insert_bound.restype = C.c_int64
        L.sk_region_alleles_insert_bound.argtypes = [C.c_int64, C.c_int32]
        L.sk_region_alleles_scratch_bytes.restype = C.c_size_t
        L.sk_region_alleles_scratch_bytes.argtypes = [C.c_int64, C.c_int32]
        L.sk_debug_region_alleles.argtypes = [C.c_int, C.c_int]
        L.sk_debug_region_alleles.restype = None
        L.sk_region_alleles.argtypes = [c_void_p, C.c_int32, C.c_int32, c_void_p, C.c_int32, c_void_p, c_void_p, C.c_int64, C.c_uint32, C.c_int32, C.c_int32,
                                        c_void_p, c_void_p, C.c_int64, c_void_p, C.c_int64, c_void_p, c_void_p]
        L.sk_region_alleles_dev.argtypes = [c_void_p, C.c_int32, C.c_int32, c_void_p, c_void_p, C.c_int64, c_void_p, c_void_p, C.c_int64, C.c_uint32, C.c_int32,
                                            C.c_int32, c_void_p, c_void_p, C.c_int64, c_void_p, C.c_int64, c_void_p, c_void_p, c_void_p, C.c_size_t, c_void_p]
        for f in (L.sk_indel_table_key_bound, L.sk_indel_table_id_bound, L.sk_indel_table_insert_bound):
            f.restype = C.c_int64
            f.argtypes = [C.c_int64, C.c_int64]
        L.sk_indel_table_scratch_bytes.restype = C.c_size_t
        L.sk_indel_table_scratch_bytes.argtypes = [C.c_int32, C.c_int64, C.c_int64]
        L.sk_indel_table.argtypes = [C.c_int32, c_void_p, c_void_p, C.c_int32, C.c_int32, c_void_p, C.c_int32, C.c_int32, c_void_p, C.c_int64, c_void_p, c_void_p, C.c_int64,
                                     c_void_p, C.c_int64, c_void_p]
        L.sk_indel_table_dev.argtypes = [C.c_int32, c_void_p, c_void_p, C.c_int32, C.c_int32, c_void_p, c_void_p, C.c_int64, C.c_int32, C.c_int64, c_void_p, C.c_int64,
                                         c_void_p, c_void_p, C.c_int64, c_void_p, C.c_int64, c_void_p, c_void_p, C.c_size_t, c_void_p]
        L.sk_indel_candidate_options_default.argtypes = [c_void_p]
        L.sk_indel_candidate_options_default.restype = None
        L.sk_read_depth_scratch_bytes.restype = C.c_size_t
        L.sk_read_depth_scratch_bytes.argtypes = [C.c_int32]
        L.sk_read_depth.argtypes = [C.c_int32, c_void_p, c_void_p, c_void_p, C.c_int64, c_void_p, c_void_p, C.c_int32, C.c_int32, c_void_p, c_void_p]
        L.sk_read_depth_dev.argtypes = [C.c_int32, c_void_p, c_void_p, c_void_p, C.c_int64, c_void_p, c_void_p, C.c_int32, C.c_int32, c_void_p, c_void_p, c_void_p, C.c_size_t,
                                        c_void_p]
        L.sk_indel_candidates_scratch_bytes.restype = C.c_size_t
        L.sk_indel_candidates_scratch_bytes.argtypes = []
        L.sk_indel_candidates.argtypes = [C.c_int32, c_void_p, C.c_int32, C.c_int32, c_void_p, c_void_p, C.c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
        L.sk_indel_candidates_dev.argtypes = [C.c_int32, c_void_p, C.c_int32, C.c_int32, c_void_p, c_void_p, c_void_p, C.c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                              c_void_p, C.c_size_t, c_void_p]
        L.sk_realign_gate_observed_bound.restype = C.c_int64
        L.sk_realign_gate_observed_bound.argtypes = [C.c_int64]
        L.sk_realign_gate_scratch_bytes.restype = C.c_size_t
        L.sk_realign_gate_scratch_bytes.argtypes = [C.c_int32, C.c_int64, C.c_int64]
        L.sk_realign_gate.argtypes = [C.c_int32, c_void_p, c_void_p, c_void_p, c_void_p, C.c_int64, C.c_int64, c_void_p, c_void_p, C.c_uint32, c_void_p, c_void_p, c_void_p,
                                      c_void_p]
        L.sk_realign_gate_dev.argtypes = [C.c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, C.c_int64, C.c_int64, c_void_p, c_void_p, C.c_uint32, c_void_p, c_void_p,
                                          c_void_p, c_void_p, c_void_p, C.c_size_t, c_void_p]
        L.sk_realign_preamble_scratch_bytes.restype = C.c_size_t
        L.sk_realign_preamble_scratch_bytes.argtypes = [C.c_int32, C.c_int64, C.c_int64]
        for f in (L.sk_realign_preamble, L.sk_debug_realign_preamble_host):
            f.argtypes = [C.c_int32, c_void_p, c_void_p, c_void_p, c_void_p, C.c_int64, c_void_p, C.c_int64, c_void_p, C.c_int32, C.c_int32, C.c_uint32, c_void_p, c_void_p,
                          C.c_int64, c_void_p, c_void_p]
        L.sk_realign_preamble_dev.argtypes = [C.c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, C.c_int64, c_void_p, C.c_int64, c_void_p, C.c_int32, C.c_int32,
                                              C.c_uint32, c_void_p, c_void_p, C.c_int64, c_void_p, c_void_p, c_void_p, C.c_size_t, c_void_p]
        L.sk_realign_job_add_reads_prepared.argtypes = [c_void_p, c_void_p, c_void_p, C.c_int32]
        L.sk_debug_realign_job_prepared.argtypes = [c_void_p, C.c_int32, c_void_p]
        L.sk_align_colmat_words.restype = C.c_int64
        L.sk_align_colmat_words.argtypes = [c_void_p]
        L.sk_align_prepare_cols.argtypes = [c_void_p] * 4
        L.sk_align_prepare.argtypes = [C.POINTER(AlignBatch), c_void_p, c_void_p]
        L.sk_score_alignments_dev.argtypes = [C.POINTER(AlignBatch), c_void_p, c_void_p]
        L.sk_score_alignments_dev_generic.argtypes = [C.POINTER(AlignBatch), c_void_p, c_void_p]
        L.sk_dependent_eprob.argtypes = [C.POINTER(PileupBatch), C.POINTER(GermlineOptions), c_void_p]
        L.sk_dependent_eprob_dev.argtypes = [C.POINTER(PileupBatch), C.POINTER(GermlineOptions), c_void_p, c_void_p,
                                             c_void_p]
        L.sk_site_digt_call.argtypes = [C.POINTER(PileupBatch), C.POINTER(GermlineOptions), c_void_p]
        L.sk_site_digt_call_dev.argtypes = [C.POINTER(PileupBatch), C.POINTER(GermlineOptions), c_void_p, c_void_p]
        L.sk_site_digt_call_fused.argtypes = [C.POINTER(PileupBatch), C.POINTER(GermlineOptions), c_void_p, c_void_p]
        L.sk_site_digt_call_fused_dev.argtypes = [C.POINTER(PileupBatch), C.POINTER(GermlineOptions), c_void_p, c_void_p,
                                                  C.c_int, c_void_p, C.c_int64, c_void_p]
        L.sk_somatic_snv_call_batch.argtypes = [C.POINTER(PileupBatch), C.POINTER(PileupBatch),
                                                C.POINTER(SomaticSnvOptions), C.c_int, c_void_p]
        L.sk_somatic_snv_call_batch_dev.argtypes = [C.POINTER(PileupBatch), C.POINTER(PileupBatch),
                                                    C.POINTER(SomaticSnvOptions), C.c_int, c_void_p, c_void_p, c_void_p]
        L.sk_indel_grid_lhood.argtypes = [C.POINTER(ReadScoreBatch), C.POINTER(IndelOptions), C.c_int, c_void_p]
        L.sk_indel_grid_lhood_dev.argtypes = [C.POINTER(ReadScoreBatch), C.POINTER(IndelOptions), C.c_int, c_void_p, c_void_p]
        L.sk_somatic_indel_call_batch.argtypes = [C.POINTER(ReadScoreBatch), C.POINTER(ReadScoreBatch),
                                                  C.POINTER(IndelOptions), C.POINTER(IndelOptions),
                                                  C.POINTER(SomaticIndelOptions), c_void_p, C.c_int, c_void_p]
        L.sk_allele_group_genotype_lhoods.argtypes = [C.POINTER(AlleleGroupBatch), C.POINTER(IndelOptions), c_void_p]
        L.sk_allele_group_genotype_lhoods_dev.argtypes = [C.POINTER(AlleleGroupBatch), C.POINTER(IndelOptions), c_void_p,
                                                          c_void_p]
        L.sk_allele_group_genotype_lhoods_wide_dev.argtypes = [C.POINTER(AlleleGroupBatch), C.POINTER(IndelOptions), c_void_p,
                                                          c_void_p]
        L.sk_allele_group_genotype_lhoods_wide.argtypes = [C.POINTER(AlleleGroupBatch), C.POINTER(IndelOptions), c_void_p]
        _lib = L
    return _lib


class StrelkaAmdError(RuntimeError):
    pass


def _check(rc):
    if rc != 0:
        raise StrelkaAmdError(lib().sk_last_error().decode("utf-8", "replace"))


def last_error():
    return lib().sk_last_error().decode("utf-8", "replace")


def init(device=0):
    _check(lib().sk_init(int(device)))


def init_strict(device=0):
    """sk_init_strict: also fails when the host libm is not the one the kernels restate (no bit-exactness otherwise)"""
    _check(lib().sk_init_strict(int(device)))


def shutdown():
    lib().sk_shutdown()


def debug_grown_bytes():
    """(device bytes, page-locked host bytes) the library's grown buffers hold at the moment (sk_debug_grown_bytes); (0, 0) after shutdown()"""
    dev, pinned = C.c_int64(-1), C.c_int64(-1)
    lib().sk_debug_grown_bytes(C.byref(dev), C.byref(pinned))
    return dev.value, pinned.value


def germline_options():
    o = GermlineOptions()
    lib().sk_germline_options_default(C.byref(o))
    return o


def somatic_snv_options():
    o = SomaticSnvOptions()
    lib().sk_somatic_snv_options_default(C.byref(o))
    return o


def qscore_tables():
    a = [np.zeros(71) for _ in range(3)]
    _check(lib().sk_get_qscore_tables(*[x.ctypes.data_as(c_void_p) for x in a]))
    return a


def _p(a):
    return None if a is None else a.ctypes.data_as(c_void_p)


# SK_LIBM_* of include/strelka_amd.h
LIBM_FN = {"logf": 0, "powf": 1, "expf": 2, "log1pf": 3, "exp": 4, "log": 5, "log10": 6, "log1p": 7,
           "sk_exp": 8, "sk_log": 9, "sk_log10": 10, "sk_log1p": 11, "logf_ref": 12, "dependent_eprob": 13,
           "ln_qphred_f": 14, "qphred_d": 15, "log1p_switch_d": 16, "log_sum2": 17, "log_sum2f": 18}
_LIBM_FLOAT_FNS = ("logf", "powf", "expf", "log1pf", "logf_ref", "dependent_eprob", "ln_qphred_f", "log_sum2f")


def debug_libm_eval(fn, a, b=None, variant=0):
    """(out, restated): the device's evaluation of one SK_LIBM_* function (by name) on every element of a (and b)
    (sk_debug_libm_eval); variant 0 = tables in constant memory, 1 = a block's LDS copy, 2 = the out-of-line twins"""
    t = np.float32 if fn in _LIBM_FLOAT_FNS else np.float64
    a = np.ascontiguousarray(a, t)
    if b is not None:
        b = np.ascontiguousarray(b, t)
        assert b.shape == a.shape
    out = np.zeros(len(a), np.int32 if fn in ("ln_qphred_f", "qphred_d") else t)
    restated = np.full(len(a), 255, np.uint8)
    rc = lib().sk_debug_libm_eval(LIBM_FN[fn], int(variant), len(a), _p(a), _p(b), _p(out), _p(restated))
    if rc < 0:
        raise ValueError(last_error())
    _check(rc)
    return out, restated


# ----------------------------------------------------------------------------------------------------------------------
# numpy-level views of the batches


class HostAlignBatch:
    """Host-side sk_align_batch held as numpy arrays."""

    def __init__(self, read_off, read_code, read_qual, hap_off, hap_code, cal_off, op_off, ops, max_read_len=None,
                 max_hap_len=None):
        self.read_off = np.ascontiguousarray(read_off, np.int64)
        self.read_code = np.ascontiguousarray(read_code, np.uint8)
        self.read_qual = np.ascontiguousarray(read_qual, np.uint8)
        self.hap_off = np.ascontiguousarray(hap_off, np.int64)
        self.hap_code = np.ascontiguousarray(hap_code, np.uint8)
        self.cal_off = np.ascontiguousarray(cal_off, np.int32)
        self.op_off = np.ascontiguousarray(op_off, np.int64)
        self.ops = np.ascontiguousarray(ops, SCORE_OP_DTYPE)
        self.n_reads = len(self.read_off) - 1
        self.n_cals = int(self.cal_off[-1]) if len(self.cal_off) else 0
        self.max_read_len = int(np.diff(self.read_off).max()) if max_read_len is None and self.n_reads else int(max_read_len or 0)
        self.max_hap_len = int(np.diff(self.hap_off).max()) if max_hap_len is None and self.n_reads else int(max_hap_len or 0)

        self.entries = self.evmask = None
        self.evmask_words = 0
        self.colmat = self.colmat_off = self.addmask = None

    def struct(self):
        return AlignBatch(self.n_reads, self.n_cals, len(self.ops), _p(self.read_off), _p(self.read_code),
                          _p(self.read_qual), _p(self.hap_off), _p(self.hap_code), _p(self.cal_off), _p(self.op_off),
                          _p(self.ops), self.max_read_len, self.max_hap_len,
                          None if self.entries is None else _p(self.entries),
                          None if self.evmask is None else _p(self.evmask), self.evmask_words,
                          None if self.colmat is None else _p(self.colmat),
                          None if self.colmat_off is None else _p(self.colmat_off),
                          None if self.addmask is None else _p(self.addmask))

    def prepare(self, columns=True):
        """sk_align_prepare (+ sk_align_prepare_cols): the device-ready forms of this batch -- transition entries + event masks,
        and the column form the streaming kernel reads"""
        if self.entries is None:
            self.evmask_words = lib().sk_align_evmask_words(self.max_read_len)
            ent = np.zeros(len(self.ops) + 2 * self.n_cals + 1, np.uint32)
            msk = np.zeros(self.n_reads * self.evmask_words + 1, np.uint32)
            s = self.struct()
            if lib().sk_align_prepare(C.byref(s), _p(ent), _p(msk)) != 0:
                raise StrelkaAmdError("sk_align_prepare failed")
            self.entries, self.evmask = ent, msk
        if self.colmat is None and columns:
            s = self.struct()
            words = lib().sk_align_colmat_words(C.byref(s))
            cm = np.zeros(words + 1, np.uint32)
            off = np.zeros(self.n_reads + 1, np.int64)
            am = np.zeros(self.n_reads * self.evmask_words + 1, np.uint32)
            if lib().sk_align_prepare_cols(C.byref(s), _p(cm), _p(off), _p(am)) != 0:
                raise StrelkaAmdError("sk_align_prepare_cols failed")
            self.colmat, self.colmat_off, self.addmask = cm, off, am
        return self


def score_alignments(batch):
    """Host-buffer entry point: returns float64[n_cals]."""
    out = np.zeros(batch.n_cals, np.float64)
    s = batch.struct()
    _check(lib().sk_score_alignments(C.byref(s), _p(out)))
    return out


class AlignBuilder:
    """sk_align_builder wrapper: add reads with reference-shaped candidate alignments, get a HostAlignBatch."""

    def __init__(self):
        self._b = lib().sk_align_builder_create()

    def __del__(self):
        try:
            if self._b:
                lib().sk_align_builder_destroy(self._b)
        except Exception:
            pass

    def clear(self):
        lib().sk_align_builder_clear(self._b)

    @staticmethod
    def _key(k, keep):
        if k is None:
            return IndelKey(0, 0, 0, 0, None, 0)
        seq = k.get("ins_seq", "").encode()
        keep.append(seq)
        return IndelKey(k["pos"], k["type"], k.get("del_len", 0), len(seq), seq, int(k.get("is_candidate", 1)))

    def add_read(self, read_code, read_qual, ref_seq, ref_offset, cals):
        """cals: list of dict(pos, path=[(type,len)...], indels=[dict(pos,type,del_len,ins_seq,is_candidate)],
        leading=None|dict, trailing=None|dict)"""
        read_code = np.ascontiguousarray(read_code, np.uint8)
        read_qual = np.ascontiguousarray(read_qual, np.uint8)
        keep = []
        arr = (CandidateAlignment * max(len(cals), 1))()
        for i, c in enumerate(cals):
            path = (PathSeg * max(len(c["path"]), 1))(*[PathSeg(t, l) for t, l in c["path"]])
            ind = (IndelKey * max(len(c["indels"]), 1))(*[self._key(k, keep) for k in c["indels"]])
            keep += [path, ind]
            arr[i] = CandidateAlignment(c["pos"], len(c["path"]), path, len(c["indels"]), ind,
                                        self._key(c.get("leading"), keep), self._key(c.get("trailing"), keep))
        ref = ref_seq.encode() if isinstance(ref_seq, str) else bytes(ref_seq)
        rc = lib().sk_align_builder_add_read(self._b, _p(read_code), _p(read_qual), len(read_code), ref, int(ref_offset),
                                             len(ref), arr, len(cals))
        if rc != 0:
            raise StrelkaAmdError(lib().sk_align_builder_error(self._b).decode())

    def finish(self):
        s = AlignBatch()
        if lib().sk_align_builder_finish(self._b, C.byref(s)) != 0:
            raise StrelkaAmdError("sk_align_builder_finish failed")
        return _host_batch_from_struct(s)


def _host_batch_from_struct(s):
    def arr(ptr, n, dt):
        if n == 0 or not ptr:
            return np.zeros(0, dt)
        buf = (C.c_char * (n * np.dtype(dt).itemsize)).from_address(ptr)
        return np.frombuffer(buf, dtype=dt).copy()

    n, nc = s.n_reads, s.n_cals
    read_off = arr(s.read_off, n + 1, np.int64)
    hap_off = arr(s.hap_off, n + 1, np.int64)
    return HostAlignBatch(read_off, arr(s.read_code, int(read_off[-1]), np.uint8),
                          arr(s.read_qual, int(read_off[-1]), np.uint8), hap_off,
                          arr(s.hap_code, int(hap_off[-1]), np.uint8), arr(s.cal_off, n + 1, np.int32),
                          arr(s.op_off, nc + 1, np.int64), arr(s.ops, s.n_ops, SCORE_OP_DTYPE), s.max_read_len,
                          s.max_hap_len)


class HostPileupBatch:
    def __init__(self, call_off, calls, ref_base, de=None, ploidy=None):
        self.call_off = np.ascontiguousarray(call_off, np.int64)
        self.calls = np.ascontiguousarray(calls, np.uint16)
        self.ref_base = np.ascontiguousarray(ref_base, np.uint8)
        self.de = None if de is None else np.ascontiguousarray(de, np.float32)
        self.ploidy = None if ploidy is None else np.ascontiguousarray(ploidy, np.uint8)
        self.n_loci = len(self.call_off) - 1

    def struct(self):
        return PileupBatch(self.n_loci, _p(self.call_off), _p(self.calls), _p(self.de), _p(self.ref_base), _p(self.ploidy))


def dependent_eprob(batch, opt=None):
    opt = opt or germline_options()
    out = np.zeros(len(batch.calls), np.float32)
    s = batch.struct()
    _check(lib().sk_dependent_eprob(C.byref(s), C.byref(opt), _p(out)))
    return out


def site_digt_call(batch, opt=None):
    opt = opt or germline_options()
    out = np.zeros(batch.n_loci, DIGT_CALL_DTYPE)
    s = batch.struct()
    _check(lib().sk_site_digt_call(C.byref(s), C.byref(opt), _p(out)))
    return out


def site_digt_call_fused(batch, opt=None, want_de=False):
    """a9+a10 in one pass; returns (calls, de or None)."""
    opt = opt or germline_options()
    out = np.zeros(batch.n_loci, DIGT_CALL_DTYPE)
    de = np.zeros(len(batch.calls), np.float32) if want_de else None
    s = batch.struct()
    _check(lib().sk_site_digt_call_fused(C.byref(s), C.byref(opt), _p(out), _p(de)))
    return out, de


def gvcf_site_summaries(batch, genotypes):
    """sk_gvcf_site_summary of every locus of `batch` (its cleaned columns) given the genotype records sk_site_digt_call_fused left"""
    out = np.zeros(batch.n_loci, GVCF_SITE_SUMMARY_DTYPE)
    s = batch.struct()
    g = np.ascontiguousarray(genotypes)
    _check(lib().sk_gvcf_site_summaries(C.byref(s), _p(g), _p(out)))
    return out


def gvcf_plain_runs(summary, clean_count, raw_count, mapq_count, opt, library=None):
    """sk_gvcf_run of every site (library: the ctypes handle to drive -- default the product library; the tests also drive the CPU double)"""
    L = library or lib()
    n = len(summary)
    out = np.zeros(n, GVCF_RUN_DTYPE)
    sm, cc, rc, mq = (np.ascontiguousarray(a, dt) for a, dt in ((summary, GVCF_SITE_SUMMARY_DTYPE), (clean_count, np.uint32), (raw_count, np.uint32),
                                                                (mapq_count, np.uint32)))
    L.sk_gvcf_plain_runs.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, C.c_int32, c_void_p]
    L.sk_last_error.restype = C.c_char_p
    if L.sk_gvcf_plain_runs(_p(sm), _p(cc), _p(rc), _p(mq), C.byref(opt), n, _p(out)) != 0:
        raise RuntimeError(L.sk_last_error().decode())
    return out


def somatic_snv_call(normal, tumor, opt=None, is_forced_output=False):
    opt = opt or somatic_snv_options()
    out = np.zeros(normal.n_loci, SOMATIC_CALL_DTYPE)
    sn, st = normal.struct(), tumor.struct()
    _check(lib().sk_somatic_snv_call_batch(C.byref(sn), C.byref(st), C.byref(opt), int(is_forced_output), _p(out)))
    return out


SOMATIC_GENOTYPE_DTYPE = np.dtype([
    ("ref_gt", np.uint32), ("snv_tier", np.uint8), ("snv_from_ntype_tier", np.uint8), ("is_forced_output", np.uint8),
    ("is_computed", np.uint8), ("ntype", np.uint32), ("max_gt", np.uint32), ("qphred", np.int32),
    ("from_ntype_qphred", np.int32), ("nonsomatic_qphred", np.int32), ("normal_alt_id", np.uint32),
    ("tumor_alt_id", np.uint32), ("_pad", np.int32), ("strand_bias", np.float64)], align=True)
assert SOMATIC_GENOTYPE_DTYPE.itemsize == 48


def somatic_snv_call_tiers(normal_t1, tumor_t1, normal_t2=None, tumor_t2=None, opt=None, is_forced_output=None,
                           is_compute_nonsomatic=False):
    """sk_somatic_snv_call_tiers: the whole of position_somatic_snv_call (both tiers)."""
    opt = opt or somatic_snv_options()
    n = normal_t1.n_loci
    out = np.zeros(n, SOMATIC_GENOTYPE_DTYPE)
    s1, s2 = normal_t1.struct(), tumor_t1.struct()
    if normal_t2 is not None:
        s3, s4 = normal_t2.struct(), tumor_t2.struct()
        p3, p4 = C.byref(s3), C.byref(s4)
    else:
        p3 = p4 = None
    forced = None if is_forced_output is None else np.ascontiguousarray(is_forced_output, np.uint8)
    L = lib()
    L.sk_somatic_snv_call_tiers.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_void_p]
    _check(L.sk_somatic_snv_call_tiers(C.cast(C.byref(s1), C.c_void_p), C.cast(C.byref(s2), C.c_void_p),
                                       C.cast(p3, C.c_void_p) if p3 is not None else None,
                                       C.cast(p4, C.c_void_p) if p4 is not None else None,
                                       C.cast(C.byref(opt), C.c_void_p), _p(forced), int(bool(is_compute_nonsomatic)), _p(out)))
    return out


def make_call(q, base, fwd=1, nmm=0, filt=0, tscf=0):
    """SK_MAKE_CALL (vectorised)."""
    q, base, fwd, nmm, filt, tscf = [np.asarray(x, np.uint16) for x in (q, base, fwd, nmm, filt, tscf)]
    return ((q & 0x3f) | ((base & 0xf) << 6) | ((fwd & 1) << 10) | ((nmm & 1) << 11) | ((filt & 1) << 12) |
            ((tscf & 1) << 13)).astype(np.uint16)


# ----------------------------------------------------------------------------------------------------------------------
# indels

def indel_options(is_somatic=False, exact=True):
    """sk_indel_options_default; `exact` (the default HERE: these helpers serve tests that compare doubles bit for bit with the oracle)
    asks for the reference's operation order -- the library's own default is the fast form (sk_indel_options.fast_form)."""
    o = IndelOptions()
    lib().sk_indel_options_default(C.byref(o), int(is_somatic))
    if exact:
        o.fast_form = 0
    return o


def somatic_indel_options():
    o = SomaticIndelOptions()
    lib().sk_somatic_indel_options_default(C.byref(o))
    return o


class HostReadScoreBatch:
    def __init__(self, read_off, ref_lnp, indel_lnp, alt_lnp, non_ambig, read_length, read_flags, del_len, ins_len,
                 is_breakpoint=None):
        self.read_off = np.ascontiguousarray(read_off, np.int64)
        self.ref_lnp = np.ascontiguousarray(ref_lnp, np.float32)
        self.indel_lnp = np.ascontiguousarray(indel_lnp, np.float32)
        self.alt_lnp = None if alt_lnp is None else np.ascontiguousarray(alt_lnp, np.float32)
        self.non_ambig = np.ascontiguousarray(non_ambig, np.uint16)
        self.read_length = np.ascontiguousarray(read_length, np.uint16)
        self.read_flags = np.ascontiguousarray(read_flags, np.uint8)
        self.del_len = np.ascontiguousarray(del_len, np.uint32)
        self.ins_len = np.ascontiguousarray(ins_len, np.uint32)
        self.is_breakpoint = None if is_breakpoint is None else np.ascontiguousarray(is_breakpoint, np.uint8)
        self.n_indels = len(self.read_off) - 1

    def struct(self):
        return ReadScoreBatch(self.n_indels, _p(self.read_off), _p(self.ref_lnp), _p(self.indel_lnp), _p(self.alt_lnp),
                              _p(self.non_ambig), _p(self.read_length), _p(self.read_flags), _p(self.del_len),
                              _p(self.ins_len), _p(self.is_breakpoint))


class AltAllele(C.Structure):
    _fields_ = [("begin_pos", C.c_int32), ("end_pos", C.c_int32), ("is_mismatch", C.c_int32)]


class SomaticIndelBatch(C.Structure):
    _fields_ = [("n_indels", C.c_int32), ("normal", ReadScoreBatch), ("tumor", ReadScoreBatch),
                ("normal_alt_key", c_void_p), ("normal_alt_lnp", c_void_p), ("tumor_alt_key", c_void_p),
                ("tumor_alt_lnp", c_void_p), ("alt_off", c_void_p), ("alt_alleles", c_void_p),
                ("indel_to_ref_error_prob", c_void_p), ("is_forced_output", c_void_p)]


SOMATIC_INDEL_GENOTYPE_DTYPE = np.dtype([("sindel_tier", np.uint8), ("sindel_from_ntype_tier", np.uint8),
                                         ("is_forced_output", np.uint8), ("is_overlap", np.uint8), ("ntype", np.uint32),
                                         ("max_gt", np.uint32), ("qphred", np.int32), ("from_ntype_qphred", np.int32)])
assert SOMATIC_INDEL_GENOTYPE_DTYPE.itemsize == 20


class HostSomaticIndelBatch:
    """sk_somatic_indel_batch from per-indel cases (strelka_amd.synth.somatic_indel_cases layout)."""

    def __init__(self, cases):
        n = len(cases)
        self.n = n

        def sample(name):
            off = np.zeros(n + 1, np.int64)
            np.cumsum([len(c[name]["ref_lnp"]) for c in cases], out=off[1:])
            cat = lambda k, dt: np.ascontiguousarray(np.concatenate([np.asarray(c[name][k]).reshape(len(c[name]["ref_lnp"]), -1) for c in cases] or [np.zeros((0, 1))]), dt)
            alt_key = cat("alt_key", np.int32).reshape(-1, 2)
            alt_lnp = cat("alt_lnp", np.float32).reshape(-1, 2)
            best = np.where(alt_key >= 0, alt_lnp, -np.inf).max(axis=1) if len(alt_key) else np.zeros(0)
            best = np.where((alt_key >= 0).any(axis=1), best, np.nan).astype(np.float32) if len(alt_key) else np.zeros(0, np.float32)
            t1 = cat("is_tier1", np.uint8).ravel()
            b = HostReadScoreBatch(off, cat("ref_lnp", np.float32).ravel(), cat("indel_lnp", np.float32).ravel(), best,
                                   cat("non_ambig", np.uint16).ravel(), cat("read_length", np.uint16).ravel(),
                                   (t1 & 1) | 2, [c["del_len"] for c in cases], [c["ins_len"] for c in cases])
            return b, np.ascontiguousarray(alt_key), np.ascontiguousarray(alt_lnp)

        self.normal, self.n_alt_key, self.n_alt_lnp = sample("normal")
        self.tumor, self.t_alt_key, self.t_alt_lnp = sample("tumor")
        self.alt_off = np.zeros(n + 1, np.int64)
        np.cumsum([len(c["alt_keys"]) for c in cases], out=self.alt_off[1:])
        keys = [k for c in cases for k in c["alt_keys"]]
        self.alleles = np.ascontiguousarray(np.array(keys, np.int32).reshape(-1, 3))
        self.err = np.ascontiguousarray([c["indel_to_ref_error_prob"] for c in cases], np.float64)
        self.forced = np.ascontiguousarray([c["forced"] for c in cases], np.uint8)

    def struct(self):
        return SomaticIndelBatch(self.n, self.normal.struct(), self.tumor.struct(), _p(self.n_alt_key), _p(self.n_alt_lnp),
                                 _p(self.t_alt_key), _p(self.t_alt_lnp), _p(self.alt_off), _p(self.alleles), _p(self.err),
                                 _p(self.forced))


def somatic_indel_call_tiers(cases, normal_opt=None, tumor_opt=None, sopt=None, use_tier2_evidence=True):
    """sk_somatic_indel_call_tiers: the whole of get_somatic_indel per candidate indel."""
    if normal_opt is None:
        normal_opt = indel_options(True)
        normal_opt.min_read_bp_flank = 1
    tumor_opt = tumor_opt or indel_options(True)
    sopt = sopt or somatic_indel_options()
    b = HostSomaticIndelBatch(cases)
    out = np.zeros(b.n, SOMATIC_INDEL_GENOTYPE_DTYPE)
    s = b.struct()
    _check(lib().sk_somatic_indel_call_tiers(C.byref(s), C.byref(normal_opt), C.byref(tumor_opt), C.byref(sopt),
                                             int(bool(use_tier2_evidence)), _p(out)))
    return out


def indel_grid_lhood(batch, opt=None, is_include_tier2=False):
    opt = opt or indel_options(True)
    out = np.zeros((batch.n_indels, 21), np.float64)
    s = batch.struct()
    _check(lib().sk_indel_grid_lhood(C.byref(s), C.byref(opt), int(is_include_tier2), _p(out)))
    return out


def somatic_indel_call(normal, tumor, indel_to_ref_error_prob, normal_opt=None, tumor_opt=None, sopt=None,
                       is_include_tier2=False):
    if normal_opt is None:
        normal_opt = indel_options(True)
        normal_opt.min_read_bp_flank = 1
    tumor_opt = tumor_opt or indel_options(True)
    sopt = sopt or somatic_indel_options()
    out = np.zeros(normal.n_indels, SOMATIC_INDEL_CALL_DTYPE)
    err = np.ascontiguousarray(indel_to_ref_error_prob, np.float64)
    sn, st = normal.struct(), tumor.struct()
    _check(lib().sk_somatic_indel_call_batch(C.byref(sn), C.byref(st), C.byref(normal_opt), C.byref(tumor_opt),
                                             C.byref(sopt), _p(err), int(is_include_tier2), _p(out)))
    return out


class HostAlleleGroupBatch:
    def __init__(self, read_off, n_alt, ploidy, del_len, ins_len, ref_lnp, allele_lnp, non_ambig, read_length, read_flags, width=MAX_ALT):
        assert width in (MAX_ALT, MAX_ALT_WIDE, MAX_ALT_XWIDE)
        self.width = width  # columns of the per-allele arrays: MAX_ALT, or MAX_ALT_WIDE / MAX_ALT_XWIDE for the wide entry points
        self.read_off = np.ascontiguousarray(read_off, np.int64)
        self.n_alt = np.ascontiguousarray(n_alt, np.uint8)
        self.ploidy = np.ascontiguousarray(ploidy, np.uint8)
        self.del_len = np.ascontiguousarray(del_len, np.uint32).reshape(-1, width)
        self.ins_len = np.ascontiguousarray(ins_len, np.uint32).reshape(-1, width)
        self.ref_lnp = np.ascontiguousarray(ref_lnp, np.float32).reshape(-1, width)
        self.allele_lnp = np.ascontiguousarray(allele_lnp, np.float32).reshape(-1, width)
        self.non_ambig = np.ascontiguousarray(non_ambig, np.uint16)
        self.read_length = np.ascontiguousarray(read_length, np.uint16)
        self.read_flags = np.ascontiguousarray(read_flags, np.uint8)
        self.n_groups = len(self.read_off) - 1

    def struct(self):
        return AlleleGroupBatch(self.n_groups, _p(self.read_off), _p(self.n_alt), _p(self.ploidy), _p(self.del_len),
                                _p(self.ins_len), _p(self.ref_lnp), _p(self.allele_lnp), _p(self.non_ambig),
                                _p(self.read_length), _p(self.read_flags))


def allele_group_genotype_lhoods(batch, opt=None):
    opt = opt or indel_options(False)
    width = getattr(batch, "width", MAX_ALT)
    dtype, fn = {MAX_ALT: (ALLELE_GROUP_CALL_DTYPE, "sk_allele_group_genotype_lhoods"),
                 MAX_ALT_WIDE: (ALLELE_GROUP_CALL_WIDE_DTYPE, "sk_allele_group_genotype_lhoods_wide"),
                 MAX_ALT_XWIDE: (ALLELE_GROUP_CALL_XWIDE_DTYPE, "sk_allele_group_genotype_lhoods_xwide")}[width]
    out = np.zeros(batch.n_groups, dtype)
    s = batch.struct()
    f = getattr(lib(), fn)
    f.argtypes = [C.POINTER(AlleleGroupBatch), C.POINTER(IndelOptions), c_void_p]
    _check(f(C.byref(s), C.byref(opt), _p(out)))
    return out


# ---------------------------------------------------------------------------------------------------- realign job

def cigar_to_path(cigar):
    out, num = [], ""
    for ch in cigar:
        if ch.isdigit():
            num += ch
        else:
            out.append((CIGAR_CHARS.index(ch), int(num)))
            num = ""
    return out


def path_to_cigar(path):
    return "".join("%d%s" % (l, CIGAR_CHARS[t]) for t, l in path)


def realign_options(**kw):
    o = RealignOptions()
    lib().sk_realign_options_default(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise AttributeError(k)
        setattr(o, k, v)
    return o


def _ckeys(keys, keep):
    arr = (IndelKey * max(len(keys), 1))()
    for i, k in enumerate(keys):
        arr[i] = AlignBuilder._key(k, keep)
    return arr


def make_start_pos_alignment(ref_start_pos, read_start_pos, is_fwd, read_length, indels):
    """-> dict(pos, path, leading, trailing) (indices into `indels`) or None when the arguments are rejected"""
    keep = []
    arr = _ckeys(indels, keep)
    cap = 2 * len(indels) + 4
    path = (PathSeg * cap)()
    pos, lead, trail = C.c_int32(), C.c_int32(), C.c_int32()
    n = lib().sk_make_start_pos_alignment(ref_start_pos, read_start_pos, int(is_fwd), read_length, arr, len(indels),
                                          C.byref(pos), path, cap, C.byref(lead), C.byref(trail))
    if n < 0:
        return None
    return dict(pos=pos.value, path=[(path[i].type, path[i].length) for i in range(n)], leading=lead.value,
                trailing=trail.value)


def get_end_pin_start_pos(indels, read_length, ref_end_pos, read_end_pos):
    keep = []
    arr = _ckeys(indels, keep)
    a, b = C.c_int32(), C.c_int32()
    if lib().sk_get_end_pin_start_pos(arr, len(indels), read_length, ref_end_pos, read_end_pos, C.byref(a), C.byref(b)):
        return None
    return a.value, b.value


class RealignJob:
    """sk_realign_job wrapper (realignAndScoreRead as a batched job)."""

    def __init__(self, opt=None):
        self.opt = opt or realign_options()
        self._j = lib().sk_realign_job_create(C.byref(self.opt))
        if not self._j:
            raise StrelkaAmdError("sk_realign_job_create failed")
        self._keep = []

    def __del__(self):
        try:
            if self._j:
                lib().sk_realign_job_destroy(self._j)
        except Exception:
            pass

    def _err(self):
        return StrelkaAmdError(lib().sk_realign_job_error(self._j).decode())

    def set_reference(self, seq, offset=0):
        b = seq.encode()
        if lib().sk_realign_job_set_reference(self._j, b, offset, len(b)):
            raise self._err()

    def set_indels(self, indels):
        """indels: dicts(pos,type,del_len,ins_seq,is_candidate, r2i, i2r [, arid, hap, bypass, forced, ndfr])"""
        keep = []
        arr = (IndelInfo * max(len(indels), 1))()
        for i, d in enumerate(indels):
            a = arr[i]
            a.key = AlignBuilder._key(d, keep)
            a.ref_to_indel_log_prob = d.get("r2i", 0.0)
            a.indel_to_ref_log_prob = d.get("i2r", 0.0)
            a.active_region_id = d.get("arid", -1)
            hap = d.get("hap", 0)
            byp = d.get("bypass", 0)
            for s in range(MAX_SAMPLES):
                a.haplotype_id[s] = (hap[s] if s < len(hap) else 0) if isinstance(hap, (list, tuple)) else hap
                a.is_haplotyping_bypassed[s] = (byp[s] if s < len(byp) else 0) if isinstance(byp, (list, tuple)) else byp
            a.is_forced_output = int(d.get("forced", 0))
            a.not_discovered_from_reads = int(d.get("ndfr", 0))
        if lib().sk_realign_job_set_indels(self._j, arr, len(indels)):
            raise self._err()
        self._n_indels = len(indels)

    def add_read(self, read_code, read_qual, pos, path, is_fwd=True, map_level=1, sample=0, realign_range=(0, 1 << 30),
                 observed=()):
        code = np.ascontiguousarray(read_code, np.uint8)
        qual = np.ascontiguousarray(read_qual, np.uint8)
        segs = (PathSeg * max(len(path), 1))(*[PathSeg(t, l) for t, l in path])
        obs = (C.c_int32 * max(len(observed), 1))(*observed)
        r = ReadInput(_p(code), _p(qual), len(code), pos, len(path), segs, int(is_fwd), map_level, sample,
                      realign_range[0], realign_range[1], len(observed), obs)
        i = lib().sk_realign_job_add_read(self._j, C.byref(r))
        if i < 0:
            raise self._err()
        return i

    def add_reads(self, reads):
        """reads: [(read_code, read_qual, pos, path, is_fwd, map_level, sample, realign_range, observed)] -> first index"""
        n = len(reads)
        arr = (ReadInput * max(n, 1))()
        keep = []
        for i, (read_code, read_qual, pos, path, is_fwd, map_level, sample, realign_range, observed) in enumerate(reads):
            code = np.ascontiguousarray(read_code, np.uint8)
            qual = np.ascontiguousarray(read_qual, np.uint8)
            segs = (PathSeg * max(len(path), 1))(*[PathSeg(t, l) for t, l in path])
            obs = (C.c_int32 * max(len(observed), 1))(*observed)
            keep.append((code, qual, segs, obs))
            arr[i] = ReadInput(_p(code), _p(qual), len(code), pos, len(path), segs, int(is_fwd), map_level, sample,
                               realign_range[0], realign_range[1], len(observed), obs)
        first = lib().sk_realign_job_add_reads(self._j, arr, n)
        if first < 0:
            raise self._err()
        return first

    def add_reads_prepared(self, reads, prepared):
        """reads as add_reads takes them (their observed lists are not read), prepared: REALIGN_PREPARED_READ_DTYPE[len(reads)] as realign_preamble
        leaves them -> first index.  Needs enumeration == 2 and set_indels given the gate's keys in table order; the job then reports only the
        consulted marks of the search: gate_consulted | preamble_consulted are the caller's to add."""
        n = len(reads)
        prepared = np.ascontiguousarray(prepared, REALIGN_PREPARED_READ_DTYPE)
        assert len(prepared) == n
        arr = (ReadInput * max(n, 1))()
        keep = []
        for i, (read_code, read_qual, pos, path, is_fwd, map_level, sample, realign_range, observed) in enumerate(reads):
            code = np.ascontiguousarray(read_code, np.uint8)
            qual = np.ascontiguousarray(read_qual, np.uint8)
            segs = (PathSeg * max(len(path), 1))(*[PathSeg(t, l) for t, l in path])
            keep.append((code, qual, segs))
            arr[i] = ReadInput(_p(code), _p(qual), len(code), pos, len(path), segs, int(is_fwd), map_level, sample, realign_range[0], realign_range[1], 0, None)
        first = lib().sk_realign_job_add_reads_prepared(self._j, arr, _p(prepared) if n else None, n)
        if first < 0:
            raise self._err()
        return first

    def debug_prepared(self, i):
        """the record the job's own preamble makes for read i (sk_debug_realign_job_prepared) as a REALIGN_PREPARED_READ_DTYPE scalar, or None when the read
        has none (it left at the gate, at a capacity or at a negative position)"""
        out = np.zeros(1, REALIGN_PREPARED_READ_DTYPE)
        rc = lib().sk_debug_realign_job_prepared(self._j, int(i), _p(out))
        if rc < 0:
            raise StrelkaAmdError("sk_debug_realign_job_prepared: bad argument")
        return None if rc else out[0]

    def batch(self):
        s = AlignBatch()
        if lib().sk_realign_job_get_batch(self._j, C.byref(s)):
            raise self._err()
        return _host_batch_from_struct(s)

    def finish(self, scores):
        scores = np.ascontiguousarray(scores, np.float64)
        if lib().sk_realign_job_finish(self._j, _p(scores)):
            raise self._err()

    def run(self):
        if lib().sk_realign_job_run(self._j):
            raise self._err()

    def n_reads(self):
        return lib().sk_realign_job_n_reads(self._j)

    def indels_consulted(self):
        """uint8 per indel of the table as given to set_indels: candidate status consulted by any read so far"""
        out = np.zeros(max(self._n_indels, 1), np.uint8)
        if lib().sk_realign_job_indels_consulted(self._j, _p(out), self._n_indels):
            raise self._err()
        return out[:self._n_indels]

    def enumeration_counts(self):
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        lib().sk_realign_job_enumeration_counts(self._j, C.byref(a), C.byref(b), C.byref(c))
        return a.value, b.value, c.value

    @staticmethod
    def device_job_counts():
        """(jobs run as one fixed sequence with one wait, of those run again the staged way, jobs run the staged way) of this process"""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        lib().sk_realign_device_job_counts(C.byref(a), C.byref(b), C.byref(c))
        return a.value, b.value, c.value

    @staticmethod
    def f5_tail_launches():
        """launches of the table kernel of F5's last hand-outs by this process's job runs (sk_debug_f5_tail_launches)"""
        return int(lib().sk_debug_f5_tail_launches())

    @staticmethod
    def f5_shared_rounds():
        """rounds of F5 scored by a wave other than their read's owner, over this process's job runs (sk_debug_f5_shared_rounds)"""
        return int(lib().sk_debug_f5_shared_rounds())

    @staticmethod
    def f5_late_turn_downs():
        """rounds after a read's first in which F5 left the job to the staged kernels, over this process's job runs (sk_debug_f5_late_turn_downs)"""
        return int(lib().sk_debug_f5_late_turn_downs())

    @staticmethod
    def f5_tail_order(cal_off, waves, shift):
        """(first, order): the table of F5's last hand-outs as the device builds it for reads with the offsets cal_off[n_reads + 1], a
        grid of `waves` waves and a shift of `shift` hand-outs per round (sk_debug_f5_tail_order); order is empty when none is built"""
        cal_off = np.ascontiguousarray(cal_off, np.int32)
        n_reads = len(cal_off) - 1
        first, n = C.c_int32(-1), C.c_int32(-1)
        order = np.full(max(n_reads, 1), -2, np.int32)
        if lib().sk_debug_f5_tail_order(_p(cal_off), n_reads, int(waves), int(shift), C.byref(first), C.byref(n), _p(order)):
            raise StrelkaAmdError(last_error())
        return first.value, order[:n.value].copy()

    def stage3_counts(self):
        a, b = C.c_int64(), C.c_int64()
        lib().sk_realign_job_stage3_counts(self._j, C.byref(a), C.byref(b))
        return a.value, b.value

    def clear_reads(self):
        lib().sk_realign_job_clear_reads(self._j)

    def result(self, i):
        r = ReadResult()
        if lib().sk_realign_job_read_result(self._j, i, C.byref(r)):
            raise StrelkaAmdError("bad read index")
        scores = []
        for q in range(r.n_scores):
            s = r.scores[q]
            scores.append(dict(indel=s.indel, ref_lnp=s.ref_lnp, indel_lnp=s.indel_lnp, non_ambig=s.non_ambig,
                               read_length=s.read_length, is_tier1_read=s.is_tier1_read, is_fwd_strand=s.is_fwd_strand,
                               read_pos=s.read_pos, edge_dist=s.distance_from_closest_read_edge,
                               alt=[(s.alt_indel[a], s.alt_lnp[a]) for a in range(s.n_alt)]))
        return dict(n_cals=r.n_candidate_alignments, is_realigned=bool(r.is_realigned), pos=r.realign_pos,
                    path=[(r.realign_path[i].type, r.realign_path[i].length) for i in range(r.realign_n_seg)],
                    max_score=r.max_score, scores=scores, suboverlap=[r.suboverlap[i] for i in range(r.n_suboverlap)],
                    warn_origin_skip=bool(r.warn_origin_skip), warn_max_toggle_depth=bool(r.warn_max_toggle_depth))


# ---------------------------------------------------------------------------------------------------- pileup (a8)

def pileup_options(**kw):
    o = PileupOptions()
    lib().sk_pileup_options_default(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise AttributeError(k)
        setattr(o, k, v)
    return o


def pileup_reads(rb, opt, mode):
    """rb: synth.ReadBatch (host arrays) -> (call_off, calls, spandel_count, submapped_count)"""
    ref = np.frombuffer(rb.ref_seq.encode(), np.uint8).copy()
    s = ReadBatchStruct(rb.n_reads, _p(rb.read_off), _p(rb.read_code), _p(rb.read_qual), _p(rb.path_off), _p(rb.path),
                        _p(rb.pos), _p(rb.is_fwd), _p(rb.mapq), _p(rb.map_level), _p(ref), rb.ref_offset, len(ref),
                        None if rb.cand_snv_mask is None else _p(rb.cand_snv_mask))
    n_loci = opt.report_end - opt.report_begin
    cap = 2 * rb.n_bases + 1
    call_off = np.zeros(n_loci + 1, np.int64)
    calls = np.zeros(cap, np.uint16)
    sd = np.zeros(max(n_loci, 1), np.uint32)
    sm = np.zeros(max(n_loci, 1), np.uint32)
    out = PileupColumns(n_loci, cap, _p(call_off), _p(calls), _p(sd), _p(sm))
    _check(lib().sk_pileup_reads(C.byref(s), C.byref(opt), mode, C.byref(out)))
    return call_off, calls[:call_off[-1]].copy(), sd[:n_loci], sm[:n_loci]


class PileupStream:
    """sk_pileup_stream_*: one sample's pileup over a region, pushed window by window (row a8 chained into a9+a10).
    `library`: the ctypes handle to drive (default: the product library; the tests also drive the CPU double with it)."""

    def __init__(self, opt, germline_opt=None, library=None, evs_words=False, gvcf_block_opt=None):
        self.L = library or lib()
        L = self.L
        self.evs_words = evs_words
        self.gvcf_block_opt = gvcf_block_opt
        L.sk_pileup_stream_enable_evs_words.argtypes = [c_void_p, C.c_int]
        L.sk_pileup_stream_create.restype = c_void_p
        L.sk_pileup_stream_create.argtypes = [C.POINTER(PileupOptions), c_void_p]
        L.sk_pileup_stream_destroy.argtypes = [c_void_p]
        L.sk_pileup_stream_begin_region.argtypes = [c_void_p, C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
        L.sk_pileup_stream_push.argtypes = [c_void_p, C.POINTER(ReadBatchStruct), C.c_int32, C.c_int32, C.c_int32, c_void_p, C.c_int32,
                                            C.c_int32, C.c_int32, c_void_p, C.POINTER(PileupWindow)]
        L.sk_last_error.restype = C.c_char_p
        self.genotype = germline_opt is not None
        self.h = L.sk_pileup_stream_create(C.byref(opt), C.byref(germline_opt) if self.genotype else None)
        if not self.h:
            raise RuntimeError(L.sk_last_error().decode())
        if gvcf_block_opt is not None:
            L.sk_pileup_stream_set_gvcf_block_options.argtypes = [c_void_p, c_void_p]
            if L.sk_pileup_stream_set_gvcf_block_options(self.h, C.byref(gvcf_block_opt)) != 0:
                raise RuntimeError(L.sk_last_error().decode())
        if evs_words and L.sk_pileup_stream_enable_evs_words(self.h, 1) != 0:
            raise RuntimeError(L.sk_last_error().decode())

    def close(self):
        if self.h:
            self.L.sk_pileup_stream_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise RuntimeError(self.L.sk_last_error().decode())

    def begin_region(self, ref_seq, ref_offset, report_begin, report_end, span=49):
        ref = ref_seq.encode()
        self._check(self.L.sk_pileup_stream_begin_region(self.h, ref, ref_offset, len(ref), report_begin, report_end, span))

    def push_raw(self, rb, final_to, span=49):
        """push without copying the window out (bench): -> (begin, end)"""
        s = ReadBatchStruct(rb.n_reads, _p(rb.read_off), _p(rb.read_code), _p(rb.read_qual), _p(rb.path_off), _p(rb.path),
                            _p(rb.pos), _p(rb.is_fwd), _p(rb.mapq), _p(rb.map_level), None, 0, 0, None)
        w = PileupWindow()
        self._check(self.L.sk_pileup_stream_push(self.h, C.byref(s), span, 0, 0, None, min(final_to, 2**31 - 1), 0, 0, None, C.byref(w)))
        return w.begin, w.end

    def push(self, rb, final_to, mask=None, mask_begin=0, ploidy=None, ploidy_begin=0, span=49, halves=False, between=None):
        """rb: synth.ReadBatch (its reference / mask fields are ignored) -> dict of numpy copies for [begin, end).
        halves: as sk_pileup_stream_push_begin + _finish, `between()` called while the window is in flight"""
        s = ReadBatchStruct(rb.n_reads, _p(rb.read_off), _p(rb.read_code), _p(rb.read_qual), _p(rb.path_off), _p(rb.path),
                            _p(rb.pos), _p(rb.is_fwd), _p(rb.mapq), _p(rb.map_level), None, 0, 0, None)
        w = PileupWindow()
        mask = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        ploidy = None if ploidy is None else np.ascontiguousarray(ploidy, np.uint8)
        if halves:
            self.L.sk_pileup_stream_push_begin.argtypes = self.L.sk_pileup_stream_push.argtypes[:-1]
            self.L.sk_pileup_stream_push_finish.argtypes = [c_void_p, C.POINTER(PileupWindow)]
            self._check(self.L.sk_pileup_stream_push_begin(self.h, C.byref(s), span, mask_begin, 0 if mask is None else len(mask), _p(mask),
                                                            min(final_to, 2**31 - 1), ploidy_begin, 0 if ploidy is None else len(ploidy),
                                                            _p(ploidy)))
            if between is not None:
                between()
            self._check(self.L.sk_pileup_stream_push_finish(self.h, C.byref(w)))
        else:
            self._check(self.L.sk_pileup_stream_push(self.h, C.byref(s), span, mask_begin, 0 if mask is None else len(mask), _p(mask),
                                                      min(final_to, 2**31 - 1), ploidy_begin, 0 if ploidy is None else len(ploidy), _p(ploidy),
                                                      C.byref(w)))
        n = w.end - w.begin

        def arr(ptr, dt, k):
            if k == 0 or not ptr:
                return np.zeros(0, dt)
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(np.ctypeslib.as_ctypes_type(np.dtype(dt)))), shape=(k,)).copy()

        def rec(ptr, dt, k):
            if k == 0 or not ptr:
                return np.zeros(0, dt)
            buf = (C.c_char * (dt.itemsize * k)).from_address(ptr)
            return np.frombuffer(buf, dt, k).copy()
        o1 = arr(w.tier1_off, np.int64, n + 1)
        o2 = arr(w.tier2_off, np.int64, n + 1)
        return dict(begin=w.begin, end=w.end, tier1_off=o1, tier1_calls=arr(w.tier1_calls, np.uint16, int(o1[-1]) if n else 0),
                    tier2_off=o2, tier2_calls=arr(w.tier2_calls, np.uint16, int(o2[-1]) if n else 0),
                    spandel=arr(w.spandel_count, np.uint32, n), submapped=arr(w.submapped_count, np.uint32, n),
                    mapq_count=arr(w.mapq_count, np.uint32, n), mapq_zero=arr(w.mapq_zero_count, np.uint32, n),
                    mapq_sumsq=arr(w.mapq_sum_square, np.uint64, n), clean_count=arr(w.clean_count, np.uint32, n),
                    genotype=rec(w.genotype, DIGT_CALL_DTYPE, n) if self.genotype else None,
                    site_summary=rec(w.site_summary, GVCF_SITE_SUMMARY_DTYPE, n) if self.genotype else None,
                    gvcf_runs=rec(w.gvcf_runs, GVCF_RUN_DTYPE, n) if (self.genotype and self.gvcf_block_opt is not None) else None,
                    evs_off=arr(w.evs_off, np.int64, n + 1) if self.evs_words else None,
                    evs_words=(arr(w.evs_words, np.uint64, int(arr(w.evs_off, np.int64, n + 1)[-1]) if n else 0) if self.evs_words else None))


def _window_arrays(w, genotype_dtype=None):
    n = w.end - w.begin

    def arr(ptr, dt, k):
        if k == 0 or not ptr:
            return np.zeros(0, dt)
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(np.ctypeslib.as_ctypes_type(np.dtype(dt)))), shape=(k,)).copy()
    o1 = arr(w.tier1_off, np.int64, n + 1)
    o2 = arr(w.tier2_off, np.int64, n + 1)
    return dict(begin=w.begin, end=w.end, tier1_off=o1, tier1_calls=arr(w.tier1_calls, np.uint16, int(o1[-1]) if n else 0),
                tier2_off=o2, tier2_calls=arr(w.tier2_calls, np.uint16, int(o2[-1]) if n else 0),
                spandel=arr(w.spandel_count, np.uint32, n), submapped=arr(w.submapped_count, np.uint32, n),
                mapq_count=arr(w.mapq_count, np.uint32, n), mapq_zero=arr(w.mapq_zero_count, np.uint32, n),
                mapq_sumsq=arr(w.mapq_sum_square, np.uint64, n), clean_count=arr(w.clean_count, np.uint32, n)), arr


class SomaticPileupStream:
    """sk_somatic_pileup_stream_*: the normal and the tumor sample's pileups over a region, pushed window by window together and
    chained into a12+a13.  `library` as for PileupStream."""

    def __init__(self, opt, somatic_opt=None, with_read_pos=False, library=None):
        self.L = library or lib()
        L = self.L
        L.sk_somatic_pileup_stream_create.restype = c_void_p
        L.sk_somatic_pileup_stream_create.argtypes = [C.POINTER(PileupOptions), c_void_p, C.c_int]
        L.sk_somatic_pileup_stream_destroy.argtypes = [c_void_p]
        L.sk_somatic_pileup_stream_begin_region.argtypes = [c_void_p, C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
        L.sk_somatic_pileup_stream_push.argtypes = [c_void_p, C.POINTER(ReadBatchStruct), C.POINTER(ReadBatchStruct), C.c_int32, C.c_int32,
                                                    C.c_int32, c_void_p, C.c_int32, C.c_int32, C.c_int32, c_void_p, C.c_int,
                                                    C.POINTER(SomaticPileupWindow)]
        L.sk_last_error.restype = C.c_char_p
        self.genotype = somatic_opt is not None
        self.with_read_pos = with_read_pos
        self.h = L.sk_somatic_pileup_stream_create(C.byref(opt), C.byref(somatic_opt) if self.genotype else None, 1 if with_read_pos else 0)
        if not self.h:
            raise RuntimeError(L.sk_last_error().decode())

    def close(self):
        if self.h:
            self.L.sk_somatic_pileup_stream_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise RuntimeError(self.L.sk_last_error().decode())

    def begin_region(self, ref_seq, ref_offset, report_begin, report_end, span=49):
        ref = ref_seq.encode()
        self._check(self.L.sk_somatic_pileup_stream_begin_region(self.h, ref, ref_offset, len(ref), report_begin, report_end, span))

    def push(self, normal_rb, tumor_rb, final_to, mask=None, mask_begin=0, forced=None, forced_begin=0, is_compute_nonsomatic=False,
             span=49):
        """-> dict(normal=..., tumor=... (as PileupStream.push), clean2_count per sample, read_pos, genotype)"""
        st = [ReadBatchStruct(rb.n_reads, _p(rb.read_off), _p(rb.read_code), _p(rb.read_qual), _p(rb.path_off), _p(rb.path),
                              _p(rb.pos), _p(rb.is_fwd), _p(rb.mapq), _p(rb.map_level), None, 0, 0, None) for rb in (normal_rb, tumor_rb)]
        w = SomaticPileupWindow()
        mask = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        forced = None if forced is None else np.ascontiguousarray(forced, np.uint8)
        self._check(self.L.sk_somatic_pileup_stream_push(self.h, C.byref(st[0]), C.byref(st[1]), span, mask_begin,
                                                          0 if mask is None else len(mask), _p(mask), min(final_to, 2**31 - 1), forced_begin,
                                                          0 if forced is None else len(forced), _p(forced), 1 if is_compute_nonsomatic else 0,
                                                          C.byref(w)))
        normal, arr = _window_arrays(w.normal)
        tumor, _ = _window_arrays(w.tumor)
        n = w.normal.end - w.normal.begin
        normal["clean2_count"] = arr(w.normal_clean_tier2_count, np.uint32, n)
        tumor["clean2_count"] = arr(w.tumor_clean_tier2_count, np.uint32, n)
        geno = None
        if self.genotype:
            if n and w.genotype:
                buf = (C.c_char * (SOMATIC_GENOTYPE_DTYPE.itemsize * n)).from_address(w.genotype)
                geno = np.frombuffer(buf, SOMATIC_GENOTYPE_DTYPE, n).copy()
            else:
                geno = np.zeros(0, SOMATIC_GENOTYPE_DTYPE)
        read_pos = arr(w.tumor_tier1_read_pos, np.uint32, len(tumor["tier1_calls"])) if self.with_read_pos else None
        return dict(begin=w.normal.begin, end=w.normal.end, normal=normal, tumor=tumor, read_pos=read_pos, genotype=geno)


# ---------------------------------------------------------------------------------------------------- GlobalAligner

def align_scores(**kw):
    s = AlignScores()
    lib().sk_align_scores_default(C.byref(s))
    for k, v in kw.items():
        if not hasattr(s, k):
            raise AttributeError(k)
        setattr(s, k, v)
    return s


def global_align(pairs, scores=None):
    """pairs: [(query, ref)] strings -> [(score, begin_pos, cigar)]"""
    scores = scores or align_scores()
    n = len(pairs)
    qo = np.zeros(n + 1, np.int64)
    ro = np.zeros(n + 1, np.int64)
    for i, (q, r) in enumerate(pairs):
        qo[i + 1] = qo[i] + len(q)
        ro[i + 1] = ro[i] + len(r)
    qb = np.frombuffer("".join(q for q, _ in pairs).encode(), np.uint8).copy() if n else np.zeros(1, np.uint8)
    rb = np.frombuffer("".join(r for _, r in pairs).encode(), np.uint8).copy() if n else np.zeros(1, np.uint8)
    b = GlobalAlignBatch(n, _p(qo), _p(qb), _p(ro), _p(rb))
    score = np.zeros(max(n, 1), np.int32)
    beg = np.zeros(max(n, 1), np.int32)
    nseg = np.zeros(max(n, 1), np.int32)
    path = np.zeros((int(qo[-1] + ro[-1]) + 4 * n + 1, 2), np.uint32)
    _check(lib().sk_global_align(C.byref(b), C.byref(scores), _p(score), _p(beg), _p(path), _p(nseg)))
    out = []
    for i in range(n):
        po = int(qo[i] + ro[i]) + 4 * i
        out.append((int(score[i]), int(beg[i]), "".join("%d%s" % (path[po + k, 1], CIGAR_CHARS[path[po + k, 0]]) for k in range(nseg[i]))))
    return out


class DiscoveredAllele(C.Structure):
    _fields_ = [("pos", C.c_int32), ("type", C.c_int32), ("del_len", C.c_uint32), ("ins_len", C.c_uint32), ("ins_off", C.c_int32)]


def discover_indels_and_mismatches(ref_seq, ref_offset, ar_begin, ar_end, prev_ar_end, max_indel_size, haplotype, begin_pos,
                                   cigar):
    """-> ([(pos, type, del_len, ins_seq)], n_indels); `cigar` is the '='/'X' CIGAR sk_global_align returned"""
    path = cigar_to_path(cigar)
    segs = (PathSeg * max(len(path), 1))(*[PathSeg(t, l) for t, l in path])
    cap = len(haplotype) + len(path) + 1
    out = (DiscoveredAllele * cap)()
    ins = C.create_string_buffer(2 * len(haplotype) + 16)
    n, ni = C.c_int32(), C.c_int32()
    f = lib().sk_discover_indels_and_mismatches
    f.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.c_char_p, C.c_int32, C.c_int32,
                  C.POINTER(PathSeg), C.c_int32, C.POINTER(DiscoveredAllele), C.c_int32, C.c_char_p, C.c_int32,
                  C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    r, h = ref_seq.encode(), haplotype.encode()
    _check(f(r, ref_offset, len(r), ar_begin, ar_end, prev_ar_end, max_indel_size, h, len(h), begin_pos, segs, len(path), out, cap,
             ins, len(ins), C.byref(n), C.byref(ni)))
    raw = ins.raw
    return [(out[i].pos, out[i].type, out[i].del_len, raw[out[i].ins_off:out[i].ins_off + out[i].ins_len].decode())
            for i in range(n.value)], ni.value


# ---- the feed: BGZF inflation and BAM record decoding ------------------------------------------------------------

BAM_RECORD_DTYPE = np.dtype([("ref_id", "<i4"), ("pos", "<i4"), ("mate_ref_id", "<i4"), ("mate_pos", "<i4"), ("template_size", "<i4"),
                             ("l_seq", "<i4"), ("n_cigar", "<i4"), ("flag", "<u2"), ("mapq", "u1"), ("is_fwd_strand", "u1"), ("pad", "<u4")])
PATH_SEG_DTYPE = np.dtype([("type", "<u4"), ("length", "<u4")])


def bgzf_scan(data):
    """data: uint8 array of whole BGZF blocks -> (block_off[n+1], out_off[n+1])"""
    data = np.ascontiguousarray(data, np.uint8)
    n = lib().sk_bgzf_scan(_p(data), len(data), None, None, 0)
    if n < 0:
        raise StrelkaAmdError("sk_bgzf_scan: malformed BGZF block header")
    block_off, out_off = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    if lib().sk_bgzf_scan(_p(data), len(data), _p(block_off), _p(out_off), n) != n:
        raise StrelkaAmdError("sk_bgzf_scan failed")
    return block_off, out_off


def bgzf_inflate(data):
    """the inflated stream of a BGZF file image (kernel-backed; CRC-32 and ISIZE of every block checked)"""
    data = np.ascontiguousarray(data, np.uint8)
    block_off, out_off = bgzf_scan(data)
    out = np.zeros(int(out_off[-1]), np.uint8)
    _check(lib().sk_bgzf_inflate(_p(data), _p(block_off), _p(out_off), len(block_off) - 1, _p(out)))
    return out


def bgzf_deflate_bound(n, with_eof=True):
    """room bgzf_deflate needs for n input bytes (every block stored, plus the EOF block); host arithmetic, works without a device"""
    return int(lib().sk_bgzf_deflate_bound(int(n), int(bool(with_eof))))


def bgzf_deflate(data, level=2, with_eof=True):
    """bytes -> a BGZF stream (bytes), compressed on the device: level 0 stored, 1 fixed Huffman code, 2 dynamic codes"""
    data = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, np.uint8)
    cap = bgzf_deflate_bound(len(data), with_eof)
    out = np.empty(max(cap, 1), np.uint8)
    n_out = C.c_int64(0)
    _check(lib().sk_bgzf_deflate(_p(data) if len(data) else None, len(data), int(level), int(bool(with_eof)), _p(out), cap, C.byref(n_out)))
    return out[:n_out.value].tobytes()


def bam_scan_records(stream, first=None):
    stream = np.ascontiguousarray(stream, np.uint8)
    if first is None:
        first = lib().sk_bam_header_end(_p(stream), len(stream))
        if first < 0:
            raise StrelkaAmdError("sk_bam_header_end: not a BAM stream")
    n = lib().sk_bam_scan_records(_p(stream), len(stream), first, None, None, None, 0)
    if n < 0:
        raise StrelkaAmdError("sk_bam_scan_records: malformed record")
    rec_off, read_off, path_off = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    if lib().sk_bam_scan_records(_p(stream), len(stream), first, _p(rec_off), _p(read_off), _p(path_off), n) != n:
        raise StrelkaAmdError("sk_bam_scan_records failed")
    return rec_off[:n].copy(), read_off, path_off


def bam_decode(stream, first=None):
    """-> dict(rec[BAM_RECORD_DTYPE], read_off, read_code, read_qual, path_off, path[PATH_SEG_DTYPE]) of every whole record"""
    stream = np.ascontiguousarray(stream, np.uint8)
    rec_off, read_off, path_off = bam_scan_records(stream, first)
    n = len(rec_off)
    rec = np.zeros(n, BAM_RECORD_DTYPE)
    code = np.zeros(max(int(read_off[-1]), 1), np.uint8)
    qual = np.zeros(max(int(read_off[-1]), 1), np.uint8)
    path = np.zeros(max(int(path_off[-1]), 1), PATH_SEG_DTYPE)
    _check(lib().sk_bam_decode(_p(stream), len(stream), _p(rec_off), n, _p(read_off), _p(path_off), _p(rec), _p(code), _p(qual), _p(path)))
    return dict(rec=rec, rec_off=rec_off, read_off=read_off, read_code=code[:int(read_off[-1])], read_qual=qual[:int(read_off[-1])],
                path_off=path_off, path=path[:int(path_off[-1])])


def normalize_alignments(ref_seq, ref_offset, reads, library=None):
    """reads: dicts(code uint8[], pos, path [(type, length)]) -> list of (changed, pos, path) through sk_normalize_alignments
    (`library`: another build of the ABI, e.g. the CPU double, for the no-GPU test tier)"""
    L = library or lib()
    n = len(reads)
    read_off = np.zeros(n + 1, np.int64)
    path_off = np.zeros(n + 1, np.int64)
    for i, r in enumerate(reads):
        read_off[i + 1] = read_off[i] + len(r["code"])
        path_off[i + 1] = path_off[i] + len(r["path"])
    code = np.concatenate([np.asarray(r["code"], np.uint8) for r in reads]) if n else np.zeros(1, np.uint8)
    path = np.zeros(max(int(path_off[-1]), 1), PATH_SEG_DTYPE)
    k = 0
    for r in reads:
        for t, l in r["path"]:
            path[k] = (t, l)
            k += 1
    n_seg = np.array([len(r["path"]) for r in reads], np.int32)
    pos = np.array([r["pos"] for r in reads], np.int32)
    changed = np.zeros(max(n, 1), np.uint8)
    ref_b = ref_seq.encode() if isinstance(ref_seq, str) else bytes(ref_seq)
    rc = L.sk_normalize_alignments(ref_b, int(ref_offset), len(ref_b), n, _p(read_off), _p(code), _p(path_off), _p(n_seg), _p(path), _p(pos), _p(changed))
    if rc != 0:
        raise StrelkaAmdError(L.sk_last_error().decode("utf-8", "replace"))
    out = []
    for i in range(n):
        seg = path[int(path_off[i]):int(path_off[i]) + int(n_seg[i])]
        out.append((int(changed[i]), int(pos[i]), [(int(t), int(l)) for t, l in seg]))
    return out


INTAKE_READ_DTYPE = np.dtype([("valid_begin", "<i4"), ("valid_end", "<i4"), ("total_indel_ref_span", "<u4"), ("n_obs", "<u4")])
INTAKE_OBS_DTYPE = np.dtype([("read", "<i4"), ("pos", "<i4"), ("deletion_length", "<u4"), ("ins_begin", "<u4"), ("ins_len", "<u4"), ("bp_begin", "<u4"),
                             ("bp_len", "<u4"), ("type", "u1"), ("is_noise", "u1"), ("is_low_mapq", "u1"), ("pad", "u1")])
INTAKE_SITE_DTYPE = np.dtype([("variant_count", "<u4"), ("depth", "<u4")])
assert INTAKE_READ_DTYPE.itemsize == 16 and INTAKE_OBS_DTYPE.itemsize == 32 and INTAKE_SITE_DTYPE.itemsize == 8


def intake_options():
    o = IntakeOptions()
    lib().sk_intake_options_default(C.byref(o))
    return o


def read_intake_obs_bound(n_path_segments):
    """room for the observations of paths of n_path_segments segments in all; host arithmetic, works without a device"""
    return int(lib().sk_read_intake_obs_bound(int(n_path_segments)))


def pack_reads(reads):
    """reads: dicts(code uint8[], pos, path [(type, length)]) -> (read_off, code, path_off, n_seg, path, pos): the arrays
    sk_normalize_alignments and sk_read_intake take"""
    n = len(reads)
    read_off = np.zeros(n + 1, np.int64)
    path_off = np.zeros(n + 1, np.int64)
    for i, r in enumerate(reads):
        read_off[i + 1] = read_off[i] + len(r["code"])
        path_off[i + 1] = path_off[i] + len(r["path"])
    code = np.concatenate([np.asarray(r["code"], np.uint8) for r in reads] + [np.zeros(1, np.uint8)])
    path = np.zeros(max(int(path_off[-1]), 1), PATH_SEG_DTYPE)
    k = 0
    for r in reads:
        for t, l in r["path"]:
            path[k] = (t, l)
            k += 1
    n_seg = np.array([len(r["path"]) for r in reads] + [0], np.int32)
    pos = np.array([r["pos"] for r in reads] + [0], np.int32)
    return read_off, code, path_off, n_seg, path, pos


def read_intake(ref_seq, ref_offset, reads, low_mapq, win_begin, n_pos, opt=None):
    """reads: the form normalize_alignments takes; low_mapq: one flag per read -> dict(reads[INTAKE_READ_DTYPE], obs_off,
    obs[INTAKE_OBS_DTYPE], sites[INTAKE_SITE_DTYPE], is_candidate bool[]) through sk_read_intake"""
    L = lib()
    n = len(reads)
    read_off, code, path_off, n_seg, path, pos = pack_reads(reads)
    low = np.zeros(n + 1, np.uint8)
    low[:n] = np.asarray(low_mapq, np.uint8)[:n] != 0
    opt = opt or intake_options()
    cap = read_intake_obs_bound(int(path_off[-1]))
    rec = np.zeros(max(n, 1), INTAKE_READ_DTYPE)
    obs_off = np.zeros(n + 1, np.int64)
    obs = np.zeros(max(cap, 1), INTAKE_OBS_DTYPE)
    sites = np.zeros(max(n_pos, 1), INTAKE_SITE_DTYPE)
    cand = np.zeros(max(n_pos, 1), np.uint8)
    ref_b = ref_seq.encode() if isinstance(ref_seq, str) else bytes(ref_seq)
    _check(L.sk_read_intake(ref_b, int(ref_offset), len(ref_b), n, _p(read_off), _p(code), _p(path_off), _p(n_seg), _p(path), _p(pos), _p(low),
                            C.byref(opt), int(win_begin), int(n_pos), _p(rec), _p(obs_off), _p(obs), cap, _p(sites), _p(cand)))
    return dict(reads=rec[:n], obs_off=obs_off, obs=obs[:int(obs_off[-1])], sites=sites[:n_pos], is_candidate=cand[:n_pos].astype(bool))


REPEAT_MAX_UNIT = 50
AR_STATE_DTYPE = np.dtype([("is_beginning", "<i4"), ("active_region_start_pos", "<i4"), ("anchor_pos_following_prev_variant", "<i4"),
                           ("prev_anchor_pos", "<i4"), ("prev_variant_pos", "<i4"), ("num_variants", "<u4")])
ACTIVE_REGION_DTYPE = np.dtype([("begin", "<i4"), ("end", "<i4"), ("made_at", "<i4")])
assert AR_STATE_DTYPE.itemsize == 24 and ACTIVE_REGION_DTYPE.itemsize == 12


def ar_state_initial():
    """SampleActiveRegionDetector's coordinates as its constructor leaves them -> AR_STATE_DTYPE[1]"""
    s = np.zeros(1, AR_STATE_DTYPE)
    lib().sk_ar_state_initial(_p(s))
    return s


def ar_state(values):
    """dict of the six fields (or an AR_STATE_DTYPE record) -> AR_STATE_DTYPE[1]"""
    s = np.zeros(1, AR_STATE_DTYPE)
    for k in AR_STATE_DTYPE.names:
        s[k][0] = values[k]
    return s


def active_regions_bound(n_pos):
    """room for the regions of a window of n_pos positions; host arithmetic, works without a device"""
    return int(lib().sk_active_regions_bound(int(n_pos)))


def ref_anchors(ref_seq, ref_offset, init_pos, init_span, win_begin, n_pos, span_pos=()):
    """-> (is_anchor uint8[n_pos], span rows uint32[len(span_pos)][50]) through sk_ref_anchors; init_span: 50 values or None (a fresh finder)"""
    ref_b = ref_seq.encode() if isinstance(ref_seq, str) else bytes(ref_seq)
    init = None if init_span is None else np.ascontiguousarray(init_span, np.uint32)
    assert init is None or len(init) == REPEAT_MAX_UNIT
    sp = np.ascontiguousarray(list(span_pos) + [0], np.int32)
    anchor = np.zeros(max(int(n_pos), 1), np.uint8)
    rows = np.zeros((max(len(span_pos), 1), REPEAT_MAX_UNIT), np.uint32)
    _check(lib().sk_ref_anchors(ref_b, int(ref_offset), len(ref_b), int(init_pos), _p(init), int(win_begin), int(n_pos), _p(anchor), len(span_pos), _p(sp), _p(rows)))
    return anchor[:max(int(n_pos), 0)], rows[:len(span_pos)]


def active_regions(win_begin, sites, is_candidate, is_anchor, state=None, region_cap=None):
    """sites: INTAKE_SITE_DTYPE[n_pos]; state: AR_STATE_DTYPE[1] or None (the initial one) -> (regions ACTIVE_REGION_DTYPE[], state_out
    AR_STATE_DTYPE[1]) through sk_active_regions"""
    sites = np.ascontiguousarray(sites, INTAKE_SITE_DTYPE)
    n = len(sites)
    cand = np.ascontiguousarray(np.asarray(is_candidate).astype(np.uint8))
    anchor = np.ascontiguousarray(np.asarray(is_anchor).astype(np.uint8))
    assert len(cand) == n and len(anchor) == n
    state_in = ar_state_initial() if state is None else np.ascontiguousarray(state, AR_STATE_DTYPE)
    state_out = np.zeros(1, AR_STATE_DTYPE)
    cap = active_regions_bound(n) if region_cap is None else int(region_cap)
    regions = np.zeros(max(cap, 1), ACTIVE_REGION_DTYPE)
    n_regions = np.zeros(1, np.int32)
    _check(lib().sk_active_regions(int(win_begin), n, _p(sites) if n else None, _p(cand) if n else None, _p(anchor) if n else None, _p(state_in), _p(state_out),
                                   _p(regions), cap, _p(n_regions)))
    return regions[:int(n_regions[0])], state_out


MAX_SAMPLES = 8
SYNC_CLOSED_AT_CLEAR = -1
PLOIDY_MARK_DTYPE = np.dtype([("pos", "<i4"), ("ploidy", "<i4")])
SYNC_STATE_DTYPE = np.dtype([("sample", AR_STATE_DTYPE, (MAX_SAMPLES,)), ("sync_begin", "<i4"), ("sync_end", "<i4"), ("prev_end", "<i4"), ("sample_mask", "<u4")])
SYNC_REGION_DTYPE = np.dtype([("begin", "<i4"), ("end", "<i4"), ("closed_at", "<i4"), ("prev_end", "<i4"), ("ploidy", "u1", (MAX_SAMPLES,)), ("sample_mask", "<u4"),
                              ("pad", "<u4")])
REGION_PARAMS_DTYPE = np.dtype([("buf_begin", "<i4"), ("buf_end", "<i4"), ("ploidy", "<i4"), ("pad", "<i4")])
assert SYNC_STATE_DTYPE.itemsize == 208 and SYNC_REGION_DTYPE.itemsize == 32 and REGION_PARAMS_DTYPE.itemsize == 16 and PLOIDY_MARK_DTYPE.itemsize == 8


def sync_state_initial():
    """ActiveRegionDetector's coordinates as its constructor leaves them -> SYNC_STATE_DTYPE[1]"""
    s = np.zeros(1, SYNC_STATE_DTYPE)
    lib().sk_sync_state_initial(_p(s))
    return s


def sync_state(values):
    """dict(samples [dict of the six fields], sync_begin, sync_end, prev_end, sample_mask) -> SYNC_STATE_DTYPE[1]; samples beyond the
    list are initial"""
    s = sync_state_initial()
    for k, d in enumerate(values["samples"]):
        for f in AR_STATE_DTYPE.names:
            s["sample"][0][k][f] = d[f]
    for f in ("sync_begin", "sync_end", "prev_end", "sample_mask"):
        s[f][0] = values[f]
    return s


def sync_state_dict(s, n_samples=MAX_SAMPLES):
    """SYNC_STATE_DTYPE[1] -> the dict sync_state takes, of the first n_samples samples"""
    return dict(samples=[{f: int(s["sample"][0][k][f]) for f in AR_STATE_DTYPE.names} for k in range(n_samples)], sync_begin=int(s["sync_begin"][0]),
                sync_end=int(s["sync_end"][0]), prev_end=int(s["prev_end"][0]), sample_mask=int(s["sample_mask"][0]))


def sync_regions_bound(n_pos):
    """room for the regions a window of n_pos positions can close; host arithmetic, works without a device"""
    return int(lib().sk_sync_regions_bound(int(n_pos)))


def pack_ploidy_marks(marks, n_samples):
    """[S][(pos, ploidy)] or None -> (mark_off int32[S + 1], PLOIDY_MARK_DTYPE[])"""
    marks = marks if marks is not None else [[] for _ in range(n_samples)]
    off = np.zeros(n_samples + 1, np.int32)
    flat = []
    for s in range(n_samples):
        flat += [(int(p), int(v)) for p, v in marks[s]]
        off[s + 1] = len(flat)
    arr = np.zeros(len(flat) + 1, PLOIDY_MARK_DTYPE)
    for k, m in enumerate(flat):
        arr[k] = m
    return off, arr


def sync_active_regions(win_begin, sites, is_candidate, is_anchor, marks=None, default_ploidy=2, state=None, do_clear=False, buf_begin=None, buf_end=None,
                        region_cap=None, want_region_id=True):
    """sites: INTAKE_SITE_DTYPE[S][n_pos]; is_candidate [S][n_pos]; is_anchor [n_pos]; marks [S][(pos, ploidy)]; state: SYNC_STATE_DTYPE[1] or
    None (the initial one) -> (regions SYNC_REGION_DTYPE[], state_out SYNC_STATE_DTYPE[1], region_id int32[n_pos] or None) through
    sk_sync_active_regions"""
    sites = np.ascontiguousarray(sites, INTAKE_SITE_DTYPE)
    n_samples = len(sites)
    n = len(np.asarray(is_anchor))
    sites = sites.reshape(n_samples, n)
    cand = np.ascontiguousarray(np.asarray(is_candidate).astype(np.uint8).reshape(n_samples, n))
    anchor = np.ascontiguousarray(np.asarray(is_anchor).astype(np.uint8))
    mark_off, mark_arr = pack_ploidy_marks(marks, n_samples)
    state_in = sync_state_initial() if state is None else np.ascontiguousarray(state, SYNC_STATE_DTYPE)
    state_out = np.zeros(1, SYNC_STATE_DTYPE)
    cap = sync_regions_bound(n) if region_cap is None else int(region_cap)
    regions = np.zeros(max(cap, 1), SYNC_REGION_DTYPE)
    n_regions = np.zeros(1, np.int32)
    region_id = np.full(max(n, 1), -2, np.int32) if want_region_id else None
    bb = None if buf_begin is None else np.ascontiguousarray(buf_begin, np.int32)
    be = None if buf_end is None else np.ascontiguousarray(buf_end, np.int32)
    _check(lib().sk_sync_active_regions(n_samples, int(win_begin), n, _p(sites) if n else None, _p(cand) if n else None, _p(anchor) if n else None, _p(mark_off),
                                        _p(mark_arr), int(default_ploidy), _p(state_in), _p(state_out), 1 if do_clear else 0, _p(bb), _p(be), _p(regions), cap,
                                        _p(n_regions), _p(region_id)))
    return regions[:int(n_regions[0])], state_out, None if region_id is None else region_id[:n]


def sync_region_params(sync_regions, sample, buf_begin, buf_end_at_clear=0):
    """SYNC_REGION_DTYPE[] -> (ACTIVE_REGION_DTYPE[], REGION_PARAMS_DTYPE[]) of one sample through sk_sync_region_params"""
    sync = np.ascontiguousarray(sync_regions, SYNC_REGION_DTYPE)
    m = len(sync)
    regions = np.zeros(max(m, 1), ACTIVE_REGION_DTYPE)
    params = np.zeros(max(m, 1), REGION_PARAMS_DTYPE)
    _check(lib().sk_sync_region_params(_p(sync) if m else None, m, int(sample), int(buf_begin), int(buf_end_at_clear), _p(regions), _p(params)))
    return regions[:m], params[:m]


HAP_COUNTED, HAP_BYPASSED, HAP_NO_READS, HAP_TOO_FEW_COVERING, HAP_DECLINED = range(5)
HAP_DECLINE_NONE, HAP_DECLINE_GROUPS, HAP_DECLINE_READ_INDEX_SPREAD, HAP_DECLINE_READ_SPAN = range(4)
HAP_MAX_SELECTED = 3
SELECTED_HAPLOTYPE_DTYPE = np.dtype([("seq_off", "<i8"), ("support_off", "<i8"), ("seq_len", "<u4"), ("count", "<u4"), ("is_reference", "<u4"), ("pad", "<u4")])
REGION_HAPLOTYPES_DTYPE = np.dtype([("status", "<i4"), ("reason", "<i4"), ("n_reads_aligned", "<u4"), ("n_reads_covering", "<u4"), ("n_selected", "<u4"), ("pad", "<u4"),
                                    ("hap", SELECTED_HAPLOTYPE_DTYPE, (HAP_MAX_SELECTED,))])
assert SELECTED_HAPLOTYPE_DTYPE.itemsize == 32 and REGION_HAPLOTYPES_DTYPE.itemsize == 120


def region_haplotypes_bounds(n_reads, n_regions):
    """room for the selected haplotypes' bytes and supporting reads of n_regions regions; host arithmetic, works without a device"""
    L = lib()
    return int(L.sk_region_haplotypes_seq_bound(int(n_regions))), int(L.sk_region_haplotypes_support_bound(int(n_reads), int(n_regions)))


def region_haplotype_records(recs, seq_pool, support_pool):
    """REGION_HAPLOTYPES_DTYPE[] and the two pools -> [dict(status, reason, n_reads_aligned, n_reads_covering, haps [dict(seq, count,
    is_reference, support)])]: the records with the haplotype strings and support lists looked up"""
    out = []
    for r in recs:
        haps = []
        for k in range(int(r["n_selected"])):
            h = r["hap"][k]
            so, sl, po, pc = int(h["seq_off"]), int(h["seq_len"]), int(h["support_off"]), int(h["count"])
            haps.append(dict(seq=bytes(seq_pool[so:so + sl]).decode("latin-1"), count=pc, is_reference=int(h["is_reference"]),
                             support=[int(x) for x in support_pool[po:po + pc]]))
        out.append(dict(status=int(r["status"]), reason=int(r["reason"]), n_reads_aligned=int(r["n_reads_aligned"]),
                        n_reads_covering=int(r["n_reads_covering"]), haps=haps))
    return out


def region_haplotypes(ref_seq, ref_offset, reads, low_mapq, is_fwd_strand, regions, buf_begin, buf_end, ploidy=2, intake=None, opt=None, raw=False, params=None):
    """reads: the form read_intake takes; regions: ACTIVE_REGION_DTYPE[] or [(begin, end)]; intake: read_intake's result for these reads
    (computed here when None) -> per-region records with haplotype strings and support lists (region_haplotype_records) through
    sk_region_haplotypes; raw=True: dict(recs, seq_pool, support_pool, query_off, totals) as the entry point leaves them.
    params: REGION_PARAMS_DTYPE[] or [(buf_begin, buf_end, ploidy)] per region -- then through sk_region_haplotypes_params, and buf_begin,
    buf_end and ploidy are not read"""
    L = lib()
    n = len(reads)
    opt = opt or intake_options()
    if intake is None:
        intake = read_intake(ref_seq, ref_offset, reads, low_mapq, 0, 0, opt)
    read_off, code, path_off, n_seg, path, pos = pack_reads(reads)
    low = np.zeros(n + 1, np.uint8)
    low[:n] = np.asarray(low_mapq, np.uint8)[:n] != 0
    fwd = np.zeros(n + 1, np.uint8)
    fwd[:n] = np.asarray(is_fwd_strand, np.uint8)[:n] != 0
    obs_off = np.ascontiguousarray(intake["obs_off"], np.int64)
    obs = np.ascontiguousarray(intake["obs"], INTAKE_OBS_DTYPE)
    if isinstance(regions, np.ndarray) and regions.dtype == ACTIVE_REGION_DTYPE:
        reg = np.ascontiguousarray(regions)
    else:
        reg = np.zeros(len(regions), ACTIVE_REGION_DTYPE)
        for i, r in enumerate(regions):
            reg[i] = (int(r[0]), int(r[1]), 0)
    m = len(reg)
    seq_cap, support_cap = region_haplotypes_bounds(n, m)
    recs = np.zeros(max(m, 1), REGION_HAPLOTYPES_DTYPE)
    seq_pool = np.zeros(max(seq_cap, 1), np.uint8)
    support_pool = np.zeros(max(support_cap, 1), np.int32)
    query_off = np.zeros(HAP_MAX_SELECTED * m + 1, np.int64)
    totals = np.zeros(3, np.int64)
    ref_b = ref_seq.encode() if isinstance(ref_seq, str) else bytes(ref_seq)
    if params is not None:
        if isinstance(params, np.ndarray) and params.dtype == REGION_PARAMS_DTYPE:
            par = np.ascontiguousarray(params)
        else:
            par = np.zeros(len(params), REGION_PARAMS_DTYPE)
            for i, q in enumerate(params):
                par[i] = (int(q[0]), int(q[1]), int(q[2]), 0)
        assert len(par) == m
        par = np.concatenate([par, np.zeros(1, REGION_PARAMS_DTYPE)])
        _check(L.sk_region_haplotypes_params(ref_b, int(ref_offset), len(ref_b), n, _p(read_off), _p(code), _p(path_off), _p(n_seg), _p(path), _p(pos), _p(low), _p(fwd),
                                             _p(obs_off), _p(obs) if len(obs) else None, int(opt.max_indel_size), _p(par), _p(reg) if m else None, m, _p(recs),
                                             _p(seq_pool), seq_cap, _p(support_pool), support_cap, _p(query_off), _p(totals)))
    else:
        _check(L.sk_region_haplotypes(ref_b, int(ref_offset), len(ref_b), n, _p(read_off), _p(code), _p(path_off), _p(n_seg), _p(path), _p(pos), _p(low), _p(fwd),
                                      _p(obs_off), _p(obs) if len(obs) else None, int(opt.max_indel_size), int(buf_begin), int(buf_end), int(ploidy),
                                      _p(reg) if m else None, m, _p(recs), _p(seq_pool), seq_cap, _p(support_pool), support_cap, _p(query_off), _p(totals)))
    res = dict(recs=recs[:m], seq_pool=seq_pool[:int(totals[1])], support_pool=support_pool[:int(totals[2])], query_off=query_off[:int(totals[0]) + 1], totals=totals)
    return res if raw else region_haplotype_records(res["recs"], res["seq_pool"], res["support_pool"])


ALLELE_DECLINE_BEGIN_POS, ALLELE_DECLINE_LEFT_SHIFT, ALLELE_DECLINE_ID_SUM, ALLELE_DECLINE_HAP_LEN = range(4, 8)
ALLELE_MAX_ALT = 2
REGION_ALLELE_DTYPE = np.dtype([("pos", "<i4"), ("type", "<i4"), ("del_len", "<u4"), ("ins_len", "<u4"), ("ins_off", "<i8"), ("hap_slot", "<i4"), ("haplotype_id", "<i4"),
                                ("ratio", "<f4"), ("to_indel_buffer", "<i4"), ("same_as", "<i4"), ("id_sum", "<i4"), ("ratio_sum", "<f4"), ("pad", "<i4")])
REGION_ALLELES_DTYPE = np.dtype([("status", "<i4"), ("reason", "<i4"), ("prev_end", "<i4"), ("n_alt", "<u4"), ("n_alleles", "<u4"), ("n_indels", "<u4"),
                                 ("n_distinct_mismatches", "<u4"), ("do_not_add_mismatches", "<u4"), ("allele_off", "<i8"), ("insert_off", "<i8"),
                                 ("n_insert_bytes", "<u4"), ("pad", "<u4"), ("score", "<i4", (ALLELE_MAX_ALT,)), ("hap_slot", "<i4", (ALLELE_MAX_ALT,))])
assert REGION_ALLELE_DTYPE.itemsize == 56 and REGION_ALLELES_DTYPE.itemsize == 72


class RegionAllele(C.Structure):  # sk_region_allele
    _fields_ = [("pos", C.c_int32), ("type", C.c_int32), ("del_len", C.c_uint32), ("ins_len", C.c_uint32), ("ins_off", C.c_int64), ("hap_slot", C.c_int32),
                ("haplotype_id", C.c_int32), ("ratio", C.c_float), ("to_indel_buffer", C.c_int32), ("same_as", C.c_int32), ("id_sum", C.c_int32),
                ("ratio_sum", C.c_float), ("pad", C.c_int32)]


class RegionAllelesRec(C.Structure):  # sk_region_alleles_rec
    _fields_ = [("status", C.c_int32), ("reason", C.c_int32), ("prev_end", C.c_int32), ("n_alt", C.c_uint32), ("n_alleles", C.c_uint32), ("n_indels", C.c_uint32),
                ("n_distinct_mismatches", C.c_uint32), ("do_not_add_mismatches", C.c_uint32), ("allele_off", C.c_int64), ("insert_off", C.c_int64),
                ("n_insert_bytes", C.c_uint32), ("pad", C.c_uint32), ("score", C.c_int32 * ALLELE_MAX_ALT), ("hap_slot", C.c_int32 * ALLELE_MAX_ALT)]


def region_alleles_bounds(n_regions, max_hap_len):
    """room for the allele records and insert bytes of n_regions regions; host arithmetic, works without a device"""
    L = lib()
    return int(L.sk_region_alleles_allele_bound(int(n_regions), int(max_hap_len))), int(L.sk_region_alleles_insert_bound(int(n_regions), int(max_hap_len)))


def float_bits(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


def region_allele_records(recs, alleles, insert_pool):
    """REGION_ALLELES_DTYPE[], REGION_ALLELE_DTYPE[] and the insert bytes -> [dict(status, reason, prev_end, n_alt, n_indels,
    n_distinct_mismatches, do_not_add_mismatches, score, hap_slot, alleles [dict(pos, type, del_len, ins, hap_slot, haplotype_id, ratio,
    to_indel_buffer, same_as, id_sum, ratio_sum)])]: the records with the insert sequences looked up; floats as their bits"""
    out = []
    for r in recs:
        keys = []
        for a in alleles[int(r["allele_off"]):int(r["allele_off"]) + int(r["n_alleles"])]:
            io, il = int(a["ins_off"]), int(a["ins_len"])
            keys.append(dict(pos=int(a["pos"]), type=int(a["type"]), del_len=int(a["del_len"]), ins=bytes(insert_pool[io:io + il]).decode("latin-1"),
                             hap_slot=int(a["hap_slot"]), haplotype_id=int(a["haplotype_id"]), ratio=float_bits(a["ratio"]), to_indel_buffer=int(a["to_indel_buffer"]),
                             same_as=int(a["same_as"]), id_sum=int(a["id_sum"]), ratio_sum=float_bits(a["ratio_sum"])))
        n_alt = int(r["n_alt"])
        out.append(dict(status=int(r["status"]), reason=int(r["reason"]), prev_end=int(r["prev_end"]), n_alt=n_alt, n_indels=int(r["n_indels"]),
                        n_distinct_mismatches=int(r["n_distinct_mismatches"]), do_not_add_mismatches=int(r["do_not_add_mismatches"]),
                        score=[int(x) for x in r["score"][:n_alt]], hap_slot=[int(x) for x in r["hap_slot"][:n_alt]], alleles=keys))
    return out


def region_alleles(ref_seq, ref_offset, regions, haplotypes, max_indel_size=49, max_hap_len=1024, prev_end_in=-1, raw=False):
    """regions: ACTIVE_REGION_DTYPE[] or [(begin, end)]; haplotypes: what region_haplotypes(..., raw=True) returned for them -> (per-region
    records (region_allele_records), prev_end_out) through sk_region_alleles; raw=True: dict(recs, alleles, insert_pool, totals,
    prev_end_out) as the entry point leaves them"""
    L = lib()
    if isinstance(regions, np.ndarray) and regions.dtype == ACTIVE_REGION_DTYPE:
        reg = np.ascontiguousarray(regions)
    else:
        reg = np.zeros(len(regions), ACTIVE_REGION_DTYPE)
        for i, r in enumerate(regions):
            reg[i] = (int(r[0]), int(r[1]), 0)
    m = len(reg)
    hap = np.ascontiguousarray(haplotypes["recs"], REGION_HAPLOTYPES_DTYPE)
    seq = np.ascontiguousarray(haplotypes["seq_pool"], np.uint8)
    allele_cap, insert_cap = region_alleles_bounds(m, max_hap_len)
    recs = np.zeros(max(m, 1), REGION_ALLELES_DTYPE)
    alleles = np.zeros(max(allele_cap, 1), REGION_ALLELE_DTYPE)
    insert_pool = np.zeros(max(insert_cap, 1), np.uint8)
    totals = np.zeros(2, np.int64)
    prev_end_out = np.zeros(1, np.int32)
    ref_b = ref_seq.encode() if isinstance(ref_seq, str) else bytes(ref_seq)
    _check(L.sk_region_alleles(ref_b, int(ref_offset), len(ref_b), _p(reg) if m else None, m, _p(hap) if m else None, _p(seq) if len(seq) else None, len(seq),
                               int(max_indel_size), int(max_hap_len), int(prev_end_in), _p(recs), _p(alleles), allele_cap, _p(insert_pool), insert_cap,
                               _p(totals), _p(prev_end_out)))
    res = dict(recs=recs[:m], alleles=alleles[:int(totals[0])], insert_pool=insert_pool[:int(totals[1])], totals=totals, prev_end_out=int(prev_end_out[0]))
    return res if raw else (region_allele_records(res["recs"], res["alleles"], res["insert_pool"]), res["prev_end_out"])


IAT_TIER1, IAT_TIER2, IAT_SUBMAP = range(3)
ITAB_TIER1, ITAB_TIER2, ITAB_SUBMAP, ITAB_NOISE, ITAB_N_SETS = range(5)
ITAB_DO_NOT_GENOTYPE, ITAB_AR_PENDING = 1, 2
INDEL_TABLE_KEY_DTYPE = np.dtype([("pos", "<i4"), ("type", "<i4"), ("del_len", "<u4"), ("ins_len", "<u4"), ("ins_off", "<i8"), ("active_region_id", "<i4"), ("flags", "<u4"),
                                  ("n_bp_obs", "<u4"), ("it", "<i4"), ("repeat_unit_len", "<u4"), ("ref_repeat_count", "<u4"), ("indel_repeat_count", "<u4"),
                                  ("interrupted_hpol_len", "<u4")])
INDEL_TABLE_SAMPLE_DATA_DTYPE = np.dtype([("off", "<i8", (ITAB_N_SETS,)), ("count", "<u4", (ITAB_N_SETS,)), ("haplotype_id", "<i4"), ("is_haplotyping_bypassed", "<u4"),
                                          ("ratio", "<f4"), ("pad", "<u4")])
assert INDEL_TABLE_KEY_DTYPE.itemsize == 56 and INDEL_TABLE_SAMPLE_DATA_DTYPE.itemsize == 64


class IndelTableSample(C.Structure):  # sk_indel_table_sample
    _fields_ = [("n_reads", C.c_int32), ("pad", C.c_int32), ("read_off", c_void_p), ("read_code", c_void_p), ("obs_off", c_void_p), ("obs", c_void_p), ("obs_cap", C.c_int64),
                ("align_id", c_void_p), ("iat", c_void_p), ("hap_recs", c_void_p), ("support_pool", c_void_p), ("support_cap", C.c_int64), ("recs", c_void_p),
                ("alleles", c_void_p), ("allele_cap", C.c_int64), ("insert_pool", c_void_p), ("insert_cap", C.c_int64)]


def indel_table_bounds(n_obs_total, n_allele_records_total, n_expanded_support_total, n_read_bases_total, n_allele_insert_bytes_total):
    """room for the keys, the ids and the insert bytes; host arithmetic, works without a device"""
    L = lib()
    return (int(L.sk_indel_table_key_bound(int(n_obs_total), int(n_allele_records_total))), int(L.sk_indel_table_id_bound(int(n_obs_total), int(n_expanded_support_total))),
            int(L.sk_indel_table_insert_bound(int(n_read_bases_total), int(n_allele_insert_bytes_total))))


def indel_table_records(keys, data, id_pool, insert_pool, n_samples):
    """INDEL_TABLE_KEY_DTYPE[], INDEL_TABLE_SAMPLE_DATA_DTYPE[n_keys * n_samples] and the two pools -> [dict(pos, type, del_len, ins, active_region_id,
    flags, n_bp_obs, it, repeat_unit_len, ref_repeat_count, indel_repeat_count, interrupted_hpol_len, samples [dict(ids [[tier1], [tier2],
    [submap], [noise]], haplotype_id, is_haplotyping_bypassed, ratio)])]: the table as plain records; floats as their bits"""
    out = []
    for k, key in enumerate(keys):
        io, il = int(key["ins_off"]), int(key["ins_len"])
        rec = dict(pos=int(key["pos"]), type=int(key["type"]), del_len=int(key["del_len"]), ins=bytes(insert_pool[io:io + il]).decode("latin-1"))
        for f in ("active_region_id", "flags", "n_bp_obs", "it", "repeat_unit_len", "ref_repeat_count", "indel_repeat_count", "interrupted_hpol_len"):
            rec[f] = int(key[f])
        rec["samples"] = []
        for d in data[k * n_samples:(k + 1) * n_samples]:
            ids = [[int(x) for x in id_pool[int(d["off"][c]):int(d["off"][c]) + int(d["count"][c])]] for c in range(ITAB_N_SETS)]
            rec["samples"].append(dict(ids=ids, haplotype_id=int(d["haplotype_id"]), is_haplotyping_bypassed=int(d["is_haplotyping_bypassed"]), ratio=float_bits(d["ratio"])))
        out.append(rec)
    return out


def pack_indel_table_sample(sample, n_regions):
    """dict(reads, intake (read_intake's result), align_id (or None), iat, haplotypes (region_haplotypes(..., raw=True)), alleles
    (region_alleles(..., raw=True))) -> (IndelTableSample, the arrays it points into, dict of the sizes the bounds take)"""
    n = len(sample["reads"])
    read_off, code, _, _, _, _ = pack_reads(sample["reads"])
    keep = dict(read_off=read_off, code=code, obs_off=np.ascontiguousarray(sample["intake"]["obs_off"], np.int64),
                obs=np.ascontiguousarray(sample["intake"]["obs"], INTAKE_OBS_DTYPE),
                align_id=None if sample.get("align_id") is None else np.ascontiguousarray(list(sample["align_id"]) + [0], np.uint32),
                iat=np.ascontiguousarray(list(sample["iat"]) + [0], np.uint8), hap=np.ascontiguousarray(sample["haplotypes"]["recs"], REGION_HAPLOTYPES_DTYPE),
                support=np.ascontiguousarray(sample["haplotypes"]["support_pool"], np.int32), recs=np.ascontiguousarray(sample["alleles"]["recs"], REGION_ALLELES_DTYPE),
                alleles=np.ascontiguousarray(sample["alleles"]["alleles"], REGION_ALLELE_DTYPE), ins=np.ascontiguousarray(sample["alleles"]["insert_pool"], np.uint8))
    assert len(keep["hap"]) == n_regions and len(keep["recs"]) == n_regions
    ptr = lambda x: None if x is None or len(x) == 0 else x.ctypes.data
    st = IndelTableSample(n, 0, ptr(read_off), ptr(code), ptr(keep["obs_off"]), ptr(keep["obs"]), len(keep["obs"]), ptr(keep["align_id"]), ptr(keep["iat"]), ptr(keep["hap"]),
                          ptr(keep["support"]), len(keep["support"]), ptr(keep["recs"]), ptr(keep["alleles"]), len(keep["alleles"]), ptr(keep["ins"]), len(keep["ins"]))
    n_support = 0
    for i in range(n_regions):
        h, r = keep["hap"][i], keep["recs"][i]
        for a in keep["alleles"][int(r["allele_off"]):int(r["allele_off"]) + int(r["n_alleles"])]:
            if int(a["to_indel_buffer"]) and 0 <= int(a["hap_slot"]) < HAP_MAX_SELECTED:
                n_support += int(h["hap"][int(a["hap_slot"])]["count"])
    sizes = dict(n_obs=len(keep["obs"]), n_alleles=len(keep["alleles"]), n_support=n_support, n_bases=int(read_off[-1]), n_ins=len(keep["ins"]))
    return st, keep, sizes


def indel_table(ref_seq, ref_offset, samples, regions, prev_end_in=-1, raw=False, caps=None):
    """samples: [the dicts pack_indel_table_sample takes], at most MAX_SAMPLES; regions: the shared list, ACTIVE_REGION_DTYPE[] or [(begin, end)]
    -> (the table as plain records (indel_table_records), totals [keys, ids, insert bytes, pending pairs]) through sk_indel_table;
    raw=True: dict(keys, data, id_pool, insert_pool, totals) as the entry point leaves them.  caps: (key_cap, id_cap, insert_cap) instead of
    the bounds"""
    L = lib()
    if isinstance(regions, np.ndarray) and regions.dtype == ACTIVE_REGION_DTYPE:
        reg = np.ascontiguousarray(regions)
    else:
        reg = np.zeros(len(regions), ACTIVE_REGION_DTYPE)
        for i, r in enumerate(regions):
            reg[i] = (int(r[0]), int(r[1]), 0)
    m = len(reg)
    packed = [pack_indel_table_sample(s, m) for s in samples]
    arr = (IndelTableSample * max(len(packed), 1))(*[p[0] for p in packed])
    tot = {k: sum(p[2][k] for p in packed) for k in ("n_obs", "n_alleles", "n_support", "n_bases", "n_ins")}
    key_cap, id_cap, insert_cap = caps or indel_table_bounds(tot["n_obs"], tot["n_alleles"], tot["n_support"], tot["n_bases"], tot["n_ins"])
    n_samples = len(packed)
    keys = np.zeros(max(key_cap, 1), INDEL_TABLE_KEY_DTYPE)
    data = np.zeros(max(key_cap, 1) * max(n_samples, 1), INDEL_TABLE_SAMPLE_DATA_DTYPE)
    id_pool = np.zeros(max(id_cap, 1), np.uint32)
    insert_pool = np.zeros(max(insert_cap, 1), np.uint8)
    totals = np.zeros(4, np.int64)
    ref_b = ref_seq.encode() if isinstance(ref_seq, str) else bytes(ref_seq)
    _check(L.sk_indel_table(n_samples, C.addressof(arr), ref_b, int(ref_offset), len(ref_b), _p(reg) if m else None, m, int(prev_end_in), _p(keys), key_cap, _p(data),
                            _p(id_pool), id_cap, _p(insert_pool), insert_cap, _p(totals)))
    nk = int(totals[0])
    res = dict(keys=keys[:nk], data=data[:nk * n_samples], id_pool=id_pool[:int(totals[1])], insert_pool=insert_pool[:int(totals[2])], totals=totals)
    return res if raw else (indel_table_records(res["keys"], res["data"], res["id_pool"], res["insert_pool"], n_samples), [int(x) for x in totals])


RATE_MAX_SIZES, RATE_MAX_COUNTS, ICAND_PAPPROX, ICAND_MAX_BP_OBS = 4, 40, 18, 257
ICAND_DECIDED, ICAND_AR_PENDING, ICAND_EXACT_BINOMIAL, ICAND_BP_OBS_ORDER = range(4)
INDEL_RATE_SET_DTYPE = np.dtype([("n_sizes", "<u4"), ("n_counts", "<u4", (RATE_MAX_SIZES,)), ("pad", "<u4", (3,)), ("insertion", "<f8", (RATE_MAX_SIZES, RATE_MAX_COUNTS)),
                                 ("deletion", "<f8", (RATE_MAX_SIZES, RATE_MAX_COUNTS))])
INDEL_CANDIDATE_DTYPE = np.dtype([("is_candidate", "u1"), ("undecided", "u1"), ("pad", "<u2"), ("bp_insert_size", "<u4")])
INDEL_ERROR_RATES_DTYPE = np.dtype([("ref_to_indel", "<f8"), ("indel_to_ref", "<f8"), ("candidate_ref_to_indel", "<f8"), ("candidate_indel_to_ref", "<f8")])
assert INDEL_RATE_SET_DTYPE.itemsize == 2592 and INDEL_CANDIDATE_DTYPE.itemsize == 8 and INDEL_ERROR_RATES_DTYPE.itemsize == 32


class IndelCandidateOptions(C.Structure):  # sk_indel_candidate_options
    _fields_ = [("papprox", C.c_double * ICAND_PAPPROX), ("log_indel_ref_error_factor", C.c_double), ("max_candidate_depth", C.c_double),
                ("min_candidate_indel_open_length", C.c_uint32), ("is_indel_ref_error_factor", C.c_uint8), ("is_haplotyping_enabled", C.c_uint8),
                ("is_candidate_indel_signal_test", C.c_uint8), ("is_sample_specific_rates", C.c_uint8), ("is_count_towards_depth_filter", C.c_uint8 * MAX_SAMPLES)]


class IndelCandidateSample(C.Structure):  # sk_indel_candidate_sample
    _fields_ = [("n_reads", C.c_int32), ("pad", C.c_int32), ("obs_off", c_void_p), ("obs", c_void_p), ("obs_cap", C.c_int64), ("depth1", c_void_p), ("depth2", c_void_p)]


assert C.sizeof(IndelCandidateOptions) == 176 and C.sizeof(IndelCandidateSample) == 48


def indel_candidate_options(**fields):
    """the reference's defaults (sk_indel_candidate_options_default: papprox is left zero, caller data) with `fields` set; a list for papprox and
    is_count_towards_depth_filter"""
    o = IndelCandidateOptions()
    lib().sk_indel_candidate_options_default(C.addressof(o))
    for k, v in fields.items():
        if k in ("papprox", "is_count_towards_depth_filter"):
            for i, x in enumerate(v):
                getattr(o, k)[i] = x
        else:
            setattr(o, k, v)
    return o


def pack_rate_set(sizes):
    """[[(insertion rate, deletion rate) per repeat count] per pattern size] -> one INDEL_RATE_SET_DTYPE record; sizes past what the record
    holds are cut (the count stays, for the refusal)"""
    rs = np.zeros((), INDEL_RATE_SET_DTYPE)
    rs["n_sizes"] = len(sizes)
    for i, counts in enumerate(sizes[:RATE_MAX_SIZES]):
        rs["n_counts"][i] = len(counts)
        for j, (ins, dele) in enumerate(counts[:RATE_MAX_COUNTS]):
            rs["insertion"][i][j], rs["deletion"][i][j] = ins, dele
    return rs


def pack_paths(reads):
    """[dict(pos, path [(type, length)])] -> (path_off, n_seg, PATH_SEG_DTYPE-like uint32 pairs, pos) as sk_read_depth takes them"""
    n = len(reads)
    path_off = np.zeros(n + 1, np.int64)
    n_seg = np.zeros(n + 1, np.int32)
    pos = np.zeros(n + 1, np.int32)
    segs = []
    for r, rd in enumerate(reads):
        path_off[r], n_seg[r], pos[r] = len(segs), len(rd["path"]), rd["pos"]
        segs += [(int(t), int(l)) for t, l in rd["path"]]
    path_off[n] = len(segs)
    return path_off, n_seg, np.array(segs + [(0, 0)], np.uint32).reshape(-1, 2), pos


def read_depth(reads, iat, win_begin, n_pos, packed=None):
    """one sample's reads [dict(pos, path)] and iat -> (depth1, depth2) over [win_begin, win_begin + n_pos) through sk_read_depth; packed:
    (path_off, n_seg, path, pos, path_cap) instead of the reads"""
    L = lib()
    n = len(iat)
    path_off, n_seg, path, pos, path_cap = packed or (pack_paths(reads) + (None,))
    path_cap = len(path) - 1 if path_cap is None else path_cap
    iat_a = np.ascontiguousarray(list(iat) + [0], np.uint8)
    d1, d2 = np.zeros(max(n_pos, 1), np.uint32), np.zeros(max(n_pos, 1), np.uint32)
    _check(L.sk_read_depth(n, _p(path_off), _p(n_seg), _p(path), path_cap, _p(pos), _p(iat_a), int(win_begin), int(n_pos), _p(d1), _p(d2)))
    return d1[:max(n_pos, 0)], d2[:max(n_pos, 0)]


def indel_candidates(samples, win_begin, n_pos, keys, data, rate_sets, opt, n_samples=None, n_keys=None):
    """samples: [dict(n_reads, obs_off, obs (INTAKE_OBS_DTYPE), depth1, depth2)]; keys / data as sk_indel_table leaves them; rate_sets:
    INDEL_RATE_SET_DTYPE[], the candidate set first -> dict(out INDEL_CANDIDATE_DTYPE[n_keys], rates INDEL_ERROR_RATES_DTYPE[n_keys * n_samples], totals)
    through sk_indel_candidates"""
    L = lib()
    keep = []
    for s in samples:
        obs_off = np.ascontiguousarray(s["obs_off"], np.int64)
        obs = np.ascontiguousarray(s["obs"], INTAKE_OBS_DTYPE)
        d1, d2 = np.ascontiguousarray(s["depth1"], np.uint32), np.ascontiguousarray(s["depth2"], np.uint32)
        keep.append((obs_off, obs, d1, d2))
    ptr = lambda x: None if len(x) == 0 else x.ctypes.data
    arr = (IndelCandidateSample * max(len(samples), 1))(*[IndelCandidateSample(int(s["n_reads"]), 0, ptr(k[0]), ptr(k[1]), s.get("obs_cap", len(k[1])), ptr(k[2]), ptr(k[3]))
                                                          for s, k in zip(samples, keep)])
    n_samples = len(samples) if n_samples is None else n_samples
    keys = np.ascontiguousarray(keys, INDEL_TABLE_KEY_DTYPE)
    data = np.ascontiguousarray(data, INDEL_TABLE_SAMPLE_DATA_DTYPE)
    nk = len(keys) if n_keys is None else n_keys
    sets = np.ascontiguousarray(rate_sets, INDEL_RATE_SET_DTYPE)
    out = np.zeros(max(nk, 1), INDEL_CANDIDATE_DTYPE)
    rates = np.zeros(max(nk, 1) * max(n_samples, 1), INDEL_ERROR_RATES_DTYPE)
    totals = np.zeros(2, np.int64)
    _check(L.sk_indel_candidates(n_samples, C.addressof(arr), int(win_begin), int(n_pos), _p(keys) if len(keys) else None, _p(data) if len(data) else None, nk, _p(sets),
                                 C.addressof(opt), _p(out), _p(rates), _p(totals)))
    return dict(out=out[:max(nk, 0)], rates=rates[:max(nk, 0) * n_samples], totals=[int(x) for x in totals])


RGATE_NONE, RGATE_PASS, RGATE_OVERMAX, RGATE_OUTSIDE_RANGE, RGATE_NO_CANDIDATE, RGATE_UNDECIDED, RGATE_SPLICED = range(7)
RGATE_SORT_CAP = 64
REALIGN_GATE_KEY_DTYPE = np.dtype([("pos", "<i4"), ("type", "<i4"), ("del_len", "<u4"), ("ins_len", "<u4"), ("ins_off", "<i8"), ("active_region_id", "<i4"), ("is_candidate", "u1"),
                                   ("undecided", "u1"), ("gate_consulted", "u1"), ("pad", "u1"), ("haplotype_id", "i1", (MAX_SAMPLES,)),
                                   ("is_haplotyping_bypassed", "u1", (MAX_SAMPLES,))])
REALIGN_GATE_LOG_RATES_DTYPE = np.dtype([("ref_to_indel_log_prob", "<f8"), ("indel_to_ref_log_prob", "<f8")])
REALIGN_GATE_READ_DTYPE = np.dtype([("zone_begin", "<i4"), ("zone_end", "<i4"), ("status", "u1"), ("asked_undecided", "u1"), ("pad", "<u2")])
assert REALIGN_GATE_KEY_DTYPE.itemsize == 48 and REALIGN_GATE_LOG_RATES_DTYPE.itemsize == 16 and REALIGN_GATE_READ_DTYPE.itemsize == 12


class RealignGateSample(C.Structure):  # sk_realign_gate_sample
    _fields_ = [("n_reads", C.c_int32), ("pad", C.c_int32), ("pos", c_void_p), ("path_off", c_void_p), ("n_seg", c_void_p), ("path", c_void_p), ("path_cap", C.c_int64),
                ("read_len", c_void_p), ("align_id", c_void_p), ("realign_begin", c_void_p), ("realign_end", c_void_p)]


class RealignGateSampleOut(C.Structure):  # sk_realign_gate_sample_out
    _fields_ = [("reads", c_void_p), ("observed_off", c_void_p), ("observed", c_void_p), ("observed_cap", C.c_int64)]


assert C.sizeof(RealignGateSample) == 80 and C.sizeof(RealignGateSampleOut) == 32


def realign_gate_observed_bound(n_ids):
    """room for one sample's observed entries; host arithmetic, works without a device"""
    return int(lib().sk_realign_gate_observed_bound(int(n_ids)))


def pack_gate_sample(reads, align_id=None):
    """[dict(pos, path [(type, length)], read_len, realign (begin, end))] and the reads' align ids (None: their indices) -> the arrays of one
    sk_realign_gate_sample, each with one element of slack: dict(n_reads, pos, path_off, n_seg, path, path_cap, read_len, align_id,
    realign_begin, realign_end)"""
    path_off, n_seg, path, pos = pack_paths(reads)
    n = len(reads)
    return dict(n_reads=n, pos=pos, path_off=path_off, n_seg=n_seg, path=path, path_cap=len(path) - 1,
                read_len=np.array([int(r["read_len"]) for r in reads] + [0], np.int32),
                align_id=None if align_id is None else np.array(list(align_id) + [0], np.uint32),
                realign_begin=np.array([int(r["realign"][0]) for r in reads] + [0], np.int32), realign_end=np.array([int(r["realign"][1]) for r in reads] + [0], np.int32))


def realign_gate_sample_struct(p, ptr=None):
    """pack_gate_sample's dict -> RealignGateSample over its arrays (ptr: array -> address; the default takes host arrays)"""
    ptr = ptr or (lambda x: x.ctypes.data)
    return RealignGateSample(int(p["n_reads"]), 0, ptr(p["pos"]), ptr(p["path_off"]), ptr(p["n_seg"]), ptr(p["path"]), int(p["path_cap"]), ptr(p["read_len"]),
                             None if p["align_id"] is None else ptr(p["align_id"]), ptr(p["realign_begin"]), ptr(p["realign_end"]))


def realign_gate(samples, keys, data, id_pool, cand, rates, max_indel_size, n_samples=None, n_keys=None, n_ids=None, observed_cap=None, slack=0):
    """samples: [pack_gate_sample's dicts]; keys / data / id_pool as sk_indel_table leaves them, cand / rates as sk_indel_candidates leaves them ->
    dict(keys REALIGN_GATE_KEY_DTYPE[n_keys], logs REALIGN_GATE_LOG_RATES_DTYPE[n_keys * n_samples], samples [dict(reads REALIGN_GATE_READ_DTYPE[],
    observed_off, observed)], totals [reads that pass, reads undecided, observed entries per sample]) through sk_realign_gate.  slack: so
    many extra elements of 0x5a bytes behind every output array, returned with it (the tests' canaries)"""
    L = lib()
    n_samples = len(samples) if n_samples is None else n_samples
    keys = np.ascontiguousarray(keys, INDEL_TABLE_KEY_DTYPE)
    data = np.ascontiguousarray(data, INDEL_TABLE_SAMPLE_DATA_DTYPE)
    id_pool = np.ascontiguousarray(id_pool, np.uint32)
    cand = np.ascontiguousarray(cand, INDEL_CANDIDATE_DTYPE)
    rates = np.ascontiguousarray(rates, INDEL_ERROR_RATES_DTYPE)
    nk = len(keys) if n_keys is None else n_keys
    ni = len(id_pool) if n_ids is None else n_ids
    ns = max(n_samples, 1)

    def room(n, dtype):
        a = np.zeros(max(n, 0) + max(slack, 1), dtype)
        a.view(np.uint8)[max(n, 0) * a.dtype.itemsize:] = 0x5a
        return a
    keys_out, logs = room(nk, REALIGN_GATE_KEY_DTYPE), room(nk * ns, REALIGN_GATE_LOG_RATES_DTYPE)
    totals = np.zeros(2 + MAX_SAMPLES, np.int64)
    cap = max(ni, 0) if observed_cap is None else observed_cap
    outs = [dict(reads=room(int(p["n_reads"]), REALIGN_GATE_READ_DTYPE), observed_off=room(int(p["n_reads"]) + 1, np.int64), observed=room(cap, np.int32)) for p in samples]
    arr_in = (RealignGateSample * max(len(samples), 1))(*[realign_gate_sample_struct(p) for p in samples])
    arr_out = (RealignGateSampleOut * max(len(samples), 1))(*[RealignGateSampleOut(o["reads"].ctypes.data, o["observed_off"].ctypes.data, o["observed"].ctypes.data, cap) for o in outs])
    ptr = lambda x: _p(x) if len(x) else None
    _check(L.sk_realign_gate(n_samples, C.addressof(arr_in), ptr(keys), ptr(data), ptr(id_pool), nk, ni, ptr(cand), ptr(rates), int(max_indel_size), _p(keys_out), _p(logs),
                             C.addressof(arr_out), _p(totals)))
    cut = (lambda a, n: a[:max(n, 0) + slack])
    res = dict(keys=cut(keys_out, nk), logs=cut(logs, nk * ns), totals=[int(x) for x in totals], samples=[])
    for s, (p, o) in enumerate(zip(samples, outs)):
        n = int(p["n_reads"])
        res["samples"].append(dict(reads=cut(o["reads"], n), observed_off=cut(o["observed_off"], n + 1), observed=cut(o["observed"], cap), n_observed=int(totals[2 + s])))
    return res


def realign_job_inputs(gate, sample, reads, insert_pool):
    """what a realignment job of one sample is made of, from sk_realign_gate's outputs: gate: realign_gate's result (or the same arrays read back from
    the device); reads: the sample's [dict(code, qual, pos, path, fwd, map_level, realign)] -> (indels as RealignJob.set_indels takes them, reads as
    RealignJob.add_reads takes them).  Every read is handed on, whatever its status: the job runs its own gate."""
    n_samples = len(gate["logs"]) // max(len(gate["keys"]), 1) if len(gate["keys"]) else 1
    indels = []
    for k, key in enumerate(gate["keys"]):
        io, il = int(key["ins_off"]), int(key["ins_len"])
        lg = gate["logs"][k * n_samples + sample]
        indels.append(dict(pos=int(key["pos"]), type=int(key["type"]), del_len=int(key["del_len"]), ins_seq=bytes(insert_pool[io:io + il]).decode("latin-1"),
                           is_candidate=int(key["is_candidate"]), r2i=float(lg["ref_to_indel_log_prob"]), i2r=float(lg["indel_to_ref_log_prob"]),
                           arid=int(key["active_region_id"]), hap=[int(x) for x in key["haplotype_id"]], bypass=[int(x) for x in key["is_haplotyping_bypassed"]]))
    so = gate["samples"][sample]
    out = []
    for r, rd in enumerate(reads):
        b, e = int(so["observed_off"][r]), int(so["observed_off"][r + 1])
        out.append((rd["code"], rd["qual"], rd["pos"], rd["path"], rd.get("fwd", True), rd.get("map_level", MAPLEVEL["TIER1"]), sample, tuple(rd["realign"]),
                    [int(x) for x in so["observed"][b:e]]))
    return indels, out


(RPRE_NONE, RPRE_OK, RPRE_NOT_PASSED, RPRE_NEGATIVE_POS, RPRE_EDGE_KEY_MISSING, RPRE_EXEMPLAR_KEY_MISSING, RPRE_CAP_K, RPRE_CAP_OBS, RPRE_CAP_P,
 RPRE_N_STATUS) = range(10)  # SK_RPRE_*
RPRE_NAMES = ("NONE", "OK", "NOT_PASSED", "NEGATIVE_POS", "EDGE_KEY_MISSING", "EXEMPLAR_KEY_MISSING", "CAP_K", "CAP_OBS", "CAP_P")
RPRE_K, RPRE_P, RPRE_OBS, RPRE_N_TOTALS = 40, 48, 64, 1 + RPRE_N_STATUS
REALIGN_PREPARED_RANGE_DTYPE = np.dtype([("b", "<i4"), ("e", "<i4"), ("has_b", "u1"), ("has_e", "u1"), ("pad", "u1", (2,))])
REALIGN_PREPARED_ALIGNMENT_DTYPE = np.dtype([("pos", "<i4"), ("lead", "<i2"), ("trail", "<i2"), ("is_fwd_strand", "u1"), ("n_seg", "u1"), ("n_indels", "u1"), ("pad", "u1"),
                                             ("path", [("type", "<u2"), ("length", "<u2")], (RPRE_P,)), ("indels", "<i2", (RPRE_K + 2,))])
REALIGN_PREPARED_STATUS_DTYPE = np.dtype([("idx", "<i2"), ("is_present", "u1"), ("is_remove_only", "u1"), ("in_original", "u1"), ("pad", "u1")])
REALIGN_PREPARED_READ_DTYPE = np.dtype([("realign_begin", "<i4"), ("realign_end", "<i4"), ("read_length", "<i4"), ("sample", "<i4"), ("exemplar_range", REALIGN_PREPARED_RANGE_DTYPE),
                                        ("alignment", REALIGN_PREPARED_ALIGNMENT_DTYPE), ("status_map", REALIGN_PREPARED_STATUS_DTYPE, (RPRE_K,)), ("order", "<i2", (RPRE_K,)),
                                        ("observed", "<i2", (RPRE_OBS,)), ("n_status", "u1"), ("n_order", "u1"), ("n_observed", "u1"), ("clipped", "u1"), ("hc_lead", "<u4"),
                                        ("hc_trail", "<u4"), ("sc_lead", "<u4"), ("sc_trail", "<u4")])
REALIGN_PREPARED_SOURCE_DTYPE = np.dtype([("sample", "<i4"), ("read", "<i4")])
assert REALIGN_PREPARED_READ_DTYPE.itemsize == 784 and REALIGN_PREPARED_ALIGNMENT_DTYPE.itemsize == 288 and REALIGN_PREPARED_SOURCE_DTYPE.itemsize == 8


class RealignPreambleSample(C.Structure):  # sk_realign_preamble_sample
    _fields_ = [("read_code", c_void_p), ("read_off", c_void_p), ("code_cap", C.c_int64), ("is_fwd_strand", c_void_p), ("status", c_void_p)]


assert C.sizeof(RealignPreambleSample) == 40


def pack_preamble_sample(codes, is_fwd=None):
    """the reads' BAM codes (one array per read) and strands (None: all forward) -> the input arrays of one sk_realign_preamble_sample, each with one
    element of slack: dict(read_code, read_off, code_cap, is_fwd_strand)"""
    off = np.zeros(len(codes) + 1, np.int64)
    for i, c in enumerate(codes):
        off[i + 1] = off[i] + len(c)
    flat = np.concatenate([np.asarray(c, np.uint8) for c in codes] + [np.zeros(1, np.uint8)]) if len(codes) else np.zeros(1, np.uint8)
    return dict(read_code=flat, read_off=off, code_cap=int(off[-1]), is_fwd_strand=None if is_fwd is None else np.array([int(bool(f)) for f in is_fwd] + [0], np.uint8))


def realign_preamble(samples, gate, pre, insert_pool, ref, ref_offset, max_indel_size, record_cap=None, n_keys=None, slack=0, host=False):
    """samples: [pack_gate_sample's dicts]; gate: realign_gate's result (keys, and per sample reads, observed_off, observed); pre: [pack_preamble_sample's
    dicts]; insert_pool: the table's; ref: the job's reference segment -> dict(records REALIGN_PREPARED_READ_DTYPE[record_cap], source
    REALIGN_PREPARED_SOURCE_DTYPE[record_cap], status [uint8 per read, per sample], consulted uint8[n_keys], totals [the record count, then the reads per
    SK_RPRE_* status]) through sk_realign_preamble, or with host=True through sk_debug_realign_preamble_host (the same rules on the host; needs no device).
    record_cap: None = the reads that passed the gate.  slack: so many extra elements of 0x5a bytes behind every output array, returned with it"""
    L = lib()
    n_samples = len(samples)
    keys = np.ascontiguousarray(gate["keys"], REALIGN_GATE_KEY_DTYPE)
    nk = len(keys) if n_keys is None else n_keys
    insert_pool = np.ascontiguousarray(insert_pool, np.uint8)
    refb = np.frombuffer(ref.encode("latin-1") if isinstance(ref, str) else bytes(ref), np.uint8)
    if record_cap is None:
        record_cap = sum(int((np.asarray(g["reads"]["status"][:p["n_reads"]]) == RGATE_PASS).sum()) for g, p in zip(gate["samples"], samples))

    def room(n, dtype):
        a = np.zeros(max(n, 0) + max(slack, 1), dtype)
        a.view(np.uint8)[max(n, 0) * a.dtype.itemsize:] = 0x5a
        return a
    records, source, consulted = room(record_cap, REALIGN_PREPARED_READ_DTYPE), room(record_cap, REALIGN_PREPARED_SOURCE_DTYPE), room(nk, np.uint8)
    status = [room(int(p["n_reads"]), np.uint8) for p in samples]
    totals = np.zeros(RPRE_N_TOTALS, np.int64)
    keep = []

    def arr(a, dtype):
        a = np.ascontiguousarray(a, dtype)
        keep.append(a)
        return a.ctypes.data
    arr_in = (RealignGateSample * max(n_samples, 1))(*[realign_gate_sample_struct(dict(p, align_id=None)) for p in samples])
    arr_gate = (RealignGateSampleOut * max(n_samples, 1))(*[RealignGateSampleOut(arr(g["reads"], REALIGN_GATE_READ_DTYPE), arr(g["observed_off"], np.int64),
                                                                                 arr(g["observed"], np.int32), int(g.get("observed_cap", len(g["observed"]))))
                                                             for g in gate["samples"]])
    arr_pre = (RealignPreambleSample * max(n_samples, 1))(*[RealignPreambleSample(arr(q["read_code"], np.uint8), arr(q["read_off"], np.int64), int(q["code_cap"]),
                                                                                  None if q["is_fwd_strand"] is None else arr(q["is_fwd_strand"], np.uint8), st.ctypes.data)
                                                            for q, st in zip(pre, status)])
    ptr = lambda x: _p(x) if len(x) else None
    f = L.sk_debug_realign_preamble_host if host else L.sk_realign_preamble
    _check(f(n_samples, C.addressof(arr_in), C.addressof(arr_gate), C.addressof(arr_pre), ptr(keys), nk, ptr(insert_pool), len(insert_pool), ptr(refb), int(ref_offset), len(refb),
             int(max_indel_size), _p(records), _p(source), record_cap, _p(consulted), _p(totals)))
    cut = (lambda a, n: a[:max(n, 0) + slack])
    return dict(records=cut(records, record_cap), source=cut(source, record_cap), consulted=cut(consulted, nk), totals=[int(x) for x in totals],
                status=[cut(st, int(p["n_reads"])) for st, p in zip(status, samples)])


def realign_preamble_dev(n_samples, samples_addr, gate_addr, pre_addr, dev_keys, dev_table_totals, key_cap, dev_insert_pool, insert_cap, dev_ref, ref_offset, ref_len,
                         max_indel_size, dev_records, dev_source, record_cap, dev_consulted, dev_totals, dev_scratch, scratch_bytes, stream):
    """sk_realign_preamble_dev: the three sample arrays are the addresses of host arrays of RealignGateSample / RealignGateSampleOut / RealignPreambleSample whose
    pointers are device memory, every dev_* an address in device memory; only enqueues on `stream`"""
    _check(lib().sk_realign_preamble_dev(int(n_samples), samples_addr, gate_addr, pre_addr, dev_keys, dev_table_totals, int(key_cap), dev_insert_pool, int(insert_cap), dev_ref,
                                         int(ref_offset), int(ref_len), int(max_indel_size), dev_records, dev_source, int(record_cap), dev_consulted, dev_totals, dev_scratch,
                                         int(scratch_bytes), stream))


def realign_preamble_scratch_bytes(n_samples, key_cap, record_cap):
    """bytes of device scratch sk_realign_preamble_dev needs; host arithmetic, works without a device"""
    return int(lib().sk_realign_preamble_scratch_bytes(int(n_samples), int(key_cap), int(record_cap)))


BAI_CHUNK_DTYPE = np.dtype([("begin", "<u8"), ("end", "<u8")])


def bai_query(bai, ref_id, begin, end):
    """hts_itr_query over a .bai image -> the chunks (BGZF virtual offsets) that can hold records overlapping [begin, end)"""
    bai = np.ascontiguousarray(bai, np.uint8)
    L = lib()
    L.sk_bai_query.restype = C.c_int32
    L.sk_bai_query.argtypes = [c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, c_void_p, C.c_int32]
    n = L.sk_bai_query(_p(bai), len(bai), ref_id, begin, end, None, 0)
    if n < 0:
        raise StrelkaAmdError("sk_bai_query: %s" % ("malformed index" if n == -1 else "reference not in the index"))
    out = np.zeros(max(n, 1), BAI_CHUNK_DTYPE)
    if n:
        assert L.sk_bai_query(_p(bai), len(bai), ref_id, begin, end, _p(out), n) == n
    return out[:n]


def bam_region_filter(rec, path_off, path, ref_id, begin, end):
    """hts_itr_next's record test -> (keep[n] bool, how many records the iterator reads before it finishes)"""
    rec = np.ascontiguousarray(rec, BAM_RECORD_DTYPE)
    path_off = np.ascontiguousarray(path_off, np.int64)
    path = np.ascontiguousarray(path, PATH_SEG_DTYPE)
    keep = np.zeros(max(len(rec), 1), np.uint8)
    L = lib()
    L.sk_bam_region_filter.restype = C.c_int32
    L.sk_bam_region_filter.argtypes = [c_void_p, c_void_p, c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, c_void_p]
    n = L.sk_bam_region_filter(_p(rec), _p(path_off), _p(path), len(rec), ref_id, begin, end, _p(keep))
    if n < 0:
        raise StrelkaAmdError("sk_bam_region_filter: bad argument")
    return keep[:len(rec)].astype(bool), n


def _inflate_blocks(data, block_off, out_off):
    out = np.zeros(max(int(out_off[-1]), 1), np.uint8)
    _check(lib().sk_bgzf_inflate(_p(np.ascontiguousarray(data, np.uint8)), _p(np.ascontiguousarray(block_off, np.int64)),
                                 _p(np.ascontiguousarray(out_off, np.int64)), len(block_off) - 1, _p(out)))
    return out[:int(out_off[-1])]


def bam_fetch_region(bam, bai, ref_id, begin, end, inflate=None, decode=None, blocks=None):
    """What sam_itr_queryi + sam_itr_next hand the reference's bam_streamer for a region, from file images: the index gives the
    chunks (sk_bai_query), their BGZF blocks are inflated and their records decoded (the kernels behind sk_bgzf_inflate /
    sk_bam_decode, unless `inflate(data, block_off, out_off) -> bytes` / `decode(stream, first) -> dict` are given), the iterator's
    record test picks the result (sk_bam_region_filter).
    -> dict(rec, stream_offset (of each record in the inflated file), read_code, read_qual, path: one entry per record)."""
    bam = np.ascontiguousarray(bam, np.uint8)
    block_off, out_off = blocks if blocks is not None else bgzf_scan(bam)
    n_blocks = len(block_off) - 1
    starts = {int(o): i for i, o in enumerate(block_off[:-1])}
    inflate = inflate or _inflate_blocks
    decode = decode or bam_decode
    parts, offsets = [], []
    for ch in bai_query(bai, ref_id, begin, end):
        cb, ub, ce, ue = int(ch["begin"]) >> 16, int(ch["begin"]) & 0xffff, int(ch["end"]) >> 16, int(ch["end"]) & 0xffff
        i0 = starts[cb]
        i1 = starts.get(ce, n_blocks)  # (a chunk may end where the file ends)
        limit = int(out_off[i1] - out_off[i0]) + ue  # the chunk's records start before this offset of its inflated bytes
        last = min(i1, n_blocks - 1)
        while True:  # a record that starts inside the chunk may end in a later block
            stream = inflate(bam[int(block_off[i0]):int(block_off[last + 1])], block_off[i0:last + 2] - block_off[i0],
                             out_off[i0:last + 2] - out_off[i0])
            d = decode(stream, ub)
            if len(d["rec_off"]):
                at = int(d["rec_off"][-1])
                nxt = at + 4 + int(np.frombuffer(np.asarray(stream[at:at + 4], np.uint8).tobytes(), "<i4")[0])
            else:
                nxt = ub
            if nxt >= limit or last == n_blocks - 1:
                break
            last += 1
        n_in = int(np.searchsorted(d["rec_off"], limit))
        keep, n_read = bam_region_filter(d["rec"][:n_in], d["path_off"][:n_in + 1], d["path"], ref_id, begin, end)
        for i in np.nonzero(keep)[0]:
            parts.append((d, int(i)))
            offsets.append(int(out_off[i0]) + int(d["rec_off"][i]))
        if n_read < n_in:
            break  # the iterator has seen a record past the region: finished
    rec = np.array([d["rec"][i] for d, i in parts], BAM_RECORD_DTYPE) if parts else np.zeros(0, BAM_RECORD_DTYPE)
    return dict(rec=rec, stream_offset=np.array(offsets, np.int64),
                read_code=[d["read_code"][int(d["read_off"][i]):int(d["read_off"][i + 1])] for d, i in parts],
                read_qual=[d["read_qual"][int(d["read_off"][i]):int(d["read_off"][i + 1])] for d, i in parts],
                path=[d["path"][int(d["path_off"][i]):int(d["path_off"][i + 1])] for d, i in parts])


GVCF_SITE_DTYPE = np.dtype([("pos", "<i4"), ("is_compressible", "u1"), ("is_gqx", "u1"), ("ploidy", "u1"), ("flush_before", "u1"), ("gt", "<u4"),
                            ("locus_filters", "<u4"), ("sample_filters", "<u4"), ("gqx", "<i4"), ("used_basecalls", "<u4"), ("unused_basecalls", "<u4")])
GVCF_BLOCK_DTYPE = np.dtype([("pos", "<i4"), ("count", "<i4"), ("is_gqx_defined", "<i4"), ("gqx_min", "<i4"), ("dpu_min", "<i4"), ("pad", "<i4"),
                             ("dpu_mean", "<f8"), ("dpf_mean", "<f8")])


def gvcf_block_sites(sites, block_percent_tol=30, block_abs_tol=3, library=None):
    """the gVCF writer's non-variant block logic for one sample's run of sites -> (kind[n], blocks[n]: valid where kind == 1)"""
    sites = np.ascontiguousarray(sites, GVCF_SITE_DTYPE)
    kind = np.zeros(max(len(sites), 1), np.uint8)
    blocks = np.zeros(max(len(sites), 1), GVCF_BLOCK_DTYPE)
    L = library or lib()
    L.sk_gvcf_block_sites.argtypes = [c_void_p, C.c_int32, C.c_uint32, C.c_uint32, c_void_p, c_void_p]
    if L.sk_gvcf_block_sites(_p(sites), len(sites), block_percent_tol, block_abs_tol, _p(kind), _p(blocks)):
        raise StrelkaAmdError(L.sk_last_error().decode() if library else last_error())
    return kind[:len(sites)], blocks[:len(sites)]
