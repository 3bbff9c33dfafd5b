"""Which compiled kernel the bf16 span entries launch, the condition their launcher uses, the tile edges of each and the
tests that reach it: the table of tests/kernel_variants.py, in the same format, for
temporal-span-proposal-network-vidvrd_amd/csrc/spanbf16/*.hip.

tests/test_span_bf16_host.py keeps this table equal to the sources and its node ids pointing at tests that exist;
tools/check_kernel_variants.py checks a `rocprofv3 --kernel-trace --stats` run against this table too."""

SP = "tests/test_gpu_span_predicate_bf16.py::"
SR = "tests/test_gpu_span_relations_bf16.py::"
SM = "tests/test_gpu_model_span_bf16.py::"


def _row(kernel, inst, entry, when, tests, align="no alignment requirement"):
    return {"kernel": kernel, "inst": inst, "entry": entry, "when": when, "tests": list(tests), "align": align}


ALIGN = "feats and cls_packed 16-byte aligned, workspace 256-byte aligned, D % 16 == 0"
BOTH = "tspn_span_predicate_bf16, tspn_decode_span_relations_bf16"

VARIANTS = [
    # ------------------------------------------------------------------------------ spanbf16/tspn_span_bf16.hip
    _row("pack_span_cls_bf16_kernel", None, "tspn_pack_span_cls_bf16", "always (one thread per packed element; K padded to 16)",
         [SP + "test_gemm_against_float64", SM + "test_pool_top_span_forward_on_bf16_segments"],
         align="packed 16-byte aligned, D % 16 == 0"),
    _row("span_prefix_bf16_kernel", None, BOTH, "rows > 0 && NT > 0 (one thread per (tracklet, channel), 256 per workgroup)",
         [SP + "test_pooling_pinned_through_an_identity_classifier", SP + "test_cfg3_shape_sampled_pairs",
          SP + "test_nonfinite_stays_in_the_spans_that_hold_it"], align=ALIGN),
    _row("span_pool_bf16_kernel", None, BOTH, "rows > 0 && NT > 0 (one thread per (row, half, 8 channels), 256 per workgroup)",
         [SP + "test_pooling_pinned_through_an_identity_classifier", SP + "test_nonfinite_stays_in_the_spans_that_hold_it",
          SR + "test_fused_equals_the_composition"], align=ALIGN),
    _row("span_gemm_bf16_kernel", None, BOTH,
         "rows > 0 && NT > 0; tile edges: 16 rows per wave, 64 rows per workgroup, 16 columns per MFMA tile, 64 columns "
         "(1 to 4 tiles, one code path each) per workgroup, 32 channels of 2D per k-step, groups of 4 k-steps whose "
         "fragments are loaded together (2D/32 = 3, 4, 5 and 8, 9: one below, at and above one and two groups; the last "
         "group's missing steps load the last step again and are not used)",
         [SP + "test_gemm_against_float64", SP + "test_four_videos_global_ids_shuffled_table",
          SP + "test_cfg3_shape_sampled_pairs", SP + "test_whole_segment_rows_against_the_fused_pass"], align=ALIGN),
    _row("span_row_topk_q_kernel", None, "tspn_decode_span_relations_bf16", "S > 0 && P > 0 (one wave per (pair, span) row)",
         [SR + "test_fused_equals_the_composition", SR + "test_ragged_counts_and_fewer_candidates_than_topk",
          SM + "test_decode_span_relations_on_bf16_segments"], align=ALIGN),
]
