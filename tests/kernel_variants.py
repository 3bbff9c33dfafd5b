"""Which compiled kernel variant each C-ABI entry point can launch, the condition its launcher uses to pick it,
and the tests that reach it.

One row per `__global__` kernel in temporal-span-proposal-network-vidvrd_amd/csrc/*.hip; for a template, one row
per instantiation a launcher uses.  Fields:
  kernel  the `__global__` name
  inst    template arguments as the demangled kernel name spells them ("8", "0, true"), or None (not a template;
          for a template family listed in one row: any instantiation); for a name that is defined more than once,
          the overload's parameter types in parentheses, again as the demangled name spells them
          ("(float const*, long, long, long, short*)")
  entry   the C-ABI entry point(s) that launch it
  when    the launcher's condition, copied from the source
  tests   pytest node ids ("tests/<file>.py::<function>") whose runs launch it
  align   for operands that must be aligned: refused (with which TSPN_E* code) or served by a fallback

tests/test_kernel_variant_table.py keeps this table equal to the sources and its node ids pointing at tests that
exist; tools/check_kernel_variants.py checks a `rocprofv3 --kernel-trace --stats` run against it."""

KV = "tests/test_gpu_kernel_variants.py::"
OPS = "tests/test_gpu_ops.py::"
BF16 = "tests/test_gpu_bf16.py::"
HH = "tests/test_gpu_bf16_heads_h.py::"
BND = "tests/test_gpu_bf16_bound.py::"
ROI = "tests/test_gpu_roi_head.py::"
FE = "tests/test_gpu_frontend_edges.py::"
CE = "tests/test_gpu_conv2d_edges.py::"
F16N = "tests/test_gpu_nonfinite_f16x3.py::"
F16R = "tests/test_gpu_wino63_f16x3_range.py::"
SPAN = "tests/test_gpu_span_predicate.py::"
TRAIN = "tests/test_gpu_training_shapes.py::"


# tests/test_gpu_conv2d_edges.py: which of its tests reach a conv2d row (its docstring has the table of cases per row)
CE_PACK = [CE + "test_exact_operands_give_the_float64_reference_bit_for_bit", CE + "test_real_operands_within_the_suites_bounds"]
CE_RNG = CE_PACK + [CE + "test_each_epilogue_term_on_its_own", CE + "test_every_output_written_and_nothing_else",
                    CE + "test_an_infinity_reaches_exactly_the_windows_that_hold_it"]
CE_ALL = CE_RNG + [CE + "test_a_kernel_larger_than_the_padded_map_is_refused"]


def _row(kernel, inst, entry, when, tests, align="no alignment requirement"):
    return {"kernel": kernel, "inst": inst, "entry": entry, "when": when, "tests": list(tests), "align": align}


VARIANTS = [
    # ------------------------------------------------------------------------------ tspn_conv3.hip
    _row("pack_conv3_kernel", None, "tspn_pack_conv3_f32", "always", [OPS + "test_conv3_vs_fp64"]),
    _row("conv3_mfma_kernel", "false", "tspn_conv3_f32",
         "!(M % 4 == 0 && (packed & 15) == 0)",
         [OPS + "test_conv3_vs_fp64", KV + "test_conv3_every_variant_at_tile_edges", KV + "test_conv3_tile_map_with_a_short_last_group"],
         "packed not 16-byte aligned: this scalar-weight fallback; x read 4 bytes at a time"),
    _row("conv3_mfma_kernel", "true", "tspn_conv3_f32",
         "vec = (M % 4 == 0) && (packed & 15) == 0; vec && Cin % 8 != 0",
         [KV + "test_conv3_every_variant_at_tile_edges", KV + "test_forward_fused_conv_and_pair_paths", KV + "test_conv3_tile_map_with_a_short_last_group"],
         "packed 16-byte aligned by the condition; x read 4 bytes at a time"),
    _row("conv3_mfma_dma_kernel", "16", "tspn_conv3_f32",
         "vec && Cin % 8 == 0 && Cin % 16 == 0",
         [OPS + "test_conv3_vs_fp64", KV + "test_conv3_every_variant_at_tile_edges",
          KV + "test_forward_fused_conv_and_pair_paths"],
         "packed 16-byte LDS-DMA pieces: aligned by the condition; x 4-byte LDS-DMA pieces (any float view)"),
    _row("conv3_mfma_dma_kernel", "8", "tspn_conv3_f32; tspn_forward_fused_f32 (D % 16 == 8); dense training backward",
         "vec && Cin % 8 == 0 && Cin % 16 != 0",
         [KV + "test_conv3_every_variant_at_tile_edges", KV + "test_conv3_mfma_dma_kernel_8_bias_and_tail",
          KV + "test_forward_fused_conv_and_pair_paths", "tests/test_gpu_model.py::test_dense_temporal_heads_input_gradient",
          TRAIN + "test_dense_training_function_every_conv_variant", TRAIN + "test_tracklet_training_step_shapes"],
         "as conv3_mfma_dma_kernel<16>"),
    _row("conv3_mfma_cl_kernel", None, "tspn_conv3_tc_f32; tspn_forward_fused_f32",
         "conv3_tc: Cin % 16 == 0 && M % 4 == 0 (else TSPN_EUNSUPPORTED); fused: tc = D % 16 == 0 && (feats & 15) == 0 "
         "&& (conv_packed & 15) == 0",
         [OPS + "test_conv3_channels_last_vs_fp64", KV + "test_conv3_channels_last_refuses_unaligned",
          KV + "test_forward_fused_conv_and_pair_paths"],
         "x, packed: refused with TSPN_EUNSUPPORTED (conv3_tc); the fused pass falls back to transpose + direct"),
    # ------------------------------------------------------------------------------ tspn_heads.hip
    _row("heads_kernel", "0, true", "tspn_heads_f32 (mode 0); tspn_temporal_encoder_heads_f32",
         "vec2 = T % 2 == 0 && T >= 2 && (a & 7) == 0 && (mode == 0 || (b & 7) == 0) && (out & 7) == 0",
         [OPS + "test_heads_dense_and_factorised", KV + "test_heads_kernel_both_modes_vec2_and_scalar"],
         "a, out: 8-byte accesses only under vec2; otherwise the scalar form"),
    _row("heads_kernel", "0, false", "tspn_heads_f32 (mode 0)", "!vec2",
         [KV + "test_heads_kernel_both_modes_vec2_and_scalar"], "fallback for unaligned a / out"),
    _row("heads_kernel", "1, true", "tspn_heads_f32 (mode 1); tspn_forward_fused_f32 (indexed pairs)", "vec2",
         [KV + "test_heads_kernel_both_modes_vec2_and_scalar", KV + "test_forward_fused_conv_and_pair_paths"],
         "a, b, out: 8-byte accesses only under vec2"),
    _row("heads_kernel", "1, false", "tspn_heads_f32 (mode 1); tspn_forward_fused_f32 (indexed pairs, odd T)", "!vec2",
         [KV + "test_heads_kernel_both_modes_vec2_and_scalar", KV + "test_forward_fused_conv_and_pair_paths"],
         "fallback for unaligned a / b / out"),
    _row("heads_pairgrid_kernel", "true", "tspn_heads_pairgrid_f32; tspn_forward_fused_f32 (canonical pairs)",
         "!v3 && vec2 = T % 2 == 0 && ldt % 2 == 0 && (y & 7) == 0 && (out & 7) == 0",
         [OPS + "test_heads_pairgrid_matches_generic", KV + "test_heads_pairgrid_every_variant",
          KV + "test_forward_fused_conv_and_pair_paths"],
         "y, out: 8-byte accesses only under vec2"),
    _row("heads_pairgrid_kernel", "false", "tspn_heads_pairgrid_f32; tspn_forward_fused_f32 (canonical, odd T)",
         "!v3 && !vec2 (requires ldt == T, else TSPN_EUNSUPPORTED)",
         [OPS + "test_heads_pairgrid_matches_generic", KV + "test_heads_pairgrid_every_variant",
          KV + "test_forward_fused_conv_and_pair_paths"],
         "fallback for y / out not 8-byte aligned"),
    _row("heads_pairgrid3_kernel", None, "tspn_heads_pairgrid_f32; tspn_forward_fused_f32 (canonical, H != 12)",
         "v3 = ldt % 4 == 0 && ldt >= 4 && C % 16 == 0 && T % 2 == 0 && (y & 15) == 0 && (out & 7) == 0; "
         "!(H == 12 && Wp12 && fits32)",
         [KV + "test_heads_pairgrid_every_variant", KV + "test_forward_fused_conv_and_pair_paths"],
         "y 16-byte LDS-DMA pieces, out 8-byte stores: aligned by the condition"),
    _row("pack_heads12_kernel", None, "tspn_forward_fused_f32 (canonical, H == 12)", "v3 && H == 12 && Wp12 && fits32",
         [KV + "test_forward_fused_conv_and_pair_paths"]),
    _row("heads_pairgrid4_kernel", "8", "tspn_forward_fused_f32 (canonical, H == 12)",
         "v3 && H == 12 && Wp12 != nullptr && fits32 (TSPN_PAIRGRID4_CK = 8)",
         [KV + "test_forward_fused_conv_and_pair_paths"],
         "as heads_pairgrid3_kernel; y is the pass's own 256-byte aligned workspace"),
    # ------------------------------------------------------------------------------ tspn_pairs.hip
    _row("pair_index_kernel", None, "tspn_pair_index_i64", "N >= 2", [OPS + "test_pair_index"]),
    _row("transpose_gather_kernel", None, "tspn_pair_gather_f32 (feat); tspn_transpose_td_f32; tspn_forward_fused_f32",
         "pair_gather: out_feat && !rows_form; transpose_td: always",
         [OPS + "test_pair_gather", OPS + "test_transpose_mean_rows", KV + "test_pair_gather_rows_form_and_32x32_form",
          FE + "test_pair_gather_long_tracklets_second_workgroup_and_wave_edges",
          FE + "test_pair_features_beyond_65535_rows_in_both_forms[5-3-32x32]", FE + "test_transpose_td_refuses_65536_rows"],
         "fallback for feats / out_feat not 16-byte aligned"),
    _row("transpose_gather_rows_kernel", None, "tspn_pair_gather_f32 (feat)",
         "rows_form = out_feat && D % TG_C == 0 && T <= TG_TMAX && (feats & 15) == 0 && (out_feat & 15) == 0 && "
         "(2 * P) * (D / TG_C) < 2^31",
         [OPS + "test_pair_gather", KV + "test_pair_gather_rows_form_and_32x32_form",
          FE + "test_pair_features_beyond_65535_rows_in_both_forms[64-2-rows]"],
         "feats, out_feat: aligned by the condition"),
    _row("pair_geometry_kernel", None, "tspn_pair_gather_f32 (geom)", "out_geom != nullptr",
         [OPS + "test_pair_gather", FE + "test_pair_gather_long_tracklets_second_workgroup_and_wave_edges",
          FE + "test_pair_geometry_walks_its_slabs_of_65535_pairs"],
         "boxes (float4 loads): refused with TSPN_EINVAL unless 16-byte aligned"),
    _row("temporal_mean_td_kernel", None, "tspn_temporal_mean_f32 (layout_tc); tspn_temporal_sum_f32",
         "layout_tc && !(Cdim % 4 == 0 && ((x | out) & 15) == 0); temporal_sum: always",
         [OPS + "test_temporal_mean_vector_form_bit_identical_to_scalar", KV + "test_temporal_mean_td4_td_ct_by_alignment"],
         "fallback for x / out not 16-byte aligned"),
    _row("temporal_mean_td4_kernel", None, "tspn_temporal_mean_f32 (layout_tc); tspn_forward_fused_f32",
         "layout_tc && Cdim % 4 == 0 && ((x | out) & 15) == 0",
         [OPS + "test_temporal_mean_vector_form_bit_identical_to_scalar", KV + "test_temporal_mean_td4_td_ct_by_alignment"],
         "x, out float4: aligned by the condition"),
    _row("temporal_mean_ct_kernel", None, "tspn_temporal_mean_f32", "!layout_tc",
         [OPS + "test_transpose_mean_rows", KV + "test_temporal_mean_td4_td_ct_by_alignment"]),
    _row("pair_rows_kernel", None, "tspn_pair_rows_f32", "P > 0", [OPS + "test_transpose_mean_rows"]),
    # ------------------------------------------------------------------------------ tspn_dataset.hip
    _row("proposal_pair_filter_kernel", None, "tspn_proposal_pair_filter_i64", "S > 0",
         ["tests/test_gpu_dataset.py::test_proposal_pair_filter_golden"]),
    _row("gather_rows_kernel", "HIP_vector_type<float, 2u>", "tspn_gather_rows_f32",
         "v2 = F % 2 == 0 && ld % 2 == 0 && (src & 7) == 0 && (out & 7) == 0",
         ["tests/test_gpu_dataset.py::test_gather_rows_bit_exact", KV + "test_gather_rows_v2_and_scalar_by_alignment"],
         "src, out float2: aligned by the condition"),
    _row("gather_rows_kernel", "float", "tspn_gather_rows_f32", "!v2",
         [KV + "test_gather_rows_v2_and_scalar_by_alignment"], "fallback for src / out not 8-byte aligned"),
    # ------------------------------------------------------------------------------ tspn_linear.hip
    _row("linear_splitk_kernel", "false", "tspn_predicate_head_f32; pair_predicate (fused passes); tspn_span_predicate_f32",
         "always (splits = choose_splits(P, F, K) in [1, 64])",
         [OPS + "test_predicate_head_shapes", KV + "test_predicate_head_split_k_edges",
          KV + "test_forward_fused_conv_and_pair_paths"]),
    _row("linear_reduce_kernel", None, "tspn_predicate_head_f32 (reduce)", "always",
         [OPS + "test_predicate_head_shapes", KV + "test_predicate_head_split_k_edges"]),
    _row("linear_splitk_kernel", "true", "tspn_predicate_head_norm_f32", "always (slice table of <= 128 entries)",
         [OPS + "test_predicate_head_fused_preprocess_vs_oracle", KV + "test_predicate_head_norm_table_over_64_slices"]),
    _row("linear_reduce_norm_kernel", None, "tspn_predicate_head_norm_f32 (reduce)", "always",
         [OPS + "test_predicate_head_fused_preprocess_vs_oracle", KV + "test_predicate_head_norm_table_over_64_slices"]),
    _row("pair_combine_kernel", None, "tspn_forward_fused_f32; tspn_forward_fused_bf16 (pair_predicate)", "P > 0 && NT > 0",
         [OPS + "test_forward_fused_vs_dense_oracle", KV + "test_forward_fused_conv_and_pair_paths"]),
    _row("span_prefix_kernel", None, "tspn_span_predicate_f32", "P > 0 && NT > 0 (grid capped at 8192 blocks)",
         [SPAN + "test_span_predicate_cfg2_video_all_pairs", SPAN + "test_span_predicate_cfg3_shape_sampled_pairs",
          SPAN + "test_span_predicate_prefix_and_combine_grids_stride",
          BF16 + "test_bf16_and_span_entry_points_edge_cases", "tests/test_gpu_model.py::test_span_restricted_reloipool"]),
    _row("span_combine_kernel", None, "tspn_span_predicate_f32",
         "P > 0 && NT > 0 (grid capped at 8192 blocks); per output: sums the span's own frames of G when PS[e] is not finite",
         [SPAN + "test_span_predicate_cfg2_video_all_pairs", SPAN + "test_span_predicate_four_videos_global_ids_shuffled_table",
          SPAN + "test_span_predicate_ragged_small_shapes", SPAN + "test_span_predicate_prefix_and_combine_grids_stride",
          SPAN + "test_span_predicate_nonfinite_stays_in_the_spans_that_hold_it",
          BF16 + "test_bf16_and_span_entry_points_edge_cases", "tests/test_gpu_model.py::test_span_restricted_reloipool"]),
    # ------------------------------------------------------------------------------ small entry points
    _row("block_l1_kernel", None, "tspn_feature_preprocess_f32", "P > 0",
         [OPS + "test_feature_preprocess_matches_oracle", FE + "test_block_l1_small_and_ragged_blocks_vs_float64",
          FE + "test_block_l1_row_stride_longer_than_the_row", FE + "test_block_l1_refusals"]),
    _row("ppn_kernel", None, "tspn_ppn_pair_matrix_topk_f32", "always", [OPS + "test_ppn_golden"]),
    _row("traj_iou_kernel", None, "tspn_traj_iou_f32", "always", [OPS + "test_traj_iou_golden_bit_exact"]),
    _row("traj_iou_tail_f64_kernel", None, "tspn_traj_iou_tail_f64", "always",
         ["tests/test_gpu_association.py::test_traj_iou_tail_bit_exact_vs_host_recipe"]),
    _row("pair_topk_kernel", None, "tspn_decode_topk_f32", "always", [OPS + "test_decode_topk_golden"]),
    _row("segment_topk_kernel", None, "tspn_decode_topk_f32", "always", [OPS + "test_decode_topk_golden"]),
    _row("decode_spans_kernel", None, "tspn_decode_spans_f32", "always", [OPS + "test_decode_spans_bit_exact"]),
    _row("status_selftest_kernel", None, "tspn_status_selftest", "always",
         ["tests/test_gpu_status_guard.py::test_device_fault_is_reported_by_the_next_launch_entry_and_clear_rearms"]),
    _row("conv3_spot_check_kernel", None, "tspn_conv3_spot_check_f32; tspn_forward_fused_f32 (Winograd guard)", "rows > 0",
         ["tests/test_gpu_status_guard.py::test_spot_check_measures_the_error_of_a_conv_launch"]),
    # ------------------------------------------------------------------------------ tspn_wino63.hip
    # (three names are defined twice, fp32 form and split-fp16 form: their rows spell the overload's parameter types)
    _row("pack_wino63_frag_kernel", "(float const*, long, long, long, float*)", "tspn_pack_conv3_wino63_frag_f32", "always",
         ["tests/test_gpu_wino63.py::test_conv3_winograd63_vs_fp64"]),
    _row("wino63_input_transform_kernel", "(float const*, float*, int, int, int, long, long, long, unsigned long long*)",
         "tspn_conv3_tc_wino63_f32; tspn_forward_fused_f32 (Winograd)", "always",
         ["tests/test_gpu_wino63.py::test_conv3_winograd63_vs_fp64"]),
    _row("conv3_wino63_kernel", "true", "tspn_conv3_tc_wino63_f32; tspn_forward_fused_f32 (Winograd)",
         "bufv = TSPN_WINO63_BUFV && wino63_workspace_bytes < 2^32 && piece form 0",
         ["tests/test_gpu_wino63.py::test_conv3_winograd63_vs_fp64"], "x: refused with TSPN_EUNSUPPORTED unless 16-byte aligned"),
    _row("conv3_wino63_kernel", "false", "tspn_conv3_tc_wino63_f32", "!bufv",
         ["tests/test_gpu_wino63.py::test_conv3_winograd63_buffer_and_pointer_pieces_are_bit_identical"],
         "as conv3_wino63_kernel<true>"),
    # split-fp16 form (TSPN_CONV_WINOGRAD63_F16X3): overloads of the three names above
    _row("pack_wino63_frag_kernel", "(float const*, long, long, long, short*)", "tspn_pack_conv3_wino63_f16x3",
         "wino63_f16x3_supported(Cp, Mp) = Cp % 32 == 0 && Mp % F_BM == 0 (else TSPN_EUNSUPPORTED); split == 0 || Cin == 2 * split "
         "(else TSPN_EINVAL)",
         [KV + "test_wino63_f16x3_tile_grid_and_sextet_edges", KV + "test_wino63_f16x3_refusals_leave_the_output_untouched",
          F16N + "test_f16x3_weight_nonfinite_stays_in_its_row"],
         "packed: refused with TSPN_EINVAL unless 16-byte aligned"),
    _row("wino63_input_transform_kernel", "(float const*, _Float16*, int*, int, int, int, long, long, long, unsigned long long*)",
         "tspn_conv3_tc_wino63_f16x3; tspn_forward_fused_f32 (TSPN_CONV_WINOGRAD63_F16X3)",
         "wino63_f16x3_supported(Cin, M) = Cin % 32 == 0 && M % F_BM == 0 (else TSPN_EUNSUPPORTED); fused: D % 64 == 0",
         [KV + "test_wino63_f16x3_tile_grid_and_sextet_edges", KV + "test_wino63_f16x3_sextet_counts_at_the_tile_edge",
          KV + "test_wino63_f16x3_every_T_both_store_forms", KV + "test_forward_fused_f16x3_against_dense_oracle",
          KV + "test_forward_fused_f16x3_refuses_d32_before_any_launch", F16N + "test_f16x3_nonfinite_confined_to_its_sextets",
          F16N + "test_f16x3_guard_reads_inf_and_names_the_nan_sextet", F16R + "test_f16x3_wide_in_column_range"],
         "x: refused with TSPN_EINVAL unless 16-byte aligned; workspace: TSPN_EWORKSPACE when short, TSPN_EINVAL unless "
         "256-byte aligned"),
    _row("conv3_wino63_kernel",
         "(_Float16 const*, int const*, short const*, float const*, float*, float*, int, int, int, int, long, long, int, int, int, "
         "int, int, int)",
         "tspn_conv3_tc_wino63_f16x3; tspn_forward_fused_f32 (TSPN_CONV_WINOGRAD63_F16X3)",
         "wino63_f16x3_supported(Cin, M); vec2 = ldy % 2 == 0 && ldy >= 6 * nq && (y & 7) == 0 (C entry: ldy = T; fused: ldy = "
         "ceil4(T) with canonical pairs and even T, else T); GM = TSPN_WINO63_GM row tiles per group, XCD remap of the grid",
         [KV + "test_wino63_f16x3_tile_grid_and_sextet_edges", KV + "test_wino63_f16x3_sextet_counts_at_the_tile_edge",
          KV + "test_wino63_f16x3_every_T_both_store_forms", KV + "test_wino63_f16x3_contraction_depths", KV + "test_wino63_f16x3_refusals_leave_the_output_untouched",
          KV + "test_forward_fused_f16x3_against_dense_oracle", F16N + "test_f16x3_nonfinite_confined_to_its_sextets",
          F16N + "test_f16x3_inf_times_zero_and_finite_overflow", F16R + "test_f16x3_wide_in_column_range", F16R + "test_f16x3_guard_trips_on_a_dead_hot_channel"],
         "packed: refused with TSPN_EUNSUPPORTED unless 16-byte aligned; y: 8-byte stores only under vec2, else the scalar "
         "stores (any float view)"),
    # ------------------------------------------------------------------------------ tspn_bf16.hip
    _row("cast_bf16_kernel", None, "tspn_cast_bf16", "always", [BF16 + "test_cast_bf16_bit_exact"]),
    _row("pack_conv3_bf16_kernel", None, "tspn_pack_conv3_bf16", "always", [BF16 + "test_pack_layouts_bf16"]),
    _row("pack_heads_bf16_kernel", None, "tspn_pack_heads_bf16", "always",
         [BF16 + "test_pack_layouts_bf16", KV + "test_heads_pairgrid_bf16_small_and_big",
          HH + "test_pack_heads_bf16_zeroes_the_rows_from_h_up"]),
    _row("temporal_mean_bf16_kernel", None, "tspn_temporal_mean_bf16; tspn_forward_fused_bf16", "D % 8 == 0",
         [BF16 + "test_temporal_mean_bf16", BND + "test_temporal_mean_bf16_lies_in_its_interval",
          BND + "test_temporal_mean_bf16_exact_cases", BND + "test_fused_bf16_passes_equal_their_stages_at_cfg3_depth"],
         "x: refused with TSPN_EINVAL unless 16-byte aligned"),
    _row("conv3_bf16_big_kernel", None, "tspn_conv3_tc_bf16; tspn_forward_fused_bf16", "always",
         [BF16 + "test_conv3_bf16_vs_fp64", BND + "test_conv3_bf16_meets_the_budget", BND + "test_conv3_bf16_is_exact_at_cfg3_depth",
          BND + "test_fused_bf16_passes_equal_their_stages_at_cfg3_depth"], "refused with TSPN_EUNSUPPORTED unless 16-byte aligned"),
    _row("heads_pairgrid_bf16_kernel", "4, 8, 2", "tspn_heads_pairgrid_bf16; tspn_forward_fused_bf16", "N <= 12",
         [BF16 + "test_heads_pairgrid_bf16_vs_fp64", KV + "test_heads_pairgrid_bf16_small_and_big",
          KV + "test_heads_pairgrid_bf16_grids_the_xcd_remap_does_not_divide",
          HH + "test_heads_pairgrid_bf16_vs_fp64_for_every_h", BND + "test_heads_pairgrid_bf16_meets_the_budget",
          BND + "test_heads_pairgrid_bf16_meets_the_budget_with_sixteen_heads",
          BND + "test_heads_pairgrid_bf16_is_exact_where_every_partial_sum_is",
          BND + "test_fused_bf16_passes_equal_their_stages_at_cfg3_depth"],
         "y, head_packed: refused with TSPN_EUNSUPPORTED unless 16-byte aligned"),
    _row("heads_pairgrid_bf16_kernel", "8, 16, 2", "tspn_heads_pairgrid_bf16; tspn_forward_fused_bf16",
         "N > 12 (TSPN_HPB_SW = 2)",
         [BF16 + "test_heads_pairgrid_bf16_vs_fp64", KV + "test_heads_pairgrid_bf16_small_and_big",
          KV + "test_heads_pairgrid_bf16_grids_the_xcd_remap_does_not_divide",
          HH + "test_heads_pairgrid_bf16_vs_fp64_for_every_h", BND + "test_heads_pairgrid_bf16_meets_the_budget",
          BND + "test_heads_pairgrid_bf16_is_exact_where_every_partial_sum_is"],
         "as heads_pairgrid_bf16_kernel<4, 8, 2>"),
    _row("transpose_cast_bf16_kernel", None, "tspn_transpose_cast_bf16", "always",
         [BF16 + "test_dense_bf16_pieces_ragged_and_errors"]),
    _row("heads_dense_bf16_kernel", None, "tspn_temporal_encoder_heads_bf16", "always",
         [BF16 + "test_dense_bf16_encoder_heads_vs_reference_bf16_modules_g8",
          HH + "test_temporal_encoder_heads_bf16_vs_fp64_for_every_h",
          BND + "test_dense_heads_bf16_meet_the_budget_through_both_entries",
          BND + "test_dense_heads_bf16_are_exact_where_every_partial_sum_is"]),
    # ------------------------------------------------------------------------------ tspn_roi.hip (fp32 ResNet pieces)
    _row("pack_conv2d_kernel", None, "tspn_pack_conv2d_f32", "always", [ROI + "test_conv2d_nhwc_vs_torch"] + CE_PACK),
    _row("conv2d_nhwc_kernel", "16", "tspn_conv2d_nhwc_f32", "always", [ROI + "test_conv2d_nhwc_vs_torch"] + CE_ALL),
    _row("pack_conv2d_frag_kernel", None, "tspn_pack_conv2d_frag_f32", "always", [ROI + "test_conv2d_nhwc_vs_torch"] + CE_PACK),
    _row("pack_conv2d_frag_cin4_kernel", None, "tspn_pack_conv2d_frag_cin4_f32", "always",
         [ROI + "test_conv2d_stem_form_vs_torch"] + CE_PACK),
    _row("conv2d_nhwc_frag_kernel", "false", "tspn_conv2d_nhwc_frag_f32", "always", [ROI + "test_conv2d_nhwc_vs_torch"] + CE_ALL),
    _row("conv2d_nhwc_frag_kernel", "true", "tspn_conv2d_nhwc_cin4_f32", "always",
         [ROI + "test_conv2d_stem_form_vs_torch"] + CE_ALL),
    _row("roi_align_nhwc_kernel", "false, false", "tspn_roi_align_nhwc_f32", "fp32 in, fp32 out",
         [ROI + "test_roi_align_nhwc_vs_oracle", FE + "test_roi_align_thread_loop_second_trip_vs_float32_and_float64_oracle",
          FE + "test_roi_align_three_instantiations_on_a_bf16_exact_map",
          FE + "test_roi_align_single_sample_on_the_limits_of_bilinear_setup",
          FE + "test_roi_align_writes_every_element_and_nothing_else", FE + "test_roi_align_refusals_leave_the_output_alone",
          FE + "test_roi_align_many_rois_each_row_bit_identical_to_its_own_launch",
          FE + "test_roi_align_map_index_interleaved_and_clamped"]),
    _row("roi_align_nhwc_kernel", "false, true", "tspn_roi_align_nhwc_f32_bf16out", "fp32 in, bf16 out",
         [ROI + "test_roi_align_nhwc_vs_oracle", FE + "test_roi_align_three_instantiations_on_a_bf16_exact_map",
          FE + "test_roi_align_refusals_leave_the_output_alone",
          FE + "test_roi_align_writes_every_element_and_nothing_else"]),
    _row("roi_align_nhwc_kernel", "true, true", "tspn_roi_align_nhwc_bf16", "bf16 in, bf16 out",
         [ROI + "test_roi_align_nhwc_vs_oracle", FE + "test_roi_align_three_instantiations_on_a_bf16_exact_map",
          FE + "test_roi_align_refusals_leave_the_output_alone"]),
    _row("max_pool_nhwc_kernel", "false", "tspn_max_pool_nhwc_f32", "fp32 out",
         [ROI + "test_max_pool_nhwc", FE + "test_max_pool_all_three_forms_bit_for_bit_vs_torch",
          FE + "test_max_pool_refuses_channel_counts_it_cannot_vectorise"]),
    _row("max_pool_nhwc_kernel", "true", "tspn_max_pool_nhwc_f32", "bf16 out",
         [ROI + "test_max_pool_nhwc", FE + "test_max_pool_all_three_forms_bit_for_bit_vs_torch",
          FE + "test_max_pool_refuses_channel_counts_it_cannot_vectorise"]),
    # ------------------------------------------------------------------------------ tspn_roi_bf16.hip
    _row("pack_conv2d_frag_bf16_kernel", None, "tspn_pack_conv2d_frag_bf16", "always",
         [ROI + "test_conv2d_nhwc_bf16_vs_fp64", KV + "test_conv2d_nhwc_bf16_mi2_without_ring"] + CE_PACK),
    _row("conv2d_nhwc_bf16_kernel", "1, false", "tspn_conv2d_nhwc_bf16",
         "mi = (Cout % 64 == 0 && !(KH * KW == 1 && Cin <= 256)) ? 2 : 1; rng = KH == 3 && KW == 3 && stride == 1 && "
         "pad == 1; mi == 1 && !rng",
         [ROI + "test_conv2d_nhwc_bf16_vs_fp64"] + CE_ALL, "all operands: refused with TSPN_EUNSUPPORTED unless 16-byte aligned"),
    _row("conv2d_nhwc_bf16_kernel", "1, true", "tspn_conv2d_nhwc_bf16", "mi == 1 && rng",
         [ROI + "test_conv2d_nhwc_bf16_vs_fp64"] + CE_RNG, "as <1, false>"),
    _row("conv2d_nhwc_bf16_kernel", "2, false", "tspn_conv2d_nhwc_bf16", "mi == 2 && !rng",
         [KV + "test_conv2d_nhwc_bf16_mi2_without_ring"] + CE_ALL, "as <1, false>"),
    _row("conv2d_nhwc_bf16_kernel", "2, true", "tspn_conv2d_nhwc_bf16", "mi == 2 && rng",
         [ROI + "test_conv2d_nhwc_bf16_vs_fp64"] + CE_RNG, "as <1, false>"),
    # ------------------------------------------------------------------------------ stem, bottleneck tails and blocks
    _row("stem_s2d_bf16_kernel", None, "tspn_stem_conv_bf16; tspn_stem_pool_bf16", "always",
         [ROI + "test_stem_bf16_vs_oracle"]),
    _row("pack_stem_bf16_kernel", None, "tspn_pack_stem_bf16", "always", [ROI + "test_stem_bf16_vs_oracle"]),
    _row("stem_conv_bf16_kernel", "2", "tspn_stem_conv_bf16", "Cout == 64", [ROI + "test_stem_bf16_vs_oracle"]),
    _row("stem_conv_bf16_kernel", "1", "tspn_stem_conv_bf16", "Cout != 64",
         [ROI + "test_bottleneck_tail_and_stem_random_shapes"]),
    _row("stem_pool_bf16_kernel", "2", "tspn_stem_pool_bf16", "Cout == 64",
         [ROI + "test_stem_pool_fused_bit_identical_to_conv_then_pool"]),
    _row("stem_pool_bf16_kernel", "1", "tspn_stem_pool_bf16", "Cout != 64",
         [ROI + "test_bottleneck_tail_and_stem_random_shapes"]),
    _row("max_pool_nhwc_bf16_kernel", None, "tspn_max_pool_nhwc_bf16", "always",
         [ROI + "test_stem_bf16_vs_oracle", FE + "test_max_pool_all_three_forms_bit_for_bit_vs_torch",
          FE + "test_max_pool_refuses_channel_counts_it_cannot_vectorise"]),
    _row("bottleneck_bf16_kernel", "64, false", "tspn_bottleneck_tail_bf16", "CM == 64",
         [ROI + "test_bottleneck_tail_fused_bit_identical_to_two_convs", ROI + "test_bottleneck_tail_narrow_widths_on_a_ragged_grid_write_every_tile"], "refused with TSPN_EUNSUPPORTED unless 16-byte aligned"),
    _row("bottleneck_bf16_kernel", "128, false", "tspn_bottleneck_tail_bf16", "CM == 128",
         [ROI + "test_bottleneck_tail_fused_bit_identical_to_two_convs", ROI + "test_bottleneck_tail_narrow_widths_on_a_ragged_grid_write_every_tile"], "as <64, false>"),
    _row("bottleneck_bf16_kernel", "256, false", "tspn_bottleneck_tail_bf16", "CM == 256",
         [ROI + "test_bottleneck_tail_fused_bit_identical_to_two_convs"], "as <64, false>"),
    _row("bottleneck_bf16_kernel", "256, true", "tspn_bottleneck_tail_next_bf16", "CM == 256 with the next block's conv1",
         [ROI + "test_bottleneck_tail_with_next_conv1_bit_identical"], "as <64, false>"),
    _row("bottleneck_pipe_bf16_kernel", None, "tspn_bottleneck_tail_pipe_bf16", "CM == 256",
         [ROI + "test_bottleneck_tail_persistent_pipelined_bit_identical"], "as bottleneck_bf16_kernel"),
    _row("tail_io_bf16_kernel", None, "tspn_bottleneck_tail_io_bf16", "CM == 256",
         [ROI + "test_bottleneck_tail_role_split_bit_identical"], "as bottleneck_bf16_kernel"),
    _row("bottleneck_block_bf16_kernel", "128, 512, 1, 0", "tspn_bottleneck_block_bf16", "CM == 128",
         [ROI + "test_bottleneck_block_one_launch_bit_identical_to_conv1_plus_fused_tail"],
         "all operands: refused with TSPN_EUNSUPPORTED unless 16-byte aligned"),
    _row("bottleneck_block_bf16_kernel", "64, 256, 1, 0", "tspn_bottleneck_block_bf16", "CM != 128",
         [ROI + "test_bottleneck_block_one_launch_bit_identical_to_conv1_plus_fused_tail"], "as above"),
    _row("bottleneck_block_bf16_kernel", "64, 64, 1, 1", "tspn_bottleneck_block_proj_bf16",
         "CM == 64 && CIN == 64 && stride == 1 (else TSPN_EUNSUPPORTED)",
         [ROI + "test_first_block_of_a_stage_one_launch_bit_identical_to_its_four_launches"], "as above"),
    _row("bottleneck_block_bf16_kernel", "128, 256, 2, 2", "tspn_bottleneck_block_res_bf16",
         "CM == 128 && CIN == 256 && stride == 2 (else TSPN_EUNSUPPORTED)",
         [ROI + "test_res3_first_block_conv1_3x3_expand_one_launch_bit_identical"], "as above"),
]

# tests/test_gpu_fp32_bound.py: the fp32 scorer rows its exact cases, derived budgets and held outputs reach, added to the rows
# above ((kernel, inst) -> tests; the file asserts the conv and pair-grid variant with conv3_variant / pairgrid_variant)
F32 = "tests/test_gpu_fp32_bound.py::"
_CONV_F32 = [F32 + "test_conv3_every_variant_is_exact_at_tile_edges", F32 + "test_conv3_every_variant_meets_the_budget_on_every_kind",
             F32 + "test_conv3_is_exact_on_the_tile_map_with_a_short_last_group"]
_HEADS_F32 = [F32 + "test_heads_kernel_is_exact_in_both_modes_vec2_and_scalar", F32 + "test_heads_kernel_meets_the_budget_on_every_kind"]
_GRID_F32 = [F32 + "test_heads_pairgrid_is_exact_in_every_variant_and_has_the_bits_of_heads_mode_1",
             F32 + "test_heads_pairgrid_meets_the_budget_on_every_kind"]
_MEAN_F32 = [F32 + "test_temporal_mean_and_sum_are_exact_for_every_t", F32 + "test_temporal_mean_and_sum_lie_in_their_intervals"]
_LIN_F32 = [F32 + "test_predicate_head_raw_is_exact_on_every_split_k_row", F32 + "test_predicate_head_raw_meets_the_budget_on_every_kind",
            F32 + "test_training_backward_products_are_exact_on_the_split_k_gemm",
            F32 + "test_sigmoid_epilogue_against_the_float64_sigmoid_of_the_kernels_own_logits"]
_NORM_F32 = [F32 + "test_predicate_head_norm_is_exact_and_meets_the_budget",
             F32 + "test_sigmoid_epilogue_against_the_float64_sigmoid_of_the_kernels_own_logits"]
_FUSED_F32 = [F32 + "test_fused_pass_is_exact_and_equals_its_stages"]
_MOVERS_F32 = [F32 + "test_data_movers_into_held_outputs"]
FP32_BOUND_TESTS = {
    ("pack_conv3_kernel", None): _CONV_F32,
    ("conv3_mfma_kernel", "false"): _CONV_F32,
    ("conv3_mfma_kernel", "true"): _CONV_F32,
    ("conv3_mfma_dma_kernel", "16"): _CONV_F32 + [F32 + "test_conv3_at_full_depth", F32 + "test_temporal_encoder_heads_is_exact_and_equals_its_stages"],
    ("conv3_mfma_dma_kernel", "8"): _CONV_F32,
    ("conv3_mfma_cl_kernel", None): [F32 + "test_conv3_channels_last_is_exact_and_has_the_bits_of_the_channels_first_kernel",
                                     F32 + "test_conv3_channels_last_meets_the_budget_on_every_kind", F32 + "test_conv3_at_full_depth"]
    + _FUSED_F32,
    ("heads_kernel", "0, true"): _HEADS_F32 + [F32 + "test_temporal_encoder_heads_is_exact_and_equals_its_stages"],
    ("heads_kernel", "0, false"): _HEADS_F32 + [F32 + "test_heads_kernel_is_exact_at_full_depth",
                                                F32 + "test_temporal_encoder_heads_is_exact_and_equals_its_stages"],
    ("heads_kernel", "1, true"): _HEADS_F32 + _GRID_F32[:1],
    ("heads_kernel", "1, false"): _HEADS_F32 + [F32 + "test_heads_kernel_is_exact_at_full_depth"] + _GRID_F32[:1] + _FUSED_F32,
    ("heads_pairgrid_kernel", "true"): _GRID_F32,
    ("heads_pairgrid_kernel", "false"): _GRID_F32 + _FUSED_F32,
    ("heads_pairgrid3_kernel", None): _GRID_F32,
    ("pack_heads12_kernel", None): _FUSED_F32,
    ("heads_pairgrid4_kernel", "8"): _FUSED_F32,
    ("transpose_gather_kernel", None): _MOVERS_F32,
    ("transpose_gather_rows_kernel", None): _MOVERS_F32,
    ("pair_rows_kernel", None): _MOVERS_F32,
    ("temporal_mean_td_kernel", None): _MEAN_F32,
    ("temporal_mean_td4_kernel", None): _MEAN_F32 + _FUSED_F32,
    ("temporal_mean_ct_kernel", None): _MEAN_F32,
    ("gather_rows_kernel", "HIP_vector_type<float, 2u>"): [F32 + "test_gather_rows_past_one_slab"],
    ("gather_rows_kernel", "float"): [F32 + "test_gather_rows_past_one_slab"],
    ("linear_splitk_kernel", "false"): _LIN_F32 + _FUSED_F32,
    ("linear_reduce_kernel", None): _LIN_F32,
    ("linear_splitk_kernel", "true"): _NORM_F32,
    ("linear_reduce_norm_kernel", None): _NORM_F32,
    ("pair_combine_kernel", None): _FUSED_F32,
}
_rows = {(r["kernel"], r["inst"]): r for r in VARIANTS}
for _key, _tests in FP32_BOUND_TESTS.items():
    _rows[_key]["tests"] += _tests
