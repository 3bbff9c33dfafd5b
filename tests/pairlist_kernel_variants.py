"""Which compiled kernel variant the bf16 pair-list stage's C-ABI entry points launch, the condition their launcher uses
to pick it, and the tests that reach it: the table of tests/kernel_variants.py, in the same format, for
temporal-span-proposal-network-vidvrd_amd/csrc/pairlist/*.hip.

tests/test_pairlist_bf16_host.py keeps this table equal to the sources and its node ids pointing at tests that exist;
tools/check_kernel_variants.py checks a `rocprofv3 --kernel-trace --stats` run against this table too."""

PL = "tests/test_gpu_pairlist_bf16.py::"
SCAN = "tests/test_gpu_pairplan_scan.py::"
TILES = "tests/test_gpu_pairlist_tiles.py::"
HH = "tests/test_gpu_bf16_heads_h.py::"
BND = "tests/test_gpu_bf16_bound.py::"


def _row(kernel, inst, entry, when, tests, align="no alignment requirement"):
    return {"kernel": kernel, "inst": inst, "entry": entry, "when": when, "tests": list(tests), "align": align}


VARIANTS = [
    # ------------------------------------------------------------------------------ pairlist/tspn_pairlist_bf16.hip
    _row("pair_plan_lists_kernel", None, "tspn_pair_plan_i32", "B > 0 && N > 0 (one workgroup per video)",
         [PL + "test_plan_equals_the_numpy_restatement", PL + "test_arbitrary_tables_vs_fp64",
          SCAN + "test_ranks_past_the_first_wave", SCAN + "test_table_rows_past_the_first_stride",
          SCAN + "test_three_videos_with_different_occupancies_and_bad_rows_in_one_launch"]),
    _row("pair_plan_link_kernel", None, "tspn_pair_plan_i32", "B > 0 && N > 0 && P > 0",
         [PL + "test_plan_equals_the_numpy_restatement", PL + "test_arbitrary_tables_vs_fp64",
          SCAN + "test_link_kernel_second_grid_pass_and_long_chains_twice",
          SCAN + "test_five_thousand_identical_rows_are_one_chain"]),
    _row("heads_pairlist_bf16_kernel", "4, 8, 2", "tspn_heads_pairlist_bf16", "N <= 12 && P > 0",
         [PL + "test_list_rows_equal_the_grid_rows", PL + "test_arbitrary_tables_vs_fp64",
          TILES + "test_unequal_axes_small_form", TILES + "test_one_local_table_on_both_sides_of_the_form_switch",
          TILES + "test_a_nonfinite_activation_in_the_v_half_stays_in_its_object_rows_and_frame",
          HH + "test_heads_pairlist_bf16_vs_fp64_and_the_grid_rows_for_every_h",
          BND + "test_heads_pairlist_bf16_rows_off_the_benign_distribution",
          BND + "test_fused_bf16_passes_equal_their_stages_at_cfg3_depth"],
         align="y and head_packed 16-byte aligned, ldm % 4 == 0, C % 32 == 0"),
    _row("heads_pairlist_bf16_kernel", "8, 16, 2", "tspn_heads_pairlist_bf16", "N > 12 && P > 0",
         [PL + "test_list_rows_equal_the_grid_rows", PL + "test_arbitrary_tables_vs_fp64",
          PL + "test_forward_fused_bf16_on_a_pair_table", TILES + "test_unequal_axes_big_form",
          TILES + "test_three_videos_with_different_compact_extents",
          TILES + "test_every_listed_row_is_written_and_nothing_else",
          TILES + "test_a_million_rows_on_380_chains_equal_the_grid_rows",
          HH + "test_heads_pairlist_bf16_vs_fp64_and_the_grid_rows_for_every_h"],
         align="y and head_packed 16-byte aligned, ldm % 4 == 0, C % 32 == 0"),
]
