"""Which compiled kernel variant the bf16 pair-list stage's C-ABI entry points launch, the condition their launcher uses
to pick it, and the tests that reach it: the table of tests/kernel_variants.py, in the same format, for
temporal-span-proposal-network-vidvrd_amd/csrc/pairlist/*.hip.

tests/test_pairlist_bf16_host.py keeps this table equal to the sources and its node ids pointing at tests that exist;
tools/check_kernel_variants.py checks a `rocprofv3 --kernel-trace --stats` run against this table too."""

PL = "tests/test_gpu_pairlist_bf16.py::"


def _row(kernel, inst, entry, when, tests, align="no alignment requirement"):
    return {"kernel": kernel, "inst": inst, "entry": entry, "when": when, "tests": list(tests), "align": align}


VARIANTS = [
    # ------------------------------------------------------------------------------ pairlist/tspn_pairlist_bf16.hip
    _row("pair_plan_lists_kernel", None, "tspn_pair_plan_i32", "B > 0 && N > 0 (one workgroup per video)",
         [PL + "test_plan_equals_the_numpy_restatement", PL + "test_arbitrary_tables_vs_fp64"]),
    _row("pair_plan_link_kernel", None, "tspn_pair_plan_i32", "B > 0 && N > 0 && P > 0",
         [PL + "test_plan_equals_the_numpy_restatement", PL + "test_arbitrary_tables_vs_fp64"]),
    _row("heads_pairlist_bf16_kernel", "4, 8, 2", "tspn_heads_pairlist_bf16", "N <= 12 && P > 0",
         [PL + "test_list_rows_equal_the_grid_rows", PL + "test_arbitrary_tables_vs_fp64"],
         align="y and head_packed 16-byte aligned, ldm % 4 == 0, C % 32 == 0"),
    _row("heads_pairlist_bf16_kernel", "8, 16, 2", "tspn_heads_pairlist_bf16", "N > 12 && P > 0",
         [PL + "test_list_rows_equal_the_grid_rows", PL + "test_arbitrary_tables_vs_fp64",
          PL + "test_forward_fused_bf16_on_a_pair_table"],
         align="y and head_packed 16-byte aligned, ldm % 4 == 0, C % 32 == 0"),
]
