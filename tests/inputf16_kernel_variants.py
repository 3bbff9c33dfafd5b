"""Which compiled kernels the fused input side of the split-fp16 F(6,3) conv launches, the condition their launcher uses,
and the tests that reach it: the table of tests/kernel_variants.py, in the same format, for
temporal-span-proposal-network-vidvrd_amd/csrc/inputf16/*.hip.

tests/test_inputf16_variant_table.py keeps this table equal to the sources and its node ids pointing at tests that exist."""

IN = "tests/test_gpu_input_f16x3.py::"

ENTRY = ("tspn_conv3_tc_wino63_f16x3_input; tspn_conv3_tc_wino63_f16x3; tspn_forward_fused_f32 (TSPN_CONV_WINOGRAD63_F16X3), "
         "where it also writes the temporal mean")
WHEN = ("tspn_conv3_tc_wino63_f16x3_set_input_form: 0 (default) = Cin <= 2048 && Cin >= 1024 && 2 NT >= CUs "
        "(tspn_conv3_tc_wino63_f16x3_input_form), 2 = Cin <= 2048, 1 = never")
ALIGN = "x, fbar and the workspace 16-byte aligned (the entries ask 256 of the workspace), Cin % 8 == 0"


TESTS = [IN + "test_fused_input_side_equals_the_two_pass_bytes", IN + "test_value_cases_zero_column_nan_inf",
         IN + "test_hot_value_counts_in_its_own_sextet_only", IN + "test_shapes_outside_the_kernels_fall_back",
         IN + "test_conv_entry_y_is_the_same_under_both_forms",
         IN + "test_fused_pass_and_guard_reading_are_the_same_under_both_forms"]


def _row(kernel, inst, entry, when, tests, align="no alignment requirement"):
    return {"kernel": kernel, "inst": inst, "entry": entry, "when": when, "tests": list(tests), "align": align}


VARIANTS = [
    # ------------------------------------------------------------------------------ inputf16/tspn_input_f16x3.hip
    _row("input_f16x3_scan_kernel", None, ENTRY,
         WHEN + "; one workgroup of ceil64(Cin / 4) threads per tracklet + one per 64 padding sextets", TESTS, align=ALIGN),
    _row("input_f16x3_split_kernel", None, ENTRY,
         WHEN + "; behind the scan kernel, one workgroup per (8 sextets, 32 channel groups)", TESTS, align=ALIGN),
]
