"""Which compiled kernel the split-fp16 pair stage's C-ABI entry points launch, the condition their launcher uses, and the
tests that reach it: the table of tests/kernel_variants.py, in the same format, for
temporal-span-proposal-network-vidvrd_amd/csrc/pairf16/*.hip.

tests/test_pairf16_variant_table.py keeps this table equal to the sources and its node ids pointing at tests that exist."""

PF = "tests/test_gpu_pair_stage_f16x3.py::"

ENTRY = "tspn_heads_pairgrid_f16x3; tspn_forward_fused_f32 (TSPN_CONV_WINOGRAD63_F16X3, canonical pairs, H == 12)"
ALIGN = "y and split_buf 16-byte aligned, out 8-byte aligned, ldt % 4 == 0, T % 2 == 0, C % 32 == 0"


def _row(kernel, inst, entry, when, tests, align="no alignment requirement"):
    return {"kernel": kernel, "inst": inst, "entry": entry, "when": when, "tests": list(tests), "align": align}


VARIANTS = [
    # ------------------------------------------------------------------------------ pairf16/tspn_heads_pair_f16x3.hip
    _row("pairf16_scale_kernel", None, ENTRY, "B > 0 && N >= 2 (one workgroup, once per call)",
         [PF + "test_pair_stage_f16x3_vs_fp64", PF + "test_pair_stage_f16x3_flagged_weights_take_the_fp32_chain"]),
    _row("pairf16_pack_kernel", None, ENTRY, "B > 0 && N >= 2 (one workgroup per 32 channels, once per call)",
         [PF + "test_pair_stage_f16x3_vs_fp64", PF + "test_pair_stage_f16x3_flagged_weights_take_the_fp32_chain"], align=ALIGN),
    _row("heads_pair_f16x3_kernel", None, ENTRY, "B > 0 && N >= 2",
         [PF + "test_pair_stage_f16x3_vs_fp64", PF + "test_pair_stage_f16x3_range_and_nonfinite_tiles",
          PF + "test_pair_stage_f16x3_flagged_weights_take_the_fp32_chain",
          PF + "test_forward_fused_runs_the_f16x3_pair_stage_only_on_the_promoted_form"], align=ALIGN),
]
