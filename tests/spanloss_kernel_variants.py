"""Which compiled kernel the span-loss entries launch, the condition their launcher uses, the granularities of each and the
tests that reach it: the table of tests/kernel_variants.py, in the same format, for
temporal-span-proposal-network-vidvrd_amd/csrc/spanloss/*.hip.

tests/test_span_loss_host.py keeps this table equal to the sources and its node ids pointing at tests that exist;
tools/check_kernel_variants.py checks a `rocprofv3 --kernel-trace --stats` run against this table too."""

SL = "tests/test_gpu_span_loss.py::"


def _row(kernel, inst, entry, when, tests, align="no alignment requirement"):
    return {"kernel": kernel, "inst": inst, "entry": entry, "when": when, "tests": list(tests), "align": align}


VARIANTS = [
    # ------------------------------------------------------------------------------ spanloss/tspn_span_loss.hip
    _row("span_anchor_labels_kernel", None, "tspn_span_anchor_labels",
         "P > 0 (one wave per pair, 4 pairs per workgroup: idle waves when P % 4 != 0; a lane walks the pair's A*T anchors 64 "
         "apart: A*T of 60, 64, 68 around one stride, 480 for several; G of 0, 1..8 rows held in registers)",
         [SL + "test_labels_and_matches_equal_the_restatement", SL + "test_threshold_edges",
          SL + "test_sentinels_nothing_written_outside_the_outputs"], align="gt 8-byte aligned"),
    _row("span_loss_f32_kernel", None, "tspn_span_loss_f32",
         "P > 0 (one wave per pair, 4 pairs per workgroup; the same walk over the anchors; mask NULL or uint8 [P,A,T])",
         [SL + "test_losses_and_gradient_against_the_restatement", SL + "test_mask", SL + "test_nan_heads",
          SL + "test_two_launches_are_bit_equal"], align="gt and partials 8-byte aligned, heads and dheads 4-byte aligned"),
    _row("span_loss_finish_kernel", None, "tspn_span_loss_finish",
         "always (one workgroup of 256 threads: P of 1, 5, 257 = below, and one past, one pair per thread; P = 0 writes zeros)",
         [SL + "test_losses_and_gradient_against_the_restatement", SL + "test_refusals_and_the_empty_case"],
         align="partials and out 8-byte aligned"),
    _row("span_loss_scale_kernel", None, "tspn_span_loss_finish", "P > 0 (one thread per element of dheads, 256 per workgroup)",
         [SL + "test_losses_and_gradient_against_the_restatement", SL + "test_sentinels_nothing_written_outside_the_outputs"],
         align="dheads 4-byte aligned"),
]
