"""Which compiled kernel variant the span relation decode's C-ABI entry point launches, the condition its launcher uses
to pick it, and the tests that reach it: the table of tests/kernel_variants.py, in the same format, for
temporal-span-proposal-network-vidvrd_amd/csrc/relations/*.hip.

tests/test_span_relations_host.py keeps this table equal to the sources and its node ids pointing at tests that exist;
tools/check_kernel_variants.py checks a `rocprofv3 --kernel-trace --stats` run against this table too."""

SR = "tests/test_gpu_span_relations.py::"


def _row(kernel, inst, entry, when, tests, align="no alignment requirement"):
    return {"kernel": kernel, "inst": inst, "entry": entry, "when": when, "tests": list(tests), "align": align}


VARIANTS = [
    # ------------------------------------------------------------------------------ relations/tspn_span_relations.hip
    _row("span_row_topk_kernel", None, "tspn_decode_span_relations_f32", "S > 0 && P > 0 (one wave per (pair, span) row)",
         [SR + "test_fused_equals_the_composition", SR + "test_ragged_counts_and_fewer_candidates_than_topk",
          SR + "test_nonfinite_frames_rank_first_and_stay_in_their_spans"]),
    _row("segment_span_topk_kernel", None, "tspn_decode_span_relations_f32", "S > 0 && P > 0 (one workgroup per segment)",
         [SR + "test_fused_equals_the_composition", SR + "test_duplicated_tracklets_tie_by_flat_index",
          SR + "test_ragged_counts_and_fewer_candidates_than_topk"]),
]
