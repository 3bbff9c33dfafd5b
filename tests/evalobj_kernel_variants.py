"""Which compiled kernel the object detection evaluation launches, the condition its launcher uses, the granularities of
each and the tests that reach it: the table of tests/kernel_variants.py, in the same format, for
temporal-span-proposal-network-vidvrd_amd/csrc/evalobj/*.hip.

tests/test_evaluation_detection_host.py keeps this table equal to the sources and its node ids pointing at tests that
exist; tools/check_kernel_variants.py checks a `rocprofv3 --kernel-trace --stats` run against this table too.

Granularities: the tIoU kernel runs one wave per prediction, four to a workgroup (1 and 5 predictions: a partial last
workgroup), walks the ground truths of the prediction's group one after the other (groups of 0, 1, 3 and 70) and strides
its 64 lanes over the prediction's frames (0, 1, 63, 64, 65 and 129 frames); the claim kernels run one thread per ground
truth or per prediction, 256 to a workgroup (64, 65 and 200 predictions that claim inside one group, 1200 predictions in
the middle-size case)."""

EO = "tests/test_gpu_evaluation_objects.py::"
TIOU = "tspn_evalobj_tiou_f64"
CLAIM = "tspn_evalobj_claim"


def _row(kernel, inst, entry, when, tests, align="no alignment requirement"):
    return {"kernel": kernel, "inst": inst, "entry": entry, "when": when, "tests": list(tests), "align": align}


VARIANTS = [
    # -------------------------------------------------------------------------- evalobj/tspn_eval_objects.hip
    _row("evalobj_tiou_f64_kernel", None, TIOU,
         "n_pred > 0; one wave per prediction: every ground truth of its group in index order, the lanes over the "
         "prediction's frames, a binary search in the ground truth's frame ids, ballots for the four counters",
         [EO + "test_g13_objects_equal_the_reference", EO + "test_tiou_equals_the_restatement",
          EO + "test_exact_thresholds", EO + "test_argmax_and_match_rules", EO + "test_kernel_edge_sizes",
          EO + "test_flags_raise_zero_division", EO + "test_sentinels_and_null_tiou",
          EO + "test_middle_size_against_the_restatement"],
         align="boxes 32-byte aligned (one double4 per row); every other operand at its natural alignment"),
    _row("evalobj_claim_fill_kernel", None, CLAIM,
         "n_gt > 0 (n_pred == 0 included); one thread per ground truth: claim = INT32_MAX",
         [EO + "test_argmax_and_match_rules", EO + "test_kernel_edge_sizes", EO + "test_sentinels_and_null_tiou"],
         align="claim 4-byte aligned"),
    _row("evalobj_claim_min_kernel", None, CLAIM,
         "n_pred > 0 and n_gt > 0; one thread per prediction: a qualifying one does atomicMin(claim[its ground truth], "
         "its position inside its group)",
         [EO + "test_g13_objects_equal_the_reference", EO + "test_argmax_and_match_rules", EO + "test_kernel_edge_sizes",
          EO + "test_middle_size_against_the_restatement"],
         align="claim 4-byte aligned"),
    _row("evalobj_claim_hit_kernel", None, CLAIM,
         "n_pred > 0 (n_gt == 0 included: every hit 0); one thread per prediction: hit = qualifies and claim == position",
         [EO + "test_g13_objects_equal_the_reference", EO + "test_argmax_and_match_rules", EO + "test_kernel_edge_sizes",
          EO + "test_sentinels_and_null_tiou", EO + "test_middle_size_against_the_restatement"]),
]
