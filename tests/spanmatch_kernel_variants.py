"""Which compiled kernel the span-bounded association match launches, the condition its launcher uses, the granularities
of each and the tests that reach it: the table of tests/kernel_variants.py, in the same format, for
temporal-span-proposal-network-vidvrd_amd/csrc/spanmatch/*.hip.

tests/test_span_match_host.py keeps this table equal to the sources and its node ids pointing at tests that exist;
tools/check_kernel_variants.py checks a `rocprofv3 --kernel-trace --stats` run against this table too.

Granularities: a workgroup is 256 threads = 256 (relation, prediction) pairs of the U x P matrix ((U, P) of (1, 1),
(19, 14) = 266 pairs, (300, 260)); the float64 areas are summed in blocks of eight up to 128 frames and in split halves
above (windows of 1, 7, 8, 9, 127, 128, 129 frames that start off the multiples of 8); the greedy pass is one workgroup
that walks U in chunks of 256 relations (U of 0, 1, 19, 300) with one taken flag per relation in LDS (U <= 65536)."""

SM = "tests/test_gpu_span_match.py::"
ENTRY = "tspn_span_match_f64"


def _row(kernel, inst, entry, when, tests, align="no alignment requirement"):
    return {"kernel": kernel, "inst": inst, "entry": entry, "when": when, "tests": list(tests), "align": align}


VARIANTS = [
    # -------------------------------------------------------------------------- spanmatch/tspn_span_match.hip
    _row("span_match_iou_kernel", None, ENTRY,
         "U > 0 and P > 0; one thread per (relation, prediction) pair, 256 per workgroup: the gate tests, then for a "
         "candidate pair the two window IoUs; -1 for every other pair",
         [SM + "test_outputs_equal_the_restatement_to_the_bit", SM + "test_gate_edges_one_per_condition",
          SM + "test_sentinels_and_stale_outputs", SM + "test_device_spans_association_equals_the_host_path"],
         align="float64 and int64 operands 8-byte aligned, int32 and float32 ones 4-byte aligned (their natural alignment)"),
    _row("span_match_greedy_kernel", None, ENTRY,
         "P > 0 (U == 0 included: every match -1); one workgroup of 256 threads, sequential over the predictions, U in "
         "chunks of 256 relations, the first free relation whose two IoUs reach the threshold",
         [SM + "test_outputs_equal_the_restatement_to_the_bit", SM + "test_greedy_contention",
          SM + "test_no_relations_and_no_predictions", SM + "test_sentinels_and_stale_outputs"],
         align="iou and match 4-byte aligned"),
]
