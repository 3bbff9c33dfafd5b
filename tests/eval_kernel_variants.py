"""Which compiled kernel variant each evaluation C-ABI entry point can launch, the condition its launcher uses to pick
it, and the tests that reach it: the table of tests/kernel_variants.py, in the same format, for
temporal-span-proposal-network-vidvrd_amd/csrc/eval/*.hip.

tests/test_evaluation_host.py keeps this table equal to the sources and its node ids pointing at tests that exist;
tools/check_kernel_variants.py checks a `rocprofv3 --kernel-trace --stats` run against this table and
tests/kernel_variants.py."""

EV = "tests/test_gpu_evaluation.py::"


def _row(kernel, inst, entry, when, tests, align="no alignment requirement"):
    return {"kernel": kernel, "inst": inst, "entry": entry, "when": when, "tests": list(tests), "align": align}


VARIANTS = [
    # ------------------------------------------------------------------------------ eval/tspn_eval.hip
    _row("eval_traj_volume_f64_kernel", None, "tspn_eval_traj_volume_f64", "n_traj > 0",
         [EV + "test_viou_bit_equal_to_the_python_restatement", EV + "test_g12_aggregates_and_hits_equal_the_reference"],
         "boxes 32-byte aligned (double4 rows): refused with TSPN_EINVAL"),
    _row("eval_viou_f64_kernel", None, "tspn_eval_viou_f64", "n_pred > 0",
         [EV + "test_viou_bit_equal_to_the_python_restatement", EV + "test_zero_denominator_raises",
          EV + "test_g12_aggregates_and_hits_equal_the_reference"],
         "boxes 32-byte aligned (double4 rows): refused with TSPN_EINVAL"),
    _row("eval_greedy_match_kernel", "true", "tspn_eval_greedy_match_f64", "n_groups > 0 (serves groups of <= 4096 ground truths)",
         [EV + "test_greedy_ties_and_large_groups", EV + "test_g12_aggregates_and_hits_equal_the_reference"]),
    _row("eval_greedy_match_kernel", "false", "tspn_eval_greedy_match_f64",
         "max_group_gt > kRegMaskMaxGt (4096; serves those groups, detected flags in det_ws)",
         [EV + "test_greedy_ties_and_large_groups"]),
]
