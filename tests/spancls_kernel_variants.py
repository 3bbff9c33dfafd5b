"""Which compiled kernel the span-pooled predicate training launches, the condition its launcher uses, the granularities
of each and the tests that reach it: the table of tests/kernel_variants.py, in the same format, for
temporal-span-proposal-network-vidvrd_amd/csrc/spancls/*.hip.

tests/test_span_cls_host.py keeps this table equal to the sources and its node ids pointing at tests that exist;
tools/check_kernel_variants.py checks a `rocprofv3 --kernel-trace --stats` run against this table too.

Granularities (tests/span_cls_reference.py names them in its docstring and holds TILE, WAVES, MAX_K, MAX_G): the label
kernel takes 256 rows (p, g) per workgroup and ceil(K / 64) mask words per row; the loss kernel one wave per row, four
rows per workgroup; the row count, the finish and the bias gradient 256 threads per workgroup; the projection gradient
one thread per (tracklet, column 2k + h), 256 per workgroup."""

SC = "tests/test_gpu_span_cls.py::"
LABELS, LOSS, FINISH, GRAD = ("tspn_span_labels_f32", "tspn_span_predicate_loss_f32", "tspn_span_predicate_loss_finish",
                              "tspn_span_predicate_grad_f32")
ENTRIES = (LABELS, LOSS, FINISH, GRAD)


def _row(kernel, inst, entry, when, tests, align="no alignment requirement"):
    return {"kernel": kernel, "inst": inst, "entry": entry, "when": when, "tests": list(tests), "align": align}


LOSS_TESTS = [SC + "test_loss_and_gradients_against_the_restatement", SC + "test_outputs_are_written_inside_only_and_reproducible",
              SC + "test_nan_reaches_exactly_the_rows_that_read_it"]

VARIANTS = [
    # -------------------------------------------------------------------------- spancls/tspn_span_cls.hip
    _row("span_labels_kernel", None, LABELS,
         "P > 0; one workgroup per 256 rows (p, g) of the concatenated pair table, one thread per row (segment by binary "
         "search in pair_off), ceil(K / 64) mask words per row; the store in 16-byte pieces where span_labels is 16-byte "
         "aligned, scalar stores otherwise",
         [SC + "test_span_labels_equal_the_restatement", SC + "test_span_labels_sentinels_and_unaligned_output"],
         align="span_labels, span_count, inst_cols 4-byte aligned (span_labels 16-byte aligned: vector stores), int64 operands 8-byte aligned"),
    _row("span_cls_rows_kernel", None, LOSS, "S > 0; one workgroup per segment, 256 threads over its pairs", LOSS_TESTS),
    _row("span_cls_loss_kernel", None, LOSS,
         "P > 0; one wave per row r = p G + g, four rows per workgroup, lane k, k + 64, .. over the predicates; rows that "
         "are none write zeros and read nothing", LOSS_TESTS,
         align="fp32 / int32 operands 4-byte aligned, int64 / float64 operands and prefix_scratch 8-byte aligned"),
    _row("span_cls_finish_kernel", None, FINISH, "always; one workgroup of 256 threads, the segments in order", LOSS_TESTS,
         align="partials, seg_rows, pair_off, out 8-byte aligned"),
    _row("span_cls_bias_grad_kernel", None, GRAD, "always; one thread per predicate, 256 per workgroup, the rows in order",
         LOSS_TESTS),
    _row("span_cls_proj_grad_kernel", None, GRAD,
         "NT > 0; one thread per (tracklet, column 2k + h), 256 per workgroup: the pair table in ascending order into a "
         "float64 difference array in prefix_scratch, then the running sum over t", LOSS_TESTS,
         align="prefix_scratch 8-byte aligned"),
]
