"""Which compiled kernel the span anchor sampler launches, the condition its launcher uses, the granularities of each and the
tests that reach it: the table of tests/kernel_variants.py, in the same format, for
temporal-span-proposal-network-vidvrd_amd/csrc/spansample/*.hip.

tests/test_span_sample_host.py keeps this table equal to the sources and its node ids pointing at tests that exist;
tools/check_kernel_variants.py checks a `rocprofv3 --kernel-trace --stats` run against this table too.

Granularities (tests/span_sample_reference.py holds them as CHUNK, OFFSET_THREADS, SIZES and KEY_BITS): a chunk is 4096
anchors = one workgroup of 256 threads x 16 anchors, so a wave holds 1024 of them; n of 1, 63, 64, 65 sit around 64 anchors
(four threads), 1023, 1025 around one wave's share, 4095, 4096, 4097 around one chunk, 3 * 4096 + 5 has several chunks and
a ragged last thread, 257 * 4096 + 3 has more chunks than the offsets kernel has threads (two chunks per thread).
key_bits of 1, 4, 8 give one round, 9 and 16 two, 17 three, 32 four."""

SS = "tests/test_gpu_span_sample.py::"
ENTRY = "tspn_span_anchor_sample"


def _row(kernel, inst, entry, when, tests, align="no alignment requirement"):
    return {"kernel": kernel, "inst": inst, "entry": entry, "when": when, "tests": list(tests), "align": align}


VARIANTS = [
    # -------------------------------------------------------------------------- spansample/tspn_span_sample.hip
    _row("span_sample_hist_kernel", None, ENTRY,
         "n > 0, once per round (ceil(key_bits / 8) rounds: 1 .. 4); one workgroup per chunk of 4096 anchors, 16 per thread; "
         "the 16-byte label load where label and mask are both 16-byte aligned and the thread's 16 anchors lie below n, "
         "byte loads otherwise",
         [SS + "test_mask_and_counts_equal_the_restatement", SS + "test_sentinels_and_unaligned_operands",
          SS + "test_full_size_with_the_threshold_on_a_32_bit_tie"], align="label at any address"),
    _row("span_sample_select_kernel", None, ENTRY,
         "always, once per round (one workgroup of 512 threads = one per class and bin, adding the chunks in order); round 0 "
         "writes counts; n == 0 launches this kernel alone",
         [SS + "test_mask_and_counts_equal_the_restatement", SS + "test_refusals_and_the_empty_case"],
         align="counts 8-byte aligned, partials 4-byte aligned"),
    _row("span_sample_offsets_kernel", None, ENTRY,
         "n > 0 (one workgroup of 256 threads, ceil(chunks / 256) consecutive chunks per thread: 1 up to 256 chunks, 2 at "
         "n = 257 * 4096 + 3)",
         [SS + "test_mask_and_counts_equal_the_restatement", SS + "test_stale_outputs_do_not_change_the_result"]),
    _row("span_sample_write_kernel", None, ENTRY,
         "n > 0 (one workgroup per chunk; the 16-byte mask store under the same condition as the label load, byte stores "
         "otherwise and for the ragged last thread)",
         [SS + "test_mask_and_counts_equal_the_restatement", SS + "test_sentinels_and_unaligned_operands",
          SS + "test_full_size_with_the_threshold_on_a_32_bit_tie"], align="mask at any address"),
]
