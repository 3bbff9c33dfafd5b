"""The scratch contract of every workspace-taking entry of include/tspn_mi355x.h (its Conventions block): a workspace
may hold anything on entry, its contents are unspecified on return, `need` = what the size helper returns suffices,
nothing outside those bytes is touched, and a shorter one is refused with TSPN_EWORKSPACE before any device work.

One row per entry.  Fields:
  entry    the C-ABI function that takes the workspace
  desc     None for a `void* workspace` parameter, else the descriptor struct whose `workspace` member it reads
  helper   its `*_workspace_bytes` export
  wrapper  the ops.py function the tests drive it through (all of them allocate through ops._ws when not handed one)
  holds    the pieces of the layout, in order
  zeroed   which bytes somebody clears before a kernel reads them, and who: the library's own memsets are listed here;
           "nothing" = every byte a kernel reads was written by a kernel of the same call
  tests    pytest node ids that hold the entry to the contract

CALLER_ZEROED lists the two scratch arguments that are documented as zeroed BY THE CALLER; they take no part in the
"any contents" tests and are checked for writes outside their bytes only.  OTHER_SCRATCH lists scratch that keeps the
workspace contract under another parameter name and size helper (the split buffer of the split-fp16 pair stage).

tests/test_workspace_contract_table.py keeps the table equal to the header and pins, without a device, that helper and
entry agree; tests/test_gpu_workspace_contract.py is the GPU side."""

WC = "tests/test_gpu_workspace_contract.py::"
SHORT = WC + "test_a_short_or_null_workspace_is_refused_untouched"
MODEL = WC + "test_model_workspace_reused_across_videos"


def _row(entry, helper, wrapper, holds, zeroed, tests, desc=None):
    return {"entry": entry, "desc": desc, "helper": helper, "wrapper": wrapper, "holds": holds, "zeroed": zeroed,
            "tests": list(tests)}


ROWS = [
    _row("tspn_predicate_head_f32", "tspn_predicate_head_workspace_bytes", "ops.predicate_head",
         "split-K partial slabs fp32 [splits][P][K]",
         "nothing: the split-K kernel writes every (row < P, column < K) of every slab, a slice past F writes zeros",
         [WC + "test_predicate_head", SHORT]),
    _row("tspn_predicate_head_norm_f32", "tspn_predicate_head_norm_workspace_bytes", "ops.predicate_head(norm=...)",
         "partial slabs fp32 [n][P][K], then the slices' row sums of |x| fp32 [n][P]",
         "nothing: the column-tile-0 workgroups write every row sum, every workgroup its slab tile",
         [WC + "test_predicate_head_norm", SHORT]),
    _row("tspn_conv3_tc_wino63_f32", "tspn_conv3_tc_wino63_workspace_bytes", "ops.conv3_tc_wino63",
         "the transformed input V fp32 [Cin/4][8 points][sextets padded to 64][4]",
         "nothing: the input transform writes the padded sextet columns and the frames past T of a last sextet as zeros",
         [WC + "test_conv3_wino63", SHORT]),
    _row("tspn_conv3_tc_wino63_f16x3", "tspn_conv3_tc_wino63_f16x3_workspace_bytes", "ops.conv3_tc_wino63_f16x3",
         "split input fp16 hi | lo [8 points][2 Cin][sextets padded to 256], column exponents int32 [8][sextets], the "
         "contraction's parking area (one slot per 256 x 256 tile)",
         "nothing: the transform writes the padded columns; a lane reads back from the parking area what it parked there itself",
         [WC + "test_conv3_wino63_f16x3", SHORT]),
    _row("tspn_decode_topk_f32", "tspn_decode_topk_workspace_bytes", "ops.decode_topk",
         "per-pair candidates: scores fp32 [S][P][R], then predicate ids int32 [S][P][R]",
         "nothing: one wave per pair row writes its R slots",
         [WC + "test_decode_topk", SHORT]),
    _row("tspn_forward_fused_f32", "tspn_forward_fused_workspace_bytes", "ops.forward_fused",
         "xt (transposed feats, D % 16 != 0 only), y [NT][2C][ldy] (ldy = ceil4(T) on the blocked pair stage), bias2 [2C], "
         "fbar [NT][D], pooled (unused), the predicate head's slabs + rs / ro [NT][K], V of the F(6,3) forms, hwp [C][12], "
         "psplit (the split buffer of tspn_heads_pairgrid_f16x3: flag word, inverse scales, split head weights; only "
         "behind the split-fp16 conv with 3A = 12), hot (the accuracy guard's scratch)",
         "library: hipMemsetAsync of bias2[C, 2C) (tspn_fused.hip; the object half carries no bias) and, with conv_check "
         "> 0 on an F(6,3) form, of the TSPN_CONV_CHECK_SCRATCH_BYTES of `hot`.  The pad frames [T, ldy) of y reach no "
         "output, whatever they hold",
         [WC + "test_forward_fused", WC + "test_forward_fused_accuracy_guard_scratch", SHORT, MODEL],
         desc="tspn_fused_desc"),
    _row("tspn_forward_fused_bf16", "tspn_forward_fused_bf16_workspace_bytes", "ops.forward_fused_bf16",
         "bias2 [2C], y fp32 [NT*T][2C], fbar [NT][D], the predicate head's slabs + rs / ro",
         "library: hipMemsetAsync of bias2[C, 2C) (tspn_bf16.hip)",
         [WC + "test_forward_fused_bf16", SHORT, MODEL], desc="tspn_fused_bf16_desc"),
    _row("tspn_forward_fused_bf16_pairs", "tspn_forward_fused_bf16_pairs_workspace_bytes",
         "ops.forward_fused_bf16(canonical_pairs=False)",
         "the layout of tspn_forward_fused_bf16, then the plan of tspn_heads_pairlist_bf16",
         "library: bias2[C, 2C) as above and the plan's `head` array (below)",
         [WC + "test_forward_fused_bf16", SHORT, MODEL], desc="tspn_fused_bf16_desc"),
    _row("tspn_heads_pairlist_bf16", "tspn_heads_pairlist_bf16_workspace_bytes", "ops.heads_pairlist_bf16",
         "the plan: s_list, o_list int32 [B][Np], counts [B][2], head [B][Np][Np], next [P], rank_ws [B][2][N]; Np = N "
         "rounded up to 16",
         "library: hipMemsetAsync(head, 0xff) in tspn_pair_plan_i32 (pairlist/tspn_pairlist_bf16.hip): every chain "
         "empty; the list slots past the counts are written as 0 by the lists kernel, next[p] by the link kernel",
         [WC + "test_heads_pairlist_bf16", SHORT]),
    _row("tspn_span_predicate_f32", "tspn_span_predicate_workspace_bytes", "ops.span_predicate",
         "the GEMM's slabs, G fp32 [NT*T][2K], the float64 prefix sums [NT][T+1][2K]",
         "nothing: the prefix kernel writes row 0 of every prefix column itself",
         [WC + "test_span_predicate", SHORT]),
    _row("tspn_decode_span_relations_f32", "tspn_decode_span_relations_workspace_bytes", "ops.decode_span_relations",
         "the layout of tspn_span_predicate_f32 (256-byte aligned), then keys / products / predicate ids [S][P*J*R] each",
         "nothing: a row j >= count[p] writes the pad key into its R slots",
         [WC + "test_decode_span_relations", SHORT]),
    _row("tspn_span_predicate_bf16", "tspn_span_predicate_bf16_workspace_bytes", "ops.span_predicate_bf16",
         "float64 prefix sums [NT][T+1][D], the pooled rows bf16 [P][2D]",
         "nothing",
         [WC + "test_span_predicate_bf16", SHORT]),
    _row("tspn_decode_span_relations_bf16", "tspn_decode_span_relations_bf16_workspace_bytes",
         "ops.decode_span_relations_bf16",
         "the layout of tspn_span_predicate_bf16 over the S*P*J rows, q fp32 [S*P*J][K], keys / products / ids [S][P*J*R]",
         "nothing: a row j >= count[p] writes the pad key into its R slots",
         [WC + "test_decode_span_relations_bf16", SHORT]),
    _row("tspn_stem_conv_bf16", "tspn_stem_bf16_workspace_bytes", "ops.stem_conv_bf16",
         "the 2x2 space-to-depth image bf16 [NB][OH+3][OW+3][16]",
         "nothing: the space-to-depth kernel writes every pixel, the padded border and the odd last row / column as zeros",
         [WC + "test_stem_bf16", SHORT]),
    _row("tspn_stem_pool_bf16", "tspn_stem_bf16_workspace_bytes", "ops.stem_pool_bf16",
         "as tspn_stem_conv_bf16", "nothing", [WC + "test_stem_bf16", SHORT]),
]

# scratch that the header documents as zeroed by the caller: (entry, parameter, what the caller zeroes, tests)
CALLER_ZEROED = [
    ("tspn_eval_greedy_match_f64", "det_ws", "one byte per relation, all zero (read above 4096 ground truths of a group)",
     [WC + "test_caller_zeroed_scratch_is_not_overrun"]),
    ("tspn_conv3_spot_check_f32", "scratch", "TSPN_CONV_CHECK_SCRATCH_BYTES, all zero before the conv it belongs to",
     [WC + "test_caller_zeroed_scratch_is_not_overrun"]),
]

# scratch under the same contract as a workspace ("every byte of which the call writes before it reads it", a short one
# refused) that is not a `void* workspace` with a `*_workspace_bytes` helper: (entry, parameter, size helper, tests)
OTHER_SCRATCH = [
    ("tspn_heads_pairgrid_f16x3", "split_buf", "tspn_heads_pairgrid_f16x3_split_bytes",
     [WC + "test_heads_pairgrid_f16x3_split_buf", WC + "test_heads_pairgrid_f16x3_refuses_a_short_null_or_misaligned_split_buf",
      WC + "test_heads_pairgrid_f16x3_split_buf_carries_no_state"]),
]
