/*
 * tspn_mi355x.h — C ABI of the MI355X-native TSPN relation-scoring hot path.
 *
 * The reference (sangminwoo/Temporal-Span-Proposal-Network-VidVRD) is pure
 * Python and has no FFI / operator layer: the seam it offers is the
 * `BaseModel.forward()` nn.Module API (lib/modeling/model.py:20-24).  This
 * header is the native boundary *under* that API: each entry point replaces the
 * torch-op sequence cited next to it.  The Python host
 * (temporal-span-proposal-network-vidvrd_amd/_abi.py) binds these symbols with
 * ctypes; INTEGRATION.md shows the reference-side stub.
 *
 * Conventions
 *   - All pointers are raw DEVICE pointers (HBM) owned by the caller (torch's
 *     allocator); the library borrows them for the duration of the call and
 *     allocates nothing.  Scratch space is passed in explicitly (see the
 *     *_workspace_bytes helpers).
 *   - The workspace contract, for every entry that takes a `workspace` (as a parameter or as a member of its
 *     descriptor): a workspace may hold ANYTHING on entry -- the library clears what it needs cleared -- and its
 *     contents are unspecified on return; the `need` bytes its *_workspace_bytes helper returns for the same shape
 *     suffice, and nothing outside them is touched; a shorter workspace (or none, where need > 0) is refused with
 *     TSPN_EWORKSPACE (a null one possibly with TSPN_EINVAL) before any device work, outputs and workspace untouched.
 *     A helper returns 0 where its own arguments already say that the entry refuses the shape or has nothing to do
 *     (tests/test_workspace_contract_table.py pins which).  One buffer may therefore serve
 *     calls of different entries and shapes one after the other on a stream.  The two scratch arguments that are NOT
 *     a workspace in this sense say so where they are declared: `det_ws` of tspn_eval_greedy_match_f64 and `scratch`
 *     of the stand-alone tspn_conv3_spot_check_f32 are zeroed by the caller.  (tests/workspace_contracts.py has the
 *     layouts; tests/test_gpu_workspace_contract.py holds every entry to this.)
 *   - All tensors are dense, row-major, fp32 unless stated; sizes are int64.
 *   - `stream` is a hipStream_t passed as void* (torch's current stream).  The
 *     functions enqueue work and return; they never synchronise, never touch
 *     the null stream implicitly, and are re-entrant.
 *   - Return value: 0 on success, negative TSPN_E* on failure;
 *     tspn_last_error() returns a thread-local message.  No C++ exception
 *     crosses this boundary.
 *   - Target: gfx950 only.
 */
#ifndef TSPN_MI355X_H
#define TSPN_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever a struct layout or a signature changes (2: tspn_fused_desc gained conv_algo /
 * canonical_pairs in round 1 without a bump; round 2 adds the struct-size exports below, which the
 * host checks against its own view of the descriptors at load time; 3: tspn_fused_desc.ev_logits_ready;
 * 4 (round 3): the Winograd F(2,3) and the three F(4,3) temporal-conv generations and their pack / repack
 * entry points are gone, tspn_fused_desc.conv_algo is TSPN_CONV_DIRECT | TSPN_CONV_WINOGRAD63;
 * 5 (round 3): tspn_pack_conv2d_frag_bf16 lays the fragments out channel chunk by chunk (was tap by tap) and
 * the bf16 convolutions contract in that order; tspn_stem_pool_bf16 added);
 * 6 (round 5, additive): tspn_bottleneck_block_bf16, tspn_bottleneck_block_proj_bf16, tspn_bottleneck_block_res_bf16,
 * tspn_bottleneck_tail_io_bf16, tspn_conv3_tc_wino63_set_piece_form (replaces the TSPN_WINO63_PTRV environment switch);
 * 7 (round 6): the device status block (tspn_status_attach / _fault / _clear / _selftest, TSPN_EDEVICE: a kernel can
 * raise a fault that the NEXT launch entry reports without a synchronisation); tspn_fused_desc gained conv_weight /
 * conv_check at its END (the a-posteriori accuracy guard of the F(6,3) temporal conv, tspn_conv3_spot_check_f32).
 * Still 7 (additive, no layout or signature changed): tspn_pair_plan_i32, tspn_heads_pairlist_bf16 (+ _workspace_bytes),
 * tspn_forward_fused_bf16_pairs (+ _workspace_bytes): the bf16 path on an arbitrary pair table;
 * tspn_pack_span_cls_bf16, tspn_span_predicate_bf16, tspn_decode_span_relations_bf16 (+ _workspace_bytes): span pooling and
 * the relations with their spans on bf16 segments;
 * tspn_heads_pairgrid_f16x3 (+ _split_bytes, _set_force_exact): the fp32 path's pair stage on split-fp16 MFMAs. */
#define TSPN_ABI_VERSION 7

enum {
  TSPN_OK = 0,
  TSPN_EINVAL = -1,       /* bad argument (null pointer, negative size, misalignment) */
  TSPN_EUNSUPPORTED = -2, /* shape outside what the kernels implement */
  TSPN_EWORKSPACE = -3,   /* workspace too small */
  TSPN_ELAUNCH = -4,      /* HIP runtime error at launch */
  TSPN_EDEVICE = -5       /* a kernel of an EARLIER launch raised a fault through the device status block (below) */
};

/* ---- device status block (round 6) ----------------------------------------
 * The reference reports failures as Python exceptions only; a kernel has no such channel, and a
 * synchronisation after every launch to ask it would serialise the host.  Instead the caller allocates
 * TSPN_STATUS_WORDS int32 words of PINNED, DEVICE-MAPPED HOST memory (hipHostMalloc / torch .pin_memory(); zeroed,
 * 64-byte aligned) and attaches them once per device; kernels write them with system-scope atomics, the host reads
 * them with plain loads.  While word TSPN_STATUS_FAULT is non-zero every launch entry of the library on that device
 * returns TSPN_EDEVICE (checked where the HIP launch error is checked: the call that LAUNCHED the faulting kernel
 * returns TSPN_OK, the next one fails) until tspn_status_clear().  Without an attached block a kernel that has to
 * raise traps instead (the launch fails with a HIP error at the next synchronisation).  Attachment is per device
 * (the CURRENT device of the calling thread) and process-wide; the library never frees the block.            */
#define TSPN_STATUS_WORDS 16
enum {
  TSPN_STATUS_FAULT = 0,       /* OR of TSPN_FAULT_* bits; 0 = healthy */
  TSPN_STATUS_FAULT_INFO = 1,  /* raiser's detail (workgroup id of the last raiser) */
  TSPN_STATUS_CONV_ERR = 2,    /* float bits: largest |y - reference| any tspn_conv3_spot_check_f32 has measured since the
                                  host last zeroed the word (not a fault: the host policy decides) */
  TSPN_STATUS_CONV_CHECKS = 3  /* number of outputs spot-checked since the host last zeroed the word */
};
enum {
  TSPN_FAULT_HANDOVER = 1      /* an LDS hand-over between the waves of a workgroup timed out (tspn_bottleneck_tail_io_bf16,
                                  tspn_bottleneck_tail_pipe_bf16): the waiting wave raised and ENDED without touching the
                                  data it did not receive; the launch's output is incomplete */
};
int tspn_status_attach(int32_t* host_words);   /* NULL detaches */
int tspn_status_fault(void);                    /* the fault word of the current device's block (0 if none attached) */
int tspn_status_clear(void);                    /* zero fault + info (the caller has dealt with it) */
/* Raises TSPN_FAULT_HANDOVER on purpose: one wave waits, with a short bound, for an LDS counter that nobody sets --
 * through the same device code as the role-split res4 tail.  `reached_end` (device int32, optional) stays 0: the wave
 * ends inside the wait.  Tests of the channel: the call itself returns TSPN_OK, the next launch entry TSPN_EDEVICE. */
int tspn_status_selftest(int32_t* reached_end, void* stream);

#define TSPN_GEOM_CHANNELS 8

/* tspn_fused_desc.conv_algo: which temporal-conv kernel consumes `conv_packed` (the packing IS the choice) */
enum {
  TSPN_CONV_DIRECT = 0,      /* conv_packed = tspn_pack_conv3_f32(conv.weight, C, C, split = D): [3][D][2C]; any shape */
  TSPN_CONV_WINOGRAD63 = 1,  /* conv_packed = tspn_pack_conv3_wino63_frag_f32(conv.weight, C, C, split = D); D % 32 == 0 */
  TSPN_CONV_WINOGRAD63_F16X3 = 2   /* conv_packed = tspn_pack_conv3_wino63_f16x3(conv.weight, C, C, split = D) (int16
                                      storage); D % 64 == 0; the same F(6,3) on split-fp16 MFMAs */
};

int tspn_version(void);
/* sizeof(tspn_fused_desc) / sizeof(tspn_fused_bf16_desc) as this library was compiled: a host whose
 * view of the descriptors differs (stale .so, stale binding) must refuse to call the library.      */
size_t tspn_fused_desc_size(void);
size_t tspn_fused_bf16_desc_size(void);
const char* tspn_last_error(void);
const char* tspn_error_string(int code);

/* ---- a2: predicate head -------------------------------------------------
 * Replaces RelationPredictor.forward (lib/modeling/model.py:85-88):
 *   out[P,K] = sigmoid(x[P,F] @ W[K,F]^T + b[K])       (apply_sigmoid != 0)
 * `ldx` = row stride of x in elements (>= F).  W is the nn.Linear weight as
 * stored in the state_dict (classifier.rel_predictor.weight), no packing.
 * Split-K partial slabs live in `workspace`
 * (tspn_predicate_head_workspace_bytes).                                     */
size_t tspn_predicate_head_workspace_bytes(int64_t P, int64_t F, int64_t K);
int tspn_predicate_head_f32(const float* x, int64_t P, int64_t F, int64_t ldx,
                            const float* W, const float* b, int64_t K,
                            float* out, int apply_sigmoid,
                            void* workspace, size_t workspace_bytes, void* stream);

/* f2 — a15 folded into a2: same as tspn_predicate_head_f32 on RAW features, with the block-L1
 * normalisation of VRDataset._feature_preprocess (lib/dataset/vrdataset.py:219-243) applied on the
 * fly: columns [first + k*block, first + (k+1)*block), k < nblocks, of every row are divided by their
 * L1 norm (0 -> 1).  Split-K slices never straddle a block, each returns sum|x| per row, and the
 * ordered reduce divides — x is read once and never rewritten.                                    */
size_t tspn_predicate_head_norm_workspace_bytes(int64_t P, int64_t F, int64_t K, int64_t first,
                                                int64_t block, int64_t nblocks);
int tspn_predicate_head_norm_f32(const float* x, int64_t P, int64_t F, int64_t ldx,
                                 const float* W, const float* b, int64_t K,
                                 int64_t first, int64_t block, int64_t nblocks,
                                 float* out, int apply_sigmoid,
                                 void* workspace, size_t workspace_bytes, void* stream);

/* ---- a15: block-L1 feature preprocessing --------------------------------
 * Replaces VRDataset._feature_preprocess (lib/dataset/vrdataset.py:219-243,
 * lib/utils/miscellaneous.py:32-35), in place on feats[P, ld>=F].           */
int tspn_feature_preprocess_f32(float* feats, int64_t P, int64_t F, int64_t ld,
                                int64_t first, int64_t block, int64_t nblocks,
                                void* stream);

/* ---- a15: proposal pair filter ------------------------------------------
 * Replaces VRDataset._get_proposal_idx + _get_num_tracklet_proposals
 * (lib/dataset/vrdataset.py:140-148) for S segments stored back to back:
 *   segment s owns pair rows [pair_off[s], pair_off[s+1]) of `pairs` [sum P_s, 2] (track indices LOCAL
 *   to the segment, as in the `pairs` dataset of its -relation.h5 file) and tracks
 *   [track_off[s], track_off[s+1]) of `trackid` (-1 = proposal, >= 0 = ground-truth track).
 *   out_idx[pair_off[s] + r], r < out_count[s]: local indices of the kept pairs (both tracks are
 *       proposals), ascending = the order of the reference's list comprehension;
 *   out_count[s]      number kept, or -1 if a pair of the segment names a track outside it
 *                     (the reference raises IndexError there);
 *   out_num_tracks[s] = sum(trackid < 0).
 * All pointers are device pointers; one workgroup per segment, order-preserving compaction.        */
int tspn_proposal_pair_filter_i64(const int64_t* pairs, const int64_t* pair_off,
                                  const int64_t* trackid, const int64_t* track_off, int64_t S,
                                  int64_t* out_idx, int64_t* out_count, int64_t* out_num_tracks,
                                  void* stream);
/* out[r, 0:F] = src[idx_base + idx[r], 0:F] (src row stride ld): feats[proposal_idx] of
 * vrdataset.py:66-67.                                                                              */
int tspn_gather_rows_f32(const float* src, int64_t ld, int64_t F, const int64_t* idx,
                         int64_t idx_base, int64_t R, float* out, void* stream);

/* ---- a5/a6: PPN pair matrix + top-k pair indices ------------------------
 * Replaces PPNHead.forward + the sort in PPN._forward_test
 * (lib/modeling/relpn/ppn.py:107-112, 84-85) for a batch of `B` segments with
 * N tracklets each:
 *   mat[b] = sigmoid(MLP_s(cls[b]) @ MLP_o(cls[b])^T)        [B,N,N]
 *   idx[b] = first `topk` flat indices (s*N+o) of mat[b] in descending order,
 *            ties broken lower-index-first                   [B,topk] int64
 * MLP = Linear(Cin,H)+ReLU+Linear(H,Cout); weights as in the state_dict
 * (sub_emb.0.weight [H,Cin], sub_emb.2.weight [Cout,H], ...).
 * Limits: N <= 128, Cin,H,Cout <= 256, topk <= N*N, and one workgroup's LDS:
 * 4*N*(Cin+H+2*Cout) + 8*n2p bytes <= 160 KiB, n2p = N*N rounded up to a power
 * of two.  At the model's widths (Cin 35, H 64, Cout 35) that is N <= 90
 * (126 376 B); N = 91 ... 128 (n2p = 16 384) need 192 588 B and more and are
 * refused with TSPN_EUNSUPPORTED.  N = 128 fits only with narrow embeddings,
 * e.g. H = Cout = 8 (161 280 B).                                            */
int tspn_ppn_pair_matrix_topk_f32(const float* cls, int64_t B, int64_t N, int64_t Cin,
                                  int64_t H, int64_t Cout,
                                  const float* ws1, const float* bs1,
                                  const float* ws2, const float* bs2,
                                  const float* wo1, const float* bo1,
                                  const float* wo2, const float* bo2,
                                  int64_t topk, float* out_mat, int64_t* out_idx,
                                  void* stream);

/* ---- a16: trajectory (cubic) IoU ----------------------------------------
 * Replaces cubic_iou/_intersect/_union (lib/modeling/trajectory.py:85-141):
 *   out[B,N1,N2] float32, boxes [B,N,T,4] (l,t,r,b), +1 pixel-inclusive,
 *   intersection accumulated over t in fp32 in frame order.
 * boxes2 == NULL means boxes2 = boxes1 (N2 = N1), whatever N2 says: a caller
 * with an empty second operand (N2 = 0) has nothing to compute and must not
 * call with its null data pointer.                                          */
int tspn_traj_iou_f32(const float* boxes1, int64_t N1, const float* boxes2, int64_t N2,
                      int64_t B, int64_t T, float* out, void* stream);

/* ---- f3: association-time trajectory IoU, batched ------------------------
 * Replaces the per-candidate `_traj_iou(r.straj, straj)` / `_traj_iou(r.otraj, otraj)` calls of
 * lib/modeling/association.py:35-48,101-106 (-> trajectory.py:144-158 traj_iou -> cubic_iou on float64
 * boxes) by one launch per segment: a [U,L,4] = every distinct trajectory the previous segment's relations
 * hold, from the current segment's first frame on; len_a[U] int32 = how many of those frames each has (its
 * common frames with the segment's tracklets; 0 = no overlap -> IoU 0, association.py:36-37; the caller
 * guarantees len_a[u] <= L); b [N,L,4] = the current segment's tracklets; out [U,N] float32.  Rounding
 * recipe of the reference chain kept to the bit: coordinates max/min stored as float32, intersection in
 * float32 in frame order, areas float64 in numpy's pairwise summation order, quotient in float64 stored as
 * float32.  The length check is the caller's: this function reads len_a[u] frames of both rows.  L < 2^31.  */
int tspn_traj_iou_tail_f64(const double* a, const int32_t* len_a, const double* b, int64_t U, int64_t N,
                           int64_t L, float* out, void* stream);

/* ---- pair order ---------------------------------------------------------
 * All ordered pairs (i,j), i != j, i-major (lib/modeling/predict.py:133-140):
 * pairs[N*(N-1), 2] int64, tracklet ids offset by `base`.                   */
int tspn_pair_index_i64(int64_t N, int64_t base, int64_t* pairs, void* stream);

/* ---- N^2 pair builder (materialising form) ------------------------------
 * Builds what DPNHead consumes (rel_feats "NxCxT", lib/modeling/relpn/dpn_anchor.py:38):
 *   out_feat[P, 2D, T] = cat(feats[pairs[p,0]]^T, feats[pairs[p,1]]^T)
 *   out_geom[P, 8, T]  = relative box geometry (may be NULL)
 * feats [NT, T, D], boxes [NT, T, 4] (may be NULL iff out_geom is NULL),
 * pairs int64 [P,2] with ids in [0, NT).  out_feat may be NULL.             */
int tspn_pair_gather_f32(const float* feats, const float* boxes, int64_t NT, int64_t T,
                         int64_t D, const int64_t* pairs, int64_t P,
                         float* out_feat, float* out_geom, void* stream);

/* ---- weight packing for the k=3 temporal conv ---------------------------
 * packed[3][Cin][M] <- W[M][Cin][3] (nn.Conv1d weight layout).  `packed` has
 * M*Cin*3 floats.  With split > 0 the input channels are split at `split`
 * and the two halves stacked along M (factorised pair form):
 *   packed[3][split][2M]: rows [0,M) = W[:, :split, :], rows [M,2M) = W[:, split:, :]
 * (requires Cin == 2*split).                                                */
int tspn_pack_conv3_f32(const float* W, int64_t M, int64_t Cin, int64_t split,
                        float* packed, void* stream);

/* ---- a8: temporal context encoder (k=3 conv as implicit GEMM on MFMA) ----
 * Replaces self.conv + F.relu of DPNHead.forward (lib/modeling/relpn/dpn.py:70):
 *   y[B, M, T] = act(bias[M] + sum_{tap,ci} packed[tap][ci][m] * x[B, ci, t+tap-1])
 * zero padding outside [0,T).  bias may be NULL; relu != 0 applies ReLU.
 *
 * Numerical contract of the fp32 scorer entries (this one, tspn_conv3_tc_f32, tspn_heads_f32, tspn_heads_pairgrid_f32,
 * tspn_predicate_head_f32, tspn_predicate_head_norm_f32, tspn_temporal_mean_f32, tspn_temporal_sum_f32 and the passes built
 * from them), tests/fp32_reference.py, DESIGN.md §3: with u = 2^-24 and S = |bias| + sum |w| |x|,
 *   |out - exact| <= (2 (k + Kd / k + extra) + 1) u S
 * for a contraction of depth Kd on an MFMA of k products per step (conv: k = 2, Kd = 3 Cin, extra = 2; heads and pair grid:
 * k = 4, Kd = C, extra = 2; split-K GEMM: k = 4, Kd = the slice length, extra = splits + 2), and where every product and every
 * partial sum is exactly representable the output is the exact sum, bit for bit, whatever the summation order.
 * fp32 SUBNORMAL operands are KEPT: v_mfma_f32_32x32x2_f32, v_mfma_f32_16x16x4_f32 and the fp32 adds in front of them read
 * and produce subnormals (measured on gfx950: subnormal activations against weights near 2^100 stay within 0.14 of that
 * budget, where reading them as zero would miss it by a factor of 10^3 to 10^5), so the contract has no absolute floor.
 * The sign of a zero output is not part of the contract.                   */
int tspn_conv3_f32(const float* x, int64_t B, int64_t Cin, int64_t T,
                   const float* packed, int64_t M, const float* bias, int relu,
                   float* y, void* stream);

/* Same operator on channels-LAST input x[B, T, Cin] (the tracklet layout [N,T,D] itself), output
 * still y[B, M, T].  Fast path only: needs Cin % 16 == 0, M % 4 == 0, 16-byte aligned x / packed
 * (otherwise TSPN_EUNSUPPORTED: transpose with tspn_transpose_td_f32 and call tspn_conv3_f32).   */
int tspn_conv3_tc_f32(const float* x, int64_t B, int64_t T, int64_t Cin,
                      const float* packed, int64_t M, const float* bias, int relu,
                      float* y, void* stream);

/* Winograd F(6,3) form of tspn_conv3_tc_f32 (tspn_wino63.hip): six output frames from eight inputs, 8 channel-GEMMs
 * on a sixth of the columns = 4/9 of the direct MFMA work (T = 150 tiles exactly: 25 sextets; any T works, a
 * tracklet's last sextet is masked).  The input transform V = B^T d (points 0, +-1, +-2, +-1/2, inf) is its
 * own HBM-bound pass into `workspace` (tspn_conv3_tc_wino63_workspace_bytes), the MFMA kernel stages it by LDS-DMA.
 *   frag = tspn_pack_conv3_wino63_frag_f32(conv.weight [M, Cin, 3], split): U_j = G g computed in double, rounded
 *          once, stored fragment-major [M'/32][Cin'/8][8][64 lanes][4] (split as in tspn_pack_conv3_f32)
 * fp32 error against float64, measured at K = 3 x 2048 (tests/test_gpu_wino63.py, profiles/r3/conv_error_realistic.txt):
 * |err| <= 64 eps sum_k |x_k||w_k| per output element (direct form: <= 16 eps ...); on temporally smooth
 * features it equals the direct form's error, on temporally independent heavy-tailed ones it is up to ~5x larger
 * (1.3e-5 of max|y|).  Callers that need the direct form's error pass TSPN_CONV_DIRECT (2.25x the MFMA work).
 * Needs Cin % 32 == 0, M % 32 == 0, 16-byte aligned operands.  tspn_forward_fused_f32 runs it for
 * conv_algo TSPN_CONV_WINOGRAD63.                                                                           */
int tspn_pack_conv3_wino63_frag_f32(const float* W, int64_t M, int64_t Cin, int64_t split, float* frag,
                                    void* stream);
size_t tspn_conv3_tc_wino63_workspace_bytes(int64_t B, int64_t T, int64_t Cin);
int tspn_conv3_tc_wino63_f32(const float* x, int64_t B, int64_t T, int64_t Cin, const float* frag,
                             int64_t M, const float* bias, int relu, float* y,
                             void* workspace, size_t workspace_bytes, void* stream);
/* How the F(6,3) contractions fetch their operands into LDS; covers both forms, fp32 and split-fp16 (below).
 * 0 (default) = buffer loads with 32-bit offsets where the operands allow -- fp32 form: its transformed input, workspace
 * below 4 GB; split-fp16 form: weights and split input, one point's hi + lo slab of either below 2 GB -- and 64-bit
 * pointers otherwise; 1 = pointers everywhere.  Both forms land the same bytes in LDS (tests compare them bit for
 * bit).  Process-wide; returns the previous value, TSPN_EINVAL for any other `form`. */
int tspn_conv3_tc_wino63_set_piece_form(int form);

/* Split-fp16 form of the same F(6,3) conv (tspn_wino63.hip; additive, no layout change): the 8 point GEMMs run on
 * v_mfma_f32_32x32x16_f16 with every operand split into fp16 hi + lo parts, x.w ~ hi.hi + hi.lo + lo.hi (three f16
 * products, each exact in fp32, one fp32 accumulator), and power-of-two scales per (point, weight row) and per
 * (point, sextet column of the transformed input) that keep both parts inside fp16's range.  Error against float64
 * not above the fp32 form's bounds (tests/test_gpu_wino63_f16x3.py).
 *   packed = tspn_pack_conv3_wino63_f16x3(conv.weight [M, Cin, 3], split): int16 storage of
 *            [8 points][2 Cin'/8 + 1][M'][8] (hi parts, lo parts, one 16-byte slot per row holding its int32 exponent),
 *            tspn_pack_conv3_wino63_f16x3_elements(M, Cin, split) elements, 16-byte aligned
 *   workspace >= tspn_conv3_tc_wino63_f16x3_workspace_bytes(B, T, Cin, M), 256-byte aligned
 * Needs Cin % 32 == 0, M % 256 == 0.  tspn_forward_fused_f32 runs it for conv_algo TSPN_CONV_WINOGRAD63_F16X3.      */
size_t tspn_pack_conv3_wino63_f16x3_elements(int64_t M, int64_t Cin, int64_t split);
int tspn_pack_conv3_wino63_f16x3(const float* W, int64_t M, int64_t Cin, int64_t split, int16_t* packed, void* stream);
size_t tspn_conv3_tc_wino63_f16x3_workspace_bytes(int64_t B, int64_t T, int64_t Cin, int64_t M);
int tspn_conv3_tc_wino63_f16x3(const float* x, int64_t B, int64_t T, int64_t Cin, const int16_t* packed,
                               int64_t M, const float* bias, int relu, float* y,
                               void* workspace, size_t workspace_bytes, void* stream);
/* The contraction runs one 256 x 256 tile per CU at a time.  1 (default): the tiles of the last round, when they fill
 * at most half of the CUs, are cut into 2 or 4 tiles of 256 x 128 / 256 x 64 so that more CUs share that round; 0: whole
 * tiles only.  The outputs are the same bit for bit (tests/test_gpu_wino63_f16x3_tail.py).  Process-wide (additive, no
 * version bump); returns the previous value, TSPN_EINVAL for any other `on`. */
int tspn_conv3_tc_wino63_f16x3_set_tail_split(int on);
/* The input side of the split form (additive, no version bump).  Two forms produce the same bytes
 * (tests/test_gpu_input_f16x3.py): the two-pass transform (a workgroup per 8 sextets, x read twice; in
 * tspn_forward_fused_f32 the temporal mean is a third read by its own kernel) and the fused kernels of
 * csrc/inputf16/ (a scan with a workgroup per tracklet takes the column maxima AND the mean in one read, a second
 * kernel splits: x read twice in all; Cin <= 2048).
 *   tspn_conv3_tc_wino63_f16x3_input_form(NT, T, Cin, cus): 1 where the fused kernels are taken for NT tracklets on a
 *     device of `cus` compute units, 0 for the two-pass form -- a pure function, what the entries ask by default
 *   tspn_conv3_tc_wino63_f16x3_set_input_form(form): 0 (default) = by that function, 1 = two-pass everywhere,
 *     2 = fused wherever the kernels support the shape.  Process-wide; returns the previous value, TSPN_EINVAL for any
 *     other `form`.
 *   tspn_conv3_tc_wino63_f16x3_input: the input side alone -- split input and column exponents, its outputs, into the head of
 *     `split_input` (sized and aligned as the conv's buffer, tspn_conv3_tc_wino63_f16x3_workspace_bytes(B, T, Cin, M): fp16 [8][2][Cin/8][nsp2][8], 256-byte aligned
 *     int32 [8][nsp2] behind it, nsp2 = B ceil(T/6) rounded up to 256), the temporal mean into fbar [B, Cin] (may be
 *     null), the hot-sextet keys ((float bits of the largest |x| << 32) | sextet) into hot_slots (64 slots 256 bytes
 *     apart, zeroed by the caller, the reader takes their maximum; may be null). */
int tspn_conv3_tc_wino63_f16x3_input_form(int64_t NT, int64_t T, int64_t Cin, int cus);
int tspn_conv3_tc_wino63_f16x3_set_input_form(int form);
int tspn_conv3_tc_wino63_f16x3_input(const float* x, int64_t B, int64_t T, int64_t Cin, int64_t M, void* split_input,
                                     size_t split_input_bytes, float* fbar, uint64_t* hot_slots, void* stream);


/* ---- a8/a10: relationness + span-regression heads -----------------------
 * Replaces duration_pred (lib/modeling/relpn/dpn.py:71) and relness_pred
 * (lib/modeling/relpn/dpn_anchor.py:105) as ONE [H, C] 1x1 GEMM:
 *   out[P, H, T] = bh[H] + Wh[H, C] @ h_p[C, T]
 * with h_p formed on the fly (never stored):
 *   mode 0 (dense):      h_p = a[ia[p]]                         (a = ReLU'd encoder output [*,C,T])
 *   mode 1 (factorised): h_p = relu(a[ia[p]] + b[ib[p]] + bias) (a,b = tracklet projections)
 * a, b are [*, lda, T] tensors whose first C channels are used
 * (row stride lda*T floats); ia/ib are int64 row ids read at ia[p*idx_stride]
 * (NULL = identity; idx_stride = 2 walks one column of a [P,2] pair table).
 * H <= 16.                                                                  */
int tspn_heads_f32(int mode, const float* a, const float* b, int64_t lda,
                   const int64_t* ia, const int64_t* ib, int64_t idx_stride, const float* bias,
                   const float* Wh, const float* bh, int64_t H,
                   int64_t P, int64_t C, int64_t T, float* out, void* stream);

/* Blocked form of mode 1 for the CANONICAL pair table (all ordered pairs (s,o), s != o, s-major,
 * per video; lib/modeling/predict.py:133-140): y[B*N, 2C, T] holds the tracklet projections
 * (channels [0,C) subject part incl. bias, [C,2C) object part);
 *   out[b*N*(N-1) + s*(N-1) + o - (o>s)][H][T] = bh + Wh @ relu(y[b*N+s, :C] + y[b*N+o, C:])
 * 8x8 pair blocks share their 16 rows through LDS (6x less traffic than tspn_heads_f32).       */
int tspn_heads_pairgrid_f32(const float* y, int64_t B, int64_t N, int64_t C, int64_t T,
                            const float* Wh, const float* bh, int64_t H, float* out,
                            void* stream);

/* The same pair stage on split-fp16 MFMAs (csrc/pairf16): relu(U[s] + V[o]) is formed in fp32 and split into two fp16
 * pieces, the head weights likewise (scaled per head by a power of two), three f16 MFMAs per product block; every
 * product is carried to about 2^-21 of its size, the sums are fp32: with u = 2^-24 and S = |b_h| + sum_c |w_hc| a_c an
 * output is within (20 + C / 32) u S + 2^-35 (max_c |w_hc| sum_c a_c + sum_c |w_hc|) of the exact sum, the second term
 * being fp16's subnormal spacing on the low pieces (tests/test_gpu_pair_stage_f16x3_bound.py).
 * y[B*N, 2C, ldt] with ldt >= T frames per row; frames [T, ldt) reach no output, whatever they hold.
 * Needs C % 32 == 0, even T, ldt % 4 == 0, y 16-byte and out 8-byte aligned, a video's projections below 2 GB
 * (TSPN_EUNSUPPORTED otherwise); H <= 16.  A workgroup tile (8 subjects x 8 objects x 32 frames) in which some |U[s]|
 * or some |V[o]| of a written output is not <= 2^14 -- each half on its own, whatever their sum is; NaN and infinities
 * included -- and every tile when a head's weights are non-finite, all below 2^-100 or reach 2^100, is computed by one
 * fp32 fmaf chain in channel order per output instead.
 * split_buf: split_bytes >= tspn_heads_pairgrid_f16x3_split_bytes(C, H) bytes of 16-byte aligned scratch, every byte of
 * which the call writes before it reads it (0 bytes for a C or H the entry refuses).
 * tspn_heads_pairgrid_f16x3_set_force_exact(1) sends every tile of later calls (this entry and the fused pass) through
 * the fp32 chain, process-wide, for tests; returns the previous setting.
 * tspn_heads_pair_f16x3_set_diag_skip(on): 1 (default) = in a tile whose subject and object block are the same, which
 * holds no pair (s, s), a wave forms and multiplies only the seven objects it stores; 0 = all eight, as in every other
 * tile.  Same outputs bit for bit (an output's products and their order do not depend on the walk); process-wide, for
 * A/B timing; returns the previous setting.                                                                        */
size_t tspn_heads_pairgrid_f16x3_split_bytes(int64_t C, int64_t H);
int tspn_heads_pairgrid_f16x3_set_force_exact(int on);
int tspn_heads_pair_f16x3_set_diag_skip(int on);
int tspn_heads_pairgrid_f16x3(const float* y, int64_t ldt, int64_t B, int64_t N, int64_t C, int64_t T,
                              const float* Wh, const float* bh, int64_t H, void* split_buf, size_t split_bytes,
                              float* out, void* stream);

/* ---- a3: RelOIPool over time --------------------------------------------
 * mean over t of x[R, T, D] -> out[R, D]   (layout_tc = 1, tracklet layout)
 * mean over t of x[R, C, T] -> out[R, C]   (layout_tc = 0, channels-first)  */
int tspn_temporal_mean_f32(const float* x, int64_t R, int64_t T, int64_t Cdim,
                           int layout_tc, float* out, void* stream);
/* sum over t of x[R, T, D] -> out[R, D], frames added in order (with R = 1: the column sums of a matrix -- the bias
 * gradients of the training step, lib/modeling/train.py:74-78; round 4)                                          */
int tspn_temporal_sum_f32(const float* x, int64_t R, int64_t T, int64_t Cdim, float* out, void* stream);

/* gather rows: out[P, 2D] = cat(src[pairs[p,0]], src[pairs[p,1]])           */
int tspn_pair_rows_f32(const float* src, int64_t NT, int64_t D, const int64_t* pairs,
                       int64_t P, float* out, void* stream);

/* [R,T,D] -> [R,D,T] (tracklet layout -> channels-first)                     */
int tspn_transpose_td_f32(const float* x, int64_t R, int64_t T, int64_t D, float* out,
                          void* stream);

/* ---- f1: top-k triplet decode -------------------------------------------
 * Replaces the per-segment decode of lib/modeling/predict.py:66-106 for S segments of P pairs:
 * per pair the topk_pair best of the K predicate scores, per segment the topk_seg best of those
 * (both "larger first, lower index first on ties"), then for winner r of segment s:
 *   out_score[s,r]        the score
 *   out_pair_tid[s,r,:]   = pairs[s, pair(r), :]                    (local tracklet ids)
 *   out_triplet[s,r,:]    = (argmax cls_sub[row(tid_s)], predicate id, argmax cls_obj[row(tid_o)])
 * with row(tid) = s*seg_rows + row_mul*tid in a matrix of row stride `ld`, NO class columns.
 * predict.py:88-89 reads row (N-1)*tid of the pair-feature matrix (columns 0:35 / 35:70): pass
 * cls_sub = feats, cls_obj = feats + 35, ld = F, seg_rows = P, row_mul = N-1 to reproduce it, or
 * the per-tracklet class logits with seg_rows = N, row_mul = 1.
 * M = min(topk_seg, P*min(topk_pair,K)) <= 1024 rows are written per segment; K <= 256.          */
size_t tspn_decode_topk_workspace_bytes(int64_t S, int64_t P, int64_t topk_pair);
int tspn_decode_topk_f32(const float* rel_logit, const int64_t* pairs,
                         const float* cls_sub, const float* cls_obj, int64_t ld,
                         int64_t seg_rows, int64_t row_mul, int64_t S, int64_t P, int64_t K,
                         int64_t NO, int64_t topk_pair, int64_t topk_seg,
                         float* out_score, int64_t* out_triplet, int64_t* out_pair_tid,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ---- f3: temporal span decode + 1-D NMS ---------------------------------
 * Build-defined completion of the reference's stub RelNMS (lib/modeling/relpn/rel_nms.py:5-15;
 * anchors per lib/modeling/relpn/anchor_generator.py:48-59) — semantics in DESIGN.md §2 and
 * oracle.decode_spans.  heads[P, 3A, T] as produced by tspn_forward_fused_f32 /
 * tspn_temporal_encoder_heads_f32 (rows [0,A) relationness logits, [A,3A) (d_c, d_w) per anchor);
 * `sizes_host` = A anchor widths in frames (HOST pointer, copied into the launch).
 * Per pair the first `top_k` NMS survivors, best first:
 *   out_anchor[P,top_k] candidate index t*A+a (-1 = unused)   out_span[P,top_k,2] int64 frames [s,e)
 *   out_span_f[P,top_k,2] fp32 (start,end)                    out_score[P,top_k] sigmoid(logit)
 *   out_count[P] number of survivors.
 * Limits: A <= 8, A*T <= 4096, top_k <= 1024; at most min(pre_nms, 1024) candidates enter the NMS. */
int tspn_decode_spans_f32(const float* heads, int64_t P, int64_t A, int64_t T,
                          const float* sizes_host, int64_t top_k, double nms_threshold,
                          int64_t pre_nms, int64_t* out_anchor, int64_t* out_span,
                          float* out_span_f, float* out_score, int64_t* out_count, void* stream);

/* ---- whole relation-scoring pass on tracklet tensors --------------------
 * The fused/factorised product path for `B` videos of N
 * tracklets each: pair builder + temporal encoder + relationness/span heads
 * + RelOIPool + predicate head, without materialising [P, 2D, T].           */
typedef struct tspn_fused_desc {
  int64_t B, N, T, D;          /* videos, tracklets per video, frames, RoI dim; C = 2D */
  int64_t A, K;                /* anchors per location; predicates */
  const float* feats;          /* [B*N, T, D] */
  const int64_t* pairs;        /* [P,2] global tracklet ids (video b: b*N + local) */
  int64_t P;
  int64_t canonical_pairs;     /* != 0: `pairs` is the canonical table of tspn_pair_index_i64 for every
                                  video in order (P == B*N*(N-1)): enables the blocked pair stage */
  const float* conv_packed;    /* packed conv.weight [C,C,3], see TSPN_CONV_* above */
  int64_t conv_algo;           /* TSPN_CONV_DIRECT (k=3 taps as an implicit GEMM, any shape) or
                                  TSPN_CONV_WINOGRAD63 (Winograd F(6,3), 4/9 of the MFMA work, D % 32 == 0) */
  const float* conv_bias;      /* [C] */
  const float* head_w;         /* [3A, C]: rows [0,A) relness_pred, [A,3A) duration_pred */
  const float* head_b;         /* [3A] */
  const float* cls_w;          /* [K, C] */
  const float* cls_b;          /* [K] */
  float* out_heads;            /* [P, 3A, T] */
  float* out_logits;           /* [P, K] */
  void* workspace;
  size_t workspace_bytes;
  /* optional profiling hooks: hipEvent_t recorded on `stream` immediately before / after the
   * dominant kernel (the tracklet-projection implicit GEMM); NULL = off */
  void* ev_conv_begin;
  void* ev_conv_end;
  /* optional: hipEvent_t recorded on `stream` as soon as out_logits is complete.  The predicate logits depend
   * only on the tracklet means, so the driver computes them FIRST; a caller can start the top-k decode, the PPN
   * and the result gather on a second stream behind this event while the encoder is still running. */
  void* ev_logits_ready;
  /* optional accuracy guard of TSPN_CONV_WINOGRAD63 (round 6; tspn_conv3_spot_check_f32 below): the RAW conv.weight
   * [C, C, 3] and the number of output rows to spot-check per call (0 / NULL = off; needs an attached status block) */
  const float* conv_weight;
  int64_t conv_check;
} tspn_fused_desc;

size_t tspn_forward_fused_workspace_bytes(const tspn_fused_desc* d);
int tspn_forward_fused_f32(const tspn_fused_desc* d, void* stream);

/* ---- a-posteriori accuracy guard of the temporal conv (round 6) ------------
 * The encoder's contract is a plain fp32 Conv1d (lib/modeling/relpn/dpn.py:69-73).  Behind a conv launch, `rows`
 * workgroups each pick one output row (stratified over the rows, a different draw every call) and recompute that
 * row at up to 24 columns -- the six frames of four 6-frame groups ("sextets": the one named in scratch word 0, three hashed
 * ones) -- in float64 from the RAW weights, and compare with y:
 *   x [B, T, Cin]; W = conv.weight [M, Cw, 3] with `split` as in tspn_pack_conv3_f32 (split > 0: Cw = 2 split,
 *   Cin = split, y has 2M rows: [0, M) from W[:, :split], [M, 2M) from W[:, split:]); bias per y row or NULL;
 *   y [B, rows of y, ldy] (ldy >= T);  scratch: TSPN_CONV_CHECK_SCRATCH_BYTES of 8-byte aligned DEVICE memory, zeroed
 *   by the caller before the conv it belongs to: bytes [0, 32) = where the workgroups meet (the kernel leaves them
 *   zeroed); from TSPN_CONV_CHECK_HOT_OFFSET on, TSPN_CONV_CHECK_HOT_SLOTS 64-bit keys 256 bytes apart, into which the
 *   F(6,3) input transform reports (float bits of the largest |x| a wave saw) << 32 | its sextet b * ceil(T/6) + q:
 *   the sextet of the largest key is the first of the four checked -- the Winograd error peaks in the sextet that holds
 *   an input outlier.  All keys 0 = four hashed sextets.
 * Result (no fault): status word TSPN_STATUS_CONV_ERR = max(itself, float bits of the largest |y - y_ref|),
 * TSPN_STATUS_CONV_CHECKS += outputs checked -- written once per launch by the last workgroup to finish.  Needs an
 * attached status block.                                                                                          */
#define TSPN_CONV_CHECK_HOT_SLOTS 64
#define TSPN_CONV_CHECK_HOT_OFFSET 256
#define TSPN_CONV_CHECK_SCRATCH_BYTES (TSPN_CONV_CHECK_HOT_OFFSET + 256 * TSPN_CONV_CHECK_HOT_SLOTS)
int tspn_conv3_spot_check_f32(const float* x, int64_t B, int64_t T, int64_t Cin, const float* W, int64_t M,
                              int64_t Cw, int64_t split, const float* bias, int relu, const float* y, int64_t ldy,
                              uint64_t* scratch, int64_t rows, void* stream);

/* ---- span-restricted RelOIPool + predicate head --------------------------
 * Build-defined meaning of RelOIPool with duration proposals (reference lib/modeling/model.py:68-73 indexes
 * a list with a tensor and cannot run): the pair feature cat(f_s, f_o) is averaged over
 * the pair's own span [start, end) of frames before RelationPredictor (model.py:85-88):
 *   out[p] = sigmoid(cls_w . mean_{t in [start_p, end_p)} cat(f[s_p, t], f[o_p, t]) + cls_b).
 * feats [NT, T, D]; pairs [P,2] global tracklet ids; spans int64 [P,2], e.g. the top span of
 * tspn_decode_spans_f32.  A row that is not 0 <= start < end <= T is rewritten: start and end
 * are clipped into the segment, an empty or reversed span pools its first frame, and one with a negative
 * start -- the (-1, -1) of a pair without a proposal -- pools the whole segment.  A NaN / Inf feature reaches
 * exactly the outputs of the spans that contain its frame.                                           */
size_t tspn_span_predicate_workspace_bytes(int64_t NT, int64_t T, int64_t D, int64_t K);
int tspn_span_predicate_f32(const float* feats, int64_t NT, int64_t T, int64_t D, const int64_t* pairs,
                            const int64_t* spans, int64_t P, const float* cls_w, const float* cls_b,
                            int64_t K, float* out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- relations decoded with their temporal spans (csrc/relations/) ---------
 * Build-defined (the reference decodes whole-segment relations only).  For S equal-shape segments of N
 * tracklets and P pairs each, with the J = spans_per_pair proposals per pair that tspn_decode_spans_f32(top_k = J)
 * wrote for the S*P pairs:
 *   feats [S*N, T, D]; pairs int64 [S, P, 2] segment-local tracklet ids in [0, N); spans int64 [S*P, J, 2] frames
 *   [start, end); span_scores fp32 [S*P, J] (already a sigmoid); span_counts int64 [S*P]; cls_w [K, 2D], cls_b [K] or
 *   NULL; cls_logits [S, N, NO] per-tracklet class logits.
 * A candidate (p, j, k), j < span_counts[p], scores  q * span_scores[p, j]  (one fp32 product) with q the value
 * tspn_span_predicate_f32 returns for (pair p, spans[p, j]), bit for bit.  Per (p, j) the R = min(topk_per_span, K)
 * best k by q, over the segment the best min(topk_per_seg, candidates) by the product; order of torch's stable
 * descending sort (NaN above +Inf, lower flat index ((p*J + j)*R + r) on ties).
 * Outputs, Mc = min(topk_per_seg, P*J*R) slots per segment: out_score [S, Mc], out_triplet int64 [S, Mc, 3] (subject
 * class, predicate, object class; class = first argmax of the tracklet's cls_logits row), out_pair_tid int64
 * [S, Mc, 2], out_span int64 [S, Mc, 2] (the spans row as given), out_span_rank int64 [S, Mc] (j), out_valid int64 [S]:
 * the slots written; the rest are left untouched.
 * TSPN_EUNSUPPORTED: K > 256, topk_per_seg > 1024, J > 16, P*J*R >= 2^31.                                        */
size_t tspn_decode_span_relations_workspace_bytes(int64_t S, int64_t N, int64_t T, int64_t D, int64_t P, int64_t J,
                                                  int64_t K, int64_t topk_per_span);
int tspn_decode_span_relations_f32(const float* feats, int64_t S, int64_t N, int64_t T, int64_t D,
                                   const int64_t* pairs, int64_t P, const int64_t* spans, const float* span_scores,
                                   const int64_t* span_counts, int64_t J, const float* cls_w, const float* cls_b,
                                   int64_t K, const float* cls_logits, int64_t NO, int64_t topk_per_span,
                                   int64_t topk_per_seg, float* out_score, int64_t* out_triplet,
                                   int64_t* out_pair_tid, int64_t* out_span, int64_t* out_span_rank,
                                   int64_t* out_valid, void* workspace, size_t workspace_bytes, void* stream);

/* ---- bf16-operand path (BASELINE config 3: N=64, T=900, D=1024, bf16) ----
 * Semantics (build-defined; pinned by tests/golden/g8 against the reference's own DPNHead /
 * RelationPredictor modules cast with .bfloat16(), lib/modeling/relpn/dpn.py:55-73, model.py:76-88):
 * operands bf16 (stored as uint16_t bit patterns), products exact, accumulation and biases fp32; the
 * encoder activation relu(conv + b) is rounded to bf16 once, the span-pooled feature is rounded to
 * bf16, head outputs and logits are fp32.
 * Held to (tests/bf16_reference.py has the derivation): with u = 2^-24 and S the same sum over magnitudes, a contraction of
 * depth Kd on MFMAs of step k is within 2 (k + Kd / k + 2) u S of its float64 value on the same bf16 operands (k = 32, Kd = C
 * for the pair stages and the dense heads; k = 16, Kd = 3 Cin for the conv), and the mean within the bf16 roundings of
 * m -+ 2 (ceil(T / 4) + 3) u sum |x_t| / T.  This holds on eight kinds of input -- unit, large (2^13), tiny (2^-100), one
 * hot channel per k-step (2^12), cancelling sums, per-channel scales over 2^+-20, u close to -v, and bf16-SUBNORMAL
 * activations: nothing on the path flushes them, so there is no absolute floor -- and where every partial sum is exact
 * in fp32 the outputs are the correctly rounded sums bit for bit, ties at the rounding points going to even.          */
int tspn_cast_bf16(const float* src, int64_t n, uint16_t* dst, void* stream); /* round-to-nearest-even */
/* conv.weight [M, Cin, 3] fp32 -> [3][Cp/8][Mp][8] bf16; `split` as in tspn_pack_conv3_f32 */
int tspn_pack_conv3_bf16(const float* W, int64_t M, int64_t Cin, int64_t split, uint16_t* packed,
                         void* stream);
/* 1x1 head weights [H <= 16, C] fp32 -> [C/8][16][8] bf16 (rows H..15 zero) */
int tspn_pack_heads_bf16(const float* W, int64_t H, int64_t C, uint16_t* packed, void* stream);
/* k=3, pad=1 conv over time; x bf16 channels-last [B, T, Cin]; y fp32 channels-last [B*T, ldm]
 * (y[n][m], n = b*T + t), + bias[m] if given.  Needs Cin % 16 == 0, M % 4 == 0, ldm % 4 == 0 and packed weights below
 * 2 GB (the operand pieces are buffer loads with 32-bit offsets; x may have any size). */
int tspn_conv3_tc_bf16(const uint16_t* x, int64_t B, int64_t T, int64_t Cin, const uint16_t* packed,
                       int64_t M, const float* bias, float* y, int64_t ldm, void* stream);
/* pair stage on the canonical pair table: y fp32 [B*N*T, ldm] with U = channels [0,C), V = [C,2C) (ONE video's rows,
 * N*T*ldm*4 bytes, must stay below 2 GB: buffer loads with 32-bit offsets from the video's base);
 * out[p][h][t] = head_b[h] + sum_c Wh[h][c] * bf16(relu(U[s][t][c] + V[o][t][c])), out [B*N*(N-1), H, T] */
int tspn_heads_pairgrid_bf16(const float* y, int64_t ldm, int64_t B, int64_t N, int64_t C, int64_t T,
                             const uint16_t* head_packed, const float* head_b, int64_t H, float* out,
                             void* stream);
/* mean over frames of bf16 [R, T, D] -> fp32 [R, D] holding bf16-rounded values (RelOIPool over the
 * whole segment, model.py:59-60) */
int tspn_temporal_mean_bf16(const uint16_t* x, int64_t R, int64_t T, int64_t D, float* out, void* stream);

typedef struct tspn_fused_bf16_desc {
  int64_t B, N, T, D;            /* C = 2D; D % 16 == 0 */
  int64_t A, K;
  const uint16_t* feats;         /* bf16 [B*N, T, D] */
  const int64_t* pairs;          /* canonical table of tspn_pair_index_i64 for every video, global ids
                                    (tspn_forward_fused_bf16_pairs: any [P,2] table of global ids) */
  int64_t P;                     /* == B*N*(N-1) (tspn_forward_fused_bf16_pairs: any 0 <= P < 2^31) */
  const uint16_t* conv_packed;   /* tspn_pack_conv3_bf16(conv.weight [C,C,3], split=D): [3][D/8][2C][8] */
  const float* conv_bias;        /* [C] fp32 */
  const uint16_t* head_packed;   /* tspn_pack_heads_bf16([3A, C]) */
  const float* head_b;           /* [3A] fp32 */
  const float* cls_w;            /* [K, C] fp32 storage of bf16-rounded weights (products of bf16 values are
                                    exact in fp32, so the fp32 predicate kernels give the bf16-MFMA result) */
  const float* cls_b;            /* [K] */
  float* out_heads;              /* [P, 3A, T] fp32 */
  float* out_logits;             /* [P, K] fp32 */
  void* workspace;
  size_t workspace_bytes;
  void* ev_conv_begin;           /* optional hipEvent_t around the conv kernel, as in tspn_fused_desc */
  void* ev_conv_end;
  void* ev_logits_ready;         /* optional, as in tspn_fused_desc: recorded as soon as out_logits is complete (the logits
                                    are computed first) */
} tspn_fused_bf16_desc;

size_t tspn_forward_fused_bf16_workspace_bytes(const tspn_fused_bf16_desc* d);
int tspn_forward_fused_bf16(const tspn_fused_bf16_desc* d, void* stream);

/* ---- bf16-operand path on an ARBITRARY pair table (pairlist/tspn_pairlist_bf16.hip) ----
 * `pairs` int64 [P,2]: global tracklet ids (video = id / N), in any order, any subset, rows may repeat, (s, s) is a pair
 * like any other (as in tspn_heads_f32 mode 1).  Cost follows the 16 x 16 (N <= 12: 8 x 8) tiles of the grid
 * (distinct subjects of a video, ascending) x (distinct objects, ascending) that hold at least one row.
 *
 * SKIPPED ROWS: a row with an id outside [0, B*N) or with its two ids in different videos is skipped -- no access
 * anywhere is made on its behalf and its row of `out` is LEFT UNWRITTEN (the caller's previous contents).
 * LIMITS: N <= 2048 and P < 2^31, else TSPN_EUNSUPPORTED; ldm < 2C, C % 32 != 0, ldm % 4 != 0 or a y / head_packed that is
 * not 16-byte aligned are TSPN_EUNSUPPORTED too; one video's rows of y stay below 2 GB as for tspn_heads_pairgrid_bf16.
 *
 * tspn_pair_plan_i32: the plan the pair stage runs on, every array the caller's (no allocation, no synchronisation;
 * one memset node and two kernels on `stream`).  Np = N rounded up to a multiple of 16.  Per video b:
 *   s_list[b][0 .. ns_b)  int32 [B][Np]  local ids of the distinct subjects that occur, ascending (slots beyond: 0)
 *   o_list[b][0 .. no_b)  the same for the objects
 *   counts[b] = (ns_b, no_b)              int32 [B][2]
 *   head[b][i][j]         int32 [B][Np][Np] over the ranks i, j in the two lists: the first row of the chain of rows whose
 *                         pair is (s_list[b][i], o_list[b][j]), -1 for none
 *   next[p]               int32 [P]: the next row of p's chain, -1 at its end and for a skipped row
 *   rank_ws               int32 [B][2][N] scratch (tracklet -> rank, -1 where it does not occur)
 * The chains are linked with atomic exchanges: their ORDER differs from run to run, the SET of rows on each does not.
 *
 * tspn_heads_pairlist_bf16: out[p][h][t] = head_b[h] + sum_c Wh[h][c] * bf16(relu(U[s_p][t][c] + V[o_p][t][c])) for
 * every row p that is not skipped; builds the plan in `workspace` (tspn_heads_pairlist_bf16_workspace_bytes, 256-byte
 * aligned) first.  A row's values equal, bit for bit, the row of tspn_heads_pairgrid_bf16 for the same (s, o).          */
int tspn_pair_plan_i32(const int64_t* pairs, int64_t P, int64_t B, int64_t N, int32_t* s_list, int32_t* o_list,
                       int32_t* counts, int32_t* head, int32_t* next, int32_t* rank_ws, void* stream);
size_t tspn_heads_pairlist_bf16_workspace_bytes(int64_t B, int64_t N, int64_t P);
int tspn_heads_pairlist_bf16(const float* y, int64_t ldm, int64_t B, int64_t N, int64_t C, int64_t T,
                             const int64_t* pairs, int64_t P, const uint16_t* head_packed, const float* head_b,
                             int64_t H, float* out, void* workspace, size_t workspace_bytes, void* stream);
/* tspn_forward_fused_bf16 on any pair table: the same descriptor, the same order of work (tracklet means and predicate
 * logits first, ev_logits_ready, the conv, then the plan and the pair-list stage), graph-capturable like it.  Skipped rows
 * (above) keep their rows of out_heads; their rows of out_logits are computed from whatever ids they hold, so a caller
 * that cannot vouch for its table checks it first. */
size_t tspn_forward_fused_bf16_pairs_workspace_bytes(const tspn_fused_bf16_desc* d);
int tspn_forward_fused_bf16_pairs(const tspn_fused_bf16_desc* d, void* stream);

/* ---- span pooling and span relations on bf16 segments (spanbf16/tspn_span_bf16.hip) ----
 * tspn_span_predicate_f32 / tspn_decode_span_relations_f32 with the bf16 semantics of tspn_forward_fused_bf16
 * (DESIGN.md 2, 4c).  feats bf16 [NT, T, D], D % 16 == 0; a row (s, o, span) pools the frames [a, e) that
 * tspn_span_predicate_f32 pools (the same row rewrite) and gives
 *   pooled_h[c] = bf16((float)(sum_{t in [a,e)} (double) f[h][t][c] / (double)(e - a)))             h = s, o
 *   out[k]      = sigmoid(sum_c pooled_s[c] W16[k][c] + sum_c pooled_o[c] W16[k][D + c] + b16[k])
 * with W16 / b16 the classifier rounded to bf16 (round to nearest even), exact products and fp32 accumulation on the bf16
 * MFMAs.  A NaN / Inf frame reaches exactly the outputs of the spans that contain it; every other output has the bits of a
 * launch on clean features.  An output depends on its own row only, wherever the row stands in the table.
 *   tspn_pack_span_cls_bf16  cls_w fp32 [K, 2D] -> `packed`, ceil(K / 16) * 16 * 2D bf16, 16-byte aligned: fragment-major
 *                            [ceil(K/16)][2D/32][64 lanes][8], rows past K zero.  cls_b stays fp32 [K] (or NULL); the
 *                            kernels round it to bf16 themselves.
 *   tspn_span_predicate_bf16 pairs int64 [P,2] global tracklet ids (any table: repeated rows, (i, i)), spans int64 [P,2] ->
 *                            out fp32 [P, K].  Workspace (256-byte aligned): float64 prefix sums [NT, T+1, D] and the pooled
 *                            rows bf16 [P, 2D].
 *   tspn_decode_span_relations_bf16  the arguments, the selection and the outputs of tspn_decode_span_relations_f32;
 *                            q[p, j, k] is what tspn_span_predicate_bf16 returns for (pair p, spans[p, j]), bit for bit.
 *                            Its workspace also holds q fp32 [S*P*J, K] and the three candidate arrays.
 * A tracklet id out of range is NOT refused and not detected: the kernels clamp the global id (for the relations
 * seg * N + the segment-local id) into [0, NT) resp. [0, S*N), so nothing outside feats is read and the row holds the
 * values of whichever tracklet the clamped id names.  A caller that cannot vouch for its table checks it first (ops.py does).
 * TSPN_EUNSUPPORTED: D % 16 != 0, feats / cls_packed not 16-byte aligned, a workspace not 256-byte aligned, and for the
 * relations K > 256, topk_per_seg > 1024, J > 16, P*J*min(topk_per_span, K) >= 2^31.  TSPN_EINVAL: a null pointer.
 * TSPN_EWORKSPACE: a short workspace.  All are answered before any device work; P == 0 or NT == 0 (S == 0) is TSPN_OK
 * without a launch. */
int tspn_pack_span_cls_bf16(const float* cls_w, int64_t K, int64_t D, uint16_t* packed, void* stream);
size_t tspn_span_predicate_bf16_workspace_bytes(int64_t NT, int64_t T, int64_t D, int64_t K, int64_t P);
int tspn_span_predicate_bf16(const uint16_t* feats, int64_t NT, int64_t T, int64_t D, const int64_t* pairs,
                             const int64_t* spans, int64_t P, const uint16_t* cls_packed, const float* cls_b,
                             int64_t K, float* out, void* workspace, size_t workspace_bytes, void* stream);
size_t tspn_decode_span_relations_bf16_workspace_bytes(int64_t S, int64_t N, int64_t T, int64_t D, int64_t P, int64_t J,
                                                       int64_t K, int64_t topk_per_span);
int tspn_decode_span_relations_bf16(const uint16_t* feats, int64_t S, int64_t N, int64_t T, int64_t D,
                                    const int64_t* pairs, int64_t P, const int64_t* spans, const float* span_scores,
                                    const int64_t* span_counts, int64_t J, const uint16_t* cls_packed,
                                    const float* cls_b, int64_t K, const float* cls_logits, int64_t NO,
                                    int64_t topk_per_span, int64_t topk_per_seg, float* out_score, int64_t* out_triplet,
                                    int64_t* out_pair_tid, int64_t* out_span, int64_t* out_span_rank,
                                    int64_t* out_valid, void* workspace, size_t workspace_bytes, void* stream);

/* ---- dense reference-faithful encoder + heads on a materialised [P,C,T] --
 * DPNHead.forward (lib/modeling/relpn/dpn.py:69-73) on arbitrary pair feats:
 * conv3+ReLU into `h_ws` [P,C,T] (caller scratch), then tspn_heads_f32 mode 0. */
int tspn_temporal_encoder_heads_f32(const float* x, int64_t P, int64_t C, int64_t T,
                                    const float* conv_packed, const float* conv_bias,
                                    const float* head_w, const float* head_b, int64_t H,
                                    float* h_ws, float* out_heads, void* stream);

/* The same on bf16 operands (semantics of tspn_forward_fused_bf16: bf16 x / weights, exact products, fp32
 * accumulation, relu(conv + b) rounded to bf16 once, fp32 outputs) -- what `DPNHead.bfloat16()` computes
 * (lib/modeling/relpn/dpn.py:55-73), pinned by golden g8.
 *   tspn_transpose_cast_bf16   x [P,C,T] fp32 (DPNHead's input layout) -> bf16 channels-last [P,T,C]
 *   tspn_heads_dense_bf16      out[p][h][t] = head_b[h] + sum_c Wh[h][c] * bf16(relu(y[p][t][c])); y fp32 [P,T,ldm]
 *   tspn_temporal_encoder_heads_bf16 = tspn_conv3_tc_bf16 (conv_packed = tspn_pack_conv3_bf16(conv.weight, split=0),
 *                                conv_bias fp32 holding bf16 values or NULL) into y_ws [P,T,C] fp32, then the heads
 *                                (head_packed = tspn_pack_heads_bf16).  Needs C % 32 == 0, H <= 16.                 */
int tspn_transpose_cast_bf16(const float* x, int64_t P, int64_t C, int64_t T, uint16_t* out, void* stream);
int tspn_heads_dense_bf16(const float* y, int64_t ldm, int64_t P, int64_t C, int64_t T,
                          const uint16_t* head_packed, const float* head_b, int64_t H, float* out, void* stream);
int tspn_temporal_encoder_heads_bf16(const uint16_t* x_tc, int64_t P, int64_t C, int64_t T,
                                     const uint16_t* conv_packed, const float* conv_bias,
                                     const uint16_t* head_packed, const float* head_b, int64_t H,
                                     float* y_ws, float* out_heads, void* stream);

/* ---- f4 (first slice): RoI feature head ------------------------------------------------------
 * The reference extracts tracklet RoI features with detectron2's R101-C4 model, configured in
 * lib/detectron/trainer.py:23-33 (no code of its own): ROIAlign 14x14 on the res4 map -> res5
 * (3 bottleneck blocks, FrozenBN) -> mean over 7x7.  These are the operators of that head on
 * channels-last (NHWC) fp32 tensors; `temporal-span-proposal-network-vidvrd_amd/roi_head.py`
 * assembles them and hands [N,T,2048] straight to the pair builder.
 *
 * Non-finite values, every entry of this section and of the three f4 sections below: on inputs that are
 * finite except for NaN / +-Inf values (either sign, any payload) in x, a feature map or a residual, every output is NaN,
 * +Inf or -Inf exactly where a float64 evaluation's is.  relu is torch's (relu(NaN) = NaN, relu(-Inf) = 0), a max pool
 * with a NaN in its window gives NaN, a padding tap is not read (never 0 * Inf), and a bad value reaches exactly the
 * outputs whose receptive field holds it: every other output has the bits of a launch without it.  Box coordinates of
 * RoIAlign are not part of this (see there).  tests/test_gpu_nonfinite_frontend.py.
 *
 * tspn_pack_conv2d_f32: Conv2d weight [Cout][Cin][KH][KW] -> [KH*KW][Cin][Cout] (KH*KW <= 64).
 * tspn_conv2d_nhwc_f32: out[NB,OH,OW,Cout] = act( conv(x[NB,H,W,Cin]) + bias[Cout] + residual[NB,OH,OW,Cout] ),
 *   zero padding `pad`, `stride`, OH = (H + 2 pad - KH) / stride + 1; bias / residual may be NULL;
 *   relu != 0 applies torch's relu (a NaN stays a NaN).  BatchNorm is folded into (packed, bias) by the caller.  Implicit GEMM
 *   on fp32 MFMA.  Needs Cin % 16 == 0, Cout % 4 == 0, 16-byte aligned tensors (else TSPN_EUNSUPPORTED).
 *   A kernel larger than the padded map (H + 2 pad < KH or W + 2 pad < KW) has no output: TSPN_EINVAL, whatever the
 *   stride -- in this entry and in tspn_conv2d_nhwc_frag_f32, tspn_conv2d_nhwc_cin4_f32 and tspn_conv2d_nhwc_bf16. */
int tspn_pack_conv2d_f32(const float* w, int64_t Cout, int64_t Cin, int64_t KH, int64_t KW,
                         float* packed, void* stream);
int tspn_conv2d_nhwc_f32(const float* x, int64_t NB, int64_t H, int64_t W, int64_t Cin,
                         const float* packed, int64_t Cout, int64_t KH, int64_t KW, int64_t stride,
                         int64_t pad, const float* bias, const float* residual, int relu, float* out,
                         void* stream);
/* Fast variant for Cout % 32 == 0 (the res5 widths): FRAGMENT-MAJOR weights
 *   frag[Cout/32][KH*KW][Cin/16][64 lanes = 32 kh + li][8 = (g, r)] = w[32 mb + li][16 c + 4 g + 2 kh + r][tap]
 * loaded straight into MFMA operand registers (each wave owns 32 output rows; only x goes through LDS).
 * Same arguments, refusals (empty output: TSPN_EINVAL) and result as tspn_conv2d_nhwc_f32 (bit-identical: same
 * contraction order). */
int tspn_pack_conv2d_frag_f32(const float* w, int64_t Cout, int64_t Cin, int64_t KH, int64_t KW,
                              float* frag, void* stream);
int tspn_conv2d_nhwc_frag_f32(const float* x, int64_t NB, int64_t H, int64_t W, int64_t Cin,
                              const float* frag, int64_t Cout, int64_t KH, int64_t KW, int64_t stride,
                              int64_t pad, const float* bias, const float* residual, int relu, float* out,
                              void* stream);
/* Stem form for Cin <= 4 (RGB): x[NB,H,W,4] (channels zero-padded to 4); one K chunk = four taps x 4 channels,
 * so a 7x7 stem runs 13 chunks instead of 49 on 16-channel padding.
 *   frag[Cout/32][ceil(KH*KW/4)][64 lanes][8 = (g, r)] = w[32 mb + li][2 kh + r][tap = 4 c + g] (0 beyond Cin / taps)
 * H + 2 pad < KH or W + 2 pad < KW: no output, TSPN_EINVAL. */
int tspn_pack_conv2d_frag_cin4_f32(const float* w, int64_t Cout, int64_t Cin, int64_t KH, int64_t KW,
                                   float* frag, void* stream);
int tspn_conv2d_nhwc_cin4_f32(const float* x, int64_t NB, int64_t H, int64_t W, const float* frag,
                              int64_t Cout, int64_t KH, int64_t KW, int64_t stride, int64_t pad,
                              const float* bias, int relu, float* out, void* stream);
/* bf16-operand form (tspn_roi_bf16.hip; v_mfma_f32_32x32x16_bf16): x, residual, out are bf16 (uint16_t
 * bit patterns), bias fp32; products exact, fp32 accumulation, act(acc + bias + residual) rounded to bf16
 * once (round to nearest even).  Weights: tspn_pack_conv2d_frag_bf16 rounds the fp32 (BN-folded) weight
 * once into  frag[Cout/32][Cin/64][KH*KW][4 ks][64 lanes = 32 kh + li][8 j] =
 * bf16(w[32 mb + li][64 c + 16 ks + 8 kh + j][tap])  (ABI 5: channel chunk outermost -- the contraction runs chunk by
 * chunk, all taps of a chunk in a row, in tspn_conv2d_nhwc_bf16 and in tspn_bottleneck_tail_bf16 alike).
 * Needs Cin % 64 == 0, Cout % 32 == 0.  H + 2 pad < KH or W + 2 pad < KW: no output, TSPN_EINVAL. */
int tspn_pack_conv2d_frag_bf16(const float* w, int64_t Cout, int64_t Cin, int64_t KH, int64_t KW,
                               uint16_t* frag, void* stream);
int tspn_conv2d_nhwc_bf16(const uint16_t* x, int64_t NB, int64_t H, int64_t W, int64_t Cin,
                          const uint16_t* frag, int64_t Cout, int64_t KH, int64_t KW, int64_t stride,
                          int64_t pad, const float* bias, const uint16_t* residual, int relu,
                          uint16_t* out, void* stream);
/* tspn_roi_align_nhwc_f32: detectron2 ROIAlign on a channels-last map feat[NF,H,W,C]:
 *   rois[R,5] = (map index, x1, y1, x2, y2) in image coordinates, `spatial_scale` image -> map,
 *   out[R,OP,OP,C]; sampling_ratio 0 = adaptive grid ceil(roi size / P) (detectron2's POOLER_SAMPLING_RATIO 0);
 *   aligned != 0 = the half-pixel-corrected form (ROIAlignV2).  `bin_stride` >= 1: only the bins (bs i, bs j) of the
 *   P x P grid are produced, OP = ceil(P / bs) -- with bs = 2 exactly the bins the stride-2 1x1 convolutions of res5's
 *   first block read (stride_in_1x1), a quarter of the work and of the output.  Needs C % 4 == 0.
 *   The map index (rois[r][0], truncated towards zero) is CLAMPED to [0, NF): an index below 0 reads map 0, an index
 *   of NF or more reads map NF - 1 -- never memory outside feat (tests/test_gpu_frontend_edges.py pins it).  The
 *   adaptive grid makes a workgroup's trip count grow with the box (ceil(roi size / P) samples per bin and axis): box
 *   coordinates are the caller's to keep finite and of the image's order of magnitude.  Non-finite FEATURE values follow
 *   the contract above: they reach the bins one of whose samples reads them (with whatever bilinear weight, zero included). */
int tspn_roi_align_nhwc_f32(const float* feat, int64_t NF, int64_t H, int64_t W, int64_t C,
                            const float* rois, int64_t R, int64_t P, float spatial_scale,
                            int sampling_ratio, int aligned, int bin_stride, float* out, void* stream);
/* bf16 map in (values exact in fp32, interpolation in fp32), bf16 out */
int tspn_roi_align_nhwc_bf16(const uint16_t* feat, int64_t NF, int64_t H, int64_t W, int64_t C,
                             const float* rois, int64_t R, int64_t P, float spatial_scale,
                             int sampling_ratio, int aligned, int bin_stride, uint16_t* out, void* stream);
/* same interpolation in fp32, result rounded once to bf16 (input of tspn_conv2d_nhwc_bf16) */
int tspn_roi_align_nhwc_f32_bf16out(const float* feat, int64_t NF, int64_t H, int64_t W, int64_t C,
                                    const float* rois, int64_t R, int64_t P, float spatial_scale,
                                    int sampling_ratio, int aligned, int bin_stride, uint16_t* out, void* stream);

/* max_pool2d(k, stride, pad) on a channels-last fp32 map x[NB,H,W,C] -> out[NB,OH,OW,C], fp32 (out_bf16 == 0)
 * or bf16 (rounded once); padding positions do not take part, a NaN in the window gives NaN (torch), a window of only
 * -Inf gives -Inf.  detectron2 BasicStem uses 3 / 2 / 1.
 * Needs C % 4 == 0.  A window larger than the padded map (H + 2 pad < k or W + 2 pad < k) has no output: TSPN_EINVAL. */
int tspn_max_pool_nhwc_f32(const float* x, int64_t NB, int64_t H, int64_t W, int64_t C, int64_t k,
                           int64_t stride, int64_t pad, void* out, int out_bf16, void* stream);

/* ---- f4: fused tail of a bottleneck block on bf16 operands (tspn_bottleneck_bf16.hip) -----------------------
 * detectron2 BottleneckBlock.forward after conv1 (modeling/backbone/resnet.py), FrozenBN folded by the caller:
 *     out = relu( W3 . relu(W2 (*) h1 + b2) + b3 + residual )      conv2 = 3x3 / pad 1 / stride 1, conv3 = 1x1
 * h1 bf16 [NB,H,W,CM] (conv1's output), residual / out bf16 [NB,H,W,4 CM] (the block input or its projection
 * shortcut); CM = 64, 128 or 256.  frag2 = tspn_pack_conv2d_frag_bf16(W2 [CM,CM,3,3]), frag3 =
 * tspn_pack_conv2d_frag_bf16(W3 [4 CM,CM,1,1]); biases fp32.  Same rounding points and contraction order as
 * tspn_conv2d_nhwc_bf16 applied twice (h2 rounded to bf16 once): bit-identical results, one launch, h2 never in HBM.
 * Both ReLUs keep a NaN; a non-finite h1 value reaches its 3 x 3 neighbourhood inside its own image, a non-finite
 * residual element its own output element (this entry and its role-split, persistent and next-conv1 forms alike). */
int tspn_bottleneck_tail_bf16(const uint16_t* h1, int64_t NB, int64_t H, int64_t W, int64_t CM,
                              const uint16_t* frag2, const float* bias2, const uint16_t* frag3,
                              const float* bias3, const uint16_t* residual, uint16_t* out, void* stream);
/* The same operator at CM = 256 with the workgroup's waves split by ROLE (tspn_tail_io_bf16.hip, round 5): four waves issue
 * every MFMA and read only weights from L2, four waves do everything that touches HBM (the LDS-DMA of the h1 ranges, the
 * residual rows, the epilogue and the stores); fp32 sums change hands through LDS under two counters per wave pair (no
 * workgroup barrier in the expand phase), the epilogue's global accesses are line-major.  Bit-identical to
 * tspn_bottleneck_tail_bf16 and 16 - 20 % faster at the res4 shape (profiles/r5/tail_role_split.md); what
 * roi_head.BottleneckBlock launches for 256 bottleneck channels.  One workgroup of 512 threads and 147 KB of LDS per CU. */
int tspn_bottleneck_tail_io_bf16(const uint16_t* h1, int64_t NB, int64_t H, int64_t W, int64_t CM,
                                 const uint16_t* frag2, const float* bias2, const uint16_t* frag3,
                                 const float* bias3, const uint16_t* residual, uint16_t* out, void* stream);

/* A whole identity-shortcut bottleneck block in ONE launch (tspn_block_bf16.hip; detectron2 BottleneckBlock.forward,
 * modeling/backbone/resnet.py, with stride 1 and no projection shortcut -- every block of a stage but its first):
 *   out = relu(W3 . relu(W2 (*) relu(W1 . x + b1) + b2) + b3 + x)
 * x, out bf16 channels-last [NB, H, W, 4 CM]; frag1 / frag2 / frag3 = tspn_pack_conv2d_frag_bf16 of the folded
 * 1x1 (4 CM -> CM), 3x3 (CM -> CM) and 1x1 (CM -> 4 CM) weights; fp32 biases.  CM = 64 or 128 (the memory-bound stages
 * res2 / res3): the 4 CM-channel map is read once and h1 / h2 stay on the CU.  Bit-identical to tspn_conv2d_nhwc_bf16
 * (conv1) followed by tspn_bottleneck_tail_bf16, non-finite values included (the recomputed halo of a tile does not
 * widen a bad pixel's 3 x 3 reach).  out must not alias x; one image's map below 2 GB. */
int tspn_bottleneck_block_bf16(const uint16_t* x, int64_t NB, int64_t H, int64_t W, int64_t CM,
                               const uint16_t* frag1, const float* bias1, const uint16_t* frag2, const float* bias2,
                               const uint16_t* frag3, const float* bias3, uint16_t* out, void* stream);
/* The FIRST block of a stage in one launch: its 1x1 convs (conv1 and the projection shortcut) read the input x
 * [NB, Hin, Win, CIN] with stride `stride`, and
 *   out = relu(W3 . relu(W2 (*) relu(W1 . x_s + b1) + b2) + b3 + bf16(Ws . x_s + bs)),   x_s = every stride-th pixel of x,
 * out [NB, (Hin-1)/stride+1, (Win-1)/stride+1, 4 CM]: the shortcut map (4 CM channels) is neither written nor read back.
 * frags = tspn_pack_conv2d_frag_bf16 of the folded shortcut weights [4 CM, CIN, 1, 1].  Built for detectron2's res2.0
 * (CIN = 64, CM = 64, stride 1).  Bit-identical to the four launches it
 * replaces (conv1, shortcut, fused tail). */
int tspn_bottleneck_block_proj_bf16(const uint16_t* x, int64_t NB, int64_t Hin, int64_t Win, int64_t CIN, int64_t stride,
                                    int64_t CM, const uint16_t* frag1, const float* bias1, const uint16_t* frag2,
                                    const float* bias2, const uint16_t* frag3, const float* bias3, const uint16_t* frags,
                                    const float* biass, uint16_t* out, void* stream);
/* The first block of res3 (CIN = 256, CM = 128, stride 2): conv1 (1x1, stride 2) + 3x3 + expand + residual + ReLU in one
 * launch, the residual [NB, H, W, 4 CM] handed over (the output of the separately launched projection shortcut):
 *   out = relu(W3 . relu(W2 (*) relu(W1 . x_s + b1) + b2) + b3 + residual).
 * Bit-identical to tspn_conv2d_nhwc_bf16 (conv1) + tspn_bottleneck_tail_bf16. */
int tspn_bottleneck_block_res_bf16(const uint16_t* x, int64_t NB, int64_t Hin, int64_t Win, int64_t CIN, int64_t stride,
                                   int64_t CM, const uint16_t* frag1, const float* bias1, const uint16_t* frag2,
                                   const float* bias2, const uint16_t* frag3, const float* bias3, const uint16_t* residual,
                                   uint16_t* out, void* stream);

/* The same launch + conv1 of the FOLLOWING block on the tile it has just produced (round 4; CM = 256 = every res4
 * block of an R-50 / R-101 C4 backbone): additionally
 *     h1n = relu( W1n . out + b1n )        1x1, 4 CM -> CM channels, bf16 [NB,H,W,CM]
 * with frag1n = tspn_pack_conv2d_frag_bf16(W1n [CM,4 CM,1,1]) of the next block's conv1 (stride 1).  The 4 CM-channel
 * map is then read once per block (as the residual) instead of twice.  out and h1n are bit-identical to
 * tspn_bottleneck_tail_bf16 followed by tspn_conv2d_nhwc_bf16(out, frag1n, relu) (same contraction order: channels
 * 0..4 CM - 1 in k-steps of 16 on one accumulator chain). */
int tspn_bottleneck_tail_next_bf16(const uint16_t* h1, int64_t NB, int64_t H, int64_t W, int64_t CM,
                                   const uint16_t* frag2, const float* bias2, const uint16_t* frag3,
                                   const float* bias3, const uint16_t* residual, uint16_t* out,
                                   const uint16_t* frag1n, const float* bias1n, uint16_t* h1n, void* stream);

/* tspn_bottleneck_tail_bf16 as a PERSISTENT kernel pipelined across tiles (round 4, tspn_bottleneck_pipe_bf16.hip; CM =
 * 256): one workgroup of eight waves per CU walks the 128-pixel tiles; four waves run the 3x3 phase of tile t while the
 * other four run the expand + residual + store of tile t - 1 (x ring and one h2 image side by side in 136 KB of LDS, 14
 * workgroup barriers per tile on both sides).  Same arithmetic, bit-identical results.  max_workgroups: 0 = one per CU
 * (what it is built for); a smaller positive number makes every workgroup walk more tiles (tests). */
int tspn_bottleneck_tail_pipe_bf16(const uint16_t* h1, int64_t NB, int64_t H, int64_t W, int64_t CM,
                                   const uint16_t* frag2, const float* bias2, const uint16_t* frag3,
                                   const float* bias3, const uint16_t* residual, uint16_t* out,
                                   int64_t max_workgroups, void* stream);

/* ---- f4: bf16-operand stem of the C4 backbone (tspn_stem_bf16.hip) ----------------------------------------
 * detectron2 BasicStem conv (modeling/backbone/resnet.py: 7x7, stride 2, padding 3, RGB in, FrozenBN folded by the
 * caller into w / bias) + ReLU with bf16 operands: image and weights rounded to bf16, exact products, fp32
 * accumulation, relu(acc + bias) rounded to bf16 once.  x fp32 [NB,H,W,3] -> out bf16 [NB,OH,OW,Cout],
 * OH = (H - 1) / 2 + 1.  Cout = 32 or 64.  `frag` = tspn_pack_stem_bf16(w fp32 [Cout,3,7,7]) (Cout * 256 bf16);
 * `workspace` (tspn_stem_bf16_workspace_bytes) holds the 2x2 space-to-depth image the conv kernel streams.  The ReLU keeps
 * a NaN, and a NaN / Inf pixel reaches exactly the outputs whose 7 x 7 window holds it (the eighth tap row and column of
 * the space-to-depth form are cleared in the operand, not multiplied by their zero weights).
 * tspn_max_pool_nhwc_bf16: max_pool2d(k, stride, pad) on a bf16 channels-last map (C % 8 == 0); NaN in the window -> NaN.
 * tspn_stem_pool_bf16: BasicStem.forward whole (conv + FrozenBN + ReLU, then max_pool2d(3, 2, 1)) in one conv
 * launch: out bf16 [NB,PH,PW,Cout], PH = (OH - 1) / 2 + 1; bit-identical to tspn_max_pool_nhwc_bf16(3, 2, 1) of
 * tspn_stem_conv_bf16, whose map it never writes (with NaN == NaN: its maxima propagate NaN at the accumulator level
 * and in the column pool).  Same operands and workspace as tspn_stem_conv_bf16. */
size_t tspn_stem_bf16_workspace_bytes(int64_t NB, int64_t H, int64_t W);
int tspn_pack_stem_bf16(const float* w, int64_t Cout, uint16_t* frag, void* stream);
int tspn_stem_conv_bf16(const float* x, int64_t NB, int64_t H, int64_t W, const uint16_t* frag, int64_t Cout,
                        const float* bias, void* workspace, size_t workspace_bytes, uint16_t* out, void* stream);
int tspn_max_pool_nhwc_bf16(const uint16_t* x, int64_t NB, int64_t H, int64_t W, int64_t C, int64_t k,
                            int64_t stride, int64_t pad, uint16_t* out, void* stream);
int tspn_stem_pool_bf16(const float* x, int64_t NB, int64_t H, int64_t W, const uint16_t* frag, int64_t Cout,
                        const float* bias, void* workspace, size_t workspace_bytes, uint16_t* out, void* stream);

/* ---- video relation detection evaluation (csrc/eval/tspn_eval.hip) -------
 * The O(|pred| x |gt| x frames) core of the reference's eval_detection_scores
 * (lib/evaluation/visual_relation_detection.py:8-36, common.py:65-106), float64, in the reference's operation order
 * (sequential sums, Python's max / min tie rules), so every vIoU is bit-equal.  Operands (packed by evaluation.py):
 *   boxes [F,4] float64 (32-byte aligned); traj [T,3] int64 = (first row in boxes, duration begin, end) with
 *   relation r's subject trajectory at 2r and object trajectory at 2r+1; predictions are relations 0..P-1, in score
 *   order inside their group; groups [G,5] int64 = (first prediction, #predictions, first ground-truth relation,
 *   #ground truths, offset of the group's row-major #pred x #gt block in ov); pred_group [P] int32.
 * tspn_eval_traj_volume_f64: vol[t] = sum over trajectory t's end-begin boxes of (x2-x1+1)*(y2-y1+1), unclamped.
 * tspn_eval_viou_f64: ov[pair] = min(viou(subjects), viou(objects)) of every (prediction, group ground truth) pair;
 *   zden[p] = 1 if a pair of prediction p with overlapping durations has a zero vIoU denominator (the reference
 *   raises ZeroDivisionError there), else 0.
 * tspn_eval_greedy_match_f64: per group, predictions in order take the undetected ground truth of the largest
 *   ov >= viou_threshold (lowest index on a tie); hit[p] int8 = 0/1, match[p] int32 = ground-truth index within the
 *   group or -1.  max_group_gt = the largest #ground truths of a group; above 4096, det_ws (one zeroed byte per
 *   relation, indexed like the relations) holds the detected flags.  The contents of traj / groups are trusted. */
int tspn_eval_traj_volume_f64(const double* boxes, const int64_t* traj, int64_t n_traj, double* vol, void* stream);
int tspn_eval_viou_f64(const double* boxes, const int64_t* traj, const double* vol, const int64_t* groups,
                       const int32_t* pred_group, int64_t n_pred, double* ov, int32_t* zden, void* stream);
int tspn_eval_greedy_match_f64(const double* ov, const int64_t* groups, int64_t n_groups, int64_t max_group_gt,
                               double viou_threshold, uint8_t* det_ws, int8_t* hit, int32_t* match, void* stream);

/* ---- video object detection evaluation (csrc/evalobj/tspn_eval_objects.hip) -------------------------------------
 * The O(|pred| x |gt| x frames) core of the reference's trajectory mAP (lib/evaluation/video_object_detection.py:12-106,
 * common.py:40-62; DESIGN.md 2 "object detection evaluation"), float64, every result bit-equal to the reference's.
 * Operands (packed by evaluation_detection.py):
 *   boxes [F,4] float64 (32-byte aligned), one row per (trajectory, frame); frames [F] int32 = the frame id of each
 *   row, ascending inside a trajectory (frame sets may have gaps; two trajectories share a frame when the ids are
 *   equal); traj [T,2] int64 = (first row, number of rows); predictions are trajectories 0..P-1, in score order inside
 *   their group, ground truths follow; groups [G,5] int64 = (first prediction, #predictions, first ground-truth
 *   trajectory, #ground truths, offset of the group's row-major #pred x #gt block in tiou) per (video, class);
 *   pred_group [P] int32.
 * tspn_evalobj_tiou_f64: per (prediction, group ground truth) pair, total = |frames of either|, and over the common
 *   frames sIoU = ov_w * ov_h * 1.0 / (area_g + area_p - ov) with the + 1 widths, max(0, .) on the overlap sides and
 *   Python's max / min; tIoU = (#(sIoU >= 0.5) + #(sIoU >= 0.7) + #(sIoU >= 0.9)) * 1.0 / (3 * total).  tiou [C]
 *   float64 receives every pair's value (NULL: not stored).  best [P] float64 / best_index [P] int32 = the running
 *   maximum over the group's ground truths in index order, from (0, 0) with a strict `>`: a tie keeps the lower index,
 *   an all-zero row or a group without ground truths gives (0.0, 0).  flags [P] int32: bit 0 = a common frame with a
 *   zero sIoU denominator, bit 1 = a pair with total == 0 (its tIoU is stored as 0); the reference raises
 *   ZeroDivisionError at both.  Every element of best, best_index, flags (and tiou) is written.
 * tspn_evalobj_claim: a prediction qualifies when best >= thresh_t and its group has a ground truth; claim [n_gt]
 *   int32 (ground truth k of the chunk = trajectory n_pred + k) = the smallest position inside its group of a
 *   qualifying prediction that names this ground truth, INT32_MAX for none; hit [P] int8 = 1 for a qualifying
 *   prediction whose position is its ground truth's claim, else 0 (the reference's det[] flags: a prediction whose
 *   best ground truth is taken is a false positive, it does not fall back to its second best).  claim is an output:
 *   the entry fills it (a kernel on `stream`) before the integer atomicMin pass, so the result is deterministic and
 *   does not depend on what claim held.  The contents of traj / groups / pred_group are trusted; a best_index outside
 *   its group never qualifies.  n_pred == 0 still fills claim. */
int tspn_evalobj_tiou_f64(const double* boxes, const int32_t* frames, const int64_t* traj, const int64_t* groups,
                          const int32_t* pred_group, int64_t n_pred, double* tiou, double* best, int32_t* best_index,
                          int32_t* flags, void* stream);
int tspn_evalobj_claim(const double* best, const int32_t* best_index, const int64_t* groups, const int32_t* pred_group,
                       int64_t n_pred, int64_t n_gt, double thresh_t, int32_t* claim, int8_t* hit, void* stream);

/* ---- training the span heads: anchor targets and losses (csrc/spanloss/tspn_span_loss.hip) ----------------------
 * Build-defined (the reference's make_dpn_loss_evaluator, relpn/dpn_anchor.py:50-70, does not exist): the
 * RPN scheme in one dimension, on the parametrisation tspn_decode_spans_f32 decodes.  One call serves one segment of P
 * pairs, A anchors per frame, T frames.  Float64 arithmetic on the fp32 heads, the fp32 widths `sizes_host` (HOST
 * pointer, A values > 0, copied into the launch) and the integer spans, one operation per step, no contraction.
 *   heads fp32 [P, 3A, T]: rows [0, A) relationness logits, row A+2a / A+2a+1 = d_c / d_w of anchor a.
 *   gt int64 [P, G, 2]: frames [start, end) per pair; a row with end <= start is padding (anywhere among the G rows);
 *   a pair with only padding has no ground truth.
 *   Anchor (t, a): lo = t - size_a/2, hi = t + size_a/2, unclipped (candidate index c = t*A + a of the decode).
 *   IoU with a row [gs, ge): inter = max(0, min(hi, ge) - max(lo, gs)); union = (hi - lo) + (ge - gs) - inter;
 *   iou = inter / union.
 * tspn_span_anchor_labels:
 *   matched int8 [P, A, T]: the ground-truth row of the largest IoU, the lower g on ties; -1 for a pair without
 *   ground truth.  label int8 [P, A, T]: 1 if the matched IoU >= pos_iou, 0 if it is < neg_iou, else -1 (ignored);
 *   low-quality rule: for every ground-truth row whose largest IoU over the pair's A*T anchors is > 0, every anchor
 *   whose IoU with that row equals that maximum gets label 1 (its matched entry stays its own best row); every
 *   anchor of a pair without ground truth is 0.
 * tspn_span_loss_f32 (mask uint8 [P, A, T] or NULL: an anchor with mask 0 is ignored by the loss, not by the matching):
 *   relationness, over anchors with label y in {0, 1}: l = max(x, 0) - x*y + log1p(exp(-|x|)), dl/dx = sigmoid(x) - y;
 *   regression, over anchors with label 1 and matched row [gs, ge): t_c = ((gs + ge)/2 - t)/size_a,
 *   t_w = log((ge - gs)/size_a) (the inverses of the decode), smooth L1 with beta on d = head - target:
 *   |d| < beta: 0.5*d*d/beta, gradient d/beta; else |d| - 0.5*beta, gradient sign(d).
 *   partials double [P, 4] = per pair (sum l, n_lab, sum (sl1(d_c) + sl1(d_w)), n_pos), reduced in a fixed lane order
 *   and tree; dheads fp32 [P, 3A, T] = the un-normalised gradient, exactly 0 where an element enters no loss; every
 *   element of both is written.
 * tspn_span_loss_finish: out double [4] = (loss_relationness = sum l / max(1, n_lab), loss_duration_proposal =
 *   sum sl1 / max(1, n_pos), n_lab, n_pos), the pairs' partials added in a fixed order by one workgroup; a second
 *   launch divides rows [0, A) of dheads by max(1, n_lab) and rows [A, 3A) by max(1, n_pos), read from `out` on the
 *   device: no host synchronisation.  n_lab and n_pos count the segment's anchors after the mask.
 * A NaN head at an anchor that enters a loss makes that loss (and that gradient element) NaN; one at an ignored or
 * masked anchor is not read.  Results are bit-equal from run to run.
 * label, matched, partials, out and dheads are caller-owned outputs; the entries use no other scratch.
 * Limits: G <= 8, A <= 16, A*T < 2^31; 0 <= neg_iou <= pos_iou <= 1; beta > 0.  P == 0 launches nothing, except that
 * tspn_span_loss_finish still writes out = 0.  G == 0 is served: every anchor negative. */
int tspn_span_anchor_labels(const int64_t* gt, const float* sizes_host, int64_t P, int64_t G, int64_t A, int64_t T,
                            double pos_iou, double neg_iou, int8_t* label, int8_t* matched, void* stream);
int tspn_span_loss_f32(const float* heads, const int64_t* gt, const float* sizes_host, const int8_t* label,
                       const int8_t* matched, const uint8_t* mask, int64_t P, int64_t G, int64_t A, int64_t T,
                       double beta, double* partials, float* dheads, void* stream);
int tspn_span_loss_finish(const double* partials, int64_t P, int64_t A, int64_t T, double* out, float* dheads,
                          void* stream);

/* ---- a balanced mini-batch of span anchors (csrc/spansample/tspn_span_sample.hip) ------------------------------
 * Build-defined (DESIGN.md 2 "span anchor sampling"; the quota rule of the reference's
 * BalancedPositiveNegativePairSampler, lib/modeling/relpn/sampler.py): selects the anchors of one segment that enter the
 * span losses, as the `mask` of tspn_span_loss_f32.
 *   label int8 [n]: the flat [P, A, T] labels of tspn_span_anchor_labels; >= 1 positive, 0 negative, < 0 never selected.
 *   key(i) = splitmix64(stream_key + i * 0x9E3779B97F4A7C15) >> (64 - key_bits), i the flat index, wrapping 64-bit
 *   integer arithmetic (the words of hashrng.bits for a stream whose key is stream_key); 1 <= key_bits <= 32.
 *   The anchors of a class are ordered by (key, i) ascending: equal keys go to the lower index.
 *   n_pos, n_neg = the class sizes; sel_pos = min(n_pos, want_pos); sel_neg = min(n_neg, batch - sel_pos).
 *   mask uint8 [n]: 1 for the sel_pos first positives and the sel_neg first negatives, 0 elsewhere; every element is
 *   written.  counts int64 [4] = (n_pos, n_neg, sel_pos, sel_neg), written by the device: the quotas are never read back.
 *   partials uint32 [tspn_span_anchor_sample_partials(n)]: the per-chunk digit histograms, the chunk offsets among the
 *   threshold-equal anchors and the select state, a caller-owned output: the call writes every element before it reads
 *   it.  4-byte aligned; counts 8-byte aligned; label and mask at any address (16-byte aligned ones take vector forms).
 * A radix select over 8-bit digits, ceil(key_bits / 8) rounds of two launches, then two more: no host synchronisation,
 * no global atomic, no memset; the results do not depend on what partials, counts and mask held and are bit-equal from
 * run to run.  Limits: 0 <= n < 2^31; batch >= 0; 0 <= want_pos <= batch.  n == 0 writes counts = 0 and nothing else
 * (label, partials and mask may be NULL then); batch == 0 is served, the mask all zeros.
 * tspn_span_anchor_sample_partials: the number of uint32 elements of `partials`; 0 for an n the entry refuses. */
int64_t tspn_span_anchor_sample_partials(int64_t n);
int tspn_span_anchor_sample(const int8_t* label, int64_t n, uint64_t stream_key, int key_bits, int64_t batch,
                            int64_t want_pos, uint32_t* partials, int64_t* counts, uint8_t* mask, void* stream);

/* ---- training targets from ground-truth relation instances (csrc/pairlabels/tspn_pair_labels.hip) -----------------
 * Build-defined (DESIGN.md 2 "pair labels"): the intent of VRDataset._get_proposals_rel_feature (lib/dataset/
 * vrdataset.py:85-138, whose statements cannot run once a pair is positive), for a batch of S segments stored back to
 * back as tspn_proposal_pair_filter_i64 takes them, plus the ground-truth spans of every pair.
 *   pairs int64 [P, 2] (any pair table: track indices local to the segment), trackid int64 [M] (< 0 proposal, >= 0 the
 *   ground-truth track id), iou fp32 (segment s: [M_s, M_s] row-major from element iou_off[s] on), insts int64 [R, 5] =
 *   (sub_tid, obj_tid, pred, begin, end) with [begin, end) in video frames (read only when G > 0), seg_frames int64
 *   [S, 2] = (fstart, fend) per segment (read only when G > 0).  pair_off / track_off / iou_off / inst_off int64 [S + 1]
 *   on the device; all four NULL with S == 1 is the single-segment form (P, M, R its sizes; otherwise the totals).
 *   col(tid) = the largest j with trackid[j] == tid >= 0; an instance is live when both columns exist and
 *   0 <= pred < K.  A live instance covers pair (s, o) iff s != o, both in [0, M), trackid[s] < 0, trackid[o] < 0,
 *   iou[s, col(sub_tid)] >= thr and iou[o, col(obj_tid)] >= thr with thr = (float)iou_thres, compared in fp32.
 *   labels fp32 [P, K]: merge 0 ("last") the one-hot of pred of the covering instance of the largest r; merge 1 ("or")
 *   the pred of every covering instance; zero where nothing covers.
 *   spans int64 [P, G, 2], span_count int32 [P]: for the covering instances in ascending r the span
 *   [max(begin, fstart) - fstart, min(end, fend) - fstart), skipped when empty or already stored for the pair; unused
 *   rows (0, 0); span_count = the distinct spans, G + 1 when more than G were found (the excess is dropped), -1 for a
 *   pair naming a track outside [0, M) (labels zero, rows padding).  G == 0 with NULL spans / span_count: labels only.
 *   inst_cols int32 [R, 2], an output: the resolved columns, -1 for a missing one, (-2, -2) for pred outside [0, K).
 * Two launches (resolve, label), no host synchronisation, atomic, memset or scratch; every output element is written
 * exactly once.  Limits: 1 <= K <= 512, 0 <= G <= 16, S, P, M, R < 2^31, iou_thres finite.  P == 0 and R == 0 (and
 * S == 0) launch nothing; an operand without elements may be NULL.  The offsets are trusted; pair indices, instance
 * ids and predicates are checked on the device. */
int tspn_pair_labels_f32(const int64_t* pairs, const int64_t* pair_off, const int64_t* trackid,
                         const int64_t* track_off, const float* iou, const int64_t* iou_off, const int64_t* insts,
                         const int64_t* inst_off, const int64_t* seg_frames, int64_t S, int64_t P, int64_t M, int64_t R,
                         int64_t K, int64_t G, double iou_thres, int merge, float* labels, int64_t* spans,
                         int32_t* span_count, int32_t* inst_cols, void* stream);

/* ---- span-bounded association of one segment (csrc/spanmatch/tspn_span_match.hip) --------------------------------
 * Build-defined (DESIGN.md 2 "span match"): which relation of the previous segment every span-bounded prediction of a
 * segment extends, decided before the host's loop.  A span-bounded prediction owns its two trajectories, so the
 * decision depends only on state fixed when the segment starts.  Frames are local to the segment (L frames, N tracklets).
 *   rel_boxes float64 [U, 2, L, 4]: role 0 = subject, 1 = object; index f = the relation's box at frame f of THIS segment
 *   (only the frames of a candidate's window are read); rel_range int32 [U, 2, 2]: per role [start, end) =
 *   max(pstart - fstart, 0), max(pend - fstart, 0), end may exceed L; rel_fend int32 [U] = r.fend - fstart; rel_triplet
 *   int64 [U, 3]; trk_boxes float64 [N, L, 4]; pred_triplet int64 [P, 3]; pred_pair int32 [P, 2]; pred_span int32 [P, 2]
 *   = [a, e).  Rows u are in candidate order (mean confidence, descending and stable), predictions in score order.
 *   (u, p) is a candidate pair iff the triplets are equal, a < rel_fend[u], for both roles start <= a < end <= e,
 *   0 <= a < e <= L and both pair indices lie in [0, N); nothing else reads a box.
 *   iou float32 [U, P, 2]: for a candidate pair and role c the IoU of rel_boxes[u, c, a:end] against
 *   trk_boxes[pred_pair[p, c], a:end] with the rounding recipe of tspn_traj_iou_tail_f64, the float64 areas summed in
 *   numpy's pairwise order over the window that starts at a; -1 for both roles of any other pair.
 *   match int32 [P]: in order of p, the smallest u not yet taken with iou[u, p, 0] >= iou_thr and iou[u, p, 1] >= iou_thr
 *   (compared in float64: NaN fails, -1 fails for iou_thr > -1), which is then taken; -1 for none.
 * Two launches (the pairs; one workgroup for the greedy pass), no allocation, synchronisation, memset or scratch buffer;
 * every element of iou and match is written.  P == 0 launches nothing; U == 0 with P > 0 writes match = -1.  Limits:
 * sizes >= 0, iou_thr finite, U <= 65536 (the taken flags live in 8 KB of LDS), U * P < 2^31, N and L < 2^31.  An
 * operand without elements may be NULL. */
int tspn_span_match_f64(const double* rel_boxes, const int32_t* rel_range, const int32_t* rel_fend,
                        const int64_t* rel_triplet, const double* trk_boxes, const int64_t* pred_triplet,
                        const int32_t* pred_pair, const int32_t* pred_span, int64_t U, int64_t P, int64_t N, int64_t L,
                        double iou_thr, float* iou, int32_t* match, void* stream);

/* ---- training the predicate head on ground-truth-span-pooled features (csrc/spancls/tspn_span_cls.hip) ------------
 * Build-defined (DESIGN.md 2 "span-pooled predicate training"; the reference's RelOIPool, lib/modeling/model.py:68-73,
 * is a stub).  Row r = p G + g of pair p and span row g; with c = span_count[p] of tspn_pair_labels_f32:
 *   c >= 1 and g < min(c, G): a row over the frames spans[p, g];  c == 0 and g == 0: a negative pair, a row over [0, T)
 *   with a zero label;  anything else is no row (c < 0, g past the count, the rows dropped by a saturated count).
 *
 * tspn_span_labels_f32: every operand of tspn_pair_labels_f32 in its order, then that entry's outputs spans int64
 *   [P, G, 2], span_count int32 [P], inst_cols int32 [R, 2] as inputs -> span_labels fp32 [P, G, K].  For
 *   g < min(span_count[p], G), row (p, g) collects the live instances that cover pair p (the test of the pair labels: the
 *   fp32 threshold compare, NaN never covers, columns from inst_cols) and whose clipped span
 *   [max(begin, fstart) - fstart, min(end, fend) - fstart) equals spans[p, g]: merge 1 ("or") sets the pred of each,
 *   merge 0 ("last") the one-hot of the one with the largest r.  Every other row is zero.  One launch; every element
 *   written exactly once; no host synchronisation, atomic, memset or scratch.  Limits: 1 <= K <= 512, 1 <= G <= 16, S, P,
 *   M, R < 2^31, iou_thres finite.  P == 0 launches nothing.
 *
 * tspn_span_predicate_loss_f32 + tspn_span_predicate_loss_finish: feats fp32 [NT, T, D], pairs int64 [P, 2] (global
 *   tracklet ids, as tspn_span_predicate_f32 takes them), pair_off int64 [S + 1] on the device (NULL: one segment),
 *   cls_w fp32 [K, 2D], cls_b fp32 [K] or NULL.  For a row, v[r, k] = the float64 value tspn_span_predicate_f32 passes
 *   through its sigmoid for (pairs[p], spans[p, g]) ([0, T) for a negative pair), y = span_labels[r, k] (0 for a negative
 *   pair), l = max(v, 0) - v y + log1p(exp(-|v|)) in float64.  Outputs: q fp32 [P G, K] = (float)sigmoid(v), dv fp32
 *   [P G, K] = (sigmoid(v) - y) / (K rows_s) with rows_s the rows of the pair's segment, both 0 where there is no row;
 *   partials double [P G] = the row sums of l; seg_rows double [S] = rows_s.  A pair naming a tracklet outside [0, NT)
 *   has no rows.  Rows are selected, not masked: nothing is read through a row that is none.
 *   tspn_span_predicate_loss_finish: out double [1 + S]: out[1 + s] = sum of segment s's partials / (K rows_s), 0 for a
 *   segment without rows; out[0] = their sum in segment order (loss_rel).  Fixed summation orders: bit-reproducible.
 *   prefix_scratch: at least tspn_span_predicate_workspace_bytes(NT, T, D, K) bytes (TSPN_EWORKSPACE otherwise), 8-byte
 *   aligned; it holds the projections and their prefix sums until the loss kernel has run.
 *
 * tspn_span_predicate_grad_f32: db fp32 [K] = sum over r of dv[r, k] (float64, rows in ascending order); dG fp32
 *   [NT, T, 2K], the gradient with respect to the per-frame projections G[n, t, 2k + h] = feats[n, t, :] .
 *   cls_w[k, hD:(h+1)D]: dG[n, t, 2k + h] = sum of dv[r, k] / (e_r - a_r) over the rows r with pairs[p_r][h] == n and
 *   a_r <= t < e_r, accumulated per column in float64 through a difference array in ascending row order and a running
 *   sum over t (a non-finite dv therefore reaches the later frames of its columns too).  No atomics; every element of
 *   dG is written.  prefix_scratch: at least NT (T + 1) 2K doubles (the loss entries' scratch is large enough and free
 *   again).  The classifier gradient is dW[k, hD + c] = sum over (n, t) of dG[n, t, 2k + h] feats[n, t, c], a GEMM.
 * Limits of the three: T < 2^30, K < 2^20, 1 <= G <= 16, P G < 2^31.  No host synchronisation and no memset. */
int tspn_span_labels_f32(const int64_t* pairs, const int64_t* pair_off, const int64_t* trackid,
                         const int64_t* track_off, const float* iou, const int64_t* iou_off, const int64_t* insts,
                         const int64_t* inst_off, const int64_t* seg_frames, int64_t S, int64_t P, int64_t M, int64_t R,
                         int64_t K, int64_t G, double iou_thres, int merge, const int64_t* spans,
                         const int32_t* span_count, const int32_t* inst_cols, float* span_labels, void* stream);
int tspn_span_predicate_loss_f32(const float* feats, int64_t NT, int64_t T, int64_t D, const int64_t* pairs,
                                 const int64_t* pair_off, int64_t S, int64_t P, const int64_t* spans,
                                 const int32_t* span_count, const float* span_labels, int64_t G, const float* cls_w,
                                 const float* cls_b, int64_t K, float* q, float* dv, double* partials, double* seg_rows,
                                 void* prefix_scratch, size_t prefix_scratch_bytes, void* stream);
int tspn_span_predicate_loss_finish(const double* partials, const double* seg_rows, const int64_t* pair_off, int64_t S,
                                    int64_t P, int64_t G, int64_t K, double* out, void* stream);
int tspn_span_predicate_grad_f32(const float* dv, const int64_t* pairs, const int64_t* spans, const int32_t* span_count,
                                 int64_t NT, int64_t T, int64_t P, int64_t G, int64_t K, float* db, float* dG,
                                 void* prefix_scratch, size_t prefix_scratch_bytes, void* stream);

/* ---- per-frame object detection: RPN proposals, box head, box NMS (csrc/detect/tspn_detect.hip) -------------------
 * Build-defined after detectron2 v0.6's faster_rcnn_R_*_C4 (DESIGN.md 2 "box decode", "box NMS", "proposals",
 * "detections").  Boxes are fp32 (x1, y1, x2, y2) rows, 16-byte aligned (TSPN_EUNSUPPORTED otherwise; every other operand
 * at its natural alignment); image_sizes fp32 [B, 2] = (height, width) on the device.  No entry synchronises, allocates or clears memory; every element of every output is written.
 *
 * tspn_rpn_decode_f32: logits fp32 [B, H, W, A], deltas fp32 [B, H, W, 4A] (channel 4a + k), cell_anchors fp32 [A, 4].
 *   cand int64 [B, M]: flat candidate indices b H W A + (h W + w) A + a, as the selection of tspn_box_nms_f32 writes them
 *   (a value outside image b's range, -1 included, is no candidate); NULL: every anchor in order, M = H W A.  The anchor
 *   is the cell anchor plus (w, h, w, h) * stride in fp32; Box2BoxTransform.apply_deltas with weights 1 in fp32, dw / dh
 *   clamped at log(1000 / 16); then the clip to [0, width] x [0, height].  out_boxes fp32 [B, M, 4], out_logits fp32
 *   [B, M] (the candidate's logit), out_valid uint8 [B, M]: 1 iff the four corners before the clip and the logit are
 *   finite; a row with 0 holds zeros.
 *
 * tspn_box_head_decode_f32: cls_logits fp32 [B R, K+1] (background last), deltas fp32 [B R, 4K], proposals fp32
 *   [B, R, 4], proposal_count int64 [B] on the device.  Class-major outputs: out_scores fp32 [B, K, R] = softmax score,
 *   out_boxes fp32 [B, K, R, 4] = apply_deltas with weights (wx, wy, ww, wh) on the proposal, clipped, out_valid uint8
 *   [B, K, R] = 1 iff r < proposal_count[b], every softmax score and every decoded corner of the proposal's row is
 *   finite, and score > score_thresh.  Where out_valid is 0 the score is 0: the validity byte is what the selection
 *   reads.  Rows past the count and non-finite rows hold zero boxes.
 *
 * tspn_box_nms_f32: boxes fp32 [n, 4], scores fp32 [n], valid uint8 [n] or NULL (all valid), group_off int64 [G + 1] in
 *   HOST memory, read before the call returns: group g is the candidates [group_off[g], group_off[g + 1]), ascending
 *   from 0 to n.  Per group: the pre_topk best scores in selection order (tspn order key: NaN first, then descending,
 *   lower index first on ties); of those, the rows with valid == 0 and (min_size >= 0) the boxes with width <= min_size
 *   or height <= min_size are dropped; greedy NMS in that order, a kept box i suppressing a later j iff
 *   inter / (area_i + area_j - inter) > iou_threshold in fp32 (torchvision's CPU kernel); the first post_topk survivors.
 *   out_index int64 [G, post_topk]: their flat indices into boxes, best first, -1 past the count; out_count int64 [G];
 *   out_keep uint8 [n] or NULL: 1 for the candidates listed in out_index, else 0.  boxes == NULL runs the selection
 *   alone (valid and out_keep must be NULL, iou_threshold and min_size are not read).
 *   scratch: at least tspn_box_nms_scratch_bytes(group_off, G, pre_topk, boxes == NULL) bytes, 16-byte aligned
 *   (TSPN_EWORKSPACE otherwise); it may hold anything on entry, nothing outside those bytes is touched, and every byte
 *   of which the call reads it has written before.  Limits: 1 <= post_topk <= pre_topk <= 8192, n < 2^31, G < 2^24.
 *   The query returns 0 for what the entry refuses and for G == 0.
 *
 * tspn_detections_topk_f32: scores / boxes / keep as tspn_box_head_decode_f32 and tspn_box_nms_f32 (G = B K groups of R)
 *   leave them.  Per image the D best kept candidates over all classes, best first, ties to the lower r K + c:
 *   out_boxes fp32 [B, D, 4], out_scores fp32 [B, D], out_classes int64 [B, D], out_count int64 [B]; rows past the count
 *   are zero.  Limit: D <= 1024. */
int tspn_rpn_decode_f32(const int64_t* cand, const float* logits, const float* deltas, const float* cell_anchors,
                        const float* image_sizes, int64_t B, int64_t H, int64_t W, int64_t A, int64_t M, float stride,
                        float* out_boxes, float* out_logits, uint8_t* out_valid, void* stream);
int tspn_box_head_decode_f32(const float* cls_logits, const float* deltas, const float* proposals,
                             const int64_t* proposal_count, const float* image_sizes, int64_t B, int64_t R, int64_t K,
                             float wx, float wy, float ww, float wh, float score_thresh, float* out_scores,
                             float* out_boxes, uint8_t* out_valid, void* stream);
size_t tspn_box_nms_scratch_bytes(const int64_t* group_off, int64_t G, int64_t pre_topk, int select_only);
int tspn_box_nms_f32(const float* boxes, const float* scores, const uint8_t* valid, int64_t n, const int64_t* group_off,
                     int64_t G, int64_t pre_topk, float iou_threshold, int64_t post_topk, float min_size,
                     int64_t* out_index, int64_t* out_count, uint8_t* out_keep, void* scratch, size_t scratch_bytes,
                     void* stream);
int tspn_detections_topk_f32(const float* scores, const float* boxes, const uint8_t* keep, int64_t B, int64_t K, int64_t R,
                             int64_t D, float* out_boxes, float* out_scores, int64_t* out_classes, int64_t* out_count,
                             void* stream);

/* ---- tracklet linking: per-frame detections -> tracks -> dense tracklet boxes (csrc/link/tspn_link.hip) -----------
 * Build-defined (DESIGN.md 2 "tracklet linking"): a deterministic IoU tracker with constant-velocity prediction, exact
 * against the numpy restatement.  Operands as tspn_detections_topk_f32 leaves them, F frames of D detection rows:
 * boxes fp32 [F, D, 4] (16-byte aligned), scores fp32 [F, D], classes int64 [F, D], count int64 [F] on the device.
 * video_off int64 [V + 1] lives in HOST memory and is read before the call returns: video v is the frames
 * [video_off[v], video_off[v + 1]), ascending from 0 to F; a video may be empty.  Frame numbers in the outputs count
 * from the video's first frame.  No entry synchronises, allocates or clears memory.
 *
 * tspn_link_detections_f32: one persistent workgroup per video.  At frame t a detection d < count[t] whose four
 *   coordinates and score are finite and whose score >= min_score is a candidate.  A track (cls, first, t_last, t_prev,
 *   hits, the boxes at t_last and t_prev, a float64 score sum) is confirmed when hits >= min_hits; it is live at t if
 *   confirmed and t - t_last <= max_age, or tentative and t - t_last == 1.  Its predicted box is, for hits >= 2,
 *   last + (last - prev) / float(t_last - t_prev) * float(t - t_last) per coordinate in fp32, else last.  A live track
 *   and a candidate (of the track's class if class_aware) form an edge iff inter / (a + b - inter) >= iou_thresh in
 *   fp32; the edges are taken greedily in the order (IoU descending, track id ascending, d ascending), a track and a
 *   detection once.  A matched track moves last to prev, takes the detection and counts a hit.  The unmatched
 *   candidates, in ascending d, start tracks with the video's next id while fewer than max_live tracks are live and
 *   fewer than max_tracks ids are used; the others stay unlinked and are counted in dropped[v].
 *   Outputs, every element written: track_of_det int32 [F, D] (the video-local id, -1: none); n_tracks, dropped int64
 *   [V]; tables [V, max_tracks]: trk_first, trk_last, trk_hits int32, trk_cls int64, trk_score fp32 = fp32(score sum /
 *   hits); past n_tracks they hold -1, -1, 0, -1, 0.
 *   Limits: 1 <= D <= 1024, 1 <= max_live <= 4096, max_tracks < 2^24, V max_tracks < 2^31, F < 2^21, 0 < iou_thresh <= 1.
 *
 * tspn_link_fill_f32: dense boxes of R selected tracks (sel_video, sel_track int64 [R] on the device; a pair outside
 *   the tables gives an absent row; a repeated pair gives equal rows).  out_boxes fp32 [R, Fmax, 4] and out_state uint8
 *   [R, Fmax], Fmax the longest video: state 1 and the detection's box where the track was detected; inside
 *   [first, last] otherwise state 2 and a + (b - a) * (float(t - ta) / float(tb - ta)) from the neighbouring detected
 *   frames ta < t < tb; state 0 and zeros elsewhere.
 *
 * scratch: at least tspn_link_scratch_bytes(V, max_live, max_tracks, R, Fmax, fill) bytes (fill == 0: the link pass,
 *   which reads V and max_live; else the fill pass, which reads V, max_tracks, R and Fmax), 16-byte aligned
 *   (TSPN_EWORKSPACE otherwise); it may hold anything on entry, nothing outside those bytes is touched, and every byte of
 *   which a call reads it has written before.  The query returns 0 for what the entries refuse, for V == 0 and, for the
 *   fill pass, R == 0. */
size_t tspn_link_scratch_bytes(int64_t V, int64_t max_live, int64_t max_tracks, int64_t R, int64_t Fmax, int fill);
int tspn_link_detections_f32(const float* boxes, const float* scores, const int64_t* classes, const int64_t* count,
                             const int64_t* video_off, int64_t V, int64_t F, int64_t D, float iou_thresh, int64_t max_age,
                             int64_t min_hits, float min_score, int class_aware, int64_t max_live, int64_t max_tracks,
                             int32_t* track_of_det, int64_t* n_tracks, int64_t* dropped, int32_t* trk_first,
                             int32_t* trk_last, int32_t* trk_hits, int64_t* trk_cls, float* trk_score, void* scratch,
                             size_t scratch_bytes, void* stream);
int tspn_link_fill_f32(const float* boxes, const int32_t* track_of_det, const int64_t* video_off, int64_t V, int64_t F,
                       int64_t D, const int32_t* trk_first, const int32_t* trk_last, int64_t max_tracks,
                       const int64_t* sel_video, const int64_t* sel_track, int64_t R, float* out_boxes, uint8_t* out_state,
                       void* scratch, size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TSPN_MI355X_H */
