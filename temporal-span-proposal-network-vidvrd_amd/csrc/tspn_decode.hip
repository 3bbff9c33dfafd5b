// f1: top-k triplet decode on the GPU (gfx950).
//
// Replaces the per-segment Python of the reference's predict loop
// (lib/modeling/predict.py:66-106): per pair the `topk_pair` best predicates
// (torch.sort descending, first columns), over the segment the `topk_seg` best of those
// (torch.sort of the flattened [P, topk_pair] scores), then for each winner the pair's tracklet
// ids, the predicate id, and subject / object class = argmax over 35 class logits of the row
// `row_mul * tid` (predict.py:88-89 reads row (N-1)*tid of the pair-feature matrix: pass
// row_mul = N-1 and the feature matrix to reproduce that, or row_mul = 1 and the per-tracklet
// class logits).  In the reference this is ~6 ms of Python list comprehensions per segment and
// everything upstream of it must cross PCIe; here the [P,K] logits never leave HBM and only
// topk_seg x (score, triplet, pair) does — which also shrinks the multi-GPU result gather ~500x.
//
// Order: torch's stable descending sort at both levels -- larger score first, every NaN (any sign or payload) above
// +Inf, lower index first on ties (NaN ties included); the class argmax returns the first NaN, as torch.argmax.  All
// compares run on tspn::order_key, so every emitted index is in range whatever the scores hold.
// Integer / compare work only: bit-exact against the oracle.
//
//   kernel 1  one wave per pair: tspn::wave_row_topk over the K scores held in registers
//   kernel 2  one workgroup per segment: tspn::select_topk_sorted over the P*R candidates, label gathers
// (both bodies: tspn_topk_select.h)
#include <algorithm>
#include <cmath>

#include "tspn_common.h"
#include "tspn_topk_select.h"

namespace {

constexpr int SEG_THREADS = tspn::kSelectThreads;
constexpr int MAX_M = tspn::kSelectMaxM;

using tspn::argmax_first;
using tspn::order_key;

__global__ __launch_bounds__(256) void pair_topk_kernel(const float* __restrict__ logits,
                                                        int64_t rows, int K, int R,
                                                        float* __restrict__ sc,
                                                        int* __restrict__ ix) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* src = logits + row * K;
  float v[tspn::kRowTopkVPT];
#pragma unroll
  for (int i = 0; i < tspn::kRowTopkVPT; ++i) {
    const int k = lane + 64 * i;
    v[i] = k < K ? src[k] : 0.f;
  }
  tspn::wave_row_topk(v, K, R, lane, [=](int r, float value, int k) {
    sc[row * R + r] = value;
    ix[row * R + r] = k;
  });
}

__global__ __launch_bounds__(SEG_THREADS) void segment_topk_kernel(
    const float* __restrict__ sc, const int* __restrict__ ix, const int64_t* __restrict__ pairs,
    const float* __restrict__ cls_sub, const float* __restrict__ cls_obj, int64_t ld, int64_t seg_rows,
    int64_t row_mul, int P, int R, int NO, int M, float* __restrict__ out_score,
    int64_t* __restrict__ out_trip, int64_t* __restrict__ out_tid) {
  __shared__ tspn::SelectLds L;

  const int tid = threadIdx.x;
  const int64_t seg = blockIdx.x;
  const int Q = P * R;
  const float* cand = sc + seg * Q;
  tspn::select_topk_sorted(L, [cand](int i) { return order_key(cand[i]); }, Q, M);
  const int* ki = L.ki;

  // ---- gathers: pair ids, predicate id, class labels
  for (int r = tid; r < M; r += SEG_THREADS) {
    const int flat = ki[r];
    const int pi = flat / R;
    const int64_t ts = pairs[(seg * P + pi) * 2], to = pairs[(seg * P + pi) * 2 + 1];
    const int64_t o = seg * M + r;
    out_score[o] = cand[flat];
    out_tid[2 * o] = ts;
    out_tid[2 * o + 1] = to;
    out_trip[3 * o] = argmax_first(cls_sub + (seg * seg_rows + row_mul * ts) * ld, NO);
    out_trip[3 * o + 1] = ix[seg * Q + flat];
    out_trip[3 * o + 2] = argmax_first(cls_obj + (seg * seg_rows + row_mul * to) * ld, NO);
  }
}

}  // namespace

extern "C" size_t tspn_decode_topk_workspace_bytes(int64_t S, int64_t P, int64_t topk_pair) {
  if (S <= 0 || P <= 0 || topk_pair <= 0) return 0;
  return (size_t)S * (size_t)P * (size_t)topk_pair * (sizeof(float) + sizeof(int));
}

extern "C" int tspn_decode_topk_f32(const float* rel_logit, const int64_t* pairs,
                                    const float* cls_sub, const float* cls_obj, int64_t ld,
                                    int64_t seg_rows, int64_t row_mul, int64_t S, int64_t P,
                                    int64_t K, int64_t NO, int64_t topk_pair, int64_t topk_seg,
                                    float* out_score, int64_t* out_triplet, int64_t* out_pair_tid,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  TSPN_REQUIRE(S >= 0 && P >= 0 && K > 0 && NO > 0 && topk_pair > 0 && topk_seg > 0 && ld >= NO &&
                   seg_rows > 0 && row_mul >= 0,
               TSPN_EINVAL, "tspn_decode_topk_f32: bad sizes");
  TSPN_REQUIRE(K <= tspn::kRowTopkMaxK, TSPN_EUNSUPPORTED, "tspn_decode_topk_f32: K=%lld > %d", (long long)K,
               tspn::kRowTopkMaxK);
  const int64_t R = std::min<int64_t>(topk_pair, K);
  const int64_t M = std::min<int64_t>(topk_seg, P * R);
  TSPN_REQUIRE(M <= MAX_M, TSPN_EUNSUPPORTED, "tspn_decode_topk_f32: topk_seg=%lld > %d",
               (long long)M, MAX_M);
  TSPN_REQUIRE(P * R < (1LL << 30), TSPN_EUNSUPPORTED, "tspn_decode_topk_f32: P*topk_pair too large");
  if (S == 0 || P == 0) return TSPN_OK;
  TSPN_REQUIRE(rel_logit && pairs && cls_sub && cls_obj && out_score && out_triplet && out_pair_tid,
               TSPN_EINVAL, "tspn_decode_topk_f32: null pointer");
  const size_t need = tspn_decode_topk_workspace_bytes(S, P, R);
  TSPN_REQUIRE(workspace && workspace_bytes >= need, TSPN_EWORKSPACE,
               "tspn_decode_topk_f32: workspace %zu < %zu bytes", workspace_bytes, need);
  float* sc = static_cast<float*>(workspace);
  int* ix = reinterpret_cast<int*>(sc + S * P * R);
  hipStream_t s = TSPN_STREAM(stream);
  const int64_t rows = S * P;
  const int64_t nb = tspn::ceil_div(rows, 4);
  TSPN_REQUIRE(nb < (1LL << 31) && S < (1LL << 31), TSPN_EUNSUPPORTED,
               "tspn_decode_topk_f32: grid too large");
  hipLaunchKernelGGL(pair_topk_kernel, dim3((unsigned)nb), dim3(256), 0, s, rel_logit, rows, (int)K,
                     (int)R, sc, ix);
  int rc = tspn::check_launch("tspn_decode_topk_f32(pair)");
  if (rc) return rc;
  hipLaunchKernelGGL(segment_topk_kernel, dim3((unsigned)S), dim3(SEG_THREADS), 0, s, sc, ix, pairs,
                     cls_sub, cls_obj, ld, seg_rows, row_mul, (int)P, (int)R, (int)NO, (int)M,
                     out_score, out_triplet, out_pair_tid);
  return tspn::check_launch("tspn_decode_topk_f32(segment)");
}
