// f5: relations decoded WITH their temporal spans (gfx950).
//
// tspn_decode_topk_f32 decodes relations that last their whole segment and score as the predicate sigmoid alone.  Here
// every pair brings the J span proposals of tspn_decode_spans_f32; a candidate is (pair p, span j, predicate k), its
// score the fp32 product  q[p,j,k] * score[p,j]  of the span-pooled predicate sigmoid (the very value
// tspn_span_predicate_f32 returns for that row: tspn::span_logit) and the span's relationness.  Per (p, j) row the R
// best k by q, over the segment the M best candidates by the product, both in torch's stable descending order
// (tspn::order_key: NaN above +Inf, lower index on ties).  Build-defined, DESIGN.md 2: the reference has no counterpart
// (its RelNMS is a stub and predict.py never reads the duration proposals).
//
//   stage a  G = f W'^T and its float64 prefix sums over time (tspn::span_prefix_stage, shared with span pooling)
//   kernel b one wave per (pair, span) row: the K <= 256 values q formed in registers from the prefix differences, then
//            tspn::wave_row_topk (tspn_topk_select.h); writes R x (key of the product, product, k).  A row
//            j >= count[p] writes tspn::kPadKey, below every real key: [rows, K] never reaches HBM
//   kernel c one workgroup per segment: tspn::select_topk_sorted over the P*J*R keys, then the gathers (pair ids,
//            predicate, class argmax, span, span rank); its launch is tspn::segment_span_topk, which the bf16 entry
//            (spanbf16/tspn_span_bf16.hip) ends with too
#include <algorithm>

#include "tspn_common.h"
#include "tspn_span_pool.h"
#include "tspn_topk_select.h"

namespace {

constexpr int MAX_J = 16;

using tspn::order_key;

__global__ __launch_bounds__(256) void span_row_topk_kernel(
    const double* __restrict__ PS, const float* __restrict__ G, const int64_t* __restrict__ pairs,
    const int64_t* __restrict__ spans, const float* __restrict__ span_scores,
    const int64_t* __restrict__ span_counts, const float* __restrict__ b, int64_t rows, int N, int P, int J, int T,
    int K, int R, unsigned* __restrict__ key, float* __restrict__ sc, int* __restrict__ ix) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int64_t pr = row / J;                  // pair over all segments
  const int j = (int)(row - pr * J);
  if ((int64_t)j >= span_counts[pr]) {         // not a proposal: nothing the segment stage can select
    for (int r = lane; r < R; r += 64) {
      key[row * R + r] = tspn::kPadKey;
      sc[row * R + r] = 0.f;
      ix[row * R + r] = -1;
    }
    return;
  }
  const int64_t seg = pr / P;
  const int64_t s = seg * N + pairs[2 * pr], o = seg * N + pairs[2 * pr + 1];
  const int64_t a0 = spans[2 * row], e0 = spans[2 * row + 1];
  const float w = span_scores[row];
  const int64_t K2 = 2 * (int64_t)K;
  float v[tspn::kRowTopkVPT];
#pragma unroll
  for (int i = 0; i < tspn::kRowTopkVPT; ++i) {
    const int k = lane + 64 * i;
    v[i] = k < K ? tspn::span_logit(PS, G, s, o, a0, e0, T, K2, k, b) : 0.f;
  }
  tspn::wave_row_topk(v, K, R, lane, [=](int r, float value, int k) {
    const float prod = value * w;                // one rounding (-ffp-contract=off)
    key[row * R + r] = order_key(prod);
    sc[row * R + r] = prod;
    ix[row * R + r] = k;
  });
}

__global__ __launch_bounds__(tspn::kSelectThreads) void segment_span_topk_kernel(
    const unsigned* __restrict__ key, const float* __restrict__ sc, const int* __restrict__ ix,
    const int64_t* __restrict__ pairs, const int64_t* __restrict__ spans, const int64_t* __restrict__ span_counts,
    const float* __restrict__ cls, int N, int NO, int P, int J, int R, int mcap, int topk_seg,
    float* __restrict__ out_score, int64_t* __restrict__ out_trip, int64_t* __restrict__ out_tid,
    int64_t* __restrict__ out_span, int64_t* __restrict__ out_rank, int64_t* __restrict__ out_valid) {
  __shared__ tspn::SelectLds L;
  __shared__ unsigned s_rows;

  const int tid = threadIdx.x;
  const int64_t seg = blockIdx.x;
  const int Q = P * J * R;
  // ---- the segment's real candidates: R per row j < count[p], exactly the rows kernel b gave real keys
  if (tid == 0) s_rows = 0;
  __syncthreads();
  unsigned mine = 0;
  for (int p = tid; p < P; p += tspn::kSelectThreads) {
    const int64_t c = span_counts[seg * P + p];
    mine += (unsigned)(c < 0 ? 0 : (c > J ? J : c));
  }
  if (mine) atomicAdd(&s_rows, mine);
  __syncthreads();
  const int64_t valid = (int64_t)s_rows * R;
  const int M = (int)(valid < topk_seg ? valid : topk_seg);
  if (tid == 0) out_valid[seg] = M;
  if (M == 0) return;                            // the same for every thread

  const unsigned* kseg = key + seg * Q;
  tspn::select_topk_sorted(L, [kseg](int i) { return kseg[i]; }, Q, M);

  // ---- gathers: score, pair ids, predicate id, class labels, span and its rank
  for (int r = tid; r < M; r += tspn::kSelectThreads) {
    const int flat = L.ki[r];
    const int row = flat / R;
    const int p = row / J, j = row - p * J;
    const int64_t pr = seg * P + p;
    const int64_t ts = pairs[2 * pr], to = pairs[2 * pr + 1];
    const int64_t o = seg * mcap + r;
    out_score[o] = sc[seg * Q + flat];
    out_tid[2 * o] = ts;
    out_tid[2 * o + 1] = to;
    out_trip[3 * o] = tspn::argmax_first(cls + (seg * N + ts) * NO, NO);
    out_trip[3 * o + 1] = ix[seg * Q + flat];
    out_trip[3 * o + 2] = tspn::argmax_first(cls + (seg * N + to) * NO, NO);
    out_span[2 * o] = spans[2 * (pr * J + j)];
    out_span[2 * o + 1] = spans[2 * (pr * J + j) + 1];
    out_rank[o] = j;
  }
}

using tspn::span_cand_bytes;   // one of the three arrays (key, product, k)

}  // namespace

int tspn::segment_span_topk(const unsigned* key, const float* sc, const int* ix, const int64_t* pairs,
                            const int64_t* spans, const int64_t* span_counts, const float* cls_logits, int64_t S,
                            int64_t N, int64_t NO, int64_t P, int64_t J, int64_t R, int64_t topk_per_seg,
                            float* out_score, int64_t* out_triplet, int64_t* out_pair_tid, int64_t* out_span,
                            int64_t* out_span_rank, int64_t* out_valid, void* stream, const char* what) {
  const int64_t mcap = std::min<int64_t>(topk_per_seg, P * J * R);
  hipLaunchKernelGGL(segment_span_topk_kernel, dim3((unsigned)S), dim3(tspn::kSelectThreads), 0, TSPN_STREAM(stream), key,
                     sc, ix, pairs, spans, span_counts, cls_logits, (int)N, (int)NO, (int)P, (int)J, (int)R, (int)mcap,
                     (int)topk_per_seg, out_score, out_triplet, out_pair_tid, out_span, out_span_rank, out_valid);
  return tspn::check_launch(what);
}

int tspn::span_relation_sizes(const char* who, int64_t S, int64_t N, int64_t T, int64_t D, int64_t P, int64_t J, int64_t K,
                              int64_t NO, int64_t topk_per_span, int64_t topk_per_seg) {
  TSPN_REQUIRE(S >= 0 && N >= 0 && P >= 0 && T > 0 && D > 0 && J > 0 && K > 0 && NO > 0 && topk_per_span > 0 &&
                   topk_per_seg > 0 && T < (1 << 30) && N < (1LL << 31) && P < (1LL << 31) && S < (1LL << 31),
               TSPN_EINVAL, "%s: bad sizes S=%lld N=%lld T=%lld D=%lld P=%lld J=%lld K=%lld NO=%lld", who,
               (long long)S, (long long)N, (long long)T, (long long)D, (long long)P, (long long)J, (long long)K,
               (long long)NO);
  return TSPN_OK;
}

int tspn::span_relation_limits(const char* who, int64_t P, int64_t J, int64_t K, int64_t topk_per_span,
                               int64_t topk_per_seg, int64_t* R) {
  TSPN_REQUIRE(K <= tspn::kRowTopkMaxK, TSPN_EUNSUPPORTED, "%s: K=%lld > %d", who, (long long)K, tspn::kRowTopkMaxK);
  TSPN_REQUIRE(topk_per_seg <= tspn::kSelectMaxM, TSPN_EUNSUPPORTED, "%s: topk_per_seg=%lld > %d", who,
               (long long)topk_per_seg, tspn::kSelectMaxM);
  TSPN_REQUIRE(J <= MAX_J, TSPN_EUNSUPPORTED, "%s: spans_per_pair J=%lld > %d", who, (long long)J, MAX_J);
  *R = std::min<int64_t>(topk_per_span, K);
  TSPN_REQUIRE(P * J * *R < (1LL << 31), TSPN_EUNSUPPORTED, "%s: P*J*topk_per_span = %lld candidates per segment", who,
               (long long)(P * J * *R));
  return TSPN_OK;
}

extern "C" size_t tspn_decode_span_relations_workspace_bytes(int64_t S, int64_t N, int64_t T, int64_t D, int64_t P,
                                                             int64_t J, int64_t K, int64_t topk_per_span) {
  if (S <= 0 || N <= 0 || T <= 0 || D <= 0 || P <= 0 || J <= 0 || K <= 0 || topk_per_span <= 0) return 0;
  if (K > tspn::kRowTopkMaxK || J > MAX_J || S >= (1LL << 31) || P >= (1LL << 31)) return 0;     // what the entry refuses
  const int64_t R = std::min<int64_t>(topk_per_span, K);
  if (P * J * R >= (1LL << 31)) return 0;
  return tspn::align_up(tspn::span_prefix_workspace_bytes(S * N, T, D, K), 256) + 3 * span_cand_bytes(S, P, J, R);
}

extern "C" int tspn_decode_span_relations_f32(const float* feats, int64_t S, int64_t N, int64_t T, int64_t D,
                                              const int64_t* pairs, int64_t P, const int64_t* spans,
                                              const float* span_scores, const int64_t* span_counts, int64_t J,
                                              const float* cls_w, const float* cls_b, int64_t K,
                                              const float* cls_logits, int64_t NO, int64_t topk_per_span,
                                              int64_t topk_per_seg, float* out_score, int64_t* out_triplet,
                                              int64_t* out_pair_tid, int64_t* out_span, int64_t* out_span_rank,
                                              int64_t* out_valid, void* workspace, size_t workspace_bytes,
                                              void* stream) {
  const char* who = "tspn_decode_span_relations_f32";
  int64_t R;
  if (int rc = tspn::span_relation_sizes(who, S, N, T, D, P, J, K, NO, topk_per_span, topk_per_seg)) return rc;
  if (int rc = tspn::span_relation_limits(who, P, J, K, topk_per_span, topk_per_seg, &R)) return rc;
  if (S == 0 || P == 0) return TSPN_OK;
  TSPN_REQUIRE(N > 0, TSPN_EINVAL, "%s: pairs without tracklets", who);
  TSPN_REQUIRE(feats && pairs && spans && span_scores && span_counts && cls_w && cls_logits && out_score &&
                   out_triplet && out_pair_tid && out_span && out_span_rank && out_valid,
               TSPN_EINVAL, "%s: null pointer", who);
  const size_t pre = tspn::align_up(tspn::span_prefix_workspace_bytes(S * N, T, D, K), 256);
  const size_t cb = span_cand_bytes(S, P, J, R);
  TSPN_REQUIRE(workspace && workspace_bytes >= pre + 3 * cb, TSPN_EWORKSPACE, "%s: workspace %zu < %zu bytes", who,
               workspace_bytes, pre + 3 * cb);
  const int64_t rows = S * P * J;
  const int64_t nb = tspn::ceil_div(rows, 4);
  TSPN_REQUIRE(nb < (1LL << 31), TSPN_EUNSUPPORTED, "%s: grid too large", who);
  const float* G = nullptr;
  const double* PS = nullptr;
  int rc = tspn::span_prefix_stage(feats, S * N, T, D, cls_w, K, workspace, pre, stream, &G, &PS, who);
  if (rc) return rc;
  char* ws = static_cast<char*>(workspace) + pre;
  unsigned* key = reinterpret_cast<unsigned*>(ws);
  float* sc = reinterpret_cast<float*>(ws + cb);
  int* ix = reinterpret_cast<int*>(ws + 2 * cb);
  hipStream_t s = TSPN_STREAM(stream);
  hipLaunchKernelGGL(span_row_topk_kernel, dim3((unsigned)nb), dim3(256), 0, s, PS, G, pairs, spans, span_scores,
                     span_counts, cls_b, rows, (int)N, (int)P, (int)J, (int)T, (int)K, (int)R, key, sc, ix);
  if ((rc = tspn::check_launch("tspn_decode_span_relations_f32(rows)"))) return rc;
  return tspn::segment_span_topk(key, sc, ix, pairs, spans, span_counts, cls_logits, S, N, NO, P, J, R, topk_per_seg,
                                 out_score, out_triplet, out_pair_tid, out_span, out_span_rank, out_valid, stream,
                                 "tspn_decode_span_relations_f32(segment)");
}
