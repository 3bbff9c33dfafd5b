// Span pooling, the per-(row, predicate) expression: shared by span_combine_kernel (tspn_linear.hip) and
// span_row_topk_kernel (relations/tspn_span_relations.hip), which must return the same fp32 bits; and the
// row rewrite span_frames, which the bf16 span path (spanbf16/tspn_span_bf16.hip) takes from here too.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace tspn {

// The frames [a, e) a span row (a0, e0) pools over on a segment of T frames (oracle.span_frames):
// out-of-range / unused (-1) spans fall back to the whole segment / one frame, so 0 <= a < e <= T for any row.
__device__ inline void span_frames(int64_t a0, int64_t e0, int T, int64_t& a, int64_t& e) {
  a = a0 < 0 ? 0 : (a0 > T - 1 ? T - 1 : a0);
  e = e0 < a + 1 ? (a0 < 0 ? T : a + 1) : (e0 > T ? T : e0);
}

// Sum of G over the frames [a, e) of one (tracklet, column) in float64, in frame order: what PS[e] - PS[a] is when
// both are finite.  span_logit takes it when the running sum of span_prefix_kernel has met a NaN / Inf in an
// EARLIER or inner frame: every later prefix value is non-finite then, although the span's own frames may all be finite.
__device__ inline double span_sum_frames(const float* __restrict__ g, int64_t K2, int64_t a, int64_t e) {
  double acc = 0.0;
  for (int64_t t = a; t < e; ++t) acc += (double)g[t * K2];
  return acc;
}

// The float64 value span_logit passes through the sigmoid: the mean over the frames of span (a0, e0) of
// G[s, :, 2k] + G[o, :, 2k+1], + b[k], of global tracklets (s, o); PS [NT, T+1, 2K] float64 prefix sums of G [NT, T, 2K]
// over time.  The span-pooled training loss (spancls/tspn_span_cls.hip) takes its loss and gradient from this value.
__device__ inline double span_value(const double* __restrict__ PS, const float* __restrict__ G, int64_t s, int64_t o,
                                    int64_t a0, int64_t e0, int T, int64_t K2, int64_t k,
                                    const float* __restrict__ b) {
  int64_t a, e;
  span_frames(a0, e0, T, a, e);
  const double* ps = PS + (s * (T + 1)) * K2 + 2 * k;
  const double* po = PS + (o * (T + 1)) * K2 + 2 * k + 1;
  // a prefix value is non-finite from the first NaN / Inf frame on (PS[a] non-finite implies PS[e] non-finite), so
  // PS[e] alone tells whether the difference is usable; finite prefixes keep the difference and its bits
  double ds = ps[e * K2] - ps[a * K2];
  double dob = po[e * K2] - po[a * K2];
  if (!isfinite(ps[e * K2])) ds = span_sum_frames(G + (s * T) * K2 + 2 * k, K2, a, e);
  if (!isfinite(po[e * K2])) dob = span_sum_frames(G + (o * T) * K2 + 2 * k + 1, K2, a, e);
  double v = (ds + dob) / (double)(e - a);
  if (b != nullptr) v += (double)b[k];
  return v;
}

// sigmoid of span_value, rounded to fp32: what span pooling returns per (row, predicate)
__device__ inline float span_logit(const double* __restrict__ PS, const float* __restrict__ G, int64_t s, int64_t o,
                                   int64_t a0, int64_t e0, int T, int64_t K2, int64_t k,
                                   const float* __restrict__ b) {
  const double v = span_value(PS, G, s, o, a0, e0, T, K2, k, b);
  return (float)(1.0 / (1.0 + exp(-v)));
}

}  // namespace tspn
