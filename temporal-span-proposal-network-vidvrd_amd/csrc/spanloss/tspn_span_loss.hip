// Training targets and losses of the span heads (gfx950): anchor labels from ground-truth spans, the relationness and
// span-regression losses, and their gradient with respect to the heads.
//
// Semantics (DESIGN.md 2 "span training targets and losses"; the inverse of tspn_decode_spans_f32's parametrisation).
// Everything is float64 arithmetic on the fp32 heads, the fp32 anchor widths and the integer spans, one operation per
// step (the build has -ffp-contract=off).  One call serves one segment of P pairs, A anchors per frame, T frames:
//   anchor (t, a) = [t - size_a / 2, t + size_a / 2), unclipped; element (p, a, t) of label / matched / mask sits at
//   (p A + a) T + t, beside heads row a of the pair;
//   iou(anchor, row [gs, ge)) = inter / ((hi - lo) + (ge - gs) - inter), inter = max(0, min(hi, ge) - max(lo, gs));
//   a row with ge <= gs is padding.
//
//   span_anchor_labels_kernel   one wave per pair.  Pass 1: every lane walks the pair's A T anchors 64 apart and keeps, per
//                               ground-truth row, the largest IoU it saw; a wave max over the bit patterns (IoUs are >= +0,
//                               so the unsigned order is the value order) gives the row maxima.  Pass 2 forms the same
//                               IoUs again (the same device function: the same bits) and writes label and matched.
//   span_loss_f32_kernel        one wave per pair: the un-normalised gradient of every head element (0 where the element
//                               enters no loss) and the pair's four partial sums, lanes summed in anchor order, then the
//                               xor butterfly 32, 16, .., 1.
//   span_loss_finish_kernel     one workgroup: thread i adds the pairs i, i + 256, .. in order, then an LDS tree; out =
//                               (sum bce / max(1, n_lab), sum sl1 / max(1, n_pos), n_lab, n_pos).
//   span_loss_scale_kernel      dheads[p, r, t] /= max(1, n_lab) for r < A, max(1, n_pos) for r >= A; n read from `out` on
//                               the device.
// The anchors are walked in memory order ((a, t), t fastest) so that a wave's loads and stores are contiguous; nothing
// depends on the order but the summation order of the partial sums, which is fixed by it.
#include <cmath>

#include "tspn_common.h"

namespace {

constexpr int MAX_G = 8;      // ground-truth rows per pair (matched is int8; the rows live in registers)
constexpr int MAX_A = 16;     // anchors per location (the widths travel in the launch)
constexpr int WAVES = 4;      // pairs per workgroup
constexpr int FIN_THREADS = 256;

struct AnchorSizes {
  float v[MAX_A];
};

// the G rows of pair p as doubles; bit g of the result = row g is ground truth (ge > gs)
__device__ __forceinline__ unsigned load_gt(const int64_t* __restrict__ gt, int64_t p, int G, double (&gs)[MAX_G],
                                            double (&ge)[MAX_G]) {
  unsigned valid = 0;
#pragma unroll
  for (int g = 0; g < MAX_G; ++g) {
    gs[g] = 0.0;
    ge[g] = 0.0;
    if (g < G) {
      const int64_t s = gt[(p * G + g) * 2], e = gt[(p * G + g) * 2 + 1];
      gs[g] = (double)s;
      ge[g] = (double)e;
      if (e > s) valid |= 1u << g;
    }
  }
  return valid;
}

// IoU of anchor (t, size) with row [gs, ge); both passes of the labels kernel go through here
__device__ __forceinline__ double anchor_iou(int t, double size, double gs, double ge) {
  const double half = size / 2.0;
  const double lo = (double)t - half, hi = (double)t + half;
  const double a = hi < ge ? hi : ge, b = lo > gs ? lo : gs;
  const double d = a - b;
  const double inter = d > 0.0 ? d : 0.0;
  const double uni = (hi - lo) + (ge - gs) - inter;
  return inter / uni;
}

__global__ __launch_bounds__(64 * WAVES) void span_anchor_labels_kernel(const int64_t* __restrict__ gt, AnchorSizes sizes,
                                                                        int64_t P, int G, int A, int T, double pos_iou,
                                                                        double neg_iou, int8_t* __restrict__ label,
                                                                        int8_t* __restrict__ matched) {
  const int lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (p >= P) return;                                      // the whole wave; there is no barrier below
  const unsigned AT = (unsigned)A * (unsigned)T;           // < 2^31 (the entries check): e + 64 below stays below 2^32
  double gs[MAX_G], ge[MAX_G];
  const unsigned valid = load_gt(gt, p, G, gs, ge);        // wave-uniform
  int8_t* lab = label + p * (int64_t)AT;
  int8_t* mat = matched + p * (int64_t)AT;
  if (valid == 0) {                                        // a pair without ground truth: every anchor negative
    for (unsigned e = lane; e < AT; e += 64) {
      lab[e] = 0;
      mat[e] = -1;
    }
    return;
  }
  double rowmax[MAX_G];
#pragma unroll
  for (int g = 0; g < MAX_G; ++g) rowmax[g] = 0.0;
  for (unsigned e = lane; e < AT; e += 64) {
    const int a = (int)(e / (unsigned)T), t = (int)(e - (unsigned)a * (unsigned)T);
    const double size = (double)sizes.v[a];
#pragma unroll
    for (int g = 0; g < MAX_G; ++g) {
      if (valid >> g & 1) {
        const double v = anchor_iou(t, size, gs[g], ge[g]);
        rowmax[g] = v > rowmax[g] ? v : rowmax[g];
      }
    }
  }
#pragma unroll
  for (int g = 0; g < MAX_G; ++g)
    rowmax[g] = __longlong_as_double((long long)tspn::wave_max_u64((unsigned long long)__double_as_longlong(rowmax[g])));
  for (unsigned e = lane; e < AT; e += 64) {
    const int a = (int)(e / (unsigned)T), t = (int)(e - (unsigned)a * (unsigned)T);
    const double size = (double)sizes.v[a];
    double best = -1.0;
    int bg = -1;
    bool low = false;
#pragma unroll
    for (int g = 0; g < MAX_G; ++g) {
      if (valid >> g & 1) {
        const double v = anchor_iou(t, size, gs[g], ge[g]);
        if (v > best) {                                    // strictly: the lower g keeps a tie
          best = v;
          bg = g;
        }
        low = low || (rowmax[g] > 0.0 && v == rowmax[g]);
      }
    }
    int8_t l = best >= pos_iou ? 1 : (best < neg_iou ? 0 : -1);
    if (low) l = 1;
    lab[e] = l;
    mat[e] = (int8_t)bg;
  }
}

// the sum over the wave in every lane: partners 32, 16, 8, 4, 2, 1 apart, the same tree in every launch
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// smooth L1 of d with its derivative; a NaN d gives NaN for both
__device__ __forceinline__ double smooth_l1(double d, double beta, double& grad) {
  const double ad = fabs(d);
  if (ad < beta) {
    grad = d / beta;
    return 0.5 * d * d / beta;
  }
  grad = d != d ? d : (d > 0.0 ? 1.0 : -1.0);
  return ad - 0.5 * beta;
}

__global__ __launch_bounds__(64 * WAVES) void span_loss_f32_kernel(const float* __restrict__ heads,
                                                                   const int64_t* __restrict__ gt, AnchorSizes sizes,
                                                                   const int8_t* __restrict__ label,
                                                                   const int8_t* __restrict__ matched,
                                                                   const uint8_t* __restrict__ mask, int64_t P, int G,
                                                                   int A, int T, double beta,
                                                                   double* __restrict__ partials,
                                                                   float* __restrict__ dheads) {
  const int lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (p >= P) return;                                      // the whole wave; there is no barrier below
  const unsigned AT = (unsigned)A * (unsigned)T;
  double gs[MAX_G], ge[MAX_G];
  const unsigned valid = load_gt(gt, p, G, gs, ge);
  const float* h = heads + p * 3 * (int64_t)AT;
  float* dh = dheads + p * 3 * (int64_t)AT;
  double bce = 0.0, sl1 = 0.0;
  int nlab = 0, npos = 0;
  for (unsigned e = lane; e < AT; e += 64) {
    const int a = (int)(e / (unsigned)T), t = (int)(e - (unsigned)a * (unsigned)T);
    const int l = label[p * (int64_t)AT + e];
    const bool on = mask == nullptr || mask[p * (int64_t)AT + e] != 0;
    float gx = 0.f, gc = 0.f, gw = 0.f;
    if (on && (l == 0 || l == 1)) {
      const double x = (double)h[e];
      const double y = (double)l;
      bce += (x > 0.0 ? x : 0.0) - x * y + log1p(exp(-fabs(x)));
      ++nlab;
      // sigmoid(x) - y without the cancellation at y = 1: -sigmoid(-x)
      gx = (float)(l == 1 ? -1.0 / (1.0 + exp(x)) : 1.0 / (1.0 + exp(-x)));
    }
    const int m = matched[p * (int64_t)AT + e];
    if (on && l == 1 && m >= 0 && m < G && (valid >> m & 1)) {
      double s = 0.0, f = 0.0;
#pragma unroll
      for (int g = 0; g < MAX_G; ++g) {                    // a select, not an indexed read: the rows stay in registers
        s = g == m ? gs[g] : s;
        f = g == m ? ge[g] : f;
      }
      const double size = (double)sizes.v[a];
      const double tc = ((s + f) / 2.0 - (double)t) / size;
      const double tw = log((f - s) / size);
      double dc, dw;
      sl1 += smooth_l1((double)h[(int64_t)(A + 2 * a) * T + t] - tc, beta, dc);
      sl1 += smooth_l1((double)h[(int64_t)(A + 2 * a + 1) * T + t] - tw, beta, dw);
      ++npos;
      gc = (float)dc;
      gw = (float)dw;
    }
    dh[e] = gx;
    dh[(int64_t)(A + 2 * a) * T + t] = gc;
    dh[(int64_t)(A + 2 * a + 1) * T + t] = gw;
  }
  bce = wave_sum(bce);
  sl1 = wave_sum(sl1);
  const double nl = wave_sum((double)nlab), np = wave_sum((double)npos);
  if (lane == 0) {
    partials[p * 4 + 0] = bce;
    partials[p * 4 + 1] = nl;
    partials[p * 4 + 2] = sl1;
    partials[p * 4 + 3] = np;
  }
}

__global__ __launch_bounds__(FIN_THREADS) void span_loss_finish_kernel(const double* __restrict__ partials, int64_t P,
                                                                       double* __restrict__ out) {
  __shared__ double acc[4][FIN_THREADS];
  const int i = threadIdx.x;
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t p = i; p < P; p += FIN_THREADS) {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] += partials[p * 4 + k];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) acc[k][i] = v[k];
  __syncthreads();
  for (int o = FIN_THREADS / 2; o > 0; o >>= 1) {
    if (i < o) {
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[k][i] += acc[k][i + o];
    }
    __syncthreads();
  }
  if (i == 0) {
    const double nl = acc[1][0], np = acc[3][0];
    out[0] = acc[0][0] / (nl > 1.0 ? nl : 1.0);
    out[1] = acc[2][0] / (np > 1.0 ? np : 1.0);
    out[2] = nl;
    out[3] = np;
  }
}

__global__ __launch_bounds__(256) void span_loss_scale_kernel(const double* __restrict__ out, int64_t total, int A, int T,
                                                              float* __restrict__ dheads) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int r = (int)((i / T) % (3 * A));
  const double n = r < A ? out[2] : out[3];
  dheads[i] = (float)((double)dheads[i] / (n > 1.0 ? n : 1.0));
}

// the shape checks the three entries share: sizes first, then what the kernels' registers and 32-bit anchor index hold
int shape_checks(const char* who, int64_t P, int64_t A, int64_t T) {
  TSPN_REQUIRE(P >= 0 && A >= 1 && T >= 1, TSPN_EINVAL, "%s: bad sizes P=%lld A=%lld T=%lld", who, (long long)P, (long long)A,
               (long long)T);
  TSPN_REQUIRE(A <= MAX_A, TSPN_EUNSUPPORTED, "%s: A=%lld > %d", who, (long long)A, MAX_A);
  TSPN_REQUIRE(T < (1LL << 31) && A * T < (1LL << 31), TSPN_EUNSUPPORTED, "%s: A*T = %lld anchors per pair (needs < 2^31)",
               who, (long long)(A * T));
  TSPN_REQUIRE(P < (1LL << 31) && P * 3 * A * T < (1LL << 39), TSPN_EUNSUPPORTED, "%s: problem too large", who);
  return TSPN_OK;
}

int gt_checks(const char* who, int64_t G) {
  TSPN_REQUIRE(G >= 0, TSPN_EINVAL, "%s: bad sizes G=%lld", who, (long long)G);
  TSPN_REQUIRE(G <= MAX_G, TSPN_EUNSUPPORTED, "%s: G=%lld > %d", who, (long long)G, MAX_G);
  return TSPN_OK;
}

int load_sizes(const char* who, const float* sizes_host, int64_t A, AnchorSizes& out) {
  TSPN_REQUIRE(sizes_host, TSPN_EINVAL, "%s: null pointer", who);
  for (int a = 0; a < MAX_A; ++a) out.v[a] = 1.f;
  for (int64_t a = 0; a < A; ++a) {
    TSPN_REQUIRE(sizes_host[a] > 0.f && std::isfinite(sizes_host[a]), TSPN_EINVAL, "%s: anchor size %lld is not positive",
                 who, (long long)a);
    out.v[a] = sizes_host[a];
  }
  return TSPN_OK;
}

}  // namespace

extern "C" int tspn_span_anchor_labels(const int64_t* gt, const float* sizes_host, int64_t P, int64_t G, int64_t A, int64_t T,
                                       double pos_iou, double neg_iou, int8_t* label, int8_t* matched, void* stream) {
  const char* who = "tspn_span_anchor_labels";
  int rc = shape_checks(who, P, A, T);
  if (rc || (rc = gt_checks(who, G))) return rc;
  TSPN_REQUIRE(0.0 <= neg_iou && neg_iou <= pos_iou && pos_iou <= 1.0, TSPN_EINVAL,
               "%s: thresholds need 0 <= neg_iou <= pos_iou <= 1 (got %g, %g)", who, neg_iou, pos_iou);
  AnchorSizes sz;
  if ((rc = load_sizes(who, sizes_host, A, sz))) return rc;
  if (P == 0) return TSPN_OK;
  TSPN_REQUIRE((gt || G == 0) && label && matched, TSPN_EINVAL, "%s: null pointer", who);
  TSPN_REQUIRE((reinterpret_cast<uintptr_t>(gt) & 7) == 0, TSPN_EUNSUPPORTED, "%s: unaligned pointer (gt needs 8 bytes)", who);
  hipLaunchKernelGGL(span_anchor_labels_kernel, dim3((unsigned)tspn::ceil_div(P, WAVES)), dim3(64 * WAVES), 0,
                     TSPN_STREAM(stream), gt, sz, P, (int)G, (int)A, (int)T, pos_iou, neg_iou, label, matched);
  return tspn::check_launch(who);
}

extern "C" int tspn_span_loss_f32(const float* heads, const int64_t* gt, const float* sizes_host, const int8_t* label,
                                  const int8_t* matched, const uint8_t* mask, int64_t P, int64_t G, int64_t A, int64_t T,
                                  double beta, double* partials, float* dheads, void* stream) {
  const char* who = "tspn_span_loss_f32";
  int rc = shape_checks(who, P, A, T);
  if (rc || (rc = gt_checks(who, G))) return rc;
  TSPN_REQUIRE(beta > 0.0 && std::isfinite(beta), TSPN_EINVAL, "%s: beta = %g is not positive", who, beta);
  AnchorSizes sz;
  if ((rc = load_sizes(who, sizes_host, A, sz))) return rc;
  if (P == 0) return TSPN_OK;
  TSPN_REQUIRE(heads && (gt || G == 0) && label && matched && partials && dheads, TSPN_EINVAL, "%s: null pointer", who);
  TSPN_REQUIRE((reinterpret_cast<uintptr_t>(gt) & 7) == 0 && (reinterpret_cast<uintptr_t>(partials) & 7) == 0 &&
                   (reinterpret_cast<uintptr_t>(heads) & 3) == 0 && (reinterpret_cast<uintptr_t>(dheads) & 3) == 0,
               TSPN_EUNSUPPORTED, "%s: unaligned pointer", who);
  hipLaunchKernelGGL(span_loss_f32_kernel, dim3((unsigned)tspn::ceil_div(P, WAVES)), dim3(64 * WAVES), 0, TSPN_STREAM(stream),
                     heads, gt, sz, label, matched, mask, P, (int)G, (int)A, (int)T, beta, partials, dheads);
  return tspn::check_launch(who);
}

extern "C" int tspn_span_loss_finish(const double* partials, int64_t P, int64_t A, int64_t T, double* out, float* dheads,
                                     void* stream) {
  const char* who = "tspn_span_loss_finish";
  int rc = shape_checks(who, P, A, T);
  if (rc) return rc;
  TSPN_REQUIRE(out && (P == 0 || (partials && dheads)), TSPN_EINVAL, "%s: null pointer", who);
  TSPN_REQUIRE((reinterpret_cast<uintptr_t>(out) & 7) == 0 && (reinterpret_cast<uintptr_t>(partials) & 7) == 0 &&
                   (reinterpret_cast<uintptr_t>(dheads) & 3) == 0,
               TSPN_EUNSUPPORTED, "%s: unaligned pointer", who);
  hipLaunchKernelGGL(span_loss_finish_kernel, dim3(1), dim3(FIN_THREADS), 0, TSPN_STREAM(stream), partials, P, out);
  if ((rc = tspn::check_launch("tspn_span_loss_finish(reduce)"))) return rc;
  if (P == 0) return TSPN_OK;
  const int64_t total = P * 3 * A * T;
  hipLaunchKernelGGL(span_loss_scale_kernel, dim3((unsigned)tspn::ceil_div(total, 256)), dim3(256), 0, TSPN_STREAM(stream),
                     out, total, (int)A, (int)T, dheads);
  return tspn::check_launch("tspn_span_loss_finish(scale)");
}
