// Video relation detection evaluation: vIoU of every (prediction, same-triplet ground truth) pair and the greedy
// match of the reference's eval_detection_scores (lib/evaluation/visual_relation_detection.py:8-36,
// common.py:65-106), in float64 with the reference's operation order (gfx950).
//
// The host (evaluation.py) packs a chunk of videos into
//   boxes [F, 4] float64          every packed trajectory's boxes, one after the other
//   traj  [T, 3] int64            per trajectory: (first row in `boxes`, duration begin, duration end); relation r's
//                                 subject trajectory is 2r, its object trajectory 2r + 1
//   groups [G, 5] int64           per (video, triplet) group: (first prediction relation, number of predictions,
//                                 first ground-truth relation, number of ground truths, offset of its ov block)
//   pred_group [P] int32          the group of prediction relation p (predictions are relations 0 .. P-1, in
//                                 score order inside their group; ground truths follow)
// and the ov block of a group is n_pred x n_gt, row-major.
//
// Bit-equality with the reference rests on keeping its sums sequential: the overlap volume is summed in frame order
// over the common frames, each trajectory's volume in frame order over all its boxes (factors not clamped), and
// vIoU = v_ov / ((v1 + v2) - v_ov).  The library is built with -ffp-contract=off.  Python's max / min / `>` are
// restated exactly (which operand wins on equality), so even the sign of a zero follows the reference.
#include <climits>

#include "tspn_common.h"

namespace {

constexpr int kWave = 64;
constexpr int64_t kRegMaskMaxGt = 64 * kWave;   // detected flags of up to 4096 ground truths fit one 64-bit register

// Python's max(a, b) / min(a, b): the first argument unless the second compares strictly greater / smaller.
__device__ inline double py_max(double a, double b) { return b > a ? b : a; }
__device__ inline double py_min(double a, double b) { return b < a ? b : a; }

__device__ inline int64_t wave_min_i64(int64_t v) {
  for (int m = 32; m >= 1; m >>= 1) v = min(v, (int64_t)__shfl_xor((long long)v, m));
  return v;
}

__device__ inline int64_t wave_max_i64(int64_t v) {
  for (int m = 32; m >= 1; m >>= 1) v = max(v, (int64_t)__shfl_xor((long long)v, m));
  return v;
}

// A total order on finite doubles as signed integers (negative values flipped below the positive ones); the two
// zeros compare equal in the reference, so -0 is folded onto +0 first.
__device__ inline int64_t order_key(double v) {
  if (v == 0.0) v = 0.0;
  const int64_t b = __double_as_longlong(v);
  return b >= 0 ? b : (b ^ LLONG_MAX);
}

// ---- 1. v = sum over a trajectory's boxes of (x2 - x1 + 1) * (y2 - y1 + 1), in frame order (common.py:100-105)
__global__ __launch_bounds__(256) void eval_traj_volume_f64_kernel(const double* __restrict__ boxes,
                                                                   const int64_t* __restrict__ traj, int64_t n_traj,
                                                                   double* __restrict__ vol) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_traj) return;
  const double* b = boxes + 4 * traj[3 * t];
  const int64_t n = traj[3 * t + 2] - traj[3 * t + 1];
  double v = 0.0;
  for (int64_t f = 0; f < n; ++f) {
    const double4 q = *reinterpret_cast<const double4*>(b + 4 * f);
    v += ((q.z - q.x) + 1.0) * ((q.w - q.y) + 1.0);
  }
  vol[t] = v;
}

// ---- 2. ov = min(viou(subjects), viou(objects)) for every (prediction, same-triplet ground truth) pair.
// One wave per prediction, one lane per ground truth (64 at a time).  The prediction's boxes are wave-uniform and
// read once per frame for all lanes; the wave walks the union of its lanes' common frames in ascending order and a
// lane adds only inside its own, so each lane's sum runs in the reference's order.
__global__ __launch_bounds__(256) void eval_viou_f64_kernel(const double* __restrict__ boxes,
                                                            const int64_t* __restrict__ traj,
                                                            const double* __restrict__ vol,
                                                            const int64_t* __restrict__ groups,
                                                            const int32_t* __restrict__ pred_group, int64_t n_pred,
                                                            double* __restrict__ ov, int32_t* __restrict__ zden) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t p = (int64_t)blockIdx.x * (blockDim.x / kWave) + (threadIdx.x / kWave);
  if (p >= n_pred) return;   // wave-uniform
  const int64_t* g = groups + 5 * (int64_t)pred_group[p];
  const int64_t p0 = g[0], gt0 = g[2], ngt = g[3];
  double* row = ov + g[4] + (p - p0) * ngt;
  bool zero_den = false;
  for (int64_t j0 = 0; j0 < ngt; j0 += kWave) {
    const int64_t j = j0 + lane;
    const bool live = j < ngt;
    const int64_t r = gt0 + (live ? j : 0);
    double iou[2];
    for (int k = 0; k < 2; ++k) {
      const int64_t tp = 2 * p + k, tg = 2 * r + k;
      const int64_t off1 = traj[3 * tp], b1 = traj[3 * tp + 1], e1 = traj[3 * tp + 2];
      const int64_t off2 = traj[3 * tg], b2 = traj[3 * tg + 1], e2 = traj[3 * tg + 2];
      const bool overlap = live && !(b1 >= e2 || e1 <= b2);
      const int64_t lo = overlap ? max(b1, b2) : LLONG_MAX;
      const int64_t hi = overlap ? min(e1, e2) : LLONG_MIN;
      const int64_t wlo = wave_min_i64(lo), whi = wave_max_i64(hi);
      const double* pb = boxes + 4 * (off1 - b1);   // row of frame f: pb + 4 f
      const double* qb = boxes + 4 * (off2 - b2);
      double v_ov = 0.0;
      for (int64_t f = wlo; f < whi; ++f) {
        const double4 a = *reinterpret_cast<const double4*>(pb + 4 * f);
        if (f >= lo && f < hi) {
          const double4 c = *reinterpret_cast<const double4*>(qb + 4 * f);
          const double left = py_max(a.x, c.x), top = py_max(a.y, c.y);
          const double right = py_min(a.z, c.z), bottom = py_min(a.w, c.w);
          const double w = (right - left) + 1.0, h = (bottom - top) + 1.0;
          v_ov += (w > 0.0 ? w : 0.0) * (h > 0.0 ? h : 0.0);
        }
      }
      double res = 0.0;
      if (overlap) {
        const double den = (vol[tp] + vol[tg]) - v_ov;
        zero_den |= den == 0.0;
        res = v_ov / den;
      }
      iou[k] = res;
    }
    if (live) row[j] = py_min(iou[0], iou[1]);
  }
  const bool any_zero = __ballot(zero_den) != 0;
  if (lane == 0) zden[p] = any_zero ? 1 : 0;
}

// ---- 3. the greedy match: predictions of a group in score order; each takes the undetected ground truth of the
// largest ov >= threshold, the lowest index on a tie (strict `ov > ov_max`), which becomes detected.
// One wave per group.  kRegMask: groups of up to 4096 ground truths keep the detected flags in a register, bit c of
// lane l = ground truth 64 c + l; larger groups keep one byte per ground truth in `det_ws` (zeroed by the caller).
template <bool kRegMask>
__global__ __launch_bounds__(256) void eval_greedy_match_kernel(const double* __restrict__ ov,
                                                                const int64_t* __restrict__ groups, int64_t n_groups,
                                                                double threshold, uint8_t* __restrict__ det_ws,
                                                                int8_t* __restrict__ hit, int32_t* __restrict__ match) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t gi = (int64_t)blockIdx.x * (blockDim.x / kWave) + (threadIdx.x / kWave);
  if (gi >= n_groups) return;   // wave-uniform
  const int64_t* g = groups + 5 * gi;
  const int64_t p0 = g[0], npred = g[1], gt0 = g[2], ngt = g[3];
  if ((ngt <= kRegMaskMaxGt) != kRegMask) return;   // the other instantiation owns this group
  const double* blk = ov + g[4];
  uint64_t det = 0;
  for (int64_t q = 0; q < npred; ++q) {
    const double* row = blk + q * ngt;
    int64_t best_key = LLONG_MIN, best = -1;
    for (int64_t c = 0; c * kWave < ngt; ++c) {
      const int64_t j = c * kWave + lane;
      int64_t key = LLONG_MIN;
      if (j < ngt) {
        const bool done = kRegMask ? ((det >> c) & 1) != 0 : det_ws[gt0 + j] != 0;
        if (!done) {
          const double v = row[j];
          if (v >= threshold) key = order_key(v);
        }
      }
      const int64_t m = wave_max_i64(key);
      if (m > best_key) {   // strict: an earlier chunk keeps a tie
        best_key = m;
        best = c * kWave + (__ffsll((unsigned long long)__ballot(key == m)) - 1);
      }
    }
    if (best >= 0 && lane == (best & (kWave - 1))) {
      if (kRegMask)
        det |= 1ull << (best / kWave);
      else
        det_ws[gt0 + best] = 1;
    }
    if (lane == 0) {
      hit[p0 + q] = best >= 0 ? 1 : 0;
      match[p0 + q] = (int32_t)best;
    }
  }
}

}  // namespace

extern "C" int tspn_eval_traj_volume_f64(const double* boxes, const int64_t* traj, int64_t n_traj, double* vol,
                                         void* stream) {
  TSPN_REQUIRE(n_traj >= 0, TSPN_EINVAL, "tspn_eval_traj_volume_f64: bad sizes");
  if (n_traj == 0) return TSPN_OK;
  TSPN_REQUIRE(boxes && traj && vol, TSPN_EINVAL, "tspn_eval_traj_volume_f64: null pointer");
  TSPN_REQUIRE((reinterpret_cast<uintptr_t>(boxes) & 31) == 0, TSPN_EINVAL,
               "tspn_eval_traj_volume_f64: boxes must be 32-byte aligned");
  TSPN_REQUIRE(n_traj < ((int64_t)1 << 31) * 256, TSPN_EUNSUPPORTED, "tspn_eval_traj_volume_f64: too many trajectories");
  hipLaunchKernelGGL(eval_traj_volume_f64_kernel, dim3((unsigned)tspn::ceil_div(n_traj, 256)), dim3(256), 0,
                     TSPN_STREAM(stream), boxes, traj, n_traj, vol);
  return tspn::check_launch("tspn_eval_traj_volume_f64");
}

extern "C" int tspn_eval_viou_f64(const double* boxes, const int64_t* traj, const double* vol, const int64_t* groups,
                                  const int32_t* pred_group, int64_t n_pred, double* ov, int32_t* zden, void* stream) {
  TSPN_REQUIRE(n_pred >= 0, TSPN_EINVAL, "tspn_eval_viou_f64: bad sizes");
  if (n_pred == 0) return TSPN_OK;
  TSPN_REQUIRE(boxes && traj && vol && groups && pred_group && ov && zden, TSPN_EINVAL,
               "tspn_eval_viou_f64: null pointer");
  TSPN_REQUIRE((reinterpret_cast<uintptr_t>(boxes) & 31) == 0, TSPN_EINVAL,
               "tspn_eval_viou_f64: boxes must be 32-byte aligned");
  TSPN_REQUIRE(n_pred < ((int64_t)1 << 31) * 4, TSPN_EUNSUPPORTED, "tspn_eval_viou_f64: too many predictions");
  hipLaunchKernelGGL(eval_viou_f64_kernel, dim3((unsigned)tspn::ceil_div(n_pred, 4)), dim3(256), 0,
                     TSPN_STREAM(stream), boxes, traj, vol, groups, pred_group, n_pred, ov, zden);
  return tspn::check_launch("tspn_eval_viou_f64");
}

extern "C" int tspn_eval_greedy_match_f64(const double* ov, const int64_t* groups, int64_t n_groups,
                                          int64_t max_group_gt, double viou_threshold, uint8_t* det_ws, int8_t* hit,
                                          int32_t* match, void* stream) {
  TSPN_REQUIRE(n_groups >= 0 && max_group_gt >= 0, TSPN_EINVAL, "tspn_eval_greedy_match_f64: bad sizes");
  if (n_groups == 0) return TSPN_OK;
  TSPN_REQUIRE(ov && groups && hit && match, TSPN_EINVAL, "tspn_eval_greedy_match_f64: null pointer");
  TSPN_REQUIRE(max_group_gt <= kRegMaskMaxGt || det_ws, TSPN_EINVAL,
               "tspn_eval_greedy_match_f64: groups of more than 4096 ground truths need det_ws");
  TSPN_REQUIRE(n_groups < ((int64_t)1 << 31) * 4, TSPN_EUNSUPPORTED, "tspn_eval_greedy_match_f64: too many groups");
  const dim3 grid((unsigned)tspn::ceil_div(n_groups, 4));
  hipLaunchKernelGGL(eval_greedy_match_kernel<true>, grid, dim3(256), 0, TSPN_STREAM(stream), ov, groups, n_groups,
                     viou_threshold, det_ws, hit, match);
  if (max_group_gt > kRegMaskMaxGt)
    hipLaunchKernelGGL(eval_greedy_match_kernel<false>, grid, dim3(256), 0, TSPN_STREAM(stream), ov, groups,
                       n_groups, viou_threshold, det_ws, hit, match);
  return tspn::check_launch("tspn_eval_greedy_match_f64");
}
