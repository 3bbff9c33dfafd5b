// Video object detection evaluation: the "tIoU" overlap of every (prediction, same-class ground truth) trajectory pair
// of a video and the first-claimant match of the reference's evaluate (lib/evaluation/video_object_detection.py:12-106,
// common.py:40-62), in float64 with the reference's operation order (gfx950).
//
// The host (evaluation_detection.py) packs a chunk of videos into
//   boxes  [F, 4] float64         one row per (trajectory, frame), a trajectory's rows one after the other
//   frames [F]    int32           the frame id of each row, ascending inside a trajectory (frame sets may have gaps)
//   traj   [T, 2] int64           per trajectory: (first row, number of rows); predictions are trajectories 0 .. P-1, in
//                                 score order inside their group; ground truths follow
//   groups [G, 5] int64           per (video, class) group: (first prediction, number of predictions, first ground-truth
//                                 trajectory, number of ground truths, offset of its n_pred x n_gt block in tiou)
//   pred_group [P] int32          the group of prediction p
//
// Bit-equality with the reference needs no summation order: per pair, the common frames and the frames whose sIoU
// reaches 0.5 / 0.7 / 0.9 are COUNTED (wave ballots), and tIoU = (top1 + top2 + top3) * 1.0 / (3 * total) is one float64
// division of two integers.  The sIoU of a frame is the reference's expression, operation for operation; the library is
// built with -ffp-contract=off.
#include <climits>

#include "tspn_common.h"

namespace {

constexpr int kWave = 64;
constexpr int kWavesPerBlock = 4;

// Python's max(a, b) / min(a, b): the first argument unless the second compares strictly greater / smaller.
__device__ inline double py_max(double a, double b) { return b > a ? b : a; }
__device__ inline double py_min(double a, double b) { return b < a ? b : a; }

__device__ inline int count64(bool v) { return __popcll((unsigned long long)__ballot(v)); }

// ---- 1. tIoU of every (prediction, group ground truth) pair, and per prediction the strict running maximum over the
// group's ground truths in index order (max_overlap / max_index start at 0 / 0: a tie keeps the lower index, an
// all-zero row keeps (0, 0)).  One wave per prediction; for each ground truth the lanes stride over the prediction's
// frames and look each one up in the ground truth's ascending frame ids by binary search.
__global__ __launch_bounds__(256) void evalobj_tiou_f64_kernel(const double* __restrict__ boxes,
                                                               const int32_t* __restrict__ frames,
                                                               const int64_t* __restrict__ traj,
                                                               const int64_t* __restrict__ groups,
                                                               const int32_t* __restrict__ pred_group, int64_t n_pred,
                                                               double* __restrict__ tiou, double* __restrict__ best,
                                                               int32_t* __restrict__ best_index,
                                                               int32_t* __restrict__ flags) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t p = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x / kWave);
  if (p >= n_pred) return;   // wave-uniform
  const int64_t* g = groups + 5 * (int64_t)pred_group[p];
  const int64_t p0 = g[0], gt0 = g[2], ngt = g[3];
  const int64_t prow = traj[2 * p], pn = traj[2 * p + 1];
  double max_overlap = 0.0;
  int64_t max_index = 0;
  int flag = 0;
  for (int64_t j = 0; j < ngt; ++j) {
    const int64_t grow = traj[2 * (gt0 + j)], gn = traj[2 * (gt0 + j) + 1];
    const int32_t* gf = frames + grow;
    int64_t common = 0, top1 = 0, top2 = 0, top3 = 0;
    bool zero_den = false;
    for (int64_t i0 = 0; i0 < pn; i0 += kWave) {   // whole waves: the ballots below are wave-uniform
      const int64_t i = i0 + lane;
      bool found = false;
      int64_t k = 0;
      if (i < pn) {
        const int32_t fid = frames[prow + i];
        int64_t lo = 0, hi = gn;                  // lower bound of fid in gf[0, gn)
        while (lo < hi) {
          const int64_t mid = lo + ((hi - lo) >> 1);
          if (gf[mid] < fid)
            lo = mid + 1;
          else
            hi = mid;
        }
        k = lo;
        found = lo < gn && gf[lo] == fid;
      }
      bool s1 = false, s2 = false, s3 = false, zd = false;
      if (found) {
        // iou(bbox_1 = ground truth, bbox_2 = prediction), common.py:40-62
        const double4 a = *reinterpret_cast<const double4*>(boxes + 4 * (grow + k));
        const double4 b = *reinterpret_cast<const double4*>(boxes + 4 * (prow + i));
        const double area_1 = ((a.z - a.x) + 1.0) * ((a.w - a.y) + 1.0);
        const double area_2 = ((b.z - b.x) + 1.0) * ((b.w - b.y) + 1.0);
        const double left = py_max(a.x, b.x), top = py_max(a.y, b.y);
        const double right = py_min(a.z, b.z), bottom = py_min(a.w, b.w);
        const double w = (right - left) + 1.0, h = (bottom - top) + 1.0;
        const double overlap = (w > 0.0 ? w : 0.0) * (h > 0.0 ? h : 0.0);
        const double den = (area_1 + area_2) - overlap;
        zd = den == 0.0;
        const double s = (overlap * 1.0) / den;
        s1 = s >= 0.5;
        s2 = s >= 0.7;
        s3 = s >= 0.9;
      }
      common += count64(found);
      top1 += count64(s1);
      top2 += count64(s2);
      top3 += count64(s3);
      zero_den |= __ballot(zd) != 0;
    }
    const int64_t total = pn + gn - common;
    double t = 0.0;
    if (total == 0)
      flag |= 2;
    else
      t = ((double)(top1 + top2 + top3) * 1.0) / (double)(3 * total);
    if (zero_den) flag |= 1;
    if (t > max_overlap) {
      max_overlap = t;
      max_index = j;
    }
    if (tiou != nullptr && lane == 0) tiou[g[4] + (p - p0) * ngt + j] = t;
  }
  if (lane == 0) {
    best[p] = max_overlap;
    best_index[p] = (int32_t)max_index;
    flags[p] = flag;
  }
}

// ---- 2. the match.  max_index does not depend on which ground truths are taken, so a prediction is a true positive
// iff it qualifies (best >= thresh_t, its group has a ground truth) and no earlier qualifying prediction of its group
// names the same ground truth: the smallest claiming position per ground truth wins (integer atomicMin, deterministic).
__global__ __launch_bounds__(256) void evalobj_claim_fill_kernel(int32_t* __restrict__ claim, int64_t n_gt) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_gt) claim[i] = INT_MAX;
}

// The claim slot of prediction p (ground truths are numbered from 0 in `claim`), or -1 when p does not qualify.
__device__ inline int64_t claim_slot(const double* best, const int32_t* best_index, const int64_t* groups,
                                     const int32_t* pred_group, int64_t p, int64_t n_pred, int64_t n_gt,
                                     double thresh_t, int32_t* pos) {
  const int64_t* g = groups + 5 * (int64_t)pred_group[p];
  const int64_t k = best_index[p];
  *pos = (int32_t)(p - g[0]);
  if (!(best[p] >= thresh_t) || k < 0 || k >= g[3]) return -1;
  const int64_t slot = g[2] - n_pred + k;
  return (slot >= 0 && slot < n_gt) ? slot : -1;
}

__global__ __launch_bounds__(256) void evalobj_claim_min_kernel(const double* __restrict__ best,
                                                                const int32_t* __restrict__ best_index,
                                                                const int64_t* __restrict__ groups,
                                                                const int32_t* __restrict__ pred_group, int64_t n_pred,
                                                                int64_t n_gt, double thresh_t,
                                                                int32_t* __restrict__ claim) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pred) return;
  int32_t pos;
  const int64_t slot = claim_slot(best, best_index, groups, pred_group, p, n_pred, n_gt, thresh_t, &pos);
  if (slot >= 0) atomicMin(claim + slot, pos);
}

__global__ __launch_bounds__(256) void evalobj_claim_hit_kernel(const double* __restrict__ best,
                                                                const int32_t* __restrict__ best_index,
                                                                const int64_t* __restrict__ groups,
                                                                const int32_t* __restrict__ pred_group, int64_t n_pred,
                                                                int64_t n_gt, double thresh_t,
                                                                const int32_t* __restrict__ claim,
                                                                int8_t* __restrict__ hit) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pred) return;
  int32_t pos;
  const int64_t slot = claim_slot(best, best_index, groups, pred_group, p, n_pred, n_gt, thresh_t, &pos);
  hit[p] = (slot >= 0 && claim[slot] == pos) ? 1 : 0;
}

}  // namespace

extern "C" int tspn_evalobj_tiou_f64(const double* boxes, const int32_t* frames, const int64_t* traj,
                                     const int64_t* groups, const int32_t* pred_group, int64_t n_pred, double* tiou,
                                     double* best, int32_t* best_index, int32_t* flags, void* stream) {
  TSPN_REQUIRE(n_pred >= 0, TSPN_EINVAL, "tspn_evalobj_tiou_f64: bad sizes n_pred=%lld", (long long)n_pred);
  if (n_pred == 0) return TSPN_OK;
  TSPN_REQUIRE(boxes && frames && traj && groups && pred_group && best && best_index && flags, TSPN_EINVAL,
               "tspn_evalobj_tiou_f64: null pointer");
  TSPN_REQUIRE((reinterpret_cast<uintptr_t>(boxes) & 31) == 0, TSPN_EINVAL,
               "tspn_evalobj_tiou_f64: boxes must be 32-byte aligned");
  TSPN_REQUIRE(n_pred < ((int64_t)1 << 31) * kWavesPerBlock, TSPN_EUNSUPPORTED,
               "tspn_evalobj_tiou_f64: too many predictions");
  hipLaunchKernelGGL(evalobj_tiou_f64_kernel, dim3((unsigned)tspn::ceil_div(n_pred, kWavesPerBlock)),
                     dim3(kWave * kWavesPerBlock), 0, TSPN_STREAM(stream), boxes, frames, traj, groups, pred_group,
                     n_pred, tiou, best, best_index, flags);
  return tspn::check_launch("tspn_evalobj_tiou_f64");
}

extern "C" int tspn_evalobj_claim(const double* best, const int32_t* best_index, const int64_t* groups,
                                  const int32_t* pred_group, int64_t n_pred, int64_t n_gt, double thresh_t,
                                  int32_t* claim, int8_t* hit, void* stream) {
  TSPN_REQUIRE(n_pred >= 0 && n_gt >= 0, TSPN_EINVAL, "tspn_evalobj_claim: bad sizes n_pred=%lld n_gt=%lld",
               (long long)n_pred, (long long)n_gt);
  if (n_pred == 0 && n_gt == 0) return TSPN_OK;
  TSPN_REQUIRE((n_gt == 0 || claim) && (n_pred == 0 || (best && best_index && groups && pred_group && hit)),
               TSPN_EINVAL, "tspn_evalobj_claim: null pointer");
  TSPN_REQUIRE(thresh_t == thresh_t, TSPN_EINVAL, "tspn_evalobj_claim: thresh_t is NaN");
  TSPN_REQUIRE(n_pred < ((int64_t)1 << 31) * 256 && n_gt < ((int64_t)1 << 31) * 256, TSPN_EUNSUPPORTED,
               "tspn_evalobj_claim: too many trajectories");
  if (n_gt > 0)
    hipLaunchKernelGGL(evalobj_claim_fill_kernel, dim3((unsigned)tspn::ceil_div(n_gt, 256)), dim3(256), 0,
                       TSPN_STREAM(stream), claim, n_gt);
  if (n_pred > 0) {
    const dim3 grid((unsigned)tspn::ceil_div(n_pred, 256));
    if (n_gt > 0)
      hipLaunchKernelGGL(evalobj_claim_min_kernel, grid, dim3(256), 0, TSPN_STREAM(stream), best, best_index, groups,
                         pred_group, n_pred, n_gt, thresh_t, claim);
    hipLaunchKernelGGL(evalobj_claim_hit_kernel, grid, dim3(256), 0, TSPN_STREAM(stream), best, best_index, groups,
                       pred_group, n_pred, n_gt, thresh_t, claim, hit);
  }
  return tspn::check_launch("tspn_evalobj_claim");
}
