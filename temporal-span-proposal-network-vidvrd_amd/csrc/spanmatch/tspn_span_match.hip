// Span-bounded association of one segment on the device (gfx950): which relation of the previous segment every
// span-bounded prediction extends (DESIGN.md 2 "span match").
//
// A span-bounded prediction owns fresh copies of its two trajectories (association.py _span_cut), so no trajectory is
// shared between relations and a merge changes only the relation that leaves the candidate list: whether relation u can
// absorb prediction p depends on state fixed when the segment starts.  The whole decision matrix and the greedy
// assignment over it are therefore computed before the host's loop, which then only cuts and merges.
//
// Rows u of rel_* are the candidate relations in candidate order (mean confidence, descending and stable); predictions p
// are in score order.  All frames are local to the segment (frame f = video frame fstart + f), L frames, N tracklets.
//   (u, p) is a candidate pair iff the triplets are equal, a < rel_fend[u], and for both roles c
//   start_c <= a < end_c <= e with [a, e) = pred_span[p], [start_c, end_c) = rel_range[u, c]; a prediction with
//   !(0 <= a < e <= L) or a pair index outside [0, N) is a candidate of nothing.  Only candidate pairs read boxes, and
//   the conditions bound every such read: frames [a, end_c) with end_c <= e <= L of tracklet pred_pair[p, c] in [0, N).
//   iou[u, p, c] = IoU of rel_boxes[u, c, a:end_c] against trk_boxes[pred_pair[p, c], a:end_c] with the roundings of
//   traj_iou_tail_f64_kernel (tspn_iou.hip): max / min stored as float32; +1, subtraction, clip, product and the running
//   sum in float32, in frame order; areas in float64, summed in numpy's pairwise order over the window that starts at a;
//   the quotient in float64, stored as float32.  -1 for both roles of a pair that is no candidate.
//   match[p] = the smallest u not taken by an earlier prediction with iou[u, p, 0] >= iou_thr and iou[u, p, 1] >= iou_thr
//   (float64 comparisons: NaN fails, and so does the -1 of a non-candidate for any iou_thr > -1), which is then taken;
//   -1 when there is none.
//
// Two kernels:
//   span_match_iou_kernel     one thread per (u, p), 256 per workgroup: the gate tests, then the two IoUs.  Latency-bound
//                             and tiny (U, P of a few hundred, L = 30); the fp32 running sum is sequential by contract.
//   span_match_greedy_kernel  ONE workgroup of 256 threads, sequential over p.  Thread t owns the relations u = t (mod
//                             256) and keeps their taken flags in LDS words nobody else touches (word (c / 32) * 256 + t,
//                             bit c % 32 for u = 256 c + t: 8 KB for the 65536 relations the entry accepts), so the flags
//                             need no barrier.  Per chunk of 256 relations each wave finds its first passing lane with a
//                             ballot and the four firsts meet in LDS behind one barrier (two slots in turn: the next
//                             chunk's writes cannot overtake this chunk's reads).  The first chunk's two values of
//                             prediction p + 1 are loaded before prediction p is reduced.
// Every element of iou and match is written; no memset, no scratch buffer, no synchronisation.  The pair kernel holds
// np_pairwise_sum's parking (tspn_np_sum.h) in LDS, a column per thread; only windows of more than 128 frames touch it.
#include <climits>
#include <cmath>

#include "tspn_common.h"
#include "tspn_np_sum.h"

namespace {

constexpr int TILE = 256;                          // threads per workgroup
constexpr int WAVE = 64;
constexpr int WAVES = TILE / WAVE;
constexpr int MAX_U = 65536;                       // relations whose taken flags fit the LDS bitmap
constexpr int TAKEN_WORDS = MAX_U / 32;            // 2048 words = 8 KB

// IoU of n frames of two box runs with the reference chain's roundings (see traj_iou_tail_f64_kernel)
__device__ inline float window_iou(const double* __restrict__ pa, const double* __restrict__ pb, int64_t n, double* park) {
  float inters = 0.f;
  for (int64_t t = 0; t < n; ++t) {
    const double* p = pa + 4 * t;
    const double* q = pb + 4 * t;
    const float lo_x = (float)fmax(p[0], q[0]), hi_x = (float)fmin(p[2], q[2]);
    float w = (hi_x + 1.f) - lo_x;
    w = fmaxf(w, 0.f);
    const float lo_y = (float)fmax(p[1], q[1]), hi_y = (float)fmin(p[3], q[3]);
    float h = (hi_y + 1.f) - lo_y;
    h = fmaxf(h, 0.f);
    inters += w * h;
  }
  auto area_of = [](const double* r) {
    return [r](int64_t t) { return (r[4 * t + 2] - r[4 * t] + 1.) * (r[4 * t + 3] - r[4 * t + 1] + 1.); };
  };
  const double a1 = np_pairwise_sum(area_of(pa), n, park, TILE);
  const double a2 = np_pairwise_sum(area_of(pb), n, park, TILE);
  const double uni = (a1 + a2) - (double)inters;
  return (float)((double)inters / uni);
}

__global__ __launch_bounds__(TILE) void span_match_iou_kernel(
    const double* __restrict__ rel_boxes, const int32_t* __restrict__ rel_range, const int32_t* __restrict__ rel_fend,
    const int64_t* __restrict__ rel_triplet, const double* __restrict__ trk_boxes,
    const int64_t* __restrict__ pred_triplet, const int32_t* __restrict__ pred_pair,
    const int32_t* __restrict__ pred_span, int64_t U, int64_t P, int64_t N, int64_t L, float* __restrict__ iou) {
  __shared__ double park[kNpSumLevels * TILE];     // np_pairwise_sum's parking, one column per thread (windows of > 128 frames)
  const int64_t up = (int64_t)blockIdx.x * TILE + threadIdx.x;
  if (up >= U * P) return;
  const int64_t u = up / P, p = up - u * P;
  const int64_t a = pred_span[2 * p], e = pred_span[2 * p + 1];
  const int64_t trk[2] = {pred_pair[2 * p], pred_pair[2 * p + 1]};
  bool cand = 0 <= a && a < e && e <= L && trk[0] >= 0 && trk[0] < N && trk[1] >= 0 && trk[1] < N;
  for (int k = 0; k < 3; ++k) cand = cand && rel_triplet[3 * u + k] == pred_triplet[3 * p + k];
  cand = cand && a < rel_fend[u];
  int64_t end[2];
  for (int c = 0; c < 2; ++c) {
    const int64_t start = rel_range[4 * u + 2 * c];
    end[c] = rel_range[4 * u + 2 * c + 1];
    cand = cand && start <= a && a < end[c] && end[c] <= e;
  }
  float v[2] = {-1.f, -1.f};
  if (cand) {
    // frames [a, end[c]) with 0 <= a < end[c] <= e <= L, tracklet trk[c] in [0, N): inside both operands
    for (int c = 0; c < 2; ++c)
      v[c] = window_iou(rel_boxes + ((u * 2 + c) * L + a) * 4, trk_boxes + (trk[c] * L + a) * 4, end[c] - a,
                        park + threadIdx.x);
  }
  iou[2 * up] = v[0];
  iou[2 * up + 1] = v[1];
}

__global__ __launch_bounds__(TILE) void span_match_greedy_kernel(const float* __restrict__ iou, int64_t U, int64_t P,
                                                                 double iou_thr, int32_t* __restrict__ match) {
  __shared__ uint32_t taken[TAKEN_WORDS];
  __shared__ int first[2][WAVES];
  const int t = threadIdx.x, lane = t & (WAVE - 1), wave = t / WAVE;
  const int64_t chunks = (U + TILE - 1) / TILE;
  for (int64_t w = 0; w * 32 < chunks; ++w) taken[w * TILE + t] = 0;   // this thread's own words
  int slot = 0;
  float n0 = -1.f, n1 = -1.f;                       // chunk 0 of the next prediction
  if (t < U && P > 0) {
    n0 = iou[2 * ((int64_t)t * P)];
    n1 = iou[2 * ((int64_t)t * P) + 1];
  }
  for (int64_t p = 0; p < P; ++p) {
    float v0 = n0, v1 = n1;
    if (t < U && p + 1 < P) {
      n0 = iou[2 * ((int64_t)t * P + p + 1)];
      n1 = iou[2 * ((int64_t)t * P + p + 1) + 1];
    }
    int best = -1;
    for (int64_t c = 0; c < chunks; ++c) {
      const int64_t u = c * TILE + t;
      if (c > 0 && u < U) {
        v0 = iou[2 * (u * P + p)];
        v1 = iou[2 * (u * P + p) + 1];
      }
      const bool free_u = u < U && ((taken[(c >> 5) * TILE + t] >> (c & 31)) & 1u) == 0;
      const bool pass = free_u && (double)v0 >= iou_thr && (double)v1 >= iou_thr;
      const unsigned long long votes = __ballot(pass);
      if (lane == 0) first[slot][wave] = votes ? (int)(c * TILE) + wave * WAVE + (__ffsll(votes) - 1) : INT_MAX;
      __syncthreads();
      int m = INT_MAX;
      for (int k = 0; k < WAVES; ++k) m = min(m, first[slot][k]);
      slot ^= 1;
      if (m != INT_MAX) {                           // the same m in every thread: a uniform exit
        best = m;
        if (u == m) taken[(c >> 5) * TILE + t] |= 1u << (c & 31);
        break;
      }
    }
    if (t == 0) match[p] = best;
  }
}

}  // namespace

extern "C" int tspn_span_match_f64(const double* rel_boxes, const int32_t* rel_range, const int32_t* rel_fend,
                                   const int64_t* rel_triplet, const double* trk_boxes, const int64_t* pred_triplet,
                                   const int32_t* pred_pair, const int32_t* pred_span, int64_t U, int64_t P, int64_t N,
                                   int64_t L, double iou_thr, float* iou, int32_t* match, void* stream) {
  const char* who = "tspn_span_match_f64";
  TSPN_REQUIRE(U >= 0 && P >= 0 && N >= 0 && L >= 0, TSPN_EINVAL, "%s: bad sizes U=%lld P=%lld N=%lld L=%lld", who,
               (long long)U, (long long)P, (long long)N, (long long)L);
  const bool pairs = U > 0 && P > 0;
  TSPN_REQUIRE((P == 0 || (pred_triplet && pred_pair && pred_span && match)) &&
                   (!pairs || (rel_range && rel_fend && rel_triplet && iou)) &&
                   (!(pairs && N > 0 && L > 0) || (rel_boxes && trk_boxes)),
               TSPN_EINVAL, "%s: null pointer", who);
  TSPN_REQUIRE(std::isfinite(iou_thr), TSPN_EINVAL, "%s: iou_thr is not finite", who);
  TSPN_REQUIRE(U <= MAX_U, TSPN_EUNSUPPORTED, "%s: U=%lld relations (needs U <= %d: the taken flags live in LDS)", who,
               (long long)U, MAX_U);
  TSPN_REQUIRE(U == 0 || P <= (((int64_t)1 << 31) - 1) / U, TSPN_EUNSUPPORTED, "%s: U=%lld x P=%lld pairs (needs U * P < 2^31)", who,
               (long long)U, (long long)P);
  TSPN_REQUIRE(N < ((int64_t)1 << 31) && L < ((int64_t)1 << 31), TSPN_EUNSUPPORTED, "%s: N=%lld L=%lld (each needs < 2^31)", who,
               (long long)N, (long long)L);
  if (P == 0) return TSPN_OK;
  hipStream_t s = TSPN_STREAM(stream);
  if (U > 0)
    hipLaunchKernelGGL(span_match_iou_kernel, dim3((unsigned)tspn::ceil_div(U * P, TILE)), dim3(TILE), 0, s, rel_boxes,
                       rel_range, rel_fend, rel_triplet, trk_boxes, pred_triplet, pred_pair, pred_span, U, P, N, L, iou);
  hipLaunchKernelGGL(span_match_greedy_kernel, dim3(1), dim3(TILE), 0, s, iou, U, P, iou_thr, match);
  return tspn::check_launch(who);
}
