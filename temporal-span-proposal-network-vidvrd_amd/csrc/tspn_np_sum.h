// numpy's summation order for a contiguous float64 run, on the device (gfx950): the one copy that the association-time
// IoU kernels share (tspn_iou.hip traj_iou_tail_f64_kernel, spanmatch/tspn_span_match.hip span_match_iou_kernel).
//
// np.sum of a contiguous 1-D run (numpy's pairwise_sum): eight interleaved partial sums per block of <= 128 elements,
// combined as ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), the remainder added one by one; above 128 the run is
// split at n / 2 rounded down to a multiple of 8 and the two halves are summed the same way, left + right.  `f(i)` is
// element i of the run: the blocks of eight and the splits count from the run's first element, wherever it lies in memory.
// Runs of fewer than 2^31 elements.
#pragma once
#include <cstdint>

template <class F>
__device__ inline double np_block_sum(F&& f, int64_t lo, int64_t n) {
  if (n < 8) {
    double res = 0.;
    for (int64_t i = 0; i < n; ++i) res += f(lo + i);
    return res;
  }
  double r[8];
  for (int k = 0; k < 8; ++k) r[k] = f(lo + k);
  int64_t i = 8;
  for (; i < n - (n % 8); i += 8)
    for (int k = 0; k < 8; ++k) r[k] += f(lo + i + k);
  double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res += f(lo + i);
  return res;
}

// The split of a run of n > 128 elements: the left half's length.
__device__ inline int64_t np_left_half(int64_t n) {
  const int64_t n2 = n / 2;
  return n2 - n2 % 8;
}

// Levels of the split tree that a caller provides parking for: a run of n elements is at most ceil(log2(n / 64)) levels
// deep, so 26 serve every n < 2^31 (the entries refuse longer rows).
constexpr int kNpSumLevels = 26;

// The recursion above as a post-order walk.  A node of the split tree is named by its depth and the turns taken from the
// root (bit d of `turns`: 0 = left, 1 = right at depth d); its run is found again by walking down from the root, so the
// only state kept per level is the left child's sum, parked while the right child is summed.  `park` is the calling
// thread's own parking: element d * stride for level d, kNpSumLevels levels -- the kernels hand over a column of an LDS
// array (a per-thread array indexed at run time would live in scratch memory).  Touched only when n > 128; no barrier is
// needed, nobody else reads a thread's column.
template <class F>
__device__ inline double np_pairwise_sum(F&& f, int64_t n, double* park, int stride) {
  if (n <= 128) return np_block_sum(f, 0, n);
  uint32_t turns = 0;
  int depth = 0;
  for (;;) {
    // the run of the node (depth, turns), then down its left spine to a leaf
    int64_t lo = 0, len = n;
    for (int d = 0; d < depth; ++d) {
      const int64_t n2 = np_left_half(len);
      if ((turns >> d) & 1u) {
        lo += n2;
        len -= n2;
      } else {
        len = n2;
      }
    }
    while (len > 128) {
      turns &= ~(1u << depth);
      ++depth;
      len = np_left_half(len);
    }
    double ret = np_block_sum(f, lo, len);
    // up: a left child parks its sum and hands over to its sibling; a right child adds to the parked sum and goes on up
    for (;;) {
      if (depth == 0) return ret;
      --depth;
      if (((turns >> depth) & 1u) == 0) {
        park[depth * stride] = ret;
        turns |= 1u << depth;
        ++depth;
        break;
      }
      ret = park[depth * stride] + ret;
    }
  }
}
