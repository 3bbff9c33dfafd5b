// The operand tables of a batch of segments stored back to back and what one pair of them may read: shared by the pair
// labels (pairlabels/tspn_pair_labels.hip) and the per-span predicate labels (spancls/tspn_span_cls.hip), which must
// decide "instance r covers pair p" alike (DESIGN.md 2 "pair labels").
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace tspn {

struct PairTables {
  const int64_t* pairs;        // [P, 2]
  const int64_t* pair_off;     // [S + 1] or null (S == 1)
  const int64_t* trackid;      // [M]
  const int64_t* track_off;
  const float* iou;            // segment s: [M_s, M_s] from iou_off[s] on
  const int64_t* iou_off;
  const int64_t* insts;        // [R, 5]
  const int64_t* inst_off;
  const int64_t* seg_frames;   // [S, 2] or null (G == 0)
  int64_t S, P, M, R;
};

// the largest s in [0, S) with off[s] <= i, for off[0] <= i < off[S]: the segment that holds element i (empty segments
// in front of it share its offset and lose)
__device__ __forceinline__ int64_t segment_of(const int64_t* __restrict__ off, int64_t S, int64_t i) {
  int64_t lo = 0, hi = S;
  while (hi - lo > 1) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (off[mid] <= i)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

// What pair p reads of its segment: the two iou rows, the instance range, the frames; `open` = the pair can be covered
// at all (s != o, both in [0, M), both proposals), `inside` = both indices lie in [0, M).
struct PairScope {
  const float* row_a;
  const float* row_b;
  int64_t r0, r1, fstart, fend;
  bool inside, open;
};

__device__ __forceinline__ PairScope pair_scope(const PairTables& t, int64_t p, bool frames) {
  int64_t s = 0, m0 = 0, M = t.M, i0 = 0;
  PairScope v;
  v.r0 = 0;
  v.r1 = t.R;
  if (t.pair_off) {
    s = segment_of(t.pair_off, t.S, p);
    m0 = t.track_off[s];
    M = t.track_off[s + 1] - m0;
    i0 = t.iou_off[s];
    v.r0 = t.inst_off[s];
    v.r1 = t.inst_off[s + 1];
  }
  const int64_t a = t.pairs[2 * p], b = t.pairs[2 * p + 1];
  v.inside = a >= 0 && a < M && b >= 0 && b < M;
  v.open = v.inside && a != b && t.trackid[m0 + a] < 0 && t.trackid[m0 + b] < 0;
  v.fstart = frames ? t.seg_frames[2 * s] : 0;
  v.fend = frames ? t.seg_frames[2 * s + 1] : 0;
  v.row_a = t.iou + i0 + a * M;                          // formed, not read, unless the pair is open
  v.row_b = t.iou + i0 + b * M;
  return v;
}

// live instance r (both columns resolved) covers the open pair of `v`: the fp32 compare, NaN never covers
__device__ __forceinline__ bool covers(const PairScope& v, int cs, int co, float thr) {
  return cs >= 0 && co >= 0 && v.row_a[cs] >= thr && v.row_b[co] >= thr;
}

// A tile's label elements from its rows' predicate masks (LDS, word-major: bit k of row `row` is bit k & 63 of
// mask[(k >> 6) * TILE + row]), flat: element e = row * K + k of `rows` rows, consecutive threads consecutive elements,
// 16-byte stores where `aligned` (out 16-byte aligned).  The whole workgroup of TILE threads calls it after a barrier.
template <int TILE>
__device__ __forceinline__ void store_mask_rows(const unsigned long long* mask, float* __restrict__ out, int rows, int K,
                                                bool aligned) {
  const int n = rows * K;                                    // <= 256 * 512
  const int n4 = aligned ? n >> 2 : 0;
  for (int i = threadIdx.x; i < n4; i += TILE) {
    int row = (4 * i) / K, k = 4 * i - row * K;
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] = (float)((mask[(k >> 6) * TILE + row] >> (k & 63)) & 1ull);
      if (++k == K) {
        k = 0;
        ++row;
      }
    }
    reinterpret_cast<float4*>(out)[i] = make_float4(v[0], v[1], v[2], v[3]);
  }
  for (int e = 4 * n4 + threadIdx.x; e < n; e += TILE) {
    const int row = e / K, k = e - row * K;
    out[e] = (float)((mask[(k >> 6) * TILE + row] >> (k & 63)) & 1ull);
  }
}

}  // namespace tspn
