// Training targets of a batch of segments from their ground-truth relation instances (gfx950): the predicate label row
// and the ground-truth spans of every pair of a pair table -- the device form of VRDataset._get_proposals_rel_feature
// (lib/dataset/vrdataset.py:85-138), whose statements cannot run once a pair is positive (DESIGN.md 2 "pair labels").
//
// Semantics (DESIGN.md 2 "pair labels"), per segment [fstart, fend) with M tracks, its pair table and its R instances
// (sub_tid, obj_tid, pred, begin, end):
//   col(tid) = the largest j with trackid[j] == tid, tid >= 0 (the reference's dict: the last occurrence wins), else none;
//   instance r is live when both columns exist and 0 <= pred < K;
//   a live r covers pair (s, o) iff s != o, both lie in [0, M), trackid[s] < 0, trackid[o] < 0,
//   iou[s, col(sub_tid_r)] >= thr and iou[o, col(obj_tid_r)] >= thr, compared in fp32 (NaN never covers);
//   labels [P, K]: merge 0 ("last") the one-hot of pred of the covering instance of the largest r, merge 1 ("or") the
//   pred of every covering instance; a row nothing covers is zero;
//   spans [P, G, 2]: for the covering instances in ascending r, [max(begin, fstart) - fstart, min(end, fend) - fstart),
//   skipped when empty or equal to a row already stored, else stored in the next free row; unused rows (0, 0);
//   span_count [P] = the distinct spans, G + 1 when more than G were found (the excess is dropped), -1 for a pair naming a
//   track outside [0, M) (its labels zero, its rows padding);
//   inst_cols [R, 2] = the resolved columns, -1 for a missing one, (-2, -2) for pred outside [0, K).
//
// Two kernels:
//   pair_labels_resolve_kernel  one thread per instance of the concatenated instance table: its segment by binary search
//                               in inst_off, a scan of the segment's trackid, inst_cols.
//   pair_labels_kernel          one workgroup per TILE = 256 pairs of the concatenated pair table, one thread per pair: its
//                               segment by binary search in pair_off, a loop over the segment's instances (inst_cols and
//                               the instance rows are the same addresses for the threads of a segment: broadcast loads; the
//                               two iou reads are gathers in the pair's own rows), the pair's predicate mask as
//                               ceil(K / 64) 64-bit words in LDS (word-major, so that the threads of a wave touch
//                               consecutive words) and its span rows straight to spans (the duplicate test reads back the
//                               rows the same thread stored).  Then the whole workgroup writes the tile's 256 x K label
//                               elements from the masks, consecutive threads consecutive elements (16-byte stores where
//                               labels is 16-byte aligned): the label store is nearly all of the traffic.
// Every output element is written exactly once, the zero rows and the padding included: no memset, no atomics, no scratch.
#include <cmath>

#include "tspn_common.h"
#include "tspn_pair_tables.h"

namespace {

constexpr int TILE = 256;                          // pairs per workgroup = threads per workgroup
constexpr int MAX_K = 512;
constexpr int MAX_WORDS = MAX_K / 64;              // 64-bit mask words per pair
constexpr int MAX_G = 16;
constexpr int MERGE_LAST = 0, MERGE_OR = 1;

using Tables = tspn::PairTables;
using tspn::segment_of;

__global__ __launch_bounds__(TILE) void pair_labels_resolve_kernel(Tables t, int64_t K, int32_t* __restrict__ inst_cols) {
  const int64_t r = (int64_t)blockIdx.x * TILE + threadIdx.x;
  if (r >= t.R) return;
  int64_t m0 = 0, M = t.M;
  if (t.inst_off) {
    const int64_t s = segment_of(t.inst_off, t.S, r);
    m0 = t.track_off[s];
    M = t.track_off[s + 1] - m0;
  }
  const int64_t sub = t.insts[5 * r], obj = t.insts[5 * r + 1], pred = t.insts[5 * r + 2];
  int32_t cs = -1, co = -1;
  if (pred < 0 || pred >= K) {
    cs = co = -2;
  } else {
    for (int64_t j = 0; j < M; ++j) {
      const int64_t tid = t.trackid[m0 + j];
      if (tid >= 0 && tid == sub) cs = (int32_t)j;
      if (tid >= 0 && tid == obj) co = (int32_t)j;
    }
  }
  inst_cols[2 * r] = cs;
  inst_cols[2 * r + 1] = co;
}

__global__ __launch_bounds__(TILE) void pair_labels_kernel(Tables t, int K, int G, float thr, int merge,
                                                           const int32_t* __restrict__ inst_cols,
                                                           float* __restrict__ labels, int64_t* __restrict__ spans,
                                                           int32_t* __restrict__ span_count, bool aligned) {
  __shared__ unsigned long long lds_mask[MAX_WORDS * TILE];
  const int words = (K + 63) >> 6;
  const int64_t p0 = (int64_t)blockIdx.x * TILE, p = p0 + threadIdx.x;
  for (int w = 0; w < words; ++w) lds_mask[w * TILE + threadIdx.x] = 0;
  if (p < t.P) {
    const tspn::PairScope v = tspn::pair_scope(t, p, G > 0);
    const bool inside = v.inside, open = v.open;
    const int64_t fstart = v.fstart, fend = v.fend, r0 = v.r0, r1 = v.r1;
    int64_t* my_spans = spans + p * (int64_t)G * 2;       // formed, not read, when G == 0
    int last = -1, count = 0;
    if (open) {
      for (int64_t r = r0; r < r1; ++r) {
        const int cs = inst_cols[2 * r], co = inst_cols[2 * r + 1];
        if (!tspn::covers(v, cs, co, thr)) continue;
        const int pred = (int)t.insts[5 * r + 2];          // in [0, K): the instance is live
        last = pred;
        if (merge == MERGE_OR) lds_mask[(pred >> 6) * TILE + threadIdx.x] |= 1ull << (pred & 63);
        if (G > 0) {
          const int64_t begin = t.insts[5 * r + 3], end = t.insts[5 * r + 4];
          const int64_t lo = (begin > fstart ? begin : fstart) - fstart, hi = (end < fend ? end : fend) - fstart;
          if (hi <= lo) continue;
          bool seen = false;
          const int stored = count < G ? count : G;
          for (int g = 0; g < stored; ++g) seen = seen || (my_spans[2 * g] == lo && my_spans[2 * g + 1] == hi);
          if (seen) continue;
          if (count < G) {
            my_spans[2 * count] = lo;
            my_spans[2 * count + 1] = hi;
          }
          if (count <= G) ++count;                           // saturates at G + 1
        }
      }
      if (merge == MERGE_LAST && last >= 0) lds_mask[(last >> 6) * TILE + threadIdx.x] = 1ull << (last & 63);
    }
    if (G > 0) {
      for (int g = count < G ? count : G; g < G; ++g) {
        my_spans[2 * g] = 0;
        my_spans[2 * g + 1] = 0;
      }
      span_count[p] = inside ? count : -1;
    }
  }
  __syncthreads();
  // the tile's label elements, flat: element e = row * K + k of the rows p0 .. p0 + rows - 1
  const int64_t left = t.P - p0;
  const int rows = left < TILE ? (int)left : TILE;
  // p0 * K * 4 bytes is a multiple of 1024: the tile starts 16-byte aligned where labels does
  tspn::store_mask_rows<TILE>(lds_mask, labels + p0 * K, rows, K, aligned);
}

}  // namespace

extern "C" int tspn_pair_labels_f32(const int64_t* pairs, const int64_t* pair_off, const int64_t* trackid,
                                    const int64_t* track_off, const float* iou, const int64_t* iou_off,
                                    const int64_t* insts, const int64_t* inst_off, const int64_t* seg_frames, int64_t S,
                                    int64_t P, int64_t M, int64_t R, int64_t K, int64_t G, double iou_thres, int merge,
                                    float* labels, int64_t* spans, int32_t* span_count, int32_t* inst_cols, void* stream) {
  const char* who = "tspn_pair_labels_f32";
  TSPN_REQUIRE(S >= 0 && P >= 0 && M >= 0 && R >= 0, TSPN_EINVAL, "%s: bad sizes S=%lld P=%lld M=%lld R=%lld", who,
               (long long)S, (long long)P, (long long)M, (long long)R);
  TSPN_REQUIRE(S < (1LL << 31) && P < (1LL << 31) && M < (1LL << 31) && R < (1LL << 31), TSPN_EUNSUPPORTED,
               "%s: S=%lld P=%lld M=%lld R=%lld (each needs < 2^31)", who, (long long)S, (long long)P, (long long)M,
               (long long)R);
  TSPN_REQUIRE(K >= 1, TSPN_EINVAL, "%s: K=%lld predicates (needs K >= 1)", who, (long long)K);
  TSPN_REQUIRE(K <= MAX_K, TSPN_EUNSUPPORTED, "%s: K=%lld predicates (needs K <= %d)", who, (long long)K, MAX_K);
  TSPN_REQUIRE(G >= 0, TSPN_EINVAL, "%s: G=%lld span rows (needs 0 <= G)", who, (long long)G);
  TSPN_REQUIRE(G <= MAX_G, TSPN_EUNSUPPORTED, "%s: G=%lld span rows (needs G <= %d)", who, (long long)G, MAX_G);
  TSPN_REQUIRE(G == 0 || P == 0 || (spans && span_count), TSPN_EINVAL, "%s: G=%lld with a null spans or span_count", who,
               (long long)G);
  TSPN_REQUIRE(merge == MERGE_LAST || merge == MERGE_OR, TSPN_EINVAL, "%s: unknown merge=%d (0 = last, 1 = or)", who, merge);
  TSPN_REQUIRE(std::isfinite(iou_thres), TSPN_EINVAL, "%s: iou_thres is not finite", who);
  const bool offsets = pair_off && track_off && iou_off && inst_off;
  TSPN_REQUIRE(offsets || (S <= 1 && !pair_off && !track_off && !iou_off && !inst_off), TSPN_EINVAL,
               "%s: S=%lld needs pair_off, track_off, iou_off and inst_off (all null: one segment)", who, (long long)S);
  TSPN_REQUIRE(S > 0 || (P == 0 && R == 0), TSPN_EINVAL, "%s: S=0 with P=%lld pairs and R=%lld instances", who,
               (long long)P, (long long)R);
  const bool need_tracks = M > 0 && (P > 0 || R > 0);
  TSPN_REQUIRE((P == 0 || (pairs && labels)) && (R == 0 || (insts && inst_cols)) && (!need_tracks || trackid) &&
                   (!(need_tracks && P > 0 && R > 0) || iou) && (G == 0 || P == 0 || seg_frames),
               TSPN_EINVAL, "%s: null pointer", who);
  auto a8 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 7) == 0; };
  auto a4 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 3) == 0; };
  TSPN_REQUIRE(a8(pairs) && a8(pair_off) && a8(trackid) && a8(track_off) && a8(iou_off) && a8(insts) && a8(inst_off) &&
                   a8(seg_frames) && a8(spans) && a4(iou) && a4(labels) && a4(span_count) && a4(inst_cols),
               TSPN_EUNSUPPORTED, "%s: unaligned pointer (int64 operands need 8 bytes, fp32 and int32 ones 4)", who);
  if (P == 0 && R == 0) return TSPN_OK;
  const Tables t = {pairs, pair_off, trackid, track_off, iou, iou_off, insts, inst_off, seg_frames, S, P, M, R};
  hipStream_t s = TSPN_STREAM(stream);
  if (R > 0)
    hipLaunchKernelGGL(pair_labels_resolve_kernel, dim3((unsigned)tspn::ceil_div(R, TILE)), dim3(TILE), 0, s, t, K,
                       inst_cols);
  if (P > 0)
    hipLaunchKernelGGL(pair_labels_kernel, dim3((unsigned)tspn::ceil_div(P, TILE)), dim3(TILE), 0, s, t, (int)K, (int)G,
                       (float)iou_thres, merge, inst_cols, labels, spans, span_count, tspn::aligned16(labels));
  return tspn::check_launch(who);
}
