// Training the predicate head on ground-truth-span-pooled features (gfx950): a predicate label row per (pair,
// ground-truth span), and the loss and gradient of the span-pooled head on those rows (DESIGN.md 2 "span-pooled predicate
// training").  The reference only names the intent (RelOIPool, lib/modeling/model.py:68-73, a stub); the semantics are
// build-defined.
//
// Rows.  Row r = p G + g of pair p and span row g.  With c = span_count[p] (tspn_pair_labels_f32):
//   c >= 1 and g < min(c, G)   a row over the frames spans[p, g], its label span_labels[p, g];
//   c == 0 and g == 0          a negative pair: the frames [0, T), label zero (span_labels is not read);
//   anything else              no row (c < 0, g beyond the count, rows beyond a saturated count).
// The loss entries also drop the rows of a pair naming a tracklet outside [0, NT): nothing is read through such an id.
//
// Kernels:
//   span_labels_kernel        one workgroup per TILE = 256 rows, one thread per row: the covering instances of the row's
//                             pair (tspn::pair_scope / tspn::covers, the test of the pair labels) whose clipped span equals
//                             spans[p, g], as a predicate mask in LDS; then the workgroup writes the tile's TILE x K elements
//                             (tspn::store_mask_rows).  Every element written once.
//   span_cls_rows_kernel      one workgroup per segment: its number of rows (an integer sum: any order gives the same).
//   span_cls_loss_kernel      one wave per row: v = tspn::span_value per predicate (lane k, k + 64, ..), q = (float)sigmoid(v),
//                             dv = (sigmoid(v) - y) / (K rows_of_segment), and the row's loss sum (each lane in ascending k,
//                             then the xor butterfly 32 .. 1).  Rows that are none get q = dv = 0 and a zero sum by
//                             selection: none of their operands is read.
//   span_cls_finish_kernel    one workgroup: per segment, thread i adds the row sums i, i + 256, .. in order, an LDS tree,
//                             loss_s = sum / (K rows_s) (0 without rows); out[0] = the sum over the segments in order.
//   span_cls_bias_grad_kernel one thread per predicate: db[k] = the float64 sum of dv[:, k], rows in ascending order.
//   span_cls_proj_grad_kernel one thread per (tracklet n, column 2k + h): walks the pair table in ascending order; a row of
//                             a pair with pairs[p][h] == n adds dv[r, k] / (e - a) at a and subtracts it at e of a float64
//                             difference array (the caller's scratch, column-interleaved like the prefix sums); the same
//                             thread then takes the running sum over t into dG.  No atomics; every element of dG written.
#include <cmath>

#include "tspn_common.h"
#include "tspn_pair_tables.h"
#include "tspn_span_pool.h"

namespace {

constexpr int TILE = 256;                          // label rows per workgroup = threads per workgroup
constexpr int MAX_K = 512;                         // predicates of the label entry (the mask words live in LDS)
constexpr int MAX_WORDS = MAX_K / 64;
constexpr int MAX_G = 16;
constexpr int MERGE_LAST = 0, MERGE_OR = 1;
constexpr int WAVES = 4;                           // rows per workgroup of the loss kernel
constexpr int FIN_THREADS = 256;

// the rows of a pair with span count c: min(c, G) for c >= 1, one for a negative pair, none for c < 0
__device__ __forceinline__ int rows_of_pair(int c, int G) { return c >= 1 ? (c < G ? c : G) : (c == 0 ? 1 : 0); }

__global__ __launch_bounds__(TILE) void span_labels_kernel(tspn::PairTables t, int K, int G, float thr, int merge,
                                                           const int32_t* __restrict__ inst_cols,
                                                           const int64_t* __restrict__ spans,
                                                           const int32_t* __restrict__ span_count,
                                                           float* __restrict__ span_labels, bool aligned) {
  __shared__ unsigned long long lds_mask[MAX_WORDS * TILE];
  const int words = (K + 63) >> 6;
  const int64_t total = t.P * G;
  const int64_t row0 = (int64_t)blockIdx.x * TILE, row = row0 + threadIdx.x;
  for (int w = 0; w < words; ++w) lds_mask[w * TILE + threadIdx.x] = 0;
  if (row < total) {
    const int64_t p = row / G;
    const int g = (int)(row - p * G);
    const int c = span_count[p];
    if (c >= 1 && g < (c < G ? c : G)) {
      const tspn::PairScope v = tspn::pair_scope(t, p, true);
      const int64_t lo0 = spans[2 * row], hi0 = spans[2 * row + 1];
      int last = -1;
      if (v.open) {
        for (int64_t r = v.r0; r < v.r1; ++r) {
          if (!tspn::covers(v, inst_cols[2 * r], inst_cols[2 * r + 1], thr)) continue;
          const int64_t begin = t.insts[5 * r + 3], end = t.insts[5 * r + 4];
          const int64_t lo = (begin > v.fstart ? begin : v.fstart) - v.fstart;
          const int64_t hi = (end < v.fend ? end : v.fend) - v.fstart;
          if (lo != lo0 || hi != hi0) continue;
          const int pred = (int)t.insts[5 * r + 2];          // in [0, K): the instance is live
          last = pred;
          if (merge == MERGE_OR) lds_mask[(pred >> 6) * TILE + threadIdx.x] |= 1ull << (pred & 63);
        }
        if (merge == MERGE_LAST && last >= 0) lds_mask[(last >> 6) * TILE + threadIdx.x] = 1ull << (last & 63);
      }
    }
  }
  __syncthreads();
  const int64_t left = total - row0;
  // row0 * K * 4 bytes is a multiple of 1024: the tile starts 16-byte aligned where span_labels does
  tspn::store_mask_rows<TILE>(lds_mask, span_labels + row0 * K, left < TILE ? (int)left : TILE, K, aligned);
}

struct Rows {
  const int64_t* pairs;        // [P, 2] global tracklet ids
  const int64_t* pair_off;     // [S + 1] or null (one segment)
  const int64_t* spans;        // [P, G, 2]
  const int32_t* span_count;   // [P]
  int64_t S, P, NT;
  int G, T;
};

// the rows of pair p that the loss sees: rows_of_pair, none when an id lies outside [0, NT)
__device__ __forceinline__ int live_rows(const Rows& w, int64_t p) {
  const int64_t s = w.pairs[2 * p], o = w.pairs[2 * p + 1];
  const bool ok = s >= 0 && s < w.NT && o >= 0 && o < w.NT;
  return ok ? rows_of_pair(w.span_count[p], w.G) : 0;
}

// the frames [a, e) of row g of pair p (a live row): spans[p, g] through tspn::span_frames, [0, T) for a negative pair
__device__ __forceinline__ void row_span(const Rows& w, int64_t p, int g, int64_t& a0, int64_t& e0) {
  const bool neg = w.span_count[p] == 0;
  a0 = neg ? 0 : w.spans[2 * (p * w.G + g)];
  e0 = neg ? w.T : w.spans[2 * (p * w.G + g) + 1];
}

__global__ __launch_bounds__(FIN_THREADS) void span_cls_rows_kernel(Rows w, double* __restrict__ seg_rows) {
  __shared__ long long acc[FIN_THREADS];
  const int64_t s = blockIdx.x;
  const int64_t p0 = w.pair_off ? w.pair_off[s] : 0, p1 = w.pair_off ? w.pair_off[s + 1] : w.P;
  long long n = 0;
  for (int64_t p = p0 + threadIdx.x; p < p1; p += FIN_THREADS) n += live_rows(w, p);
  acc[threadIdx.x] = n;
  __syncthreads();
  for (int o = FIN_THREADS / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) acc[threadIdx.x] += acc[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) seg_rows[s] = (double)acc[0];
}

// the sum over the wave in every lane: partners 32, 16, 8, 4, 2, 1 apart, the same tree in every launch
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(64 * WAVES) void span_cls_loss_kernel(Rows w, const double* __restrict__ PS,
                                                                   const float* __restrict__ Gp,
                                                                   const float* __restrict__ span_labels,
                                                                   const float* __restrict__ cls_b, int K,
                                                                   const double* __restrict__ seg_rows,
                                                                   float* __restrict__ q, float* __restrict__ dv,
                                                                   double* __restrict__ partials) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (r >= w.P * w.G) return;                              // the whole wave; there is no barrier below
  const int64_t p = r / w.G;
  const int g = (int)(r - p * w.G);
  float* qr = q + r * K;
  float* dr = dv + r * K;
  if (g >= live_rows(w, p)) {                              // wave-uniform
    for (int k = lane; k < K; k += 64) {
      qr[k] = 0.f;
      dr[k] = 0.f;
    }
    if (lane == 0) partials[r] = 0.0;
    return;
  }
  const int64_t seg = w.pair_off ? tspn::segment_of(w.pair_off, w.S, p) : 0;
  const double denom = (double)K * seg_rows[seg];          // >= K: this row counts
  const bool neg = w.span_count[p] == 0;
  const int64_t s = w.pairs[2 * p], o = w.pairs[2 * p + 1];
  int64_t a0, e0;
  row_span(w, p, g, a0, e0);
  double loss = 0.0;
  for (int k = lane; k < K; k += 64) {
    const double v = tspn::span_value(PS, Gp, s, o, a0, e0, w.T, 2 * (int64_t)K, k, cls_b);
    const double y = neg ? 0.0 : (double)span_labels[r * K + k];
    loss += (v > 0.0 ? v : 0.0) - v * y + log1p(exp(-fabs(v)));
    const double sg = 1.0 / (1.0 + exp(-v));
    qr[k] = (float)sg;
    dr[k] = (float)((sg - y) / denom);
  }
  loss = wave_sum(loss);
  if (lane == 0) partials[r] = loss;
}

__global__ __launch_bounds__(FIN_THREADS) void span_cls_finish_kernel(const double* __restrict__ partials,
                                                                      const double* __restrict__ seg_rows,
                                                                      const int64_t* __restrict__ pair_off, int64_t S,
                                                                      int64_t P, int G, int K, double* __restrict__ out) {
  __shared__ double acc[FIN_THREADS];
  const int i = threadIdx.x;
  double total = 0.0;
  for (int64_t s = 0; s < S; ++s) {
    const int64_t r0 = (pair_off ? pair_off[s] : 0) * G, r1 = (pair_off ? pair_off[s + 1] : P) * G;
    double v = 0.0;
    for (int64_t r = r0 + i; r < r1; r += FIN_THREADS) v += partials[r];
    acc[i] = v;
    __syncthreads();
    for (int o = FIN_THREADS / 2; o > 0; o >>= 1) {
      if (i < o) acc[i] += acc[i + o];
      __syncthreads();
    }
    if (i == 0) {
      const double rows = seg_rows[s];
      const double l = rows > 0.0 ? acc[0] / ((double)K * rows) : 0.0;
      out[1 + s] = l;
      total += l;
    }
    __syncthreads();
  }
  if (i == 0) out[0] = total;
}

__global__ __launch_bounds__(256) void span_cls_bias_grad_kernel(const float* __restrict__ dv, int64_t rows, int K,
                                                                 float* __restrict__ db) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= K) return;
  double acc = 0.0;
#pragma unroll 8
  for (int64_t r = 0; r < rows; ++r) acc += (double)dv[r * K + k];   // the loads run ahead; the additions keep their order
  db[k] = (float)acc;
}

__global__ __launch_bounds__(256) void span_cls_proj_grad_kernel(Rows w, const float* __restrict__ dv, int K,
                                                                 double* __restrict__ diff, float* __restrict__ dG) {
  const int64_t K2 = 2 * (int64_t)K;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= w.NT * K2) return;
  const int64_t n = i / K2;
  const int c = (int)(i - n * K2), h = c & 1, k = c >> 1;
  double* d = diff + n * (w.T + 1) * K2 + c;               // element t at d[t * K2]
  for (int t = 0; t <= w.T; ++t) d[t * K2] = 0.0;
  for (int64_t p = 0; p < w.P; ++p) {
    if (w.pairs[2 * p + h] != n) continue;
    const int rows = live_rows(w, p);
    for (int g = 0; g < rows; ++g) {
      int64_t a0, e0, a, e;
      row_span(w, p, g, a0, e0);
      tspn::span_frames(a0, e0, w.T, a, e);                // 0 <= a < e <= T
      const double x = (double)dv[(p * w.G + g) * K + k] / (double)(e - a);
      d[a * K2] += x;
      d[e * K2] -= x;
    }
  }
  float* out = dG + n * w.T * K2 + c;
  double acc = 0.0;
  for (int t = 0; t < w.T; ++t) {
    acc += d[t * K2];
    out[t * K2] = (float)acc;
  }
}

bool a8(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 7) == 0; }
bool a4(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 3) == 0; }

// the size checks the loss and gradient entries share
int row_checks(const char* who, int64_t NT, int64_t T, int64_t S, int64_t P, int64_t G, int64_t K, const void* pair_off) {
  TSPN_REQUIRE(NT >= 0 && T > 0 && K > 0 && P >= 0 && S >= 0, TSPN_EINVAL, "%s: bad sizes NT=%lld T=%lld K=%lld P=%lld S=%lld",
               who, (long long)NT, (long long)T, (long long)K, (long long)P, (long long)S);
  TSPN_REQUIRE(G >= 1, TSPN_EINVAL, "%s: G=%lld span rows (needs 1 <= G)", who, (long long)G);
  TSPN_REQUIRE(G <= MAX_G, TSPN_EUNSUPPORTED, "%s: G=%lld span rows (needs G <= %d)", who, (long long)G, MAX_G);
  TSPN_REQUIRE(T < (1 << 30) && K < (1 << 20) && S < (1LL << 31) && P * G < (1LL << 31) && NT * 2 * K < (1LL << 39),
               TSPN_EUNSUPPORTED, "%s: NT=%lld T=%lld K=%lld P=%lld S=%lld (needs T < 2^30, K < 2^20, S < 2^31, P*G < 2^31)", who,
               (long long)NT, (long long)T, (long long)K, (long long)P, (long long)S);
  TSPN_REQUIRE(pair_off ? true : S <= 1, TSPN_EINVAL, "%s: S=%lld needs pair_off (null: one segment)", who, (long long)S);
  TSPN_REQUIRE(S > 0 || P == 0, TSPN_EINVAL, "%s: S=0 with P=%lld pairs", who, (long long)P);
  return TSPN_OK;
}

}  // namespace

extern "C" int tspn_span_labels_f32(const int64_t* pairs, const int64_t* pair_off, const int64_t* trackid,
                                    const int64_t* track_off, const float* iou, const int64_t* iou_off,
                                    const int64_t* insts, const int64_t* inst_off, const int64_t* seg_frames, int64_t S,
                                    int64_t P, int64_t M, int64_t R, int64_t K, int64_t G, double iou_thres, int merge,
                                    const int64_t* spans, const int32_t* span_count, const int32_t* inst_cols,
                                    float* span_labels, void* stream) {
  const char* who = "tspn_span_labels_f32";
  TSPN_REQUIRE(S >= 0 && P >= 0 && M >= 0 && R >= 0, TSPN_EINVAL, "%s: bad sizes S=%lld P=%lld M=%lld R=%lld", who,
               (long long)S, (long long)P, (long long)M, (long long)R);
  TSPN_REQUIRE(S < (1LL << 31) && P < (1LL << 31) && M < (1LL << 31) && R < (1LL << 31), TSPN_EUNSUPPORTED,
               "%s: S=%lld P=%lld M=%lld R=%lld (each needs < 2^31)", who, (long long)S, (long long)P, (long long)M,
               (long long)R);
  TSPN_REQUIRE(K >= 1, TSPN_EINVAL, "%s: K=%lld predicates (needs K >= 1)", who, (long long)K);
  TSPN_REQUIRE(K <= MAX_K, TSPN_EUNSUPPORTED, "%s: K=%lld predicates (needs K <= %d)", who, (long long)K, MAX_K);
  TSPN_REQUIRE(G >= 1, TSPN_EINVAL, "%s: G=%lld span rows (needs 1 <= G)", who, (long long)G);
  TSPN_REQUIRE(G <= MAX_G, TSPN_EUNSUPPORTED, "%s: G=%lld span rows (needs G <= %d)", who, (long long)G, MAX_G);
  TSPN_REQUIRE(merge == MERGE_LAST || merge == MERGE_OR, TSPN_EINVAL, "%s: unknown merge=%d (0 = last, 1 = or)", who, merge);
  TSPN_REQUIRE(std::isfinite(iou_thres), TSPN_EINVAL, "%s: iou_thres is not finite", who);
  const bool offsets = pair_off && track_off && iou_off && inst_off;
  TSPN_REQUIRE(offsets || (S <= 1 && !pair_off && !track_off && !iou_off && !inst_off), TSPN_EINVAL,
               "%s: S=%lld needs pair_off, track_off, iou_off and inst_off (all null: one segment)", who, (long long)S);
  TSPN_REQUIRE(S > 0 || (P == 0 && R == 0), TSPN_EINVAL, "%s: S=0 with P=%lld pairs and R=%lld instances", who,
               (long long)P, (long long)R);
  const bool need_tracks = M > 0 && P > 0;
  TSPN_REQUIRE(P == 0 || (pairs && spans && span_count && span_labels && seg_frames && (R == 0 || (insts && inst_cols)) &&
                          (!need_tracks || trackid) && (!(need_tracks && R > 0) || iou)),
               TSPN_EINVAL, "%s: null pointer", who);
  TSPN_REQUIRE(a8(pairs) && a8(pair_off) && a8(trackid) && a8(track_off) && a8(iou_off) && a8(insts) && a8(inst_off) &&
                   a8(seg_frames) && a8(spans) && a4(iou) && a4(span_labels) && a4(span_count) && a4(inst_cols),
               TSPN_EUNSUPPORTED, "%s: unaligned pointer (int64 operands need 8 bytes, fp32 and int32 ones 4)", who);
  if (P == 0) return TSPN_OK;
  const tspn::PairTables t = {pairs, pair_off, trackid, track_off, iou, iou_off, insts, inst_off, seg_frames, S, P, M, R};
  hipLaunchKernelGGL(span_labels_kernel, dim3((unsigned)tspn::ceil_div(P * G, TILE)), dim3(TILE), 0, TSPN_STREAM(stream), t,
                     (int)K, (int)G, (float)iou_thres, merge, inst_cols, spans, span_count, span_labels,
                     tspn::aligned16(span_labels));
  return tspn::check_launch(who);
}

extern "C" int tspn_span_predicate_loss_f32(const float* feats, int64_t NT, int64_t T, int64_t D, const int64_t* pairs,
                                            const int64_t* pair_off, int64_t S, int64_t P, const int64_t* spans,
                                            const int32_t* span_count, const float* span_labels, int64_t G,
                                            const float* cls_w, const float* cls_b, int64_t K, float* q, float* dv,
                                            double* partials, double* seg_rows, void* prefix_scratch,
                                            size_t prefix_scratch_bytes, void* stream) {
  const char* who = "tspn_span_predicate_loss_f32";
  int rc = row_checks(who, NT, T, S, P, G, K, pair_off);
  if (rc) return rc;
  TSPN_REQUIRE(D > 0, TSPN_EINVAL, "%s: D=%lld features (needs D >= 1)", who, (long long)D);
  TSPN_REQUIRE(S == 0 || seg_rows, TSPN_EINVAL, "%s: null pointer", who);
  TSPN_REQUIRE(P == 0 || (pairs && spans && span_count && span_labels && q && dv && partials), TSPN_EINVAL,
               "%s: null pointer", who);
  TSPN_REQUIRE(P == 0 || NT == 0 || (feats && cls_w), TSPN_EINVAL, "%s: null pointer", who);
  TSPN_REQUIRE(a8(pairs) && a8(pair_off) && a8(spans) && a8(partials) && a8(seg_rows) && a8(prefix_scratch) &&
                   a4(span_count) && a4(span_labels) && a4(feats) && a4(cls_w) && a4(cls_b) && a4(q) && a4(dv),
               TSPN_EUNSUPPORTED, "%s: unaligned pointer (int64 and float64 operands need 8 bytes, fp32 and int32 ones 4)", who);
  if (S == 0) return TSPN_OK;
  hipStream_t st = TSPN_STREAM(stream);
  const Rows w = {pairs, pair_off, spans, span_count, S, P, NT, (int)G, (int)T};
  const float* Gp = nullptr;
  const double* PS = nullptr;
  if (P > 0 && NT > 0) {
    rc = tspn::span_prefix_stage(feats, NT, T, D, cls_w, K, prefix_scratch, prefix_scratch_bytes, stream, &Gp, &PS, who);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(span_cls_rows_kernel, dim3((unsigned)S), dim3(FIN_THREADS), 0, st, w, seg_rows);
  if ((rc = tspn::check_launch("tspn_span_predicate_loss_f32(rows)"))) return rc;
  if (P == 0) return TSPN_OK;
  hipLaunchKernelGGL(span_cls_loss_kernel, dim3((unsigned)tspn::ceil_div(P * G, WAVES)), dim3(64 * WAVES), 0, st, w, PS, Gp,
                     span_labels, cls_b, (int)K, seg_rows, q, dv, partials);
  return tspn::check_launch("tspn_span_predicate_loss_f32(loss)");
}

extern "C" int tspn_span_predicate_loss_finish(const double* partials, const double* seg_rows, const int64_t* pair_off,
                                               int64_t S, int64_t P, int64_t G, int64_t K, double* out, void* stream) {
  const char* who = "tspn_span_predicate_loss_finish";
  int rc = row_checks(who, 0, 1, S, P, G, K, pair_off);
  if (rc) return rc;
  TSPN_REQUIRE(out && (S == 0 || seg_rows) && (P == 0 || partials), TSPN_EINVAL, "%s: null pointer", who);
  TSPN_REQUIRE(a8(partials) && a8(seg_rows) && a8(pair_off) && a8(out), TSPN_EUNSUPPORTED,
               "%s: unaligned pointer (int64 and float64 operands need 8 bytes)", who);
  hipLaunchKernelGGL(span_cls_finish_kernel, dim3(1), dim3(FIN_THREADS), 0, TSPN_STREAM(stream), partials, seg_rows, pair_off,
                     S, P, (int)G, (int)K, out);
  return tspn::check_launch(who);
}

extern "C" int tspn_span_predicate_grad_f32(const float* dv, const int64_t* pairs, const int64_t* spans,
                                            const int32_t* span_count, int64_t NT, int64_t T, int64_t P, int64_t G,
                                            int64_t K, float* db, float* dG, void* prefix_scratch,
                                            size_t prefix_scratch_bytes, void* stream) {
  const char* who = "tspn_span_predicate_grad_f32";
  int rc = row_checks(who, NT, T, 1, P, G, K, nullptr);
  if (rc) return rc;
  TSPN_REQUIRE(db && (NT == 0 || dG) && (P == 0 || (dv && pairs && spans && span_count)), TSPN_EINVAL, "%s: null pointer",
               who);
  TSPN_REQUIRE(a8(pairs) && a8(spans) && a8(prefix_scratch) && a4(span_count) && a4(dv) && a4(db) && a4(dG),
               TSPN_EUNSUPPORTED, "%s: unaligned pointer (int64 and float64 operands need 8 bytes, fp32 and int32 ones 4)", who);
  const size_t need = (size_t)NT * (size_t)(T + 1) * 2 * (size_t)K * sizeof(double);
  TSPN_REQUIRE(NT == 0 || (prefix_scratch && prefix_scratch_bytes >= need), TSPN_EWORKSPACE,
               "%s: prefix_scratch %zu < %zu bytes", who, prefix_scratch_bytes, need);
  hipStream_t st = TSPN_STREAM(stream);
  hipLaunchKernelGGL(span_cls_bias_grad_kernel, dim3((unsigned)tspn::ceil_div(K, 256)), dim3(256), 0, st, dv, P * G, (int)K,
                     db);
  if ((rc = tspn::check_launch("tspn_span_predicate_grad_f32(bias)"))) return rc;
  if (NT == 0) return TSPN_OK;
  const Rows w = {pairs, nullptr, spans, span_count, 1, P, NT, (int)G, (int)T};
  hipLaunchKernelGGL(span_cls_proj_grad_kernel, dim3((unsigned)tspn::ceil_div(NT * 2 * K, 256)), dim3(256), 0, st, w, dv,
                     (int)K, static_cast<double*>(prefix_scratch), dG);
  return tspn::check_launch("tspn_span_predicate_grad_f32(proj)");
}
