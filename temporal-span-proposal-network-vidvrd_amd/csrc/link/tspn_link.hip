// Tracklet linking ("tracklet linking"), gfx950: the per-frame detections of FasterRCNNC4 become tracks by a
// deterministic IoU tracker with constant-velocity prediction, and the tracks dense boxes.  Build-defined; exact: every
// output is bit-equal to the numpy restatement (tests/link_reference.py).
//
//   tspn_link_detections_f32   the link pass.  One persistent 1024-thread workgroup per video walks its frames: no launch
//                              and no host synchronisation per frame.  Per frame: (A) the live list, compact and ascending
//                              by id in the caller's scratch, drops the tracks that died and takes this frame's predicted
//                              boxes; (B) the frame's candidates go to LDS; (C) the greedy match runs as rounds of mutual
//                              best -- a wave per live track scans the candidates, its best edge by a wave reduction, a
//                              candidate's best edge by a 64-bit LDS atomicMax on (IoU bits, ~slot), and every pair whose
//                              two bests agree is taken -- until a round takes nothing; no L x D matrix is stored; (D) the
//                              matched tracks update; (E) the unmatched candidates start tracks, in ascending d, while
//                              slots and ids last.
//   tspn_link_fill_f32         the fill pass: the selected tracks' hit table by a scatter of track_of_det, then one wave
//                              per selected track writes its boxes and states, interpolating inside [first, last].
//
// The IoU is the expression of suppresses() in detect/tspn_detect.hip with the track as i and the detection as j; the
// prediction and the interpolation are written in the design's statement order; the library is built with
// -ffp-contract=off and a true division.  iou_thresh > 0 makes the fp32 bits of a passing IoU monotone in its value.
#include <cmath>

#include "tspn_common.h"

namespace {

using u64 = unsigned long long;

constexpr int kWave = 64;
constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / kWave;
constexpr int kMaxD = 1024;          // detections per frame: the limit of tspn_detections_topk_f32
constexpr int kMaxLive = 4096;       // live tracks per video
constexpr int kOffChunk = 256;       // video offsets per launch of the offsets kernel (2 KB of kernarg)
constexpr int kFree = -1, kNoCandidate = -2;

__device__ inline bool finite_f32(float v) { return fabsf(v) <= 3.402823466e38f; }   // false for NaN

// suppresses() of detect/tspn_detect.hip up to its comparison: bi the track's predicted box, bj the detection
__device__ inline float link_iou(float4 bi, float iarea, float4 bj) {
  const float jarea = (bj.z - bj.x) * (bj.w - bj.y);
  const float xx1 = bi.x < bj.x ? bj.x : bi.x, yy1 = bi.y < bj.y ? bj.y : bi.y;
  const float xx2 = bj.z < bi.z ? bj.z : bi.z, yy2 = bj.w < bi.w ? bj.w : bi.w;
  const float dw = xx2 - xx1, dh = yy2 - yy1;
  const float w = 0.f < dw ? dw : 0.f, h = 0.f < dh ? dh : 0.f;
  const float inter = w * h;
  return inter / (iarea + jarea - inter);
}

__device__ inline float4 sub4(float4 a, float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }

// last + (last - prev) / float(t_last - t_prev) * float(t - t_last), per coordinate
__device__ inline float4 predict_box(float4 last, float4 prev, int t_last, int t_prev, int hits, int t) {
  if (hits < 2) return last;
  const float den = (float)(t_last - t_prev), ahead = (float)(t - t_last);
  const float4 d = sub4(last, prev);
  return make_float4(last.x + d.x / den * ahead, last.y + d.y / den * ahead, last.z + d.z / den * ahead,
                     last.w + d.w / den * ahead);
}

// a + (b - a) * (float(t - ta) / float(tb - ta)), per coordinate
__device__ inline float4 interpolate_box(float4 a, float4 b, int ta, int tb, int t) {
  const float w = (float)(t - ta) / (float)(tb - ta);
  const float4 d = sub4(b, a);
  return make_float4(a.x + d.x * w, a.y + d.y * w, a.z + d.z * w, a.w + d.w * w);
}

struct OffChunk {
  int64_t v[kOffChunk];
};

__global__ __launch_bounds__(kOffChunk) void link_offsets_kernel(OffChunk c, int count, int64_t* __restrict__ dst) {
  if ((int)threadIdx.x < count) dst[threadIdx.x] = c.v[threadIdx.x];
}

// The live list of one video in the scratch: five arrays of 16-byte records, max_live slots per video, V * max_live
// records apart.  The kernel reads slots below its live count only, all of which it has written.
// meta: x id, y t_last, z t_prev, w hits;  sum: x the class, y the bits of the float64 score sum
struct LiveState {
  float4* last;
  float4* prev;
  float4* pred;
  int4* meta;
  longlong2* sum;
};

// offsets int64 [V + 1] | last | prev | pred | meta | sum, each [V, max_live] x 16 bytes
struct LinkLayout {
  size_t off, state, total;
};

LinkLayout link_layout(int64_t V, int64_t max_live) {
  LinkLayout lay;
  lay.off = 0;
  lay.state = tspn::align_up((size_t)(V + 1) * sizeof(int64_t), 256);
  lay.total = lay.state + tspn::align_up(5 * (size_t)V * (size_t)max_live * 16, 256);
  return lay;
}

struct LinkParams {
  float iou_thresh, min_score;
  int max_age, min_hits, class_aware, max_live, max_tracks, D;
};

struct LinkLds {
  float4 cbox[kMaxD];          // this frame's detections
  int64_t ccls[kMaxD];
  u64 colbest[kMaxD];          // per candidate: (IoU bits << 32) | ~slot of its best track this round
  float cscore[kMaxD];
  int32_t dslot[kMaxD];        // kFree, kNoCandidate, or the slot of the track that took the detection
  int16_t rowd[kMaxLive];      // per slot: its best candidate this round, -1: no edge
  int16_t tmatch[kMaxLive];    // per slot: the detection it took this frame, -1: none
  int32_t wsum[kWaves];
};

// exclusive rank of the threads with `flag` in thread order, and their number; two barriers
__device__ inline int block_rank(bool flag, int32_t* wsum, int* total) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const u64 b = __ballot(flag);
  if (lane == 0) wsum[wave] = __popcll(b);
  __syncthreads();
  int before = 0, all = 0;
  for (int w = 0; w < kWaves; ++w) {
    const int n = wsum[w];
    before += w < wave ? n : 0;
    all += n;
  }
  __syncthreads();
  *total = all;
  return before + __popcll(b & ((1ull << lane) - 1ull));
}

// ---- tspn_link_detections_f32: one workgroup per video
__global__ __launch_bounds__(kThreads) void link_detections_kernel(
    const float4* __restrict__ boxes, const float* __restrict__ scores, const int64_t* __restrict__ classes,
    const int64_t* __restrict__ count, const int64_t* off, LinkParams p, char* state, int32_t* __restrict__ track_of_det,
    int64_t* __restrict__ n_tracks, int64_t* __restrict__ dropped, int32_t* __restrict__ trk_first,
    int32_t* __restrict__ trk_last, int32_t* __restrict__ trk_hits, int64_t* __restrict__ trk_cls,
    float* __restrict__ trk_score) {
  __shared__ LinkLds S;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t v = blockIdx.x;
  const int64_t f0 = off[v];
  const int Fv = (int)(off[v + 1] - f0);
  const int D = p.D;
  const size_t slots = (size_t)gridDim.x * p.max_live, base = (size_t)v * p.max_live;
  float4* const rec = reinterpret_cast<float4*>(state) + base;
  const LiveState st = {rec, rec + slots, rec + 2 * slots, reinterpret_cast<int4*>(rec + 3 * slots),
                        reinterpret_cast<longlong2*>(rec + 4 * slots)};
  const size_t tb = (size_t)v * p.max_tracks;
  int L = 0, n_ids = 0;
  int64_t n_dropped = 0;
  for (int t = 0; t < Fv; ++t) {
    const int64_t f = f0 + t;
    // (A) drop what died, keep the rest in order, predict
    int kept = 0;
    for (int c0 = 0; c0 < L; c0 += kThreads) {
      const int s = c0 + tid;
      bool alive = false;
      float4 last = make_float4(0.f, 0.f, 0.f, 0.f), prev = last;
      int4 m = make_int4(0, 0, 0, 0);
      longlong2 cs = make_longlong2(0, 0);
      if (s < L) {
        last = st.last[s], prev = st.prev[s], m = st.meta[s], cs = st.sum[s];
        alive = m.w >= p.min_hits ? t - m.y <= p.max_age : t - m.y == 1;
      }
      int n_alive;
      const int to = kept + block_rank(alive, S.wsum, &n_alive);     // its barrier: every load above is done
      if (alive) {
        if (to != s) st.last[to] = last, st.prev[to] = prev, st.meta[to] = m, st.sum[to] = cs;
        st.pred[to] = predict_box(last, prev, m.y, m.z, m.w, t);
      }
      kept += n_alive;
    }
    L = kept;
    // (B) the candidates
    int64_t n = count[f];
    n = n < 0 ? 0 : (n > D ? D : n);
    bool cand = false;
    if (tid < D) {
      const float4 b = boxes[f * D + tid];
      const float sc = scores[f * D + tid];
      cand = tid < n && finite_f32(b.x) && finite_f32(b.y) && finite_f32(b.z) && finite_f32(b.w) && finite_f32(sc) &&
             sc >= p.min_score;
      S.cbox[tid] = b;
      S.cscore[tid] = sc;
      S.ccls[tid] = classes[f * D + tid];
      S.dslot[tid] = cand ? kFree : kNoCandidate;
    }
    for (int s = tid; s < L; s += kThreads) S.tmatch[s] = -1;
    const bool any_cand = __syncthreads_or(cand) != 0;
    // (C) rounds of mutual best
    while (L > 0 && any_cand) {
      if (tid < D) S.colbest[tid] = 0;
      __syncthreads();
      for (int i = wave; i < L; i += kWaves) {
        if (S.tmatch[i] >= 0) continue;                    // wave-uniform
        const float4 pb = st.pred[i];
        const int64_t cls = st.sum[i].x;
        const float iarea = (pb.z - pb.x) * (pb.w - pb.y);
        u64 best = 0;
        for (int d = lane; d < (int)n; d += kWave) {
          if (S.dslot[d] != kFree || (p.class_aware && S.ccls[d] != cls)) continue;
          const float iou = link_iou(pb, iarea, S.cbox[d]);
          if (iou >= p.iou_thresh) {
            const u64 bits = (u64)__float_as_uint(iou) << 32;
            const u64 key = bits | (unsigned)~d;
            best = key > best ? key : best;
            atomicMax(&S.colbest[d], bits | (unsigned)~i);
          }
        }
        best = tspn::wave_max_u64(best);
        if (lane == 0) S.rowd[i] = best != 0 ? (int16_t)(~(unsigned)best) : (int16_t)-1;
      }
      __syncthreads();
      bool took = false;
      for (int i = tid; i < L; i += kThreads) {
        if (S.tmatch[i] >= 0) continue;
        const int d = S.rowd[i];
        if (d >= 0 && (unsigned)S.colbest[d] == (unsigned)~i) {
          S.tmatch[i] = (int16_t)d;
          S.dslot[d] = i;
          took = true;
        }
      }
      if (!__syncthreads_or(took)) break;
    }
    // (D) the matched tracks
    for (int i = tid; i < L; i += kThreads) {
      const int d = S.tmatch[i];
      if (d < 0) continue;
      const int4 m = st.meta[i];
      const longlong2 cs = st.sum[i];
      const int id = m.x, hits = m.w + 1;
      const double ssum = __longlong_as_double(cs.y) + (double)S.cscore[d];
      st.prev[i] = st.last[i];
      st.last[i] = S.cbox[d];
      st.meta[i] = make_int4(id, t, m.y, hits);
      st.sum[i] = make_longlong2(cs.x, __double_as_longlong(ssum));
      trk_last[tb + id] = t;
      trk_hits[tb + id] = hits;
      trk_score[tb + id] = (float)(ssum / (double)hits);
      track_of_det[f * D + d] = id;
    }
    // (E) births, in ascending d
    const bool orphan = tid < D && S.dslot[tid] == kFree;
    int n_orphans;
    const int r = block_rank(orphan, S.wsum, &n_orphans);
    int room = p.max_live - L < p.max_tracks - n_ids ? p.max_live - L : p.max_tracks - n_ids;
    room = room < n_orphans ? room : n_orphans;
    if (tid < D && S.dslot[tid] < 0) {
      const bool born = orphan && r < room;
      if (born) {
        const int s = L + r, id = n_ids + r;
        st.last[s] = S.cbox[tid], st.prev[s] = S.cbox[tid];
        st.meta[s] = make_int4(id, t, t, 1);
        st.sum[s] = make_longlong2(S.ccls[tid], __double_as_longlong((double)S.cscore[tid]));
        trk_first[tb + id] = t, trk_last[tb + id] = t, trk_hits[tb + id] = 1;
        trk_cls[tb + id] = S.ccls[tid];
        trk_score[tb + id] = (float)((double)S.cscore[tid] / 1.0);
      }
      track_of_det[f * D + tid] = born ? n_ids + r : -1;
    }
    L += room;
    n_ids += room;
    n_dropped += n_orphans - room;
    __syncthreads();            // the slots and the LDS of this frame are settled before the next one reads them
  }
  for (int k = n_ids + tid; k < p.max_tracks; k += kThreads) {
    trk_first[tb + k] = -1, trk_last[tb + k] = -1, trk_hits[tb + k] = 0;
    trk_cls[tb + k] = -1;
    trk_score[tb + k] = 0.f;
  }
  if (tid == 0) {
    n_tracks[v] = n_ids;
    dropped[v] = n_dropped;
  }
}

// ---- tspn_link_fill_f32
// scratch: offsets int64 [V + 1] | rowof int32 [V, max_tracks]: the lowest selected row of a track, INT_MAX: not selected |
// hit int32 [R, Fmax]: the detection of the row's track at a frame, -1: none
struct FillLayout {
  size_t off, rowof, hit, total;
};

FillLayout fill_layout(int64_t V, int64_t max_tracks, int64_t R, int64_t Fmax) {
  FillLayout lay;
  lay.off = 0;
  lay.rowof = tspn::align_up((size_t)(V + 1) * sizeof(int64_t), 256);
  lay.hit = lay.rowof + tspn::align_up((size_t)V * max_tracks * sizeof(int32_t), 256);
  lay.total = lay.hit + tspn::align_up((size_t)R * Fmax * sizeof(int32_t), 256);
  return lay;
}

constexpr int32_t kNoRow = 0x7fffffff;

__global__ __launch_bounds__(256) void link_fill_clear_kernel(int32_t* __restrict__ rowof, int64_t n_rowof,
                                                              int32_t* __restrict__ hit, int64_t n_hit) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_rowof) rowof[i] = kNoRow;
  if (i < n_hit) hit[i] = -1;
}

__global__ __launch_bounds__(256) void link_fill_rows_kernel(const int64_t* __restrict__ sel_video,
                                                             const int64_t* __restrict__ sel_track, int64_t R, int64_t V,
                                                             int64_t max_tracks, int32_t* rowof) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const int64_t v = sel_video[r], k = sel_track[r];
  if (v >= 0 && v < V && k >= 0 && k < max_tracks) atomicMin(&rowof[v * max_tracks + k], (int32_t)r);
}

// one thread per detection slot: the frame's video by bisection of the offsets
__global__ __launch_bounds__(256) void link_fill_scatter_kernel(const int32_t* __restrict__ track_of_det,
                                                                const int64_t* __restrict__ off,
                                                                const int32_t* __restrict__ rowof, int64_t V, int64_t F,
                                                                int64_t D, int64_t max_tracks, int64_t Fmax,
                                                                int32_t* __restrict__ hit) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= F * D) return;
  const int64_t k = track_of_det[i];
  if (k < 0 || k >= max_tracks) return;
  const int64_t f = i / D;
  int64_t lo = 0, hi = V - 1;                  // the last video with off[v] <= f
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) / 2;
    if (off[mid] <= f)
      lo = mid;
    else
      hi = mid - 1;
  }
  const int32_t r = rowof[lo * max_tracks + k];
  if (r != kNoRow) hit[(int64_t)r * Fmax + (f - off[lo])] = (int32_t)(i - f * D);
}

// one wave per selected row
__global__ __launch_bounds__(kWave) void link_fill_kernel(const float4* __restrict__ boxes,
                                                          const int64_t* __restrict__ sel_video,
                                                          const int64_t* __restrict__ sel_track,
                                                          const int32_t* __restrict__ trk_first,
                                                          const int32_t* __restrict__ trk_last,
                                                          const int64_t* __restrict__ off,
                                                          const int32_t* __restrict__ rowof,
                                                          const int32_t* __restrict__ hit, int64_t V, int64_t D,
                                                          int64_t max_tracks, int64_t Fmax, float4* __restrict__ out_boxes,
                                                          uint8_t* __restrict__ out_state) {
  const int64_t r = blockIdx.x;
  const int64_t v = sel_video[r], k = sel_track[r];
  const bool known = v >= 0 && v < V && k >= 0 && k < max_tracks;
  int first = 0, last = -1, Fv = 0;
  int64_t f0 = 0;
  const int32_t* h = hit;
  if (known) {
    const int32_t r0 = rowof[v * max_tracks + k];          // the row that holds the track's hits: r, or a lower twin
    f0 = off[v];
    Fv = (int)(off[v + 1] - f0);
    first = trk_first[v * max_tracks + k], last = trk_last[v * max_tracks + k];
    first = first < 0 ? 0 : first;
    last = last > Fv - 1 ? Fv - 1 : last;
    h = hit + (int64_t)r0 * Fmax;
  }
  for (int t = threadIdx.x; t < Fmax; t += kWave) {
    float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
    uint8_t state = 0;
    if (t >= first && t <= last) {
      if (h[t] >= 0) {
        b = boxes[(f0 + t) * D + h[t]];
        state = 1;
      } else {
        int ta = t - 1, tn = t + 1;
        while (ta >= first && h[ta] < 0) --ta;
        while (tn <= last && h[tn] < 0) ++tn;
        if (ta >= first && tn <= last) {
          b = interpolate_box(boxes[(f0 + ta) * D + h[ta]], boxes[(f0 + tn) * D + h[tn]], ta, tn, t);
          state = 2;
        }
      }
    }
    out_boxes[r * Fmax + t] = b;
    out_state[r * Fmax + t] = state;
  }
}

// the video offsets: host checks, then 256 per launch by value into the scratch
int check_offsets(const char* who, const int64_t* video_off, int64_t V, int64_t F, int64_t* Fmax) {
  TSPN_REQUIRE(video_off != nullptr, TSPN_EINVAL, "%s: null pointer", who);
  bool sorted = video_off[0] == 0;
  int64_t longest = 0;
  for (int64_t v = 0; v < V && sorted; ++v) {
    const int64_t len = video_off[v + 1] - video_off[v];
    sorted = len >= 0;
    longest = len > longest ? len : longest;
  }
  TSPN_REQUIRE(sorted && video_off[V] == F, TSPN_EINVAL, "%s: video_off must ascend from 0 to F=%lld", who, (long long)F);
  *Fmax = longest;
  return TSPN_OK;
}

void send_offsets(const int64_t* video_off, int64_t V, int64_t* d_off, hipStream_t st) {
  for (int64_t at = 0; at <= V; at += kOffChunk) {
    OffChunk c;
    const int count = (int)(V + 1 - at < kOffChunk ? V + 1 - at : kOffChunk);
    for (int k = 0; k < kOffChunk; ++k) c.v[k] = k < count ? video_off[at + k] : 0;
    hipLaunchKernelGGL(link_offsets_kernel, dim3(1), dim3(kOffChunk), 0, st, c, count, d_off + at);
  }
}

int link_sizes(const char* who, int64_t V, int64_t F, int64_t D, int64_t max_live, int64_t max_tracks) {
  TSPN_REQUIRE(V >= 0 && F >= 0 && D >= 1 && max_live >= 1 && max_tracks >= 1, TSPN_EINVAL,
               "%s: bad sizes V=%lld F=%lld D=%lld max_live=%lld max_tracks=%lld", who, (long long)V, (long long)F,
               (long long)D, (long long)max_live, (long long)max_tracks);
  TSPN_REQUIRE(D <= kMaxD, TSPN_EUNSUPPORTED, "%s: D=%lld > %d", who, (long long)D, kMaxD);
  TSPN_REQUIRE(max_live <= kMaxLive, TSPN_EUNSUPPORTED, "%s: max_live=%lld > %d", who, (long long)max_live, kMaxLive);
  TSPN_REQUIRE(V < ((int64_t)1 << 24) && F < ((int64_t)1 << 31) / kMaxD && max_tracks < ((int64_t)1 << 24) &&
                   V * max_tracks < ((int64_t)1 << 31),
               TSPN_EUNSUPPORTED, "%s: dimension too large", who);
  return TSPN_OK;
}

}  // namespace

extern "C" size_t tspn_link_scratch_bytes(int64_t V, int64_t max_live, int64_t max_tracks, int64_t R, int64_t Fmax,
                                          int fill) {
  if (V <= 0 || max_tracks < 1 || max_tracks >= ((int64_t)1 << 24) || V >= ((int64_t)1 << 24) ||
      V * max_tracks >= ((int64_t)1 << 31))
    return 0;
  if (fill) {
    if (R <= 0 || Fmax < 0 || Fmax >= ((int64_t)1 << 31) / kMaxD || R * (Fmax > 0 ? Fmax : 1) >= ((int64_t)1 << 31)) return 0;
    return fill_layout(V, max_tracks, R, Fmax).total;
  }
  if (max_live < 1 || max_live > kMaxLive) return 0;
  return link_layout(V, max_live).total;
}

extern "C" int tspn_link_detections_f32(const float* boxes, const float* scores, const int64_t* classes,
                                        const int64_t* count, const int64_t* video_off, int64_t V, int64_t F, int64_t D,
                                        float iou_thresh, int64_t max_age, int64_t min_hits, float min_score,
                                        int class_aware, int64_t max_live, int64_t max_tracks, int32_t* track_of_det,
                                        int64_t* n_tracks, int64_t* dropped, int32_t* trk_first, int32_t* trk_last,
                                        int32_t* trk_hits, int64_t* trk_cls, float* trk_score, void* scratch,
                                        size_t scratch_bytes, void* stream) {
  const char* who = "tspn_link_detections_f32";
  if (int rc = link_sizes(who, V, F, D, max_live, max_tracks)) return rc;
  TSPN_REQUIRE(iou_thresh > 0.f && iou_thresh <= 1.f, TSPN_EINVAL, "%s: iou_thresh must lie in (0, 1]", who);
  TSPN_REQUIRE(max_age >= 0 && max_age < ((int64_t)1 << 31) && min_hits >= 1 && min_hits < ((int64_t)1 << 31) &&
                   min_score == min_score,
               TSPN_EINVAL, "%s: needs max_age >= 0, min_hits >= 1 and min_score a number", who);
  int64_t Fmax;
  if (int rc = check_offsets(who, video_off, V, F, &Fmax)) return rc;
  if (V == 0) return TSPN_OK;
  TSPN_REQUIRE((F == 0 || (boxes && scores && classes && count && track_of_det)) && n_tracks && dropped && trk_first &&
                   trk_last && trk_hits && trk_cls && trk_score,
               TSPN_EINVAL, "%s: null pointer", who);
  TSPN_REQUIRE(tspn::all_aligned16(boxes, scratch), TSPN_EUNSUPPORTED, "%s: boxes and scratch must be 16-byte aligned", who);
  const LinkLayout lay = link_layout(V, max_live);
  TSPN_REQUIRE(scratch != nullptr && scratch_bytes >= lay.total, TSPN_EWORKSPACE, "%s: scratch %zu < %zu bytes", who,
               scratch != nullptr ? scratch_bytes : (size_t)0, lay.total);
  char* base = static_cast<char*>(scratch);
  int64_t* d_off = reinterpret_cast<int64_t*>(base + lay.off);
  hipStream_t st = TSPN_STREAM(stream);
  send_offsets(video_off, V, d_off, st);
  const LinkParams p = {iou_thresh, min_score, (int)max_age, (int)min_hits, class_aware != 0, (int)max_live, (int)max_tracks,
                        (int)D};
  hipLaunchKernelGGL(link_detections_kernel, dim3((unsigned)V), dim3(kThreads), 0, st,
                     reinterpret_cast<const float4*>(boxes), scores, classes, count, d_off, p, base + lay.state, track_of_det, n_tracks,
                     dropped, trk_first, trk_last, trk_hits, trk_cls, trk_score);
  return tspn::check_launch(who);
}

extern "C" int tspn_link_fill_f32(const float* boxes, const int32_t* track_of_det, const int64_t* video_off, int64_t V,
                                  int64_t F, int64_t D, const int32_t* trk_first, const int32_t* trk_last,
                                  int64_t max_tracks, const int64_t* sel_video, const int64_t* sel_track, int64_t R,
                                  float* out_boxes, uint8_t* out_state, void* scratch, size_t scratch_bytes, void* stream) {
  const char* who = "tspn_link_fill_f32";
  if (int rc = link_sizes(who, V, F, D, 1, max_tracks)) return rc;
  TSPN_REQUIRE(R >= 0, TSPN_EINVAL, "%s: bad sizes R=%lld", who, (long long)R);
  int64_t Fmax;
  if (int rc = check_offsets(who, video_off, V, F, &Fmax)) return rc;
  if (R == 0 || Fmax == 0) return TSPN_OK;
  TSPN_REQUIRE(R * Fmax < ((int64_t)1 << 31), TSPN_EUNSUPPORTED, "%s: dimension too large", who);
  TSPN_REQUIRE(boxes && track_of_det && trk_first && trk_last && sel_video && sel_track && out_boxes && out_state,
               TSPN_EINVAL, "%s: null pointer", who);
  TSPN_REQUIRE(tspn::all_aligned16(boxes, out_boxes, scratch), TSPN_EUNSUPPORTED,
               "%s: boxes, out_boxes and scratch must be 16-byte aligned", who);
  const FillLayout lay = fill_layout(V, max_tracks, R, Fmax);
  TSPN_REQUIRE(scratch != nullptr && scratch_bytes >= lay.total, TSPN_EWORKSPACE, "%s: scratch %zu < %zu bytes", who,
               scratch != nullptr ? scratch_bytes : (size_t)0, lay.total);
  char* base = static_cast<char*>(scratch);
  int64_t* d_off = reinterpret_cast<int64_t*>(base + lay.off);
  int32_t* rowof = reinterpret_cast<int32_t*>(base + lay.rowof);
  int32_t* hit = reinterpret_cast<int32_t*>(base + lay.hit);
  hipStream_t st = TSPN_STREAM(stream);
  send_offsets(video_off, V, d_off, st);
  const int64_t n_rowof = V * max_tracks, n_hit = R * Fmax;
  const int64_t n_clear = n_rowof > n_hit ? n_rowof : n_hit;
  hipLaunchKernelGGL(link_fill_clear_kernel, dim3((unsigned)tspn::ceil_div(n_clear, 256)), dim3(256), 0, st, rowof, n_rowof,
                     hit, n_hit);
  hipLaunchKernelGGL(link_fill_rows_kernel, dim3((unsigned)tspn::ceil_div(R, 256)), dim3(256), 0, st, sel_video, sel_track, R,
                     V, max_tracks, rowof);
  hipLaunchKernelGGL(link_fill_scatter_kernel, dim3((unsigned)tspn::ceil_div(F * D, 256)), dim3(256), 0, st, track_of_det,
                     d_off, rowof, V, F, D, max_tracks, Fmax, hit);
  hipLaunchKernelGGL(link_fill_kernel, dim3((unsigned)R), dim3(kWave), 0, st, reinterpret_cast<const float4*>(boxes),
                     sel_video, sel_track, trk_first, trk_last, d_off, rowof, hit, V, D, max_tracks, Fmax,
                     reinterpret_cast<float4*>(out_boxes), out_state);
  return tspn::check_launch(who);
}
