// Per-frame object detection, the post-processing of detectron2 v0.6's faster_rcnn_R_*_C4 ("box decode",
// "box NMS", "proposals", "detections"), gfx950.  Three staged entries and the final gather:
//
//   tspn_rpn_decode_f32        anchors + RPN deltas -> boxes (Box2BoxTransform.apply_deltas, weights 1), clipped, with the
//                              gathered logits and a validity byte per row.  Inexact (expf).
//   tspn_box_head_decode_f32   softmax over K+1 logits, class-specific deltas on the proposals, clipped; class-major
//                              scores [B,K,R], boxes [B,K,R,4] and validity bytes [B,K,R].  Inexact (expf).
//   tspn_box_nms_f32           exact.  Per contiguous group of candidates: top-pre_topk by tspn::select_topk_sorted at
//                              the 8192 capacity, invalid / small rows dropped, torchvision's greedy NMS in fp32, the first
//                              post_topk survivors.  boxes == null: the selection alone.
//   tspn_detections_topk_f32   exact.  Per image the D best NMS survivors over its K class groups, ties by r * K + c.
//
// The NMS runs in three kernels over the caller's scratch (tspn_box_nms_scratch_bytes): (1) one 1024-thread workgroup
// per group selects and sorts, and writes the sorted flat indices (-1: dropped) and boxes; (2) 64 x 64 tiles of the upper
// triangle write one 64-bit suppression word per (row, column block); (3) one wave per group resolves a 64-candidate
// diagonal block in registers, then ORs the kept rows' words over the remaining column blocks: the dependent chain is
// M / 64 long.  Every scratch byte a kernel reads was written by a kernel of the same call.
//
// The IoU is torchvision's CPU kernel (ops/cpu/nms_kernel.cpp) in fp32, operation for operation, with a true division;
// the library is built with -ffp-contract=off.
#include <cmath>

#include "tspn_topk_select.h"

namespace {

using tspn::order_key;
using u64 = unsigned long long;

constexpr int kWave = 64;
constexpr int kMaxPre = tspn::kSelectMaxMBig;
constexpr int kOffChunk = 256;                       // group offsets per launch of the offsets kernel (2 KB of kernarg)
constexpr float kScaleClamp = 4.135166556742356f;    // log(1000 / 16), detectron2's _DEFAULT_SCALE_CLAMP

__device__ inline bool finite_f32(float v) { return fabsf(v) <= 3.402823466e38f; }   // false for NaN

// torch.clamp(v, min=0, max=hi): a NaN stays a NaN
__device__ inline float clip_f32(float v, float hi) {
  v = v < 0.f ? 0.f : v;
  return v > hi ? hi : v;
}

// Box2BoxTransform.apply_deltas on one box, in detectron2's statement order; `fin`: all four corners finite (before the
// clip, as find_top_rpn_proposals and fast_rcnn_inference test them)
__device__ inline float4 apply_deltas(float4 b, float dx, float dy, float dw, float dh, float wx, float wy, float ww,
                                      float wh, float img_h, float img_w, bool* fin) {
  const float w = b.z - b.x, h = b.w - b.y;
  const float cx = b.x + 0.5f * w, cy = b.y + 0.5f * h;
  dx = dx / wx;
  dy = dy / wy;
  dw = dw / ww;
  dh = dh / wh;
  dw = dw > kScaleClamp ? kScaleClamp : dw;   // torch.clamp(max=): a NaN stays
  dh = dh > kScaleClamp ? kScaleClamp : dh;
  const float pcx = dx * w + cx, pcy = dy * h + cy;
  const float pw = expf(dw) * w, ph = expf(dh) * h;
  const float x1 = pcx - 0.5f * pw, y1 = pcy - 0.5f * ph, x2 = pcx + 0.5f * pw, y2 = pcy + 0.5f * ph;
  *fin = finite_f32(x1) && finite_f32(y1) && finite_f32(x2) && finite_f32(y2);
  return make_float4(clip_f32(x1, img_w), clip_f32(y1, img_h), clip_f32(x2, img_w), clip_f32(y2, img_h));
}

// ---- tspn_rpn_decode_f32: one thread per (image, candidate)
__global__ __launch_bounds__(256) void rpn_decode_f32_kernel(const int64_t* __restrict__ cand,
                                                             const float* __restrict__ logits,
                                                             const float* __restrict__ deltas,
                                                             const float* __restrict__ cell,
                                                             const float* __restrict__ image_sizes, int64_t B, int W,
                                                             int A, int64_t HWA, int64_t M, float stride,
                                                             float4* __restrict__ out_boxes,
                                                             float* __restrict__ out_logits,
                                                             uint8_t* __restrict__ out_valid) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= B * M) return;
  const int64_t b = t / M;
  const int64_t i = cand != nullptr ? cand[t] - b * HWA : t - b * M;
  float4 box = make_float4(0.f, 0.f, 0.f, 0.f);
  float logit = 0.f;
  bool ok = false;
  if (i >= 0 && i < HWA) {
    const int a = (int)(i % A);
    const int64_t cellidx = i / A;
    const float sx = (float)(cellidx % W) * stride, sy = (float)(cellidx / W) * stride;
    const float4 anchor = make_float4(sx + cell[4 * a], sy + cell[4 * a + 1], sx + cell[4 * a + 2], sy + cell[4 * a + 3]);
    const float* d = deltas + (b * HWA + i) * 4;    // [B,H,W,4A], channel 4a + k
    logit = logits[b * HWA + i];
    bool fin;
    box = apply_deltas(anchor, d[0], d[1], d[2], d[3], 1.f, 1.f, 1.f, 1.f, image_sizes[2 * b], image_sizes[2 * b + 1], &fin);
    ok = fin && finite_f32(logit);
    if (!ok) {
      box = make_float4(0.f, 0.f, 0.f, 0.f);
      logit = 0.f;
    }
  }
  out_boxes[t] = box;
  out_logits[t] = logit;
  out_valid[t] = ok ? 1 : 0;
}

// ---- tspn_box_head_decode_f32: one thread per (image, proposal); consecutive lanes write consecutive r of a class row
__global__ __launch_bounds__(256) void box_head_decode_f32_kernel(const float* __restrict__ cls_logits,
                                                                  const float* __restrict__ deltas,
                                                                  const float4* __restrict__ proposals,
                                                                  const int64_t* __restrict__ proposal_count,
                                                                  const float* __restrict__ image_sizes, int64_t B,
                                                                  int64_t R, int K, float wx, float wy, float ww, float wh,
                                                                  float score_thresh, float* __restrict__ out_scores,
                                                                  float4* __restrict__ out_boxes,
                                                                  uint8_t* __restrict__ out_valid) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= B * R) return;
  const int64_t b = t / R, r = t - b * R;
  const int64_t o0 = b * K * R + r;        // (b, class 0, r); a class further is R further
  if (r >= proposal_count[b]) {
    for (int c = 0; c < K; ++c) {
      out_scores[o0 + c * R] = 0.f;
      out_boxes[o0 + c * R] = make_float4(0.f, 0.f, 0.f, 0.f);
      out_valid[o0 + c * R] = 0;
    }
    return;
  }
  const float* z = cls_logits + t * (K + 1);
  float m = z[0];
  for (int j = 1; j <= K; ++j) m = fmaxf(m, z[j]);
  float sum = 0.f;
  for (int j = 0; j <= K; ++j) sum += expf(z[j] - m);
  const float4 p = proposals[t];
  const float img_h = image_sizes[2 * b], img_w = image_sizes[2 * b + 1];
  bool row_ok = finite_f32(sum);           // a NaN, a +Inf or K+1 times -Inf among the logits makes the sum a NaN
  const float* d = deltas + t * 4 * K;
  for (int c = 0; c < K; ++c) {
    bool fin;
    out_boxes[o0 + c * R] = apply_deltas(p, d[4 * c], d[4 * c + 1], d[4 * c + 2], d[4 * c + 3], wx, wy, ww, wh, img_h, img_w, &fin);
    row_ok = row_ok && fin;
  }
  for (int c = 0; c < K; ++c) {
    const float s = expf(z[c] - m) / sum;
    const bool ok = row_ok && s > score_thresh;
    out_scores[o0 + c * R] = ok ? s : 0.f;
    out_valid[o0 + c * R] = ok ? 1 : 0;
    if (!row_ok) out_boxes[o0 + c * R] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// ---- tspn_box_nms_f32
struct OffChunk {
  int64_t v[kOffChunk];
};

__global__ __launch_bounds__(kOffChunk) void box_nms_offsets_kernel(OffChunk c, int count, int64_t* __restrict__ dst) {
  if ((int)threadIdx.x < count) dst[threadIdx.x] = c.v[threadIdx.x];
}

// (1) per group: the M = min(pre_topk, n) best candidates in selection order.  SELECT_ONLY: they are the result.
template <bool SELECT_ONLY>
__global__ __launch_bounds__(tspn::kSelectThreads) void box_nms_select_kernel(
    const float* __restrict__ scores, const uint8_t* __restrict__ valid, const float4* __restrict__ boxes,
    const int64_t* __restrict__ off, int pre_topk, int cap, float min_size, int post_topk, int32_t* __restrict__ selcount,
    int32_t* __restrict__ sidx, float4* __restrict__ sbox, uint8_t* __restrict__ out_keep, int64_t* __restrict__ out_index,
    int64_t* __restrict__ out_count) {
  __shared__ tspn::SelectLdsBig L;
  const int g = blockIdx.x, tid = threadIdx.x;
  const int64_t o = off[g];
  const int n = (int)(off[g + 1] - o);
  const int M = n < pre_topk ? n : pre_topk;      // <= cap: cap = min(pre_topk, the largest group)
  const float* s = scores + o;
  if (M > 0) tspn::select_topk_sorted(L, [s](int i) { return order_key(s[i]); }, n, M);
  if (SELECT_ONLY) {
    for (int r = tid; r < post_topk; r += tspn::kSelectThreads)
      out_index[(int64_t)g * post_topk + r] = r < M ? o + L.ki[r] : (int64_t)-1;
    if (tid == 0) out_count[g] = M < post_topk ? M : post_topk;
    return;
  }
  if (out_keep != nullptr)
    for (int i = tid; i < n; i += tspn::kSelectThreads) out_keep[o + i] = 0;
  for (int r = tid; r < M; r += tspn::kSelectThreads) {
    const int64_t flat = o + L.ki[r];
    const float4 bx = boxes[flat];
    bool ok = valid == nullptr || valid[flat] != 0;
    if (min_size >= 0.f) ok = ok && (bx.z - bx.x) > min_size && (bx.w - bx.y) > min_size;
    sidx[(int64_t)g * cap + r] = ok ? (int32_t)flat : -1;
    sbox[(int64_t)g * cap + r] = bx;
  }
  if (tid == 0) selcount[g] = M;
}

// torchvision nms_kernel_impl: is candidate j suppressed by the kept candidate i
__device__ inline bool suppresses(float4 bi, float iarea, float4 bj, float thr) {
  const float jarea = (bj.z - bj.x) * (bj.w - bj.y);
  const float xx1 = bi.x < bj.x ? bj.x : bi.x, yy1 = bi.y < bj.y ? bj.y : bi.y;     // std::max(i, j)
  const float xx2 = bj.z < bi.z ? bj.z : bi.z, yy2 = bj.w < bi.w ? bj.w : bi.w;     // std::min(i, j)
  const float dw = xx2 - xx1, dh = yy2 - yy1;
  const float w = 0.f < dw ? dw : 0.f, h = 0.f < dh ? dh : 0.f;                     // std::max(0, d)
  const float inter = w * h;
  const float ovr = inter / (iarea + jarea - inter);
  return ovr > thr;
}

// (2) one wave per 64 x 64 tile (row block rb <= column block cb) of a group's M x M suppression matrix: lane t owns
// row rb * 64 + t and writes the word of column block cb, bit jj set iff column cb * 64 + jj comes after the row and the
// row would suppress it
__global__ __launch_bounds__(kWave) void box_nms_mask_kernel(const int32_t* __restrict__ selcount,
                                                             const float4* __restrict__ sbox, int cap, int w64, int nb,
                                                             float thr, u64* __restrict__ mask) {
  __shared__ float4 cbox[kWave];
  const int64_t id = blockIdx.x;
  const int cb = (int)(id % nb), rb = (int)((id / nb) % nb);
  const int64_t g = id / ((int64_t)nb * nb);
  const int M = selcount[g];
  if (cb < rb || cb * kWave >= M) return;       // block-uniform
  const int t = threadIdx.x;
  const int jc = cb * kWave + t;
  cbox[t] = jc < M ? sbox[g * cap + jc] : make_float4(0.f, 0.f, 0.f, 0.f);
  __syncthreads();
  const int i = rb * kWave + t;
  if (i >= M) return;
  const float4 bi = sbox[g * cap + i];
  const float iarea = (bi.z - bi.x) * (bi.w - bi.y);
  u64 bits = 0;
  for (int jj = 0; jj < kWave; ++jj) {
    const int j = cb * kWave + jj;
    if (j > i && j < M && suppresses(bi, iarea, cbox[jj], thr)) bits |= 1ull << jj;
  }
  mask[(g * cap + i) * w64 + cb] = bits;
}

// (3) one wave per group: the greedy scan.  Lane l keeps the removed bits of column blocks l and l + 64.
__global__ __launch_bounds__(kWave) void box_nms_scan_kernel(const int32_t* __restrict__ selcount,
                                                             const int32_t* __restrict__ sidx,
                                                             const u64* __restrict__ mask, int cap, int w64,
                                                             int post_topk, int64_t* __restrict__ out_index,
                                                             int64_t* __restrict__ out_count,
                                                             uint8_t* __restrict__ out_keep) {
  const int64_t g = blockIdx.x;
  const int lane = threadIdx.x;
  const int M = selcount[g];
  const int nblk = (M + kWave - 1) / kWave;
  const int32_t* si = sidx + g * cap;
  u64 rem0 = 0, rem1 = 0;
  for (int blk = 0; blk < nblk; ++blk) {       // dropped rows and the rows past M start out removed
    const int i = blk * kWave + lane;
    const u64 dead = __ballot(i < M ? si[i] < 0 : true);
    if ((blk & 63) == lane) {
      if (blk < kWave)
        rem0 = dead;
      else
        rem1 = dead;
    }
  }
  int cnt = 0;
  for (int blk = 0; blk < nblk && cnt < post_topk; ++blk) {
    u64 cur = __shfl(blk < kWave ? rem0 : rem1, blk & 63);
    const int i = blk * kWave + lane;
    const u64 diag = i < M ? mask[(g * cap + i) * w64 + blk] : 0ull;
    for (int t = 0; t < kWave; ++t) {
      const u64 dt = __shfl(diag, t);
      if (!((cur >> t) & 1ull)) cur |= dt;       // t is kept: it removes what it suppresses (bits above t only)
    }
    const u64 kept = ~cur;
    const int rank = cnt + __popcll(kept & ((1ull << lane) - 1ull));
    if (((kept >> lane) & 1ull) && rank < post_topk) {
      const int64_t flat = si[i];
      out_index[g * post_topk + rank] = flat;
      if (out_keep != nullptr) out_keep[flat] = 1;
    }
    cnt += __popcll(kept);
    if (cnt >= post_topk) break;
    for (u64 k = kept; k != 0; k &= k - 1) {
      const int row = blk * kWave + (__ffsll((long long)k) - 1);
      const u64* mr = mask + (g * cap + row) * w64;
      if (lane > blk && lane < nblk) rem0 |= mr[lane];
      if (lane + kWave > blk && lane + kWave < nblk) rem1 |= mr[lane + kWave];
    }
  }
  const int kept_n = cnt < post_topk ? cnt : post_topk;
  for (int r = kept_n + lane; r < post_topk; r += kWave) out_index[g * post_topk + r] = -1;
  if (lane == 0) out_count[g] = kept_n;
}

// ---- tspn_detections_topk_f32: one workgroup per image; candidate i = r * K + c, so that ties go to the lower r * K + c
__global__ __launch_bounds__(tspn::kSelectThreads) void detections_topk_kernel(
    const float* __restrict__ scores, const float4* __restrict__ boxes, const uint8_t* __restrict__ keep, int K, int R,
    int D, float4* __restrict__ out_boxes, float* __restrict__ out_scores, int64_t* __restrict__ out_classes,
    int64_t* __restrict__ out_count) {
  __shared__ tspn::SelectLds L;
  __shared__ int total;
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int Q = K * R;
  const float* sc = scores + b * Q;
  const uint8_t* kp = keep + b * Q;
  if (tid == 0) total = 0;
  __syncthreads();
  int mine = 0;
  for (int q = tid; q < Q; q += tspn::kSelectThreads) mine += kp[q] != 0;
  if (mine) atomicAdd(&total, mine);
  __syncthreads();
  const int M = total < D ? total : D;
  if (M > 0)
    tspn::select_topk_sorted(L, [sc, kp, K, R](int i) {
      const int q = (i % K) * R + i / K;
      return kp[q] ? order_key(sc[q]) : tspn::kPadKey;
    }, Q, M);
  for (int d = tid; d < D; d += tspn::kSelectThreads) {
    float4 bx = make_float4(0.f, 0.f, 0.f, 0.f);
    float s = 0.f;
    int64_t c = 0;
    if (d < M) {
      const int i = L.ki[d];
      c = i % K;
      const int q = (int)c * R + i / K;
      bx = boxes[b * Q + q];
      s = sc[q];
    }
    out_boxes[b * D + d] = bx;
    out_scores[b * D + d] = s;
    out_classes[b * D + d] = c;
  }
  if (tid == 0) out_count[b] = M;
}

// The layout of the NMS scratch: offsets int64 [G+1] | selected counts int32 [G] | sorted flat indices int32 [G][cap] |
// sorted boxes float4 [G][cap] | suppression words u64 [G][cap][w64]; every piece 256-byte aligned.  The selection alone
// takes the offsets only.
struct NmsLayout {
  int64_t cap, w64;
  size_t off, selcount, sidx, sbox, mask, total;
};

// 0: fine.  Fills `lay` from the host-side group offsets.
int nms_layout(const char* who, const int64_t* group_off, int64_t G, int64_t n, int64_t pre_topk, int64_t post_topk,
               bool select_only, bool check_n, NmsLayout* lay) {
  TSPN_REQUIRE(n >= 0 && G >= 0 && pre_topk >= 1 && post_topk >= 1, TSPN_EINVAL,
               "%s: bad sizes n=%lld G=%lld pre_topk=%lld post_topk=%lld", who, (long long)n, (long long)G,
               (long long)pre_topk, (long long)post_topk);
  TSPN_REQUIRE(pre_topk <= kMaxPre, TSPN_EUNSUPPORTED, "%s: pre_topk=%lld > %d", who, (long long)pre_topk, kMaxPre);
  TSPN_REQUIRE(post_topk <= pre_topk, TSPN_EUNSUPPORTED, "%s: post_topk=%lld > pre_topk=%lld", who, (long long)post_topk,
               (long long)pre_topk);
  TSPN_REQUIRE(n < ((int64_t)1 << 31) && G < ((int64_t)1 << 24), TSPN_EUNSUPPORTED,
               "%s: n=%lld G=%lld (needs n < 2^31, G < 2^24)", who, (long long)n, (long long)G);
  TSPN_REQUIRE(group_off != nullptr, TSPN_EINVAL, "%s: null pointer", who);
  int64_t largest = 0;
  bool sorted = group_off[0] == 0;
  for (int64_t g = 0; g < G && sorted; ++g) {
    const int64_t len = group_off[g + 1] - group_off[g];
    sorted = len >= 0 && group_off[g + 1] < ((int64_t)1 << 31);
    largest = len > largest ? len : largest;
  }
  TSPN_REQUIRE(sorted && (!check_n || group_off[G] == n), TSPN_EINVAL,
               "%s: group_off must ascend from 0 to n=%lld", who, (long long)n);
  lay->cap = largest < pre_topk ? largest : pre_topk;
  lay->w64 = (lay->cap + kWave - 1) / kWave;
  size_t at = 0;
  auto piece = [&at](size_t bytes) {
    const size_t here = at;
    at += tspn::align_up(bytes, 256);
    return here;
  };
  lay->off = piece((size_t)(G + 1) * sizeof(int64_t));
  lay->selcount = lay->sidx = lay->sbox = lay->mask = at;
  if (!select_only) {
    lay->selcount = piece((size_t)G * sizeof(int32_t));
    lay->sidx = piece((size_t)G * lay->cap * sizeof(int32_t));
    lay->sbox = piece((size_t)G * lay->cap * sizeof(float4));
    lay->mask = piece((size_t)G * lay->cap * lay->w64 * sizeof(u64));
  }
  lay->total = at;
  return TSPN_OK;
}

}  // namespace

extern "C" int tspn_rpn_decode_f32(const int64_t* cand, const float* logits, const float* deltas, const float* cell_anchors,
                                   const float* image_sizes, int64_t B, int64_t H, int64_t W, int64_t A, int64_t M,
                                   float stride, float* out_boxes, float* out_logits, uint8_t* out_valid, void* stream) {
  const char* who = "tspn_rpn_decode_f32";
  TSPN_REQUIRE(B >= 0 && H > 0 && W > 0 && A > 0 && M >= 0, TSPN_EINVAL, "%s: bad sizes B=%lld H=%lld W=%lld A=%lld M=%lld",
               who, (long long)B, (long long)H, (long long)W, (long long)A, (long long)M);
  TSPN_REQUIRE(H < (1 << 20) && W < (1 << 20) && A < (1 << 10) && H * W * A < ((int64_t)1 << 31) &&
                   B < ((int64_t)1 << 31) && M < ((int64_t)1 << 31) && B * M < ((int64_t)1 << 31) * 256,
               TSPN_EUNSUPPORTED, "%s: dimension too large", who);
  TSPN_REQUIRE(cand != nullptr || M == H * W * A, TSPN_EINVAL, "%s: without candidates M must be H*W*A=%lld (got %lld)",
               who, (long long)(H * W * A), (long long)M);
  TSPN_REQUIRE(stride > 0.f, TSPN_EINVAL, "%s: stride must be positive", who);
  if (B == 0 || M == 0) return TSPN_OK;
  TSPN_REQUIRE(logits && deltas && cell_anchors && image_sizes && out_boxes && out_logits && out_valid, TSPN_EINVAL,
               "%s: null pointer", who);
  TSPN_REQUIRE(tspn::aligned16(out_boxes), TSPN_EUNSUPPORTED, "%s: out_boxes must be 16-byte aligned", who);
  hipLaunchKernelGGL(rpn_decode_f32_kernel, dim3((unsigned)tspn::ceil_div(B * M, 256)), dim3(256), 0, TSPN_STREAM(stream),
                     cand, logits, deltas, cell_anchors, image_sizes, B, (int)W, (int)A, H * W * A, M, stride,
                     reinterpret_cast<float4*>(out_boxes), out_logits, out_valid);
  return tspn::check_launch(who);
}

extern "C" int tspn_box_head_decode_f32(const float* cls_logits, const float* deltas, const float* proposals,
                                        const int64_t* proposal_count, const float* image_sizes, int64_t B, int64_t R,
                                        int64_t K, float wx, float wy, float ww, float wh, float score_thresh,
                                        float* out_scores, float* out_boxes, uint8_t* out_valid, void* stream) {
  const char* who = "tspn_box_head_decode_f32";
  TSPN_REQUIRE(B >= 0 && R >= 0 && K > 0, TSPN_EINVAL, "%s: bad sizes B=%lld R=%lld K=%lld", who, (long long)B,
               (long long)R, (long long)K);
  TSPN_REQUIRE(K < (1 << 16) && B < ((int64_t)1 << 31) && R < ((int64_t)1 << 31) && B * R * K < ((int64_t)1 << 31),
               TSPN_EUNSUPPORTED, "%s: dimension too large", who);
  TSPN_REQUIRE(wx > 0.f && wy > 0.f && ww > 0.f && wh > 0.f && score_thresh == score_thresh, TSPN_EINVAL,
               "%s: weights must be positive and score_thresh a number", who);
  if (B == 0 || R == 0) return TSPN_OK;
  TSPN_REQUIRE(cls_logits && deltas && proposals && proposal_count && image_sizes && out_scores && out_boxes && out_valid,
               TSPN_EINVAL, "%s: null pointer", who);
  TSPN_REQUIRE(tspn::all_aligned16(proposals, out_boxes), TSPN_EUNSUPPORTED,
               "%s: proposals and out_boxes must be 16-byte aligned", who);
  hipLaunchKernelGGL(box_head_decode_f32_kernel, dim3((unsigned)tspn::ceil_div(B * R, 256)), dim3(256), 0,
                     TSPN_STREAM(stream), cls_logits, deltas, reinterpret_cast<const float4*>(proposals), proposal_count,
                     image_sizes, B, R, (int)K, wx, wy, ww, wh, score_thresh, out_scores,
                     reinterpret_cast<float4*>(out_boxes), out_valid);
  return tspn::check_launch(who);
}

extern "C" size_t tspn_box_nms_scratch_bytes(const int64_t* group_off, int64_t G, int64_t pre_topk, int select_only) {
  NmsLayout lay;
  if (G < 0 || group_off == nullptr) return 0;
  if (nms_layout("tspn_box_nms_scratch_bytes", group_off, G, 0, pre_topk, 1, select_only != 0, false, &lay)) return 0;
  return G == 0 ? 0 : lay.total;
}

extern "C" int tspn_box_nms_f32(const float* boxes, const float* scores, const uint8_t* valid, int64_t n,
                                const int64_t* group_off, int64_t G, int64_t pre_topk, float iou_threshold,
                                int64_t post_topk, float min_size, int64_t* out_index, int64_t* out_count,
                                uint8_t* out_keep, void* scratch, size_t scratch_bytes, void* stream) {
  const char* who = "tspn_box_nms_f32";
  NmsLayout lay;
  if (int rc = nms_layout(who, group_off, G, n, pre_topk, post_topk, boxes == nullptr, true, &lay)) return rc;
  if (G == 0) return TSPN_OK;
  const bool select_only = boxes == nullptr;
  TSPN_REQUIRE((n == 0 || scores) && out_index && out_count, TSPN_EINVAL, "%s: null pointer", who);
  TSPN_REQUIRE(!select_only || (valid == nullptr && out_keep == nullptr), TSPN_EINVAL,
               "%s: the selection alone (boxes == null) takes no validity array and writes no keep bytes", who);
  TSPN_REQUIRE(select_only || (iou_threshold == iou_threshold && min_size == min_size), TSPN_EINVAL,
               "%s: iou_threshold and min_size must be numbers", who);
  TSPN_REQUIRE(tspn::all_aligned16(boxes, scratch) && (reinterpret_cast<uintptr_t>(out_index) & 7) == 0 &&
                   (reinterpret_cast<uintptr_t>(out_count) & 7) == 0 && (reinterpret_cast<uintptr_t>(scores) & 3) == 0,
               TSPN_EUNSUPPORTED, "%s: boxes and scratch must be 16-byte aligned, the outputs 8-byte aligned", who);
  const int64_t nb = lay.w64;
  TSPN_REQUIRE(G * nb * nb < ((int64_t)1 << 31), TSPN_EUNSUPPORTED, "%s: too many groups for pre_topk (G=%lld)", who,
               (long long)G);
  TSPN_REQUIRE(scratch != nullptr && scratch_bytes >= lay.total, TSPN_EWORKSPACE, "%s: scratch %zu < %zu bytes", who,
               scratch != nullptr ? scratch_bytes : (size_t)0, lay.total);
  char* base = static_cast<char*>(scratch);
  int64_t* d_off = reinterpret_cast<int64_t*>(base + lay.off);
  hipStream_t st = TSPN_STREAM(stream);
  for (int64_t at = 0; at <= G; at += kOffChunk) {
    OffChunk c;
    const int count = (int)(G + 1 - at < kOffChunk ? G + 1 - at : kOffChunk);
    for (int k = 0; k < kOffChunk; ++k) c.v[k] = k < count ? group_off[at + k] : 0;
    hipLaunchKernelGGL(box_nms_offsets_kernel, dim3(1), dim3(kOffChunk), 0, st, c, count, d_off + at);
  }
  int32_t* selcount = reinterpret_cast<int32_t*>(base + lay.selcount);
  int32_t* sidx = reinterpret_cast<int32_t*>(base + lay.sidx);
  float4* sbox = reinterpret_cast<float4*>(base + lay.sbox);
  u64* mask = reinterpret_cast<u64*>(base + lay.mask);
  if (select_only) {
    hipLaunchKernelGGL(box_nms_select_kernel<true>, dim3((unsigned)G), dim3(tspn::kSelectThreads), 0, st, scores, valid,
                       reinterpret_cast<const float4*>(boxes), d_off, (int)pre_topk, (int)lay.cap, min_size, (int)post_topk,
                       selcount, sidx, sbox, out_keep, out_index, out_count);
    return tspn::check_launch(who);
  }
  hipLaunchKernelGGL(box_nms_select_kernel<false>, dim3((unsigned)G), dim3(tspn::kSelectThreads), 0, st, scores, valid,
                     reinterpret_cast<const float4*>(boxes), d_off, (int)pre_topk, (int)lay.cap, min_size, (int)post_topk,
                     selcount, sidx, sbox, out_keep, out_index, out_count);
  if (nb > 0)
    hipLaunchKernelGGL(box_nms_mask_kernel, dim3((unsigned)(G * nb * nb)), dim3(kWave), 0, st, selcount, sbox, (int)lay.cap,
                       (int)lay.w64, (int)nb, iou_threshold, mask);
  hipLaunchKernelGGL(box_nms_scan_kernel, dim3((unsigned)G), dim3(kWave), 0, st, selcount, sidx, mask, (int)lay.cap,
                     (int)lay.w64, (int)post_topk, out_index, out_count, out_keep);
  return tspn::check_launch(who);
}

extern "C" int tspn_detections_topk_f32(const float* scores, const float* boxes, const uint8_t* keep, int64_t B, int64_t K,
                                        int64_t R, int64_t D, float* out_boxes, float* out_scores, int64_t* out_classes,
                                        int64_t* out_count, void* stream) {
  const char* who = "tspn_detections_topk_f32";
  TSPN_REQUIRE(B >= 0 && K > 0 && R >= 0 && D >= 1, TSPN_EINVAL, "%s: bad sizes B=%lld K=%lld R=%lld D=%lld", who,
               (long long)B, (long long)K, (long long)R, (long long)D);
  TSPN_REQUIRE(D <= tspn::kSelectMaxM, TSPN_EUNSUPPORTED, "%s: D=%lld > %d", who, (long long)D, tspn::kSelectMaxM);
  TSPN_REQUIRE(K < ((int64_t)1 << 31) && R < ((int64_t)1 << 31) && K * R < ((int64_t)1 << 31) && B < ((int64_t)1 << 31),
               TSPN_EUNSUPPORTED, "%s: dimension too large", who);
  if (B == 0) return TSPN_OK;
  TSPN_REQUIRE((R == 0 || (scores && boxes && keep)) && out_boxes && out_scores && out_classes && out_count, TSPN_EINVAL,
               "%s: null pointer", who);
  TSPN_REQUIRE(tspn::all_aligned16(boxes, out_boxes), TSPN_EUNSUPPORTED, "%s: operands must be 16-byte aligned", who);
  hipLaunchKernelGGL(detections_topk_kernel, dim3((unsigned)B), dim3(tspn::kSelectThreads), 0, TSPN_STREAM(stream), scores,
                     reinterpret_cast<const float4*>(boxes), keep, (int)K, (int)R, (int)D,
                     reinterpret_cast<float4*>(out_boxes), out_scores, out_classes, out_count);
  return tspn::check_launch(who);
}
