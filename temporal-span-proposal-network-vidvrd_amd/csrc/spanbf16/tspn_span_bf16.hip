// Span-restricted RelOIPool + predicate head, and the relations decoded with their spans, on bf16 segments (gfx950).
//
// Semantics (DESIGN.md 2 "bf16 semantics", 4c).  For a row (subject s, object o, span (start, end)) on features
// f [NT, T, D] bf16, classifier W [K, 2D], b [K]:
//   frames [a, e) = tspn::span_frames(start, end, T)                                  (tspn_span_pool.h, oracle.span_frames)
//   pooled_h[c]   = bf16_rne((float)(sum_{t in [a, e)} (double) f[h, t, c] / (double)(e - a)))       h in {s, o}
//   out[k]        = sigmoid(sum_c pooled_s[c] W16[k, c] + sum_c pooled_o[c] W16[k, D + c] + b16[k])
// W16, b16 = the bf16-rounded parameters; products exact, accumulation fp32.  A float64 sum of a few thousand bf16
// values of ordinary range is exact, so the pooled operand does not depend on how the sum is organised.
//
//   span_prefix_bf16_kernel    PS [NT, T+1, D] float64: prefix sums of f over time, one thread per (tracklet, channel);
//   span_pool_bf16_kernel      A [rows, 2D] bf16: per (row, half) the difference PS[e] - PS[a], divided, rounded.  A NaN /
//                              Inf frame makes every later prefix value non-finite; where PS[e] is, the span's own frames
//                              are summed in frame order instead, so such a frame reaches the spans that hold it only.
//                              A tracklet id outside [0, NT) is CLAMPED into it, not refused: nothing outside f is read,
//                              and the row's values are those of the clamped tracklet (ops.py checks the table first);
//   span_gemm_bf16_kernel      out [rows, K] = sigmoid(A W16^T + b16) on v_mfma_f32_16x16x32_bf16.  A wave owns 16 rows x up to
//                              SG_CT 16-column tiles and walks the 2D / 32 k-steps in order, the fragment loads of
//                              SG_KU = 4 k-steps issued together (the last group clamped); both operand fragments come
//                              straight from memory (A: 16 bytes of the lane's own row; W16: the fragment-major image of
//                              pack_span_cls_bf16_kernel, 1 KiB per wave and k-step).  An output depends on its own A row
//                              only, and its k-steps run in the same order wherever the row sits in the launch;
//   span_row_topk_q_kernel     relations: the R best predicates of a (pair, span) row of q, tspn::wave_row_topk on values
//                              read from memory.
// The segment stage of the relations entry is tspn::segment_span_topk (relations/tspn_span_relations.hip).
#include <algorithm>

#include "tspn_common.h"
#include "tspn_device.h"
#include "tspn_span_pool.h"
#include "tspn_topk_select.h"

namespace {

using namespace tspn_dev;

constexpr int SG_WAVES = 4;
constexpr int SG_ROWS = 16 * SG_WAVES;   // rows of a workgroup
constexpr int SG_CT = 4;                 // 16-column tiles of a workgroup
constexpr int SG_KC = 32;                // channels of a k-step
constexpr int SG_KU = 4;                 // k-steps whose fragments are loaded together
constexpr int MAX_J = 16;

// cls_w [K, F = 2D] fp32 -> [ceil(K / 16)][F / 32][64 lanes][8] bf16: lane l of column tile kt and k-step ks holds
// W16[16 kt + (l & 15)][32 ks + 8 (l >> 4) + j], j = 0..7 (the B operand of v_mfma_f32_16x16x32_bf16); rows >= K are 0
__global__ void pack_span_cls_bf16_kernel(const float* __restrict__ W, int64_t K, int64_t F, __bf16* __restrict__ packed) {
  const int64_t KS = F / SG_KC;
  const int64_t total = (K + 15) / 16 * 16 * F;
  const int64_t o = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (o >= total) return;
  const int64_t j = o & 7, l = (o >> 3) & 63, ks = (o >> 9) % KS, kt = (o >> 9) / KS;
  const int64_t k = kt * 16 + (l & 15), c = ks * SG_KC + 8 * (l >> 4) + j;
  packed[o] = k < K ? (__bf16)W[k * F + c] : (__bf16)0.f;
}

__global__ __launch_bounds__(256) void span_prefix_bf16_kernel(const __bf16* __restrict__ f, int64_t NT, int T, int D,
                                                               double* __restrict__ PS) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= NT * D) return;
  const int64_t trk = i / D, c = i - trk * D;
  const __bf16* x = f + (trk * T) * (int64_t)D + c;
  double* ps = PS + (trk * (T + 1)) * (int64_t)D + c;
  double acc = 0.0;
  ps[0] = 0.0;
#pragma unroll 8
  for (int t = 0; t < T; ++t) {
    acc += (double)(float)x[(int64_t)t * D];
    ps[(int64_t)(t + 1) * D] = acc;
  }
}

// One thread per (row, half, 8 channels).  Row `row` is span `row % J` of pair `row / J`; the pair's tracklets are
// seg * N + pairs[pair] with seg = pair / Pseg (the predicate entry passes J = 1, Pseg = P and global ids: seg = 0).
__global__ __launch_bounds__(256) void span_pool_bf16_kernel(const double* __restrict__ PS, const __bf16* __restrict__ f,
                                                             const int64_t* __restrict__ pairs,
                                                             const int64_t* __restrict__ spans, int64_t rows, int64_t NT,
                                                             int T, int D, int J, int64_t Pseg, int64_t N,
                                                             __bf16* __restrict__ A) {
  const int G = D >> 3;
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= rows * 2 * G) return;
  const int64_t row = i / (2 * G);
  const int r = (int)(i - row * 2 * G);
  const int h = r / G, g = r - h * G;
  const int64_t pr = row / J;
  int64_t trk = (pr / Pseg) * N + pairs[2 * pr + h];
  trk = trk < 0 ? 0 : (trk > NT - 1 ? NT - 1 : trk);      // the callers check the table; no read outside f either way
  int64_t a, e;
  tspn::span_frames(spans[2 * row], spans[2 * row + 1], T, a, e);
  const double* pa = PS + ((trk * (T + 1) + a) * (int64_t)D + g * 8);
  const double* pe = PS + ((trk * (T + 1) + e) * (int64_t)D + g * 8);
  const double len = (double)(e - a);
  bf16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    double d = pe[j] - pa[j];
    if (!isfinite(pe[j])) {                                // a NaN / Inf frame before e: the span's own frames, in order
      const __bf16* x = f + (trk * T) * (int64_t)D + g * 8 + j;
      d = 0.0;
      for (int64_t t = a; t < e; ++t) d += (double)(float)x[t * D];
    }
    o[j] = (__bf16)(float)(d / len);
  }
  *reinterpret_cast<bf16x8*>(A + row * 2 * (int64_t)D + (int64_t)h * D + g * 8) = o;
}

// the k-steps of a wave's 16 rows x NCT column tiles, in order; ap / wp: the lane's pieces of k-step 0.  SG_KU k-steps
// at a time: their 1 + NCT fragment loads each are issued together (a step past the end loads the last step's again and
// is not used), then the MFMAs follow in k order, so a wave has up to SG_KU (1 + NCT) loads in flight.
template <int NCT>
__device__ __forceinline__ void span_gemm_ksteps(const bf16x8* __restrict__ ap, const bf16x8* __restrict__ wp, int KS,
                                                 f32x4 (&acc)[SG_CT]) {
  for (int ks = 0; ks < KS; ks += SG_KU) {
    bf16x8 a[SG_KU], w[SG_KU][NCT];
#pragma unroll
    for (int u = 0; u < SG_KU; ++u) {
      const int kk = min(ks + u, KS - 1);
      a[u] = ap[kk * (SG_KC / 8)];
#pragma unroll
      for (int c = 0; c < NCT; ++c) w[u][c] = wp[((int64_t)c * KS + kk) * 64];
    }
#pragma unroll
    for (int u = 0; u < SG_KU; ++u) {
      if (ks + u < KS) {                                    // wave-uniform
#pragma unroll
        for (int c = 0; c < NCT; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[u], w[u][c], acc[c], 0, 0, 0);
      }
    }
  }
}

// grid (ceil(rows / SG_ROWS), ceil(ceil(K / 16) / SG_CT)); F = 2D, a multiple of SG_KC
__global__ __launch_bounds__(64 * SG_WAVES) void span_gemm_bf16_kernel(const __bf16* __restrict__ A, int64_t rows, int F,
                                                                       const __bf16* __restrict__ Wp,
                                                                       const float* __restrict__ b, int K,
                                                                       float* __restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row0 = (int64_t)blockIdx.x * SG_ROWS + wave * 16;
  if (row0 >= rows) return;                                 // the whole wave; there is no barrier below
  const int KS = F / SG_KC, KT = (K + 15) >> 4;
  const int kt0 = blockIdx.y * SG_CT;
  const int nct = min(SG_CT, KT - kt0);                     // wave-uniform
  // rows past the end load the last row again; their accumulators are not stored
  const int64_t arow = min(row0 + (lane & 15), rows - 1);
  const bf16x8* ap = reinterpret_cast<const bf16x8*>(A + arow * F + 8 * (lane >> 4));
  const bf16x8* wp = reinterpret_cast<const bf16x8*>(Wp) + (int64_t)kt0 * KS * 64 + lane;
  f32x4 acc[SG_CT];
#pragma unroll
  for (int c = 0; c < SG_CT; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
  switch (nct) {
    case 1: span_gemm_ksteps<1>(ap, wp, KS, acc); break;
    case 2: span_gemm_ksteps<2>(ap, wp, KS, acc); break;
    case 3: span_gemm_ksteps<3>(ap, wp, KS, acc); break;
    default: span_gemm_ksteps<4>(ap, wp, KS, acc); break;
  }
  // lane = (column lane & 15, rows 4 (lane >> 4) .. + 3) of each tile
#pragma unroll
  for (int c = 0; c < SG_CT; ++c) {
    const int k = (kt0 + c) * 16 + (lane & 15);
    if (c < nct && k < K) {
      const float bias = b != nullptr ? (float)(__bf16)b[k] : 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t row = row0 + 4 * (lane >> 4) + r;
        if (row < rows) {
          const float v = acc[c][r] + bias;
          out[row * K + k] = 1.f / (1.f + expf(-v));
        }
      }
    }
  }
}

// span_row_topk_kernel of relations/tspn_span_relations.hip with the K values of the row read from q [rows, K]
__global__ __launch_bounds__(256) void span_row_topk_q_kernel(const float* __restrict__ q,
                                                              const float* __restrict__ span_scores,
                                                              const int64_t* __restrict__ span_counts, int64_t rows, int J,
                                                              int K, int R, unsigned* __restrict__ key,
                                                              float* __restrict__ sc, int* __restrict__ ix) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int64_t pr = row / J;
  const int j = (int)(row - pr * J);
  if ((int64_t)j >= span_counts[pr]) {           // not a proposal: nothing the segment stage can select
    for (int r = lane; r < R; r += 64) {
      key[row * R + r] = tspn::kPadKey;
      sc[row * R + r] = 0.f;
      ix[row * R + r] = -1;
    }
    return;
  }
  const float w = span_scores[row];
  float v[tspn::kRowTopkVPT];
#pragma unroll
  for (int i = 0; i < tspn::kRowTopkVPT; ++i) {
    const int k = lane + 64 * i;
    v[i] = k < K ? q[row * K + k] : 0.f;
  }
  tspn::wave_row_topk(v, K, R, lane, [=](int r, float value, int k) {
    const float prod = value * w;                // one rounding (-ffp-contract=off)
    key[row * R + r] = tspn::order_key(prod);
    sc[row * R + r] = prod;
    ix[row * R + r] = k;
  });
}

struct SpanBf16Layout {
  size_t ps, a, total;
};
// PS [NT, T+1, D] float64, then A [rows, 2D] bf16
SpanBf16Layout span_layout(int64_t NT, int64_t T, int64_t D, int64_t rows) {
  SpanBf16Layout L{};
  L.ps = 0;
  L.a = tspn::align_up((size_t)NT * (size_t)(T + 1) * (size_t)D * sizeof(double), 256);
  L.total = L.a + tspn::align_up((size_t)rows * 2 * (size_t)D * sizeof(uint16_t), 256);
  return L;
}

// Every product the layout and the grids form stays far inside int64 / size_t: each factor is bounded first, then the
// products themselves (the prefix table below 2^46 bytes, the pooled rows and q below 2^43 / 2^51).
bool sizes_fit(int64_t NT, int64_t T, int64_t D, int64_t K, int64_t rows) {
  return T < (1 << 30) && D < (1 << 24) && K < (1 << 20) && NT >= 0 && NT < (1LL << 31) && rows >= 0 &&
         rows < (1LL << 31) && NT * (T + 1) < (1LL << 40) && NT * (T + 1) * D < (1LL << 43) &&
         tspn::ceil_div(NT * D, 256) < (1LL << 31) && rows * D < (1LL << 41) &&
         tspn::ceil_div(rows * 2 * (D / 8), 256) < (1LL << 31);
}
// S * P * J of the relations entries, or -1 where the product does not stay below 2^31 (S, P < 2^31 and J <= MAX_J are
// the callers' checks, so S * P cannot overflow int64)
int64_t relation_rows(int64_t S, int64_t P, int64_t J) {
  if (S <= 0 || P <= 0) return 0;
  if (S * P >= (1LL << 31)) return -1;
  const int64_t rows = S * P * J;
  return rows < (1LL << 31) ? rows : -1;
}

// prefix sums, pooled rows and the predicate GEMM: q [rows, K].  `ws` holds span_layout(NT, T, D, rows).total bytes.
int span_q_stage(const uint16_t* feats, int64_t NT, int64_t T, int64_t D, const int64_t* pairs, const int64_t* spans,
                 int64_t rows, int64_t J, int64_t Pseg, int64_t N, const uint16_t* cls_packed, const float* cls_b, int64_t K,
                 float* q, void* ws, void* stream, const char* who) {
  const SpanBf16Layout L = span_layout(NT, T, D, rows);
  const __bf16* f = reinterpret_cast<const __bf16*>(feats);
  double* PS = reinterpret_cast<double*>(static_cast<char*>(ws) + L.ps);
  __bf16* A = reinterpret_cast<__bf16*>(static_cast<char*>(ws) + L.a);
  hipStream_t s = TSPN_STREAM(stream);
  hipLaunchKernelGGL(span_prefix_bf16_kernel, dim3((unsigned)tspn::ceil_div(NT * D, 256)), dim3(256), 0, s, f, NT, (int)T,
                     (int)D, PS);
  hipLaunchKernelGGL(span_pool_bf16_kernel, dim3((unsigned)tspn::ceil_div(rows * 2 * (D / 8), 256)), dim3(256), 0, s, PS, f,
                     pairs, spans, rows, NT, (int)T, (int)D, (int)J, Pseg, N, A);
  const dim3 grid((unsigned)tspn::ceil_div(rows, SG_ROWS), (unsigned)tspn::ceil_div(tspn::ceil_div(K, 16), SG_CT));
  hipLaunchKernelGGL(span_gemm_bf16_kernel, grid, dim3(64 * SG_WAVES), 0, s, A, rows, (int)(2 * D),
                     reinterpret_cast<const __bf16*>(cls_packed), cls_b, (int)K, q);
  return tspn::check_launch(who);
}

}  // namespace

extern "C" int tspn_pack_span_cls_bf16(const float* cls_w, int64_t K, int64_t D, uint16_t* packed, void* stream) {
  TSPN_REQUIRE(K > 0 && D > 0 && K < (1 << 20) && D < (1 << 24), TSPN_EINVAL, "tspn_pack_span_cls_bf16: bad sizes K=%lld D=%lld",
               (long long)K, (long long)D);
  TSPN_REQUIRE(D % 16 == 0, TSPN_EUNSUPPORTED, "tspn_pack_span_cls_bf16: needs D %% 16 == 0 (D=%lld)", (long long)D);
  TSPN_REQUIRE(cls_w && packed, TSPN_EINVAL, "tspn_pack_span_cls_bf16: null pointer");
  TSPN_REQUIRE(tspn::aligned16(packed), TSPN_EUNSUPPORTED, "tspn_pack_span_cls_bf16: packed must be 16-byte aligned");
  const int64_t total = tspn::ceil_div(K, 16) * 16 * 2 * D;
  hipLaunchKernelGGL(pack_span_cls_bf16_kernel, dim3((unsigned)tspn::ceil_div(total, 256)), dim3(256), 0, TSPN_STREAM(stream),
                     cls_w, K, 2 * D, reinterpret_cast<__bf16*>(packed));
  return tspn::check_launch("tspn_pack_span_cls_bf16");
}

extern "C" size_t tspn_span_predicate_bf16_workspace_bytes(int64_t NT, int64_t T, int64_t D, int64_t K, int64_t P) {
  if (NT <= 0 || T <= 0 || D <= 0 || K <= 0 || P <= 0 || D % 16 || !sizes_fit(NT, T, D, K, P)) return 0;
  return span_layout(NT, T, D, P).total;
}

extern "C" int tspn_span_predicate_bf16(const uint16_t* feats, int64_t NT, int64_t T, int64_t D, const int64_t* pairs,
                                        const int64_t* spans, int64_t P, const uint16_t* cls_packed, const float* cls_b,
                                        int64_t K, float* out, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "tspn_span_predicate_bf16";
  TSPN_REQUIRE(NT >= 0 && T > 0 && D > 0 && K > 0 && P >= 0, TSPN_EINVAL, "%s: bad sizes NT=%lld T=%lld D=%lld K=%lld P=%lld",
               who, (long long)NT, (long long)T, (long long)D, (long long)K, (long long)P);
  TSPN_REQUIRE(D % 16 == 0, TSPN_EUNSUPPORTED, "%s: needs D %% 16 == 0 (D=%lld)", who, (long long)D);
  TSPN_REQUIRE(sizes_fit(NT, T, D, K, P), TSPN_EUNSUPPORTED, "%s: problem too large", who);
  if (P == 0 || NT == 0) return TSPN_OK;
  TSPN_REQUIRE(feats && pairs && spans && cls_packed && out, TSPN_EINVAL, "%s: null pointer", who);
  TSPN_REQUIRE(tspn::all_aligned16(feats, cls_packed) && (reinterpret_cast<uintptr_t>(out) & 3) == 0 &&
                   (reinterpret_cast<uintptr_t>(pairs) & 7) == 0 && (reinterpret_cast<uintptr_t>(spans) & 7) == 0,
               TSPN_EUNSUPPORTED, "%s: unaligned pointer (feats and cls_packed need 16 bytes)", who);
  const size_t need = span_layout(NT, T, D, P).total;
  TSPN_REQUIRE(workspace && workspace_bytes >= need, TSPN_EWORKSPACE, "%s: workspace %zu < %zu bytes", who, workspace_bytes,
               need);
  TSPN_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, TSPN_EUNSUPPORTED,
               "%s: unaligned pointer (the workspace needs 256 bytes)", who);
  return span_q_stage(feats, NT, T, D, pairs, spans, P, 1, P, 0, cls_packed, cls_b, K, out, workspace, stream, who);
}

extern "C" size_t tspn_decode_span_relations_bf16_workspace_bytes(int64_t S, int64_t N, int64_t T, int64_t D, int64_t P,
                                                                  int64_t J, int64_t K, int64_t topk_per_span) {
  if (S <= 0 || N <= 0 || T <= 0 || D <= 0 || P <= 0 || J <= 0 || K <= 0 || topk_per_span <= 0 || D % 16 ||
      S >= (1LL << 31) || P >= (1LL << 31) || N >= (1LL << 31) || J > MAX_J)
    return 0;
  const int64_t rows = relation_rows(S, P, J);
  if (rows < 0 || S * N >= (1LL << 31) || !sizes_fit(S * N, T, D, K, rows)) return 0;
  const int64_t R = std::min<int64_t>(topk_per_span, K);
  return span_layout(S * N, T, D, rows).total + tspn::align_up((size_t)rows * K * sizeof(float), 256) +
         3 * tspn::span_cand_bytes(S, P, J, R);
}

extern "C" int tspn_decode_span_relations_bf16(const uint16_t* feats, int64_t S, int64_t N, int64_t T, int64_t D,
                                               const int64_t* pairs, int64_t P, const int64_t* spans,
                                               const float* span_scores, const int64_t* span_counts, int64_t J,
                                               const uint16_t* cls_packed, const float* cls_b, int64_t K,
                                               const float* cls_logits, int64_t NO, int64_t topk_per_span,
                                               int64_t topk_per_seg, float* out_score, int64_t* out_triplet,
                                               int64_t* out_pair_tid, int64_t* out_span, int64_t* out_span_rank,
                                               int64_t* out_valid, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "tspn_decode_span_relations_bf16";
  int64_t R;
  if (int rc = tspn::span_relation_sizes(who, S, N, T, D, P, J, K, NO, topk_per_span, topk_per_seg)) return rc;
  TSPN_REQUIRE(D % 16 == 0, TSPN_EUNSUPPORTED, "%s: needs D %% 16 == 0 (D=%lld)", who, (long long)D);
  if (int rc = tspn::span_relation_limits(who, P, J, K, topk_per_span, topk_per_seg, &R)) return rc;
  if (S == 0 || P == 0) return TSPN_OK;
  TSPN_REQUIRE(N > 0, TSPN_EINVAL, "%s: pairs without tracklets", who);
  const int64_t rows = relation_rows(S, P, J);
  TSPN_REQUIRE(rows > 0 && S * N < (1LL << 31) && sizes_fit(S * N, T, D, K, rows), TSPN_EUNSUPPORTED,
               "%s: problem too large", who);
  TSPN_REQUIRE(feats && pairs && spans && span_scores && span_counts && cls_packed && cls_logits && out_score &&
                   out_triplet && out_pair_tid && out_span && out_span_rank && out_valid,
               TSPN_EINVAL, "%s: null pointer", who);
  TSPN_REQUIRE(tspn::all_aligned16(feats, cls_packed), TSPN_EUNSUPPORTED,
               "%s: unaligned pointer (feats and cls_packed need 16 bytes)", who);
  const SpanBf16Layout L = span_layout(S * N, T, D, rows);
  const size_t qb = tspn::align_up((size_t)rows * K * sizeof(float), 256);
  const size_t cb = tspn::span_cand_bytes(S, P, J, R);
  TSPN_REQUIRE(workspace && workspace_bytes >= L.total + qb + 3 * cb, TSPN_EWORKSPACE, "%s: workspace %zu < %zu bytes", who,
               workspace_bytes, L.total + qb + 3 * cb);
  TSPN_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, TSPN_EUNSUPPORTED,
               "%s: unaligned pointer (the workspace needs 256 bytes)", who);
  char* ws = static_cast<char*>(workspace) + L.total;
  float* q = reinterpret_cast<float*>(ws);
  unsigned* key = reinterpret_cast<unsigned*>(ws + qb);
  float* sc = reinterpret_cast<float*>(ws + qb + cb);
  int* ix = reinterpret_cast<int*>(ws + qb + 2 * cb);
  int rc = span_q_stage(feats, S * N, T, D, pairs, spans, rows, J, P, N, cls_packed, cls_b, K, q, workspace, stream,
                        "tspn_decode_span_relations_bf16(q)");
  if (rc) return rc;
  hipLaunchKernelGGL(span_row_topk_q_kernel, dim3((unsigned)tspn::ceil_div(rows, 4)), dim3(256), 0, TSPN_STREAM(stream), q,
                     span_scores, span_counts, rows, (int)J, (int)K, (int)R, key, sc, ix);
  if ((rc = tspn::check_launch("tspn_decode_span_relations_bf16(rows)"))) return rc;
  return tspn::segment_span_topk(key, sc, ix, pairs, spans, span_counts, cls_logits, S, N, NO, P, J, R, topk_per_seg,
                                 out_score, out_triplet, out_pair_tid, out_span, out_span_rank, out_valid, stream,
                                 "tspn_decode_span_relations_bf16(segment)");
}
