// Shared host-side helpers for the TSPN C-ABI (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "tspn_mi355x.h"

namespace tspn {

// thread-local last-error buffer (tspn_last_error)
char* err_buf();
constexpr int kErrBufLen = 512;

inline int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(err_buf(), kErrBufLen, fmt, ap);
  va_end(ap);
  return code;
}

// (tspn_status.hip) TSPN_EDEVICE if a kernel of an earlier launch raised a fault through the device status block
int status_check(const char* what);

// Every launch entry ends here: the HIP launch error of THIS call, else a device fault raised by an EARLIER one
// (read from pinned host memory: no synchronisation).
inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(TSPN_ELAUNCH, "%s: %s", what, hipGetErrorString(e));
  return status_check(what);
}

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
// 16-byte alignment, which every vector load, LDS-DMA piece and buffer descriptor of the kernels asks of its operands
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
template <class... P>
inline bool all_aligned16(const P*... p) {
  return (aligned16(p) && ...);
}
// the smallest power of two >= n (1 for n <= 1)
__host__ __device__ inline int64_t next_pow2(int64_t n) {
  int64_t p = 1;
  while (p < n) p <<= 1;
  return p;
}

// ---- non-finite contract
// ReLU as torch's F.relu: NaN in -> NaN out (fmaxf(v, 0) would return 0).  One v_maximum3_f32 on gfx950.
__device__ __forceinline__ float relu_f32(float v) { return __builtin_elementwise_maximum(v, 0.f); }
// The maximum of a pool window as torch's F.max_pool2d: a NaN operand -> NaN (fmaxf would return the other operand).
__device__ __forceinline__ float maximum_f32(float a, float b) { return __builtin_elementwise_maximum(a, b); }

// torch's descending sort order as an unsigned key: larger value -> larger key, every NaN (any sign, any payload)
// -> 0xffffffff above +Inf (0xff800000), -0 == +0.  Real values never map to 0, which is left for padding.
__device__ __forceinline__ unsigned order_key(float v) {
  if (v != v) return 0xffffffffu;
  const unsigned u = __float_as_uint(v + 0.f);   // -0 + 0 = +0
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// (key, index) order of a stable descending sort: larger key first, lower index first on ties
__device__ __forceinline__ bool key_before(unsigned ka, int ia, unsigned kb, int ib) {
  return ka > kb || (ka == kb && ia < ib);
}

// the largest v over the wave, in every lane
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(v, o, 64);
    v = other > v ? other : v;
  }
  return v;
}

// hipFuncAttributeMaxDynamicSharedMemorySize is a PER-DEVICE attribute of a kernel.  One static
// LdsLimit per launch site remembers, per device ordinal, the largest limit already set there, so the
// attribute call is paid once per (kernel, device) — not once per thread, which left every device but
// the first one a thread used without the raised limit.
struct LdsLimit {
  static constexpr int kMaxDevices = 64;
  std::atomic<size_t> set[kMaxDevices] = {};
  int ensure(const void* fn, size_t bytes, const char* what) {
    int dev = -1;
    (void)hipGetDevice(&dev);
    const bool tracked = dev >= 0 && dev < kMaxDevices;
    if (tracked && set[dev].load(std::memory_order_relaxed) >= bytes) return TSPN_OK;
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess)
      return fail(TSPN_ELAUNCH, "%s: hipFuncSetAttribute(%zu bytes of LDS): %s", what, bytes,
                  hipGetErrorString(e));
    if (tracked) set[dev].store(bytes, std::memory_order_relaxed);
    return TSPN_OK;
  }
};

// Internal (not exported) forms with explicit row strides, shared between translation units.
// y[b][m][ldy]: the fused driver pads rows of the tracklet projections to a multiple of 4 frames so
// that the pair stage can stage them with 16-byte LDS-DMA pieces.
int conv3_tc_direct(const float* x, int64_t B, int64_t T, int64_t Cin, const float* packed, int64_t M,
                    const float* bias, int relu, float* y, int64_t ldy, void* stream);
// Winograd F(6,3) (tspn_wino63.hip): input transform V = B^T d as its own pass into `workspace`, then the
// MFMA contraction on fragment-major weights; Cin % 32 == 0, M % 32 == 0
bool wino63_supported(int64_t Cin, int64_t M);
size_t wino63_workspace_bytes(int64_t B, int64_t T, int64_t Cin);
int wino63_input_transform(const float* x, int64_t B, int64_t T, int64_t Cin, void* workspace,
                           size_t workspace_bytes, void* stream, uint64_t* hot = nullptr);
int wino63_contract(const void* workspace, int64_t B, int64_t T, int64_t Cin, const float* frag, int64_t M,
                    const float* bias, int relu, float* y, int64_t ldy, void* stream);
int conv3_tc_wino63(const float* x, int64_t B, int64_t T, int64_t Cin, const float* frag, int64_t M,
                    const float* bias, int relu, float* y, int64_t ldy, void* workspace,
                    size_t workspace_bytes, void* stream);
// Split-fp16 F(6,3) (TSPN_CONV_WINOGRAD63_F16X3, tspn_wino63.hip): Cin % 32 == 0, M % 256 == 0; the workspace holds the
// split transformed input and the contraction's parking area
bool wino63_f16x3_supported(int64_t Cin, int64_t M);
size_t wino63_f16x3_workspace_bytes(int64_t B, int64_t T, int64_t Cin, int64_t M);
// `fused_in`: which input kernels run -- wino63_f16x3_fused_input()'s answer, asked once per pass.  The fused form (scan +
// split kernels) also writes the temporal mean `fbar` [B, Cin] where that is not null (the two-pass transform ignores it).
int wino63_f16x3_input_transform(const float* x, int64_t B, int64_t T, int64_t Cin, int64_t M, void* workspace,
                                 size_t workspace_bytes, void* stream, uint64_t* hot = nullptr, bool fused_in = false,
                                 float* fbar = nullptr, int stages = 3);
// whether a launch of B tracklets takes the fused input kernels: tspn_conv3_tc_wino63_f16x3_set_input_form()'s switch,
// else wino63_f16x3_input_form() on the current device's CUs
bool wino63_f16x3_fused_input(int64_t B, int64_t T, int64_t Cin);
// The fused input kernels (inputf16/tspn_input_f16x3.hip): split input, column exponents, hot-sextet report and
// (fbar != nullptr) the temporal mean from two reads of x.  nsp2: the padded sextet count of the workspace layout.
// `stages`: TSPN_INPUT_SCAN (column exponents, hot sextet, mean) | TSPN_INPUT_SPLIT (the halves, behind a scan on the same
// stream) -- the fused pass puts the predicate head and its event between the two.
constexpr int TSPN_INPUT_SCAN = 1, TSPN_INPUT_SPLIT = 2;
bool input_f16x3_supported(int64_t T, int64_t Cin);
int input_f16x3(const float* x, int64_t NT, int64_t T, int64_t Cin, int64_t nsp2, _Float16* Vh, int* Ve, float* fbar,
                uint64_t* hot, void* stream, int stages = TSPN_INPUT_SCAN | TSPN_INPUT_SPLIT);
int wino63_f16x3_contract(void* workspace, size_t workspace_bytes, int64_t B, int64_t T, int64_t Cin,
                          const int16_t* packed, int64_t M, const float* bias, int relu, float* y, int64_t ldy,
                          void* stream);
int heads_pairgrid(const float* y, int64_t ldt, int64_t B, int64_t N, int64_t C, int64_t T,
                   const float* Wh, const float* bh, int64_t H, float* out, void* stream, float* Wp12 = nullptr);
// The canonical pair stage on split-fp16 MFMAs (pairf16/tspn_heads_pair_f16x3.hip).  `split_buf`: the call's split head
// weights and flag word, heads_pair_f16x3_split_bytes(C, H) bytes (0 where C or H is refused), all written by the call.
size_t heads_pair_f16x3_split_bytes(int64_t C, int64_t H);
bool heads_pair_f16x3_supported(const float* y, int64_t ldt, int64_t N, int64_t C, int64_t T, int64_t H, const float* out);
int heads_pair_f16x3(const float* y, int64_t ldt, int64_t B, int64_t N, int64_t C, int64_t T, const float* Wh,
                     const float* bh, int64_t H, void* split_buf, size_t split_bytes, float* out, void* stream);
inline size_t align_up(size_t a, size_t b) { return (a + b - 1) / b * b; }
int linear(const float* x, int64_t P, int64_t F, int64_t ldx, const float* W, int64_t ldw,
           const float* b, int64_t K, float* out, int apply_sigmoid, void* workspace,
           size_t workspace_bytes, void* stream);
size_t pair_predicate_workspace_bytes(int64_t NT, int64_t D, int64_t K);
int pair_predicate(const float* fbar, int64_t NT, int64_t D, const int64_t* pairs, int64_t P,
                   const float* cls_w, const float* cls_b, int64_t K, float* out, void* workspace,
                   size_t workspace_bytes, void* stream);
// First stage of span pooling (tspn_linear.hip), shared by tspn_span_predicate_f32 and tspn_decode_span_relations_f32:
// G [NT*T, 2K] = feats . cls_w read as [2K, D], and PS [NT, T+1, 2K], its float64 prefix sums over time.  Both live in
// the first span_prefix_workspace_bytes() of `workspace`; `who` names the entry point in the workspace error.
size_t span_prefix_workspace_bytes(int64_t NT, int64_t T, int64_t D, int64_t K);
int span_prefix_stage(const float* feats, int64_t NT, int64_t T, int64_t D, const float* cls_w, int64_t K,
                      void* workspace, size_t workspace_bytes, void* stream, const float** G_out,
                      const double** PS_out, const char* who);
// Last stage of the span relation decode (relations/tspn_span_relations.hip), shared by tspn_decode_span_relations_f32
// and tspn_decode_span_relations_bf16: per segment the topk_per_seg best of the P*J*R candidates a row top-k left in
// key / sc / ix (each [S, P*J*R], span_cand_bytes() apart in the entries' workspaces), and the gathers.
inline size_t span_cand_bytes(int64_t S, int64_t P, int64_t J, int64_t R) {
  return align_up((size_t)S * P * J * R * sizeof(float), 256);
}
int segment_span_topk(const unsigned* key, const float* sc, const int* ix, const int64_t* pairs, const int64_t* spans,
                      const int64_t* span_counts, const float* cls_logits, int64_t S, int64_t N, int64_t NO, int64_t P,
                      int64_t J, int64_t R, int64_t topk_per_seg, float* out_score, int64_t* out_triplet,
                      int64_t* out_pair_tid, int64_t* out_span, int64_t* out_span_rank, int64_t* out_valid, void* stream,
                      const char* what);
// The size checks both entries open with (defined beside segment_span_topk), in two steps because the bf16 entry's D % 16
// rule stands between them: the sizes, then the limits on K, topk_per_seg, J and the candidates; R = min(topk_per_span, K).
int span_relation_sizes(const char* who, int64_t S, int64_t N, int64_t T, int64_t D, int64_t P, int64_t J, int64_t K,
                        int64_t NO, int64_t topk_per_span, int64_t topk_per_seg);
int span_relation_limits(const char* who, int64_t P, int64_t J, int64_t K, int64_t topk_per_span, int64_t topk_per_seg,
                         int64_t* R);

}  // namespace tspn

#define TSPN_REQUIRE(cond, code, ...)                 \
  do {                                                \
    if (!(cond)) return tspn::fail(code, __VA_ARGS__); \
  } while (0)

#define TSPN_STREAM(s) reinterpret_cast<hipStream_t>(s)

namespace tspn {

// The opening checks of the four res4 tail entries (tail, tail_next, tail_io, tail_pipe), in two steps with the entry's
// own `if (NB == 0) return TSPN_OK;` between them -- an empty batch is accepted without a look at its operands.  The
// order decides which error a doubly wrong call gets.  First the sizes and the channel count (`channels_ok`;
// `channel_rule` words the refusal) ...
inline int tail_shape_checks(const char* what, int64_t NB, int64_t H, int64_t W, int64_t CM, bool channels_ok,
                             const char* channel_rule) {
  TSPN_REQUIRE(NB >= 0 && H > 0 && W > 0, TSPN_EINVAL, "%s: bad sizes", what);
  TSPN_REQUIRE(channels_ok, TSPN_EUNSUPPORTED, "%s: %s (got %lld)", what, channel_rule, (long long)CM);
  return TSPN_OK;
}
// ... then null operands, their alignment, and H, W below 2^20 (32-bit pixel arithmetic in the tap mask).  The fused
// bottleneck block entries call operand_checks, with their aliasing rule (`alias_rule` words the refusal) between the two.
inline int operand_checks(const char* what, std::initializer_list<const void*> operands, bool alias_free = true,
                          const char* alias_rule = nullptr) {
  bool all = true, aligned = true;
  for (const void* p : operands) {
    all = all && p != nullptr;
    aligned = aligned && aligned16(p);
  }
  TSPN_REQUIRE(all, TSPN_EINVAL, "%s: null pointer", what);
  TSPN_REQUIRE(alias_free, TSPN_EINVAL, "%s: %s", what, alias_rule);
  TSPN_REQUIRE(aligned, TSPN_EUNSUPPORTED, "%s: operands must be 16-byte aligned", what);
  return TSPN_OK;
}
inline int tail_operand_checks(const char* what, int64_t H, int64_t W, std::initializer_list<const void*> operands) {
  if (int rc = operand_checks(what, operands)) return rc;
  TSPN_REQUIRE(H < (1 << 20) && W < (1 << 20), TSPN_EUNSUPPORTED, "%s: dimension too large", what);
  return TSPN_OK;
}

// The opening checks of the conv2d and max-pool entries, again around the entry's own `if (NB == 0) return TSPN_OK;`.
// First the sizes (`sizes_ok`: each entry has its list), the entry's rule on the window (`window_rule` words the refusal; the
// pools have none) and a window larger than the padded map (the truncating division would still give one pixel) ...
inline int window_shape_checks(const char* what, bool sizes_ok, bool window_ok, const char* window_rule, int64_t H,
                               int64_t W, int64_t KH, int64_t KW, int64_t stride, int64_t pad, int64_t* OH, int64_t* OW) {
  TSPN_REQUIRE(sizes_ok, TSPN_EINVAL, "%s: bad sizes", what);
  TSPN_REQUIRE(window_ok, TSPN_EUNSUPPORTED, "%s: %s", what, window_rule);
  TSPN_REQUIRE(H + 2 * pad >= KH && W + 2 * pad >= KW, TSPN_EINVAL, "%s: empty output", what);
  *OH = (H + 2 * pad - KH) / stride + 1, *OW = (W + 2 * pad - KW) / stride + 1;
  return TSPN_OK;
}
// ... then the operands of the f32, frag and bf16 conv entries: null, the entry's divisibility rule (`channel_rule` words
// it), alignment (bias and residual may be null) and the sizes the kernels' 32-bit arithmetic holds.
inline int conv_operand_checks(const char* what, const void* x, const void* w, const void* out, const void* bias,
                               const void* residual, bool channels_ok, const char* channel_rule, int64_t H, int64_t W,
                               int64_t Cin, int64_t Cout) {
  TSPN_REQUIRE(x && w && out, TSPN_EINVAL, "%s: null pointer", what);
  TSPN_REQUIRE(channels_ok, TSPN_EUNSUPPORTED, "%s: needs %s (Cin=%lld Cout=%lld)", what, channel_rule, (long long)Cin,
               (long long)Cout);
  TSPN_REQUIRE(all_aligned16(x, w, out, bias, residual), TSPN_EUNSUPPORTED, "%s: operands must be 16-byte aligned", what);
  TSPN_REQUIRE(H < (1 << 20) && W < (1 << 20) && Cin < (1 << 24) && Cout < (1 << 24), TSPN_EUNSUPPORTED,
               "%s: dimension too large", what);
  return TSPN_OK;
}

}  // namespace tspn
