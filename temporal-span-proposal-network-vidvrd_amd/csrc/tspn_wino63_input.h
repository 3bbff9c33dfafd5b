// Pieces of the F(6,3) input transform, shared by the fp32 form and the split-fp16 forms (tspn_wino63.hip,
// inputf16/tspn_input_f16x3.hip): the kernels must agree bit for bit (the accuracy guard treats them as one algorithm,
// and the fused input kernels are held byte for byte to the two-pass one).  Everything here is force-inlined:
// -fno-gpu-rdc gives no device symbols across translation units.
#pragma once
#include "tspn_common.h"
#include "tspn_device.h"

namespace tspn_dev {

// NF consecutive frames t0 .. t0 + NF - 1 of tracklet b, four channels from `channel_offset`.  Frames outside the
// tracklet are zero (the conv's padding) and so is everything of a lane that is not `ok`; their addresses are clamped
// into the tracklet.
template <int NF>
__device__ __forceinline__ void wino63_load_frames(const float* __restrict__ x, int64_t b, int t0, int T, int Cin, bool ok,
                                                   int channel_offset, f32x4* d) {
#pragma unroll
  for (int i = 0; i < NF; ++i) {
    const int t = t0 + i;
    const int64_t n = b * T + (t < 0 ? 0 : (t < T ? t : T - 1));
    const f32x4 v = *reinterpret_cast<const f32x4*>(x + n * Cin + channel_offset);
    d[i] = (ok && t >= 0 && t < T) ? v : f32x4{0.f, 0.f, 0.f, 0.f};
  }
}
// The eight frames 6 q - 1 .. 6 q + 6 of sextet q of tracklet b; a sextet past the end of the launch (!ok) is zero.
__device__ __forceinline__ void wino63_load_sextet(const float* __restrict__ x, int64_t b, int q, int T, int Cin, bool ok,
                                                   int channel_offset, f32x4* d) {
  wino63_load_frames<8>(x, b, 6 * q - 1, T, Cin, ok, channel_offset, d);
}
// V = B^T d (d: the sextet's eight frames)
__device__ __forceinline__ void wino63_bt(const f32x4* d, f32x4 (&V)[8]) {
  V[0] = d[0] - d[6] + 5.25f * (d[4] - d[2]);
  V[7] = d[7] - d[1] + 5.25f * (d[3] - d[5]);
  {
    const f32x4 t1 = d[2] + d[6] - 4.25f * d[4], t2 = d[1] + d[5] - 4.25f * d[3];
    V[1] = t1 + t2;
    V[2] = t1 - t2;
  }
  {
    const f32x4 t1 = d[6] + 0.25f * d[2] - 1.25f * d[4], t2 = 0.5f * d[1] - 2.5f * d[3] + 2.f * d[5];
    V[3] = t1 + t2;
    V[4] = t1 - t2;
  }
  {
    const f32x4 t1 = d[6] + 4.f * (d[2] - 1.25f * d[4]), t2 = 2.f * d[1] - 2.5f * d[3] + 0.5f * d[5];
    V[5] = t1 + t2;
    V[6] = t1 - t2;
  }
}
// max(m, |v|) over the four channels, NaN-propagating (fmaxf drops NaN)
__device__ __forceinline__ float wino63_absmax4(float m, const f32x4 v) {
  return __builtin_elementwise_maximum(
      __builtin_elementwise_maximum(m, __builtin_elementwise_maximum(fabsf(v[0]), fabsf(v[1]))),
      __builtin_elementwise_maximum(fabsf(v[2]), fabsf(v[3])));
}
// m = max(m, |d[1..6]|) for the hot-sextet key.  NaN-propagating maxima: a NaN input makes its sextet
// hot, and |NaN| (sign cleared by fabsf) has larger bits than +Inf, so NaN ranks above Inf in the key.  Only the sextet's
// OWN frames d[1..6] count: a value in the halo d[0] / d[7] enters one transformed column of the neighbour (one of its
// outputs), while the sextet that holds it carries it into all six -- with the window counted, the equal keys of both went
// to the later sextet.
__device__ __forceinline__ void wino63_absmax_own_frames(const f32x4* d, float& m) {
#pragma unroll
  for (int i = 1; i < 7; ++i) m = wino63_absmax4(m, d[i]);
}
// the wave's largest key into slot `slot` of `hot`: one 64-bit atomic max per wave, no return value
__device__ __forceinline__ void wino63_hot_publish(unsigned long long* __restrict__ hot, unsigned long long key, unsigned slot) {
  key = tspn::wave_max_u64(key);
  if ((threadIdx.x & 63) == 0)
    __hip_atomic_fetch_max(hot + 32 * (slot & (TSPN_CONV_CHECK_HOT_SLOTS - 1)), key, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
}

// power-of-two exponent e with max * 2^e in [2^14, 2^15); 0 for a zero or non-finite maximum (a non-finite value then
// stays non-finite through the split, and so does every output it reaches)
__device__ __forceinline__ int split_exponent(double mx) {
  if (!(mx > 0.0) || !(mx <= 1.7976931348623157e308)) return 0;
  int k;
  (void)frexp(mx, &k);           // mx = f 2^k, f in [0.5, 1)
  return 15 - k;
}
// the two fp16 parts of v 2^e: hi = fp16(u), lo = fp16(u - hi)
__device__ __forceinline__ void wino63_split_f16(float v, int e, _Float16& hi, _Float16& lo) {
  const float u = ldexpf(v, e);
  hi = (_Float16)u;
  lo = (_Float16)(u - (float)hi);     // exact in fp32
}

}  // namespace tspn_dev
