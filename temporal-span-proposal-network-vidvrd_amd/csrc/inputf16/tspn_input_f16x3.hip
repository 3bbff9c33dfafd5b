// Input side of the split-fp16 F(6,3) conv in TWO reads of the features x [NT, T, Cin] instead of three (gfx950).  It
// produces what wino63_input_transform_kernel (split form, tspn_wino63.hip) and temporal_mean_td4_kernel (tspn_pairs.hip)
// produce, byte for byte: the split transformed input Vh / Vl [8 j][2 hl][Cin/8][nsp2][8 ch], the column exponents
// Ve [8 j][nsp2], the guard's hot-sextet report and, optionally, the temporal mean fbar [NT, Cin].
//
// A column's scale needs the maximum over ALL channels of a (sextet, point) column, so the two-pass transform reads x for
// the maxima and again for the split, and the mean kernel reads it a third time.  Here
//   input_f16x3_scan_kernel   one workgroup per tracklet, a thread owns four channels and walks the frames ONCE, in
//     order: the running per-channel sum (the mean's additions, in its order), V = B^T d per sextet for the 8 column
//     maxima (wave shuffle, one LDS row per wave, finished per chunk of 32 sextets), the hot-sextet key.  It carries the
//     two frames a sextet shares with the next in registers and holds nothing else, so many waves stream per CU.
//   input_f16x3_split_kernel  the second pass of the two-pass transform with the exponents read from Ve: a workgroup is
//     8 sextets x 32 channel groups, so the 8 sextets of a (point, channel group) are one 128-byte line -- a workgroup
//     per tracklet cannot write those: a line holds 8 sextets of the launch, a tracklet's do not start on one, and runs
//     of 32 bytes cost more than the read they save (profiles/r31/README.md).
// The scan kernel needs Cin % 8 == 0 and Cin <= 4 * IN_THREADS; its block is Cin / 4 threads rounded up to whole waves.
#include "tspn_common.h"
#include "tspn_device.h"
#include "tspn_wino63_input.h"

namespace {

using namespace tspn_dev;

constexpr int IN_THREADS = 512;          // at most: 4 channels per thread, Cin <= 2048
constexpr int IN_WAVES = IN_THREADS / 64;
constexpr int NJ = 8;                    // positions
constexpr int SCAN_Q = 32;               // sextets per chunk of the scan: their column maxima meet in LDS
constexpr int PAD_SEXTETS = 64;          // padding sextets per padding workgroup

__global__ __launch_bounds__(IN_THREADS) void input_f16x3_scan_kernel(
    const float* __restrict__ x, int* __restrict__ Ve, float* __restrict__ fbar, int T, int Cin, int nq, int64_t NT,
    int64_t nsext, int64_t nsp2, unsigned long long* __restrict__ hot) {
  __shared__ float red[IN_WAVES][SCAN_Q * NJ];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = blockDim.x >> 6;

  if ((int64_t)blockIdx.x >= NT) {                    // ---- padding sextets: exponent 0
    const int64_t S0 = nsext + (int64_t)(blockIdx.x - NT) * PAD_SEXTETS;
    const int ns = (int)(nsp2 - S0 < PAD_SEXTETS ? nsp2 - S0 : PAD_SEXTETS);
    for (int c = tid; c < NJ * ns; c += blockDim.x) Ve[(int64_t)(c / ns) * nsp2 + S0 + c % ns] = 0;
    return;
  }

  const int64_t b = blockIdx.x;
  const bool act = 4 * tid < Cin;
  const int ch = act ? 4 * tid : 0;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  unsigned long long key = 0;
  f32x4 d[8];
  wino63_load_frames<2>(x, b, -1, T, Cin, act, ch, d + 6);      // what sextet 0 takes over as its first two frames
  for (int q0 = 0; q0 < nq; q0 += SCAN_Q) {
    const int nqc = nq - q0 < SCAN_Q ? nq - q0 : SCAN_Q;
    for (int ql = 0; ql < nqc; ++ql) {
      const int q = q0 + ql;
      d[0] = d[6];
      d[1] = d[7];
      wino63_load_frames<6>(x, b, 6 * q + 1, T, Cin, act, ch, d + 2);
      if (fbar != nullptr) {                          // uniform
#pragma unroll
        for (int k = 1; k <= 6; ++k)
          if (6 * q + k - 1 < T) {                    // uniform
            const f32x4 v = d[k];
            acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
          }
      }
      if (hot != nullptr) {                           // uniform
        float m = 0.f;
        wino63_absmax_own_frames(d, m);
        const unsigned long long k = ((unsigned long long)__float_as_uint(m) << 32) | (unsigned)(b * nq + q);
        key = k > key ? k : key;
      }
      // column maxima (NaN-propagating) of this sextet over the wave's channels
      f32x4 V[NJ];
      wino63_bt(d, V);
      float cm[NJ];
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        float m = wino63_absmax4(0.f, V[j]);
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) m = __builtin_elementwise_maximum(m, __shfl_xor(m, o, 64));
        cm[j] = m;
      }
      if (lane == 0) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) red[wave][ql * NJ + j] = cm[j];
      }
    }
    __syncthreads();
    for (int c = tid; c < nqc * NJ; c += blockDim.x) {
      float m = red[0][c];
      for (int w = 1; w < nwaves; ++w) m = __builtin_elementwise_maximum(m, red[w][c]);
      Ve[(int64_t)(c & 7) * nsp2 + b * nq + q0 + (c >> 3)] = split_exponent((double)m);
    }
    __syncthreads();
  }
  if (hot != nullptr) wino63_hot_publish(hot, key, (unsigned)(blockIdx.x * IN_WAVES + wave));     // uniform
  if (fbar != nullptr && act) {
    const float ft = (float)T;
    *reinterpret_cast<float4*>(fbar + b * Cin + ch) = make_float4(acc.x / ft, acc.y / ft, acc.z / ft, acc.w / ft);
  }
}

// thread = (sextet s = tid & 7, channel group 32 blockIdx.y + (tid >> 3)), 8 channels per group: for each (j, hi / lo) the
// 8 sextets of the workgroup are one 128-byte run.  Sextets past the end of the launch are zeros (their exponent is 0).
__global__ __launch_bounds__(256) void input_f16x3_split_kernel(
    const float* __restrict__ x, const int* __restrict__ Ve, _Float16* __restrict__ Vh, int T, int Cin, int nq,
    int64_t nsext, int64_t nsp2) {
  const int tid = threadIdx.x, s = tid & 7, cg = blockIdx.y * 32 + (tid >> 3);
  const int ncg = Cin >> 3;
  if (cg >= ncg) return;
  const int64_t S = (int64_t)blockIdx.x * 8 + s;        // < nsp2 by construction of the grid
  const bool ok = S < nsext;
  const int64_t b = ok ? S / nq : 0;
  const int q = ok ? (int)(S - b * nq) : 0;
  int ecol[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) ecol[j] = Ve[(int64_t)j * nsp2 + S];
  f32x4 V[2][NJ];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    f32x4 d[8];
    wino63_load_sextet(x, b, q, T, Cin, ok, 8 * cg + 4 * h, d);
    wino63_bt(d, V[h]);
  }
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    f16x8 hi, lo;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      _Float16 h, l;
      wino63_split_f16(V[i >> 2][j][i & 3], ecol[j], h, l);
      hi[i] = h;
      lo[i] = l;
    }
    _Float16* dst = Vh + (((int64_t)j * 2 * ncg + cg) * nsp2 + S) * 8;
    *reinterpret_cast<f16x8*>(dst) = hi;
    *reinterpret_cast<f16x8*>(dst + (int64_t)ncg * nsp2 * 8) = lo;
  }
}

}  // namespace

bool tspn::input_f16x3_supported(int64_t T, int64_t Cin) {
  return T > 0 && Cin > 0 && Cin % 8 == 0 && Cin <= 4 * IN_THREADS;
}

int tspn::input_f16x3(const float* x, int64_t NT, int64_t T, int64_t Cin, int64_t nsp2, _Float16* Vh, int* Ve, float* fbar,
                      uint64_t* hot, void* stream, int stages) {
  const char* what = "tspn_conv3_tc_wino63_f16x3(fused input)";
  TSPN_REQUIRE(NT > 0 && tspn::input_f16x3_supported(T, Cin), TSPN_EUNSUPPORTED, "%s: needs Cin %% 8 == 0, Cin <= %d (Cin=%lld)",
               what, 4 * IN_THREADS, (long long)Cin);
  TSPN_REQUIRE(x && Vh && Ve && tspn::all_aligned16(x, Vh, Ve, fbar), TSPN_EINVAL, "%s: null or unaligned pointer", what);
  const int64_t nq = tspn::ceil_div(T, 6), nsext = NT * nq;
  TSPN_REQUIRE(nsp2 >= nsext && nsp2 % 8 == 0, TSPN_EINVAL, "%s: %lld padded sextets for %lld", what, (long long)nsp2,
               (long long)nsext);
  const int64_t grid = NT + tspn::ceil_div(nsp2 - nsext, PAD_SEXTETS);
  TSPN_REQUIRE(grid < (1LL << 31) && nsp2 / 8 < (1LL << 31), TSPN_EUNSUPPORTED, "%s: grid too large", what);
  const int threads = (int)tspn::align_up((size_t)(Cin / 4), 64);
  if (stages & TSPN_INPUT_SCAN)
    hipLaunchKernelGGL(input_f16x3_scan_kernel, dim3((unsigned)grid), dim3(threads), 0, TSPN_STREAM(stream), x, Ve, fbar, (int)T,
                       (int)Cin, (int)nq, NT, nsext, nsp2, reinterpret_cast<unsigned long long*>(hot));
  if (stages & TSPN_INPUT_SPLIT)
    hipLaunchKernelGGL(input_f16x3_split_kernel, dim3((unsigned)(nsp2 / 8), (unsigned)tspn::ceil_div(Cin / 8, 32)), dim3(256), 0,
                       TSPN_STREAM(stream), x, Ve, Vh, (int)T, (int)Cin, (int)nq, nsext, nsp2);
  return tspn::check_launch(what);
}
