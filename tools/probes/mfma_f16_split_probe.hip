// Probe: how v_mfma_f32_32x32x16_f16 sums its 16 products, and whether it keeps fp16 subnormal operands -- the two
// facts the split-fp16 F(6,3) form (tspn_wino63.hip, TSPN_CONV_WINOGRAD63_F16X3) rests on.  Every case is one
// 32 x 32 x 16 product with a zero accumulator, compared against the float64 sum of the same products.
//   hipcc --offload-arch=gfx950 -O3 -o tools/bin/mfma_f16_split_probe tools/probes/mfma_f16_split_probe.hip
// Cases (row 0 of A against column 0 of B; every other row / column zero):
//   cancel   2^24, 1, -2^24: 1 if the products are added without rounding between them, 0 if rounded one by one
//   ulp      2^24, 1, 1, 1, 1 (no cancellation): 2^24 + 4 exact, 2^24 if each +1 is rounded away
//   sub      16 x (2^-24 * 1): the smallest fp16 subnormal as an operand, sum 2^-20 (0 if flushed)
//   sub2     2^-14 (normal) * 2^-10 (normal) + 2^-20 (subnormal) * 0.5: products below the fp16 range, exact in fp32
//   mix      random hi/lo split of 16 fp32 values against 16 fp32 values: |MFMA - float64| in fp32 ulps of sum |x||w|
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// A [32][16] and B [16][32] row-major fp16; D [32][32] fp32
__global__ void probe(const _Float16* A, const _Float16* B, float* D) {
  const int l = threadIdx.x, li = l & 31, kh = l >> 5;
  f16x8 a, b;
  for (int i = 0; i < 8; ++i) {
    a[i] = A[li * 16 + 8 * kh + i];
    b[i] = B[(8 * kh + i) * 32 + li];
  }
  f32x16 acc;
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc, 0, 0, 0);
  for (int e = 0; e < 16; ++e) D[((e & 3) + 8 * (e >> 2) + 4 * kh) * 32 + li] = acc[e];
}

static double run(const std::vector<float>& a16, const std::vector<float>& b16, float* got) {
  std::vector<_Float16> A(32 * 16, (_Float16)0.f), B(16 * 32, (_Float16)0.f);
  double ref = 0.0;
  for (int k = 0; k < 16; ++k) {
    A[k] = (_Float16)a16[k];
    B[k * 32] = (_Float16)b16[k];
    ref += (double)(float)A[k] * (double)(float)B[k * 32];
  }
  _Float16 *dA, *dB;
  float* dD;
  (void)hipMalloc(&dA, A.size() * 2);
  (void)hipMalloc(&dB, B.size() * 2);
  (void)hipMalloc(&dD, 32 * 32 * 4);
  (void)hipMemcpy(dA, A.data(), A.size() * 2, hipMemcpyHostToDevice);
  (void)hipMemcpy(dB, B.data(), B.size() * 2, hipMemcpyHostToDevice);
  hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, dA, dB, dD);
  float D[32 * 32];
  (void)hipMemcpy(D, dD, sizeof(D), hipMemcpyDeviceToHost);
  (void)hipFree(dA);
  (void)hipFree(dB);
  (void)hipFree(dD);
  *got = D[0];
  return ref;
}

int main() {
  struct Case { const char* name; std::vector<float> a, b; };
  std::vector<Case> cases;
  auto z = [] { return std::vector<float>(16, 0.f); };
  { Case c{"cancel", z(), z()}; c.a[0] = 4096; c.b[0] = 4096; c.a[1] = 1; c.b[1] = 1; c.a[2] = -4096; c.b[2] = 4096; cases.push_back(c); }
  { Case c{"cancel_rev", z(), z()}; c.a[15] = 4096; c.b[15] = 4096; c.a[9] = 1; c.b[9] = 1; c.a[3] = -4096; c.b[3] = 4096; cases.push_back(c); }
  { Case c{"ulp", z(), z()}; c.a[0] = 4096; c.b[0] = 4096; for (int k = 1; k < 5; ++k) { c.a[k] = 1; c.b[k] = 1; } cases.push_back(c); }
  { Case c{"half_ulp", z(), z()}; c.a[0] = 4096; c.b[0] = 4096; c.a[7] = 0.5f; c.b[7] = 1; c.a[8] = 0.5f; c.b[8] = 1; cases.push_back(c); }
  { Case c{"sub", z(), z()}; for (int k = 0; k < 16; ++k) { c.a[k] = std::ldexp(1.f, -24); c.b[k] = 1; } cases.push_back(c); }
  { Case c{"sub2", z(), z()}; c.a[0] = std::ldexp(1.f, -14); c.b[0] = std::ldexp(1.f, -10); c.a[1] = std::ldexp(1.f, -20); c.b[1] = 0.5f; cases.push_back(c); }
  int bad = 0;
  for (auto& c : cases) {
    float got;
    const double ref = run(c.a, c.b, &got);
    std::printf("%-10s mfma %.9g  float64 %.9g  %s\n", c.name, got, ref, (double)got == ref ? "exact" : "DIFFERS");
    bad += (double)got != ref;
  }
  // random split operands: the worst |MFMA - float64| over 2000 draws in units of 2^-24 sum |x||w|
  srand(7);
  double worst = 0.0;
  for (int it = 0; it < 2000; ++it) {
    std::vector<float> a(16), b(16);
    double sa = 0.0;
    for (int k = 0; k < 16; ++k) {
      a[k] = (float)((rand() / (double)RAND_MAX - 0.5) * std::ldexp(1.0, rand() % 12));
      b[k] = (float)((rand() / (double)RAND_MAX - 0.5) * std::ldexp(1.0, rand() % 12));
    }
    float got;
    const double ref = run(a, b, &got);
    for (int k = 0; k < 16; ++k) sa += std::fabs((double)(float)(_Float16)a[k] * (double)(float)(_Float16)b[k]);
    if (sa > 0) worst = std::fmax(worst, std::fabs(got - ref) / (sa * std::ldexp(1.0, -24)));
  }
  std::printf("random    worst |mfma - float64| = %.3f u * sum|x||w| (2000 draws of 16 products)\n", worst);
  std::printf("%s\n", bad ? "SOME CASES DIFFER" : "all exact cases exact");
  return 0;
}
