// Blocked pair stage of the fp32 path on split-fp16 MFMAs (gfx950), canonical pair table, H <= 16 (tuned for H = 12):
//     out[(p * H + h) * T + t] = bh[h] + sum_c Wh[h][c] * relu(U[s][c][t] + V[o][c][t])
// with y[B*N][2C][ldt] holding U (channels [0, C)) and V (channels [C, 2C)) of every tracklet, as heads_pairgrid4_kernel
// (tspn_heads.hip) reads it.  That kernel forms the H sums per activation on the vector pipe (2 + H / 2 instructions per
// activation).  Here the activation a = relu(u + v) is formed in fp32 as there and then split into two fp16 pieces
//     ah = f16(a),   al = f16((a - ah) * 2^11)
// (the residual is exact in the fma that forms it, al carries the next 11 bits; the 2^11 keeps it out of fp16's subnormals),
// and the head weights, scaled per head by a power of two so that the largest |w| of the head lies in [0.5, 1), are
// split the same way once per call (pairf16_pack_kernel).  Three v_mfma_f32_16x16x32_f16 per 16 frames x 32 channels,
//     acc_hi += wh * ah,     acc_lo += wh * al + wl * ah,
// and  (acc_hi + 2^-11 acc_lo) / scale_h + bh[h]  in the epilogue: every product is carried to about 2^-21 of |w a|
// (the wl * al term, 2^-22 relative, is dropped), the sums are fp32.  Held to a relative bound against float64 by
// tests/test_gpu_pair_stage_f16x3_bound.py: (20 + C / 32) 2^-24 S with S = |bh| + sum_c |w| a, plus the floor of fp16's
// subnormal spacing on the lo pieces (a lo piece below 2^-14 rounds to 2^-25 absolute: 2^-36 per activation and 2^-36
// of the head's scale per weight; fp16 subnormals themselves are kept by every instruction on the path); the
// derivation is tests/pairf16_reference.py.
//
// Range: fp16 holds ah up to 65504.  Wave w keeps the largest |U| of its subject row and the largest |V| of object
// row w over the frames whose output is written (NaN-propagating maximum, so NaN and both infinities count).  After the
// k-loop the workgroup votes: if any such value of a real tracklet is not <= 2^14 -- the rule is per half, |u| <= 2^14
// and |v| <= 2^14, which gives relu(u + v) <= 2^15; a large u that v cancels is out of range all the same -- or the
// pack kernels flagged the weights (non-finite, all below 2^-100 in a head, or 2^100 and above), the MFMA sums of the tile are discarded
// and the tile is recomputed by exact_tile(): one fmaf chain in channel order per (pair, head, frame), the sum
// heads_pairgrid4_kernel forms.  Rare by construction, untuned.
//
// Tile: 8 subjects x 8 objects x 32 frames per workgroup of 8 waves, wave w = subject w.  Stages of 32 channels x 16 rows
// x 32 frames (64 KB) land by LDS-DMA buffer loads, double-buffered.  The k index of an MFMA operand is free as long as
// A and B agree: lane (j = lane & 15, kg = lane >> 4) takes channels kg + 4 i (i = 0 .. 7) of the stage and the frame
// pair (2 j, 2 j + 1), so its ds_read_b64 of channel row kg + 4 i is conflict-free (two lane groups of a half wave sit in
// an even and an odd 128-byte row); the even frames feed one 16-column block, the odd frames the other.
#include "tspn_common.h"
#include "tspn_device.h"

#include <type_traits>

namespace {
using namespace tspn_dev;

constexpr int PF_S = 8, PF_O = 8, PF_T = 32, PF_CK = 32;
constexpr int PF_ROWS = PF_S + PF_O;
constexpr int PF_STAGE = PF_ROWS * PF_CK * PF_T;          // floats per stage (64 KB)
constexpr int PF_THREADS = 64 * PF_S;
constexpr size_t PF_SMEM = sizeof(float) * 2 * PF_STAGE;
constexpr int PF_HDR_BYTES = 256;                          // header of the split buffer: flag word, 16 inverse scales, zeros
constexpr int PF_KSTEP_BYTES = 2 * 64 * 16;                // wh and wl fragments of one k-step (64 lanes x 8 fp16 each)
constexpr float PF_LO = 2048.f, PF_LO_INV = 1.f / 2048.f;
constexpr float PF_RANGE = 16384.f;   // |u|, |v| <= 2^14: relu(u + v) <= 2^15, inside fp16

typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

std::atomic<int> g_force_exact{0};
std::atomic<int> g_diag_skip{1};   // tspn_heads_pair_f16x3_set_diag_skip

// The lo pieces of two activations whose hi pieces are the fp16 pair `h2`:  f16(as - 2^11 f32(h)) per half, `as` = 2^11 a.
// v_fma_mixlo_f16 / v_fma_mixhi_f16 read the fp16 half as an fma operand and round the fp32 result once into the low /
// high half of the destination, which a convert back, an fma and a convert would take three instructions for.
__device__ __forceinline__ unsigned split_lo(unsigned h2, float as0, float as1) {
  unsigned d;
  const float neg = -PF_LO;
  asm("v_fma_mixlo_f16 %0, %1, %2, %3 op_sel_hi:[1,0,0]" : "=v"(d) : "v"(h2), "s"(neg), "v"(as0));
  asm("v_fma_mixhi_f16 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(d) : "v"(h2), "s"(neg), "v"(as1));
  return d;
}

// ---- per-call weight split, pass 1: per head the power-of-two scale and the flag word.  One workgroup of 16 waves,
// wave h = head h.  hdr[0] = flag, hdr[1 + h] = 1 / scale_h (h < 16), hdr[17 ..] = 0: every dword of the header is written.
__global__ __launch_bounds__(1024) void pairf16_scale_kernel(const float* __restrict__ Wh, int C, int H,
                                                            unsigned* __restrict__ hdr) {
  __shared__ unsigned bad_s[16];
  const int lane = threadIdx.x & 63, h = threadIdx.x >> 6;
  float mx = 0.f;
  bool finite = true;
  // The maximum (fmaxf: of the values that are not NaN) and the finite test do not depend on the order, so a lane takes
  // 16-byte loads, four of them in flight into four partial maxima: a row of 4096 weights is 4 round trips, not 64.
  auto take = [&](float w, float& m) {
    const float a = fabsf(w);
    finite = finite && (a < __builtin_inff());         // false for NaN and Inf
    m = fmaxf(m, a);
  };
  if (h < H && (reinterpret_cast<uintptr_t>(Wh) & 15) == 0) {     // (C % 32 == 0 keeps every row aligned as Wh is)
    const float4* row = reinterpret_cast<const float4*>(Wh + (int64_t)h * C);
    const int n4 = C >> 2;
    float m[4] = {0.f, 0.f, 0.f, 0.f};
    int c = lane;
    for (; c + 192 < n4; c += 256) {
      float4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = row[c + 64 * u];
#pragma unroll
      for (int u = 0; u < 4; ++u) { take(v[u].x, m[u]); take(v[u].y, m[u]); take(v[u].z, m[u]); take(v[u].w, m[u]); }
    }
    for (; c < n4; c += 64) {
      const float4 v = row[c];
      take(v.x, m[0]); take(v.y, m[0]); take(v.z, m[0]); take(v.w, m[0]);
    }
    mx = fmaxf(fmaxf(m[0], m[1]), fmaxf(m[2], m[3]));
  } else if (h < H) {
    for (int c = lane; c < C; c += 64) take(Wh[(int64_t)h * C + c], mx);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  const bool all_finite = __all(finite);
  int e = 0;
  (void)frexpf(mx, &e);                                // mx = f * 2^e, f in [0.5, 1)
  const bool bad = h < H && (!all_finite || !(mx >= 0x1p-100f) || e > 100);
  if (lane == 0) {
    bad_s[h] = bad ? 1u : 0u;
    hdr[1 + h] = __float_as_uint((h < H && !bad) ? ldexpf(1.f, e) : 1.f);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned f = 0;
    for (int i = 0; i < 16; ++i) f |= bad_s[i];
    hdr[0] = f;
  }
  if (threadIdx.x >= 17 && threadIdx.x < PF_HDR_BYTES / 4) hdr[threadIdx.x] = 0;
}

// ---- pass 2: the A fragments.  Block = one k-step of 32 channels, thread = lane (row h = lane & 15, kg = lane >> 4);
// element i of the lane's 8 = channel 32 k + kg + 4 i.  Rows H .. 15 are zeros.
__global__ __launch_bounds__(64) void pairf16_pack_kernel(const float* __restrict__ Wh, int C, int H,
                                                         const unsigned* __restrict__ hdr, u32x4* __restrict__ frag) {
  const int lane = threadIdx.x, h = lane & 15, kg = lane >> 4;
  const float scale = 1.f / __uint_as_float(hdr[1 + h]);   // a power of two: exact
  unsigned hi[4], lo[4];
#pragma unroll
  for (int ip = 0; ip < 4; ++ip) {
    f16x2 wh, wl;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int c = blockIdx.x * PF_CK + kg + 4 * (2 * ip + e);
      const float w = (h < H) ? Wh[(int64_t)h * C + c] * scale : 0.f;
      const _Float16 a = (_Float16)w;
      wh[e] = a;
      wl[e] = (_Float16)((w - (float)a) * PF_LO);
    }
    hi[ip] = __builtin_bit_cast(unsigned, wh);
    lo[ip] = __builtin_bit_cast(unsigned, wl);
  }
  frag[(int64_t)blockIdx.x * 128 + lane] = u32x4{hi[0], hi[1], hi[2], hi[3]};
  frag[(int64_t)blockIdx.x * 128 + 64 + lane] = u32x4{lo[0], lo[1], lo[2], lo[3]};
}

// ---- the exact form of one tile: heads_pairgrid4_kernel's sum (fmaf chain in channel order from 0, bias added last)
__device__ __noinline__ void exact_tile(const float* __restrict__ y, int64_t ldt, int C, int T, int N, int H,
                                        const float* __restrict__ Wh, const float* __restrict__ bh,
                                        float* __restrict__ out, int64_t b, int sb, int ob, int t0) {
  const int t = t0 + (threadIdx.x & 31);
  if (t >= T) return;
  for (int idx = threadIdx.x >> 5; idx < PF_S * PF_O * H; idx += PF_THREADS / 32) {
    const int pair = idx / H, h = idx - pair * H;
    const int s = sb * PF_S + (pair >> 3), o = ob * PF_O + (pair & 7);
    if (s >= N || o >= N || s == o) continue;
    const float* up = y + ((b * N + s) * 2 * (int64_t)C) * ldt + t;
    const float* vp = y + ((b * N + o) * 2 * (int64_t)C + C) * ldt + t;
    const float* w = Wh + (int64_t)h * C;
    float sum = 0.f;
    for (int c = 0; c < C; ++c) sum = __builtin_fmaf(w[c], tspn::relu_f32(up[c * ldt] + vp[c * ldt]), sum);
    const int64_t p = b * N * (int64_t)(N - 1) + (int64_t)s * (N - 1) + o - (o > s ? 1 : 0);
    out[(p * H + h) * (int64_t)T + t] = sum + (bh ? bh[h] : 0.f);
  }
}

__global__ __launch_bounds__(PF_THREADS, 1) void heads_pair_f16x3_kernel(
    const float* __restrict__ y, int64_t ldt, int C, int T, int N, int H, const float* __restrict__ Wh,
    const float* __restrict__ bh, const unsigned* __restrict__ hdr, const u32x4* __restrict__ frag,
    float* __restrict__ out, int ntb, int nob, int nsb, int64_t ngroups, int force_exact, int diag_skip) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* S = reinterpret_cast<float*>(smem_raw);   // [2][16 rows][32 ch][32 t]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 15, kg = lane >> 4;
  int sb, ob;
  const int64_t G = pair_stage_group(blockIdx.x, nsb, nob, sb, ob);
  if (G >= ngroups) return;
  const int64_t b = G / ntb;
  const int t0 = (int)(G - b * ntb) * PF_T;
  const int64_t rowlen = 2 * (int64_t)C * ldt;

  if (force_exact | (int)hdr[0]) {                  // uniform over the grid
    exact_tile(y, ldt, C, T, N, H, Wh, bh, out, b, sb, ob, t0);
    return;
  }

  // ---- DMA: wave w stages tile rows 2w, 2w + 1, four pieces (8 channels x 32 frames) each
  const __amdgpu_buffer_rsrc_t rsrc_y = buffer_rsrc(y + b * N * rowlen, (int)(unsigned)((int64_t)N * rowlen * 4));
  unsigned voff[2];
  const unsigned loff = (unsigned)((lane >> 3) * ldt + min((int64_t)t0 + (lane & 7) * 4, ldt - 4));
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int row = 2 * wave + r;
    const int local = row < PF_S ? sb * PF_S + row : ob * PF_O + (row - PF_S);
    const int64_t trk = min(local, N - 1);
    voff[r] = (unsigned)((trk * rowlen + (row < PF_S ? 0 : (int64_t)C * ldt) + loff) * 4);
  }
  const int piece_bytes = (int)(8 * ldt * 4);
  int y_soff = 0;
  auto stage = [&](int buf) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        bglds16(rsrc_y, voff[r], y_soff + q * piece_bytes, S + buf * PF_STAGE + ((2 * wave + r) * PF_CK + 8 * q) * PF_T);
    }
    y_soff += 4 * piece_bytes;
  };

  f32x4 acc_hi[PF_O][2], acc_lo[PF_O][2];
#pragma unroll
  for (int o = 0; o < PF_O; ++o) {
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) acc_hi[o][cb] = acc_lo[o][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  const int nk = C / PF_CK;
  stage(0);
  u32x4 wh = frag[lane], wl = frag[64 + lane];
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  const float* urow = S + (wave * PF_CK + kg) * PF_T + 2 * j;        // + buffer + 4 i channels
  const float* vrow = S + (PF_S * PF_CK + kg) * PF_T + 2 * j;        // + buffer + object * 32 channels + 4 i channels
  const float* trow = vrow + wave * PF_CK * PF_T;                    // the object row whose range this wave tracks
  float mu = 0.f, mv = 0.f;
  // A diagonal tile (sb == ob) has no pair (s, s): wave w walks the seven objects (w + 1 + i) & 7, i = 0 .. 6, slot i
  // into accumulator i, and forms nothing for object w.  Every other tile walks object i in slot i.  Two instances of
  // the loop: the identity walk keeps its objects as immediate offsets of the LDS reads.
  const bool diag = diag_skip && sb == ob;
  auto kloop = [&](auto diag_c) {
    constexpr bool DIAG = decltype(diag_c)::value;
    constexpr int NS = DIAG ? PF_O - 1 : PF_O;
    for (int k = 0; k < nk; ++k) {
      const int buf = k & 1;
      u32x4 whn = wh, wln = wl;
      if (k + 1 < nk) {
        stage(buf ^ 1);
        whn = frag[(int64_t)(k + 1) * 128 + lane];
        wln = frag[(int64_t)(k + 1) * 128 + 64 + lane];
      }
      const float* ub = urow + buf * PF_STAGE;
      const float* vb = vrow + buf * PF_STAGE;
      const float* tb = trow + buf * PF_STAGE;
      auto vobj = [&](int i) { return vb + (DIAG ? ((wave + 1 + i) & 7) : i) * (PF_CK * PF_T); };
      f32x2 u[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        u[i] = *reinterpret_cast<const f32x2*>(ub + 4 * i * PF_T);
        const f32x2 vt = *reinterpret_cast<const f32x2*>(tb + 4 * i * PF_T);
        mu = __builtin_elementwise_maximum(__builtin_elementwise_maximum(mu, __builtin_fabsf(u[i][0])), __builtin_fabsf(u[i][1]));
        mv = __builtin_elementwise_maximum(__builtin_elementwise_maximum(mv, __builtin_fabsf(vt[0])), __builtin_fabsf(vt[1]));
      }
      const f16x8 a_hi = __builtin_bit_cast(f16x8, wh), a_lo = __builtin_bit_cast(f16x8, wl);
      // Software pipeline over the slots: slot o forms the fragments of its object on the vector pipe while the six
      // MFMAs of slot o - 1 run, and reads the V values of slot o + 1 from LDS; the two MFMAs into one acc_lo are
      // issued two MFMAs apart.  The add and the 2^11 stay packed fp32 (v_pk_add_f32, v_pk_mul_f32): the same chain in
      // single fp32 instructions, and with the 2^11 carried through an fma, timed slower here (profiles/r33/README.md).
      f32x2 v[8], vn[8];
      u32x4 fh[2], fl[2], gh[2], gl[2];
      {
        const float* vp = vobj(0);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = *reinterpret_cast<const f32x2*>(vp + 4 * i * PF_T);
      }
#pragma unroll
      for (int o = 0; o <= NS; ++o) {
        if (o + 1 < NS) {
          const float* vp = vobj(o + 1);
#pragma unroll
          for (int i = 0; i < 8; ++i) vn[i] = *reinterpret_cast<const f32x2*>(vp + 4 * i * PF_T);
        }
        if (o < NS) {
          f32x2 a[8], as[8];
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const f32x2 x = u[i] + v[i];
            a[i] = f32x2{tspn::relu_f32(x[0]), tspn::relu_f32(x[1])};
            as[i] = a[i] * PF_LO;
          }
#pragma unroll
          for (int cb = 0; cb < 2; ++cb) {
            unsigned ph[4], pl[4];
#pragma unroll
            for (int ip = 0; ip < 4; ++ip) {
              // ah = f16(a) (round to nearest), al = f16(2^11 a - 2^11 ah): the fma is exact before its one rounding to fp16
              const f16x2 h = __builtin_convertvector(f32x2{a[2 * ip][cb], a[2 * ip + 1][cb]}, f16x2);
              ph[ip] = __builtin_bit_cast(unsigned, h);
              pl[ip] = split_lo(ph[ip], as[2 * ip][cb], as[2 * ip + 1][cb]);
            }
            gh[cb] = u32x4{ph[0], ph[1], ph[2], ph[3]};
            gl[cb] = u32x4{pl[0], pl[1], pl[2], pl[3]};
          }
        }
        if (o > 0) {
          const f16x8 h0 = __builtin_bit_cast(f16x8, fh[0]), h1 = __builtin_bit_cast(f16x8, fh[1]);
          const f16x8 l0 = __builtin_bit_cast(f16x8, fl[0]), l1 = __builtin_bit_cast(f16x8, fl[1]);
          acc_hi[o - 1][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_hi, h0, acc_hi[o - 1][0], 0, 0, 0);
          acc_lo[o - 1][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_hi, l0, acc_lo[o - 1][0], 0, 0, 0);
          acc_hi[o - 1][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_hi, h1, acc_hi[o - 1][1], 0, 0, 0);
          acc_lo[o - 1][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_hi, l1, acc_lo[o - 1][1], 0, 0, 0);
          acc_lo[o - 1][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_lo, h0, acc_lo[o - 1][0], 0, 0, 0);
          acc_lo[o - 1][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_lo, h1, acc_lo[o - 1][1], 0, 0, 0);
        }
        if (o > 0 && o < NS) {
#define TSPN_G                                         \
  __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   \
  __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);   \
  __builtin_amdgcn_sched_group_barrier(0x002, 10, 0);
          TSPN_G TSPN_G TSPN_G TSPN_G TSPN_G TSPN_G
#undef TSPN_G
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
          fh[cb] = gh[cb];
          fl[cb] = gl[cb];
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = vn[i];
      }
      wh = whn;
      wl = wln;
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's LDS-DMA pieces have landed before the barrier publishes them
      __syncthreads();
    }
  };
  if (diag) kloop(std::true_type{});
  else kloop(std::false_type{});

  // ---- range vote over the staged values that a written output reads: frame pair in range, row a real tracklet
  const int tA = t0 + 2 * j;
  const int s = sb * PF_S + wave;
  const bool bad = tA < T && ((s < N && !(mu <= PF_RANGE)) || (ob * PF_O + wave < N && !(mv <= PF_RANGE)));
  if (__syncthreads_or(bad)) {
    exact_tile(y, ldt, C, T, N, H, Wh, bh, out, b, sb, ob, t0);
    return;
  }

  if (tA >= T || s >= N) return;
  float inv[4], bias[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int h = 4 * kg + r;
    inv[r] = __uint_as_float(hdr[1 + h]);
    bias[r] = (h < H && bh) ? bh[h] : 0.f;
  }
#pragma unroll
  for (int o = 0; o < PF_O; ++o) {             // slot o holds object (w + 1 + o) & 7 of a diagonal tile, object o elsewhere
    if (diag && o == PF_O - 1) continue;
    const int ot = ob * PF_O + (diag ? (wave + 1 + o) & 7 : o);
    if (ot >= N || ot == s) continue;
    const int64_t p = b * N * (int64_t)(N - 1) + (int64_t)s * (N - 1) + ot - (ot > s ? 1 : 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int h = 4 * kg + r;
      if (h >= H) continue;
      const float v0 = __builtin_fmaf(acc_lo[o][0][r], PF_LO_INV, acc_hi[o][0][r]) * inv[r] + bias[r];
      const float v1 = __builtin_fmaf(acc_lo[o][1][r], PF_LO_INV, acc_hi[o][1][r]) * inv[r] + bias[r];
      *reinterpret_cast<float2*>(out + (p * H + h) * (int64_t)T + tA) = make_float2(v0, v1);   // T is even: tA + 1 < T
    }
  }
}

}  // namespace

size_t tspn::heads_pair_f16x3_split_bytes(int64_t C, int64_t H) {
  if (C <= 0 || C % PF_CK != 0 || C >= (1 << 24) || H <= 0 || H > 16) return 0;
  return (size_t)PF_HDR_BYTES + (size_t)(C / PF_CK) * PF_KSTEP_BYTES;
}

bool tspn::heads_pair_f16x3_supported(const float* y, int64_t ldt, int64_t N, int64_t C, int64_t T, int64_t H,
                                      const float* out) {
  return H > 0 && H <= 16 && C > 0 && C % PF_CK == 0 && C < (1 << 24) && T > 0 && T % 2 == 0 && ldt >= T && ldt % 4 == 0 &&
         ldt < (1 << 24) && N < (1 << 15) && N * 2 * C * ldt * 4 < (1LL << 31) && tspn::aligned16(y) &&
         (reinterpret_cast<uintptr_t>(out) & 7) == 0;
}

int tspn::heads_pair_f16x3(const float* y, int64_t ldt, int64_t B, int64_t N, int64_t C, int64_t T, const float* Wh,
                           const float* bh, int64_t H, void* split_buf, size_t split_bytes, float* out, void* stream) {
  const char* what = "tspn_heads_pairgrid_f16x3";
  TSPN_REQUIRE(B >= 0 && N >= 0 && C > 0 && T > 0 && ldt >= T, TSPN_EINVAL,
               "%s: bad sizes B=%lld N=%lld C=%lld T=%lld ldt=%lld", what, (long long)B, (long long)N, (long long)C,
               (long long)T, (long long)ldt);
  TSPN_REQUIRE(H > 0 && H <= 16, TSPN_EUNSUPPORTED, "%s: H=%lld not in [1,16]", what, (long long)H);
  if (B == 0 || N < 2) return TSPN_OK;
  TSPN_REQUIRE(y && Wh && out && split_buf, TSPN_EINVAL, "%s: null pointer", what);
  TSPN_REQUIRE(tspn::heads_pair_f16x3_supported(y, ldt, N, C, T, H, out), TSPN_EUNSUPPORTED,
               "%s: needs C %% 32 == 0, even T, ldt %% 4 == 0, a video's projections below 2 GB, y 16-byte and out 8-byte "
               "aligned", what);
  const size_t need = tspn::heads_pair_f16x3_split_bytes(C, H);
  TSPN_REQUIRE(split_bytes >= need, TSPN_EWORKSPACE, "%s: split buffer %zu < %zu bytes", what, split_bytes, need);
  TSPN_REQUIRE(tspn::aligned16(split_buf), TSPN_EINVAL, "%s: split buffer must be 16-byte aligned", what);
  const int ntb = (int)tspn::ceil_div(T, PF_T);
  const int nsb = (int)tspn::ceil_div(N, PF_S), nob = (int)tspn::ceil_div(N, PF_O);
  const int64_t ngroups = B * ntb;
  const int64_t nwg = tspn::ceil_div(ngroups, 8) * 8 * nsb * nob;
  TSPN_REQUIRE(nwg < (1LL << 31), TSPN_EUNSUPPORTED, "%s: grid too large", what);
  hipStream_t s = TSPN_STREAM(stream);
  unsigned* hdr = static_cast<unsigned*>(split_buf);
  u32x4* frag = reinterpret_cast<u32x4*>(static_cast<char*>(split_buf) + PF_HDR_BYTES);
  hipLaunchKernelGGL(pairf16_scale_kernel, dim3(1), dim3(1024), 0, s, Wh, (int)C, (int)H, hdr);
  hipLaunchKernelGGL(pairf16_pack_kernel, dim3((unsigned)(C / PF_CK)), dim3(64), 0, s, Wh, (int)C, (int)H, hdr, frag);
  static tspn::LdsLimit lds;
  if (int rc = lds.ensure(reinterpret_cast<const void*>(heads_pair_f16x3_kernel), PF_SMEM, what)) return rc;
  hipLaunchKernelGGL(heads_pair_f16x3_kernel, dim3((unsigned)nwg), dim3(PF_THREADS), PF_SMEM, s, y, ldt, (int)C, (int)T,
                     (int)N, (int)H, Wh, bh, hdr, frag, out, ntb, nob, nsb, ngroups,
                     g_force_exact.load(std::memory_order_relaxed), g_diag_skip.load(std::memory_order_relaxed));
  return tspn::check_launch(what);
}

extern "C" size_t tspn_heads_pairgrid_f16x3_split_bytes(int64_t C, int64_t H) {
  return tspn::heads_pair_f16x3_split_bytes(C, H);
}

extern "C" int tspn_heads_pairgrid_f16x3_set_force_exact(int on) {
  TSPN_REQUIRE(on == 0 || on == 1, TSPN_EINVAL, "tspn_heads_pairgrid_f16x3_set_force_exact: on must be 0 or 1");
  return g_force_exact.exchange(on, std::memory_order_relaxed);
}

extern "C" int tspn_heads_pair_f16x3_set_diag_skip(int on) {
  TSPN_REQUIRE(on == 0 || on == 1, TSPN_EINVAL, "tspn_heads_pair_f16x3_set_diag_skip: on must be 0 or 1");
  return g_diag_skip.exchange(on, std::memory_order_relaxed);
}

extern "C" int tspn_heads_pairgrid_f16x3(const float* y, int64_t ldt, int64_t B, int64_t N, int64_t C, int64_t T,
                                         const float* Wh, const float* bh, int64_t H, void* split_buf, size_t split_bytes,
                                         float* out, void* stream) {
  return tspn::heads_pair_f16x3(y, ldt, B, N, C, T, Wh, bh, H, split_buf, split_bytes, out, stream);
}
