// Winograd F(6,3) temporal conv (gfx950, fp32): six output frames from eight inputs, 8 channel-GEMMs on a sixth
// of the columns = 4/9 of the direct MFMA work; T = 150 tiles exactly (25 sextets), any other T masks the last
// sextet of a tracklet.
//
// Accuracy: exact in real arithmetic.  In fp32, at the K = 3 x 2048 contraction of the headline config, the
// error against float64 is <= 64 eps sum_k |x_k||w_k| per output (direct kernel: <= 16 eps ...); on temporally
// smooth features it equals the direct kernel's, on temporally independent heavy-tailed ones it is up to 5x
// larger (tests/test_gpu_wino63.py, profiles/r3/conv_error_realistic.txt).
//
// Points 0, +-1, +-2, +-1/2, inf (Lavin & Gray).  d_i = x[6s + i - 1], i = 0..7 (zero outside the tracklet):
//   V0 = d0 - d6 + 5.25 (d4 - d2)                       V7 = d7 - d1 + 5.25 (d3 - d5)
//   V1,V2 = (d2 + d6 - 4.25 d4) +- (d1 + d5 - 4.25 d3)
//   V3,V4 = (d6 + 0.25 d2 - 1.25 d4) +- (0.5 d1 - 2.5 d3 + 2 d5)
//   V5,V6 = (d6 + 4 (d2 - 1.25 d4)) +- (2 d1 - 2.5 d3 + 0.5 d5)
//   U0 = g0, U1,U2 = -2/9 (g0 +- g1 + g2), U3,U4 = g0/90 +- g1/45 + 2 g2/45, U5,U6 = (32 g0 +- 16 g1 + 8 g2)/45, U7 = g2
//   y0 = M0 + p12 + p34 + p56        y1 = m12 + 2 m34 + m56/2       y2 = p12 + 4 p34 + p56/4
//   y3 = m12 + 8 m34 + m56/8         y4 = p12 + 16 p34 + p56/16     y5 = m12 + 32 m34 + m56/32 + M7
//   (p_ab = M_a + M_b, m_ab = M_a - M_b, M_j = U_j . V_j contracted over the channels)
//
// Structure: the input transform is its own HBM-bound pass (fp32 MFMA and VALU do not overlap on gfx950);
// V [Cin/4][8][sextets padded to 64][4] is staged by LDS-DMA in super-stages of 32 channels (64 KB, ring of 2 =
// 128 KB of LDS); fragment-major weights go straight into MFMA operand registers.  Workgroup = 128 rows x 64
// sextets on FOUR waves, one per SIMD, each with the whole 512-register file: wave w owns rows 32 w .. 32 w + 31
// for BOTH sextet halves (256 accumulator registers, all AGPRs), so a weight fragment is loaded once per
// workgroup and feeds two MFMAs, and there is room for the weights of TWO chunks ahead.  That distance is the
// point: VMEM returns in order, so the V pieces a wave requests from HBM (2-4 us under load) hold back every
// younger weight load of that wave.  An earlier 8-wave form (2 waves per SIMD, 128 accumulators, one chunk of
// lookahead, weight rows shared through L1) stalled the MFMA pipe 12 % of the time on exactly that, and its
// workgroups drifted apart until L2 no longer served a weight panel to its sharers (42.6 M KiB fetched per
// launch against 16.8 M here); numbers in profiles/r2/wino63_ablation.md.
// One barrier per super-stage, at the end of its THIRD chunk: by then every wave has seen its pieces of S + 1
// land (in-order return behind a counted wait) and has issued its last reads of S; the fourth chunk refills its
// V registers from S + 1, and the pieces of S + 2 go into the buffer S left during the first chunk of S + 1.
// Needs Cin % 32 == 0 and M % 32 == 0.
#include <algorithm>
#include <atomic>
#include <type_traits>

#include "tspn_common.h"
#include "tspn_device.h"
#include "tspn_wino63_input.h"

namespace {

using namespace tspn_dev;

constexpr int NW = 4;                     // waves per workgroup: one per SIMD, 512 registers each
constexpr int THREADS = 64 * NW;
constexpr int BM = 128;                   // output rows per workgroup (4 blocks of 32)
constexpr int ST = 32;                    // sextets per V half-tile (a wave multiplies both halves)
constexpr int SWG = 64;                   // sextets per workgroup (two halves)
constexpr int KC = 8;                     // channels per chunk
constexpr int NJ = 8;                     // positions
constexpr int VROW = ST * 4;              // floats per (channel group, position) row: 512 B
constexpr int VCH = 2 * NJ * VROW;        // floats per chunk and half-tile: [2 g][8 j][32 sextets][4 ch] = 8 KB
constexpr int VHALF = 4 * VCH;            // floats per super-stage and half-tile: 32 KB
constexpr int VSS = 2 * VHALF;            // floats per super-stage: 64 KB
constexpr int NVB = 2;                    // ring of super-stage buffers
constexpr int NPIECE = 16;                // DMA pieces (1 KiB) per wave and super-stage: 64 / 4
constexpr size_t SMEM_BYTES = sizeof(float) * NVB * VSS;
#ifndef TSPN_WINO63_GM
// Weight panels (128 rows) per tile group: the 32 workgroups an XCD runs at a time are GM panels x 32 / GM sextet
// tiles and stream GM x 8.4 MB of weights + 32 / GM x 4.2 MB of V through its L2 -- least for GM = 4 (67 MB per
// round, 26.9 GB per launch at cfg2:16).  Measured on one box (kernel + pre-pass ms / FETCH_SIZE M KiB):
// 1: 24.20 / 28.2, 2: 23.76 / 16.8, 3: 23.94 / 14.8, 4: 23.76 / 13.4, 8: 24.33 / 16.4.
#define TSPN_WINO63_GM 4
#endif

#ifndef TSPN_WINO63_VAUX
#define TSPN_WINO63_VAUX 0                // cache policy bits of the V bursts (2 = nt: 29.2 M KiB fetched but 27.6 ms)
#endif

// nn.Conv1d weight W [M, Cin, 3] -> fragment-major transformed weights
//   frag[m' / 32][chunk = ch / 8][j = 0..7][lane = 32 kh + li][e = 0..3] = U_j[8 chunk + 4 kh + e][32 (m'/32) + li]
// `split` (the factorised pair form): Cin == 2 * split; rows [0, M) take W[:, :split], rows [M, 2M) take W[:, split:].
__global__ void pack_wino63_frag_kernel(const float* __restrict__ W, int64_t M, int64_t Cin, int64_t split,
                                        float* __restrict__ out) {
  const int64_t Mp = split ? 2 * M : M, Cp = split ? split : Cin;
  const int64_t nch = Cp / KC;
  const int64_t total = NJ * Cp * Mp;
  for (int64_t o = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; o < total;
       o += (int64_t)gridDim.x * blockDim.x) {
    const int e = (int)(o & 3);
    const int lane = (int)((o >> 2) & 63);
    const int64_t r = o >> 8;
    const int j = (int)(r % NJ);
    const int64_t c = (r / NJ) % nch;
    const int64_t mb = r / (NJ * nch);
    const int64_t ch = 8 * c + 4 * (lane >> 5) + e;
    const int64_t m = 32 * mb + (lane & 31);
    const float* g = (split && m >= M) ? W + ((m - M) * Cin + split + ch) * 3 : W + (m * Cin + ch) * 3;
    const double g0 = g[0], g1 = g[1], g2 = g[2];
    double u;
    switch (j) {
      case 0: u = g0; break;
      case 1: u = -2.0 / 9.0 * (g0 + g1 + g2); break;
      case 2: u = -2.0 / 9.0 * (g0 - g1 + g2); break;
      case 3: u = g0 / 90.0 + g1 / 45.0 + 2.0 * g2 / 45.0; break;
      case 4: u = g0 / 90.0 - g1 / 45.0 + 2.0 * g2 / 45.0; break;
      case 5: u = (32.0 * g0 + 16.0 * g1 + 8.0 * g2) / 45.0; break;
      case 6: u = (32.0 * g0 - 16.0 * g1 + 8.0 * g2) / 45.0; break;
      default: u = g2; break;
    }
    out[o] = (float)u;
  }
}

// (the pieces of the input transform that the fp32 form and the split-fp16 forms share: tspn_wino63_input.h)

// Input transform V = B^T d.  A wave = 8 sextets x 8 channel groups (loads: whole 128-byte lines of x; stores:
// 128-byte runs of Vg).  Frames outside the tracklet are zero (the conv's padding); sextets past the end of the
// launch are zero too.
// `hot` (optional, for the accuracy guard of tspn_conv_guard.hip): the kernel reads every input value anyway, so it also
// reports WHERE the launch's largest |x| sits -- key = (float bits << 32 | sextet), one 64-bit atomic max per wave, no return
// value, into one of TSPN_CONV_CHECK_HOT_SLOTS slots 256 bytes apart (the reader takes the max over the slots).  Measured
// forms (profiles/r6/conv_guard.md): ONE word with an atomic load as a filter in front: +50 - 70 us (100 000 waves on one
// L2 line); one word with a cached plain load as the filter: +300 - 600 us (the stale filter lets thousands of atomics
// through to one address); 64 slots, unfiltered: within the noise of the kernel without it.
__global__ __launch_bounds__(256) void wino63_input_transform_kernel(
    const float* __restrict__ x, float* __restrict__ Vg, int T, int Cin, int nq, int64_t nsext, int64_t nsp,
    int64_t ncols, unsigned long long* __restrict__ hot) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int cgl = lane & 7, ql = lane >> 3;
  const int64_t S = ((int64_t)blockIdx.x * 4 + wave) * 8 + ql;     // < nsp by construction of the grid
  const int cg = blockIdx.y * 8 + cgl;
  if (4 * cg >= Cin) return;
  const bool ok = S < nsext;
  const int64_t b = ok ? S / nq : 0;
  const int q = ok ? (int)(S - b * nq) : 0;
  f32x4 d[8], V[8];
  wino63_load_sextet(x, b, q, T, Cin, ok, 4 * cg, d);
  if (hot) {                                                         // uniform
    float m = 0.f;
    wino63_absmax_own_frames(d, m);
    wino63_hot_publish(hot, ((unsigned long long)__float_as_uint(m) << 32) | (unsigned)(S < nsext ? S : 0),
                       blockIdx.x * 4 + wave + 7 * blockIdx.y);
  }
  wino63_bt(d, V);
#pragma unroll
  for (int j = 0; j < 8; ++j)
    *reinterpret_cast<f32x4*>(Vg + (((int64_t)cg * NJ + j) * nsp + S) * 4) = V[j];
}

// BUFV: the V pieces are buffer loads (buffer_load_dwordx4 ... offen lds: one SGPR descriptor of the workspace, a fixed
// 32-bit lane offset per piece, a scalar offset per super-stage) instead of global_load_lds_dwordx4 with sixteen 64-bit
// pointers per lane that are bumped by vector adds every super-stage: cheaper to issue in the MFMA shadows
// (tools/probes/lds_dma_issue_probe.hip) and 16 registers less.  Needs a workspace below 4 GB (the launcher chooses).
template <bool BUFV>
__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(1, 1))) void conv3_wino63_kernel(
    const float* __restrict__ Vg, const float* __restrict__ Wf, const float* __restrict__ bias,
    float* __restrict__ y, int Cin, int T, int M, int nq, int64_t nsext, int64_t nsp, int tiles_m,
    int tiles_n, int relu, int ldy, int GM, int vec2) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* Vs = reinterpret_cast<float*>(smem_raw);

  // workgroup -> tile: bijective XCD remap, then groups of GM weight panels x all sextet tiles
  int tile_m, tile_n;
  grouped_tile(xcd_remap(blockIdx.x, gridDim.x), GM, tiles_m, tiles_n, tile_m, tile_n);
  const int m0 = tile_m * BM;
  const int64_t S0 = (int64_t)tile_n * SWG;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);     // = 32-row block of the tile
  const int li = lane & 31, kh = lane >> 5;
  const int nsuper = Cin >> 5;

  const char* abase;            // wave-uniform; points at the chunk TWO ahead of the one being multiplied
  const unsigned aoff = lane * 16;
  {
    int mb = (m0 >> 5) + wave;
    mb = mb < (M >> 5) ? mb : 0;
    abase = reinterpret_cast<const char*>(Wf) + (int64_t)mb * (Cin / KC) * (NJ * 64 * 16);
  }

  // V super-stage DMA: piece pp = 16 wave + k, same LDS image as the 8-wave form
  const float* vsrc[BUFV ? 1 : NPIECE];
  unsigned voff[BUFV ? NPIECE : 1];
#pragma unroll
  for (int k = 0; k < NPIECE; ++k) {
    const int pp = NPIECE * wave + k;
    const int rr = 2 * (pp & 31) + kh;
    const int cl = rr >> 4, rem = rr & 15;
    const int g = rem >> 3, j = rem & 7;
    const int64_t e = (((int64_t)(2 * cl + g) * NJ + j) * nsp + S0 + ST * (pp >> 5) + li) * 4;
    if constexpr (BUFV) voff[k] = (unsigned)(e * 4); else vsrc[k] = Vg + e;
  }
  const int64_t super_step = (int64_t)8 * NJ * nsp * 4;
  const __amdgpu_buffer_rsrc_t rsrc_v = buffer_rsrc(Vg, (int)0xffffffffu);
  const unsigned super_bytes = (unsigned)(super_step * 4);
  auto stage_piece = [&](int S, int k) {          // piece k of this wave, super-stage S -> ring buffer S & 1
    if constexpr (BUFV) {
      const int soff = (int)((unsigned)S * super_bytes);
      bglds16(rsrc_v, voff[k], soff, Vs + (S & 1) * VSS + (NPIECE * wave + k) * 256);
    } else {
      glds16<TSPN_WINO63_VAUX>(vsrc[k], Vs + (S & 1) * VSS + (NPIECE * wave + k) * 256);
    }
    if constexpr (!BUFV) vsrc[k] += super_step;
  };

  f32x16 acc[2][NJ];
#pragma unroll
  for (int cb = 0; cb < 2; ++cb)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[cb][j][e] = 0.f;

  f32x4 a[2][NJ], v[2][NJ];
  const float* vlane = Vs + (kh * NJ * ST + li) * 4;     // + buffer + half + chunk + position offsets
  auto load_v = [&](const float* vbuf, int cl, int j) {
    v[0][j] = *reinterpret_cast<const f32x4*>(vbuf + cl * VCH + j * VROW);
    v[1][j] = *reinterpret_cast<const f32x4*>(vbuf + VHALF + cl * VCH + j * VROW);
  };
  auto load_a_pair = [&](f32x4* ap, auto jp_tag, const char* base) {     // positions 2 jp, 2 jp + 1 of the chunk at base
    constexpr int JP = decltype(jp_tag)::value;
    if (JP == 0) { load_wfrag<0>(ap[0], aoff, base); load_wfrag<1024>(ap[1], aoff, base); }
    if (JP == 1) { load_wfrag<2048>(ap[2], aoff, base); load_wfrag<3072>(ap[3], aoff, base); }
    if (JP == 2) { load_wfrag<0>(ap[4], aoff, base + 4096); load_wfrag<1024>(ap[5], aoff, base + 4096); }
    if (JP == 3) { load_wfrag<2048>(ap[6], aoff, base + 4096); load_wfrag<3072>(ap[7], aoff, base + 4096); }
  };
  using P0 = std::integral_constant<int, 0>;
  using P1 = std::integral_constant<int, 1>;
  using P2 = std::integral_constant<int, 2>;
  using P3 = std::integral_constant<int, 3>;
  // 16 MFMAs of a position pair.  With one wave per SIMD nothing else feeds the MFMA pipe while this wave issues
  // VMEM instructions, so the 16 DMA pieces of a super-stage go out ONE per four MFMAs (S1 >= 0: pieces 4 slot ..
  // 4 slot + 3 of super-stage S1), in the shadow of the MFMA that was issued just before: issued as one burst they
  // cost 8 % of the kernel (GRBM cycles 59.2 M vs 54.5 M without DMA, profiles/r2/wino63_ablation.md).
  auto mfma_pair = [&](const f32x4* ap, int ja, int jb, int S1, int slot) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      acc[0][ja] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[ja][e], v[0][ja][e], acc[0][ja], 0, 0, 0);
      acc[0][jb] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[jb][e], v[0][jb][e], acc[0][jb], 0, 0, 0);
      acc[1][ja] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[ja][e], v[1][ja][e], acc[1][ja], 0, 0, 0);
      if (S1 >= 0) {
        __builtin_amdgcn_sched_barrier(0);
        stage_piece(S1, 4 * slot + e);
        __builtin_amdgcn_sched_barrier(0);
      }
      acc[1][jb] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[jb][e], v[1][jb][e], acc[1][jb], 0, 0, 0);
    }
  };

  // ---- prologue: super-stage 0 landed, V of chunk 0 in registers, the weights of chunks 0 and 1 in flight
#pragma unroll
  for (int k = 0; k < NPIECE; ++k) stage_piece(0, k);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
#pragma unroll
  for (int j = 0; j < NJ; ++j) load_v(vlane, 0, j);
  load_a_pair(a[0], P0{}, abase); load_a_pair(a[0], P1{}, abase); load_a_pair(a[0], P2{}, abase); load_a_pair(a[0], P3{}, abase);
  abase += NJ * 1024;
  load_a_pair(a[1], P0{}, abase); load_a_pair(a[1], P1{}, abase); load_a_pair(a[1], P2{}, abase); load_a_pair(a[1], P3{}, abase);
  abase += NJ * 1024;
  __builtin_amdgcn_sched_barrier(0);

  // chunk c = 4 S + cl multiplies (A_c in a[c & 1], V_c); position pair by position pair (slot p) it refills
  // a[c & 1] with A_{c+2} and v with V_{c+1}.  VMEM issue order of slot p: [4 V pieces of super-stage S + 1, cl == 0]
  // then the two weight loads.  The wait before slot p needs the weight loads of slot p of chunk c - 2: younger
  // than those are the later slots of chunk c - 2, everything chunk c - 1 issued, and slots < p of this chunk.
  auto chunk_body = [&](auto cl_tag, const float* vcur, const float* vnext, int S, auto has1_tag, auto has2_tag,
                        auto more_tag) {
    constexpr int CL = decltype(cl_tag)::value;
    constexpr bool HAS1 = decltype(has1_tag)::value;   // chunk c + 1 exists: refill v
    constexpr bool HAS2 = decltype(has2_tag)::value;   // chunk c + 2 exists: refill a[c & 1]
    constexpr bool MORE = decltype(more_tag)::value;   // super-stage S + 1 exists: pieces at CL 0, barrier at CL 2
    constexpr int PAR = CL & 1;
    constexpr int N1 = (HAS1 ? 8 : 0) + ((MORE && CL == 1) ? NPIECE : 0);   // issued by chunk c - 1
    constexpr int N2 = (MORE && CL == 2) ? 6 : 2;      // per later slot of chunk c - 2 (CL 2: it carried the pieces)
    constexpr int N0 = (HAS2 ? 2 : 0) + ((MORE && CL == 0) ? 4 : 0);         // per earlier slot of this chunk
    const int S1 = (MORE && CL == 0) ? S + 1 : -1;
    const float* vn = CL == 3 ? vnext : vcur;
    constexpr int NCL = (CL + 1) & 3;
    f32x4* ap = a[PAR];
    wait_w<3 * N2 + N1>(ap[0], ap[1]);
    mfma_pair(ap, 0, 1, S1, 0);
    if (HAS2) load_a_pair(ap, P0{}, abase);
    if (HAS1) { load_v(vn, NCL, 0); load_v(vn, NCL, 1); }
    __builtin_amdgcn_sched_barrier(0);
    wait_w<2 * N2 + N1 + N0>(ap[2], ap[3]);
    mfma_pair(ap, 2, 3, S1, 1);
    if (HAS2) load_a_pair(ap, P1{}, abase);
    if (HAS1) { load_v(vn, NCL, 2); load_v(vn, NCL, 3); }
    __builtin_amdgcn_sched_barrier(0);
    wait_w<N2 + N1 + 2 * N0>(ap[4], ap[5]);
    mfma_pair(ap, 4, 5, S1, 2);
    if (HAS2) load_a_pair(ap, P2{}, abase);
    if (HAS1) { load_v(vn, NCL, 4); load_v(vn, NCL, 5); }
    __builtin_amdgcn_sched_barrier(0);
    wait_w<N1 + 3 * N0>(ap[6], ap[7]);
    mfma_pair(ap, 6, 7, S1, 3);
    if (HAS2) {
      load_a_pair(ap, P3{}, abase);
      abase += NJ * 1024;
    }
    if (HAS1) { load_v(vn, NCL, 6); load_v(vn, NCL, 7); }
    __builtin_amdgcn_sched_barrier(0);
    if (MORE && CL == 2) {
      // the last wait of this chunk needed the weight loads chunk 4 S issued AFTER its last piece of super-stage
      // S + 1 (in-order VMEM return): this wave's pieces have landed; the reads above (V of chunk 4 S + 3) were the last
      // ones of buffer S & 1; the next chunk refills v from buffer S + 1
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  {
    using TT = std::true_type;
    using FF = std::false_type;
    using C0 = std::integral_constant<int, 0>;
    using C1 = std::integral_constant<int, 1>;
    using C2 = std::integral_constant<int, 2>;
    using C3 = std::integral_constant<int, 3>;
    int S = 0;
    for (; S + 1 < nsuper; ++S) {
      const float* vcur = vlane + (S & 1) * VSS;
      const float* vnext = vlane + ((S + 1) & 1) * VSS;
      chunk_body(C0{}, vcur, vnext, S, TT{}, TT{}, TT{});
      chunk_body(C1{}, vcur, vnext, S, TT{}, TT{}, TT{});
      chunk_body(C2{}, vcur, vnext, S, TT{}, TT{}, TT{});
      chunk_body(C3{}, vcur, vnext, S, TT{}, TT{}, TT{});
    }
    const float* vcur = vlane + (S & 1) * VSS;
    chunk_body(C0{}, vcur, vcur, S, TT{}, TT{}, FF{});
    chunk_body(C1{}, vcur, vcur, S, TT{}, TT{}, FF{});
    chunk_body(C2{}, vcur, vcur, S, TT{}, FF{}, FF{});
    chunk_body(C3{}, vcur, vcur, S, FF{}, FF{}, FF{});
  }

  // ---- output transform + store: lane column = sextet -> frames 6s .. 6s+5
#pragma unroll
  for (int cb = 0; cb < 2; ++cb) {
    const int64_t Sx = S0 + ST * cb + li;
    if (Sx < nsext) {
      const int64_t b = Sx / nq;
      const int q = (int)(Sx - b * nq);
      const int t = 6 * q;
      float* ycol = y + (b * M) * (int64_t)ldy + t;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int m = m0 + wave * 32 + (e & 3) + 8 * (e >> 2) + 4 * kh;
        if (m < M) {
          const float p12 = acc[cb][1][e] + acc[cb][2][e], m12 = acc[cb][1][e] - acc[cb][2][e];
          const float p34 = acc[cb][3][e] + acc[cb][4][e], m34 = acc[cb][3][e] - acc[cb][4][e];
          const float p56 = acc[cb][5][e] + acc[cb][6][e], m56 = acc[cb][5][e] - acc[cb][6][e];
          float o[6];
          o[0] = acc[cb][0][e] + p12 + p34 + p56;
          o[1] = m12 + 2.f * m34 + 0.5f * m56;
          o[2] = p12 + 4.f * p34 + 0.25f * p56;
          o[3] = m12 + 8.f * m34 + 0.125f * m56;
          o[4] = p12 + 16.f * p34 + 0.0625f * p56;
          o[5] = m12 + 32.f * m34 + 0.03125f * m56 + acc[cb][7][e];
          if (bias != nullptr) {
            const float bb = bias[m];
#pragma unroll
            for (int i = 0; i < 6; ++i) o[i] += bb;
          }
          if (relu) {
#pragma unroll
            for (int i = 0; i < 6; ++i) o[i] = tspn::relu_f32(o[i]);
          }
          float* dst = ycol + (int64_t)m * ldy;
          if (vec2) {
            *reinterpret_cast<f32x2*>(dst) = f32x2{o[0], o[1]};
            *reinterpret_cast<f32x2*>(dst + 2) = f32x2{o[2], o[3]};
            *reinterpret_cast<f32x2*>(dst + 4) = f32x2{o[4], o[5]};
          } else {
#pragma unroll
            for (int i = 0; i < 6; ++i)
              if (t + i < T) dst[i] = o[i];
          }
        }
      }
    }
  }
}

// ================================================================================================================
// Split-fp16 form (TSPN_CONV_WINOGRAD63_F16X3): the same F(6,3) algorithm, its 8 point GEMMs on the f16 MFMA
// (v_mfma_f32_32x32x16_f16, 16x the FLOP per clock of the fp32 one).  Every operand is split into two fp16 parts,
// x ~ hi + lo (11 + 11 significand bits), and a product is x.w ~ hi_x.hi_w + hi_x.lo_w + lo_x.hi_w (Ootomo & Yokota
// 2022): three f16 MFMAs, each product exact in fp32, one fp32 accumulator.  fp16's exponent range is handled by
// power-of-two scales, exact and free to undo: one per (point, output row) of the weights, one per (point, sextet)
// column of the transformed input, chosen so that the largest |value| of the row / column lies in [2^14, 2^15).  The
// unscale 2^-(e_row + e_col) is applied to each point's accumulator before the inverse transform.  Measured accuracy
// in tests/test_gpu_wino63_f16x3.py, the MFMA's rounding behaviour in tools/probes/mfma_f16_split_probe.hip.
//
// Split weights, int16 [8 j][2 Cp/8 + 1][Mp][8]: per point j the hi parts [Cp/8][Mp][8 ch] (an A fragment = 16 bytes
// of one row), the lo parts in the same layout, then one 16-byte slot per row whose first int32 is e_row.
// Split input (workspace): fp16 [8 j][2 hl][Cin/8][nsp2][8 ch], then int32 e_col [8 j][nsp2] (nsp2: sextets padded
// to the 256-sextet tile), then the parking area of the contraction.
constexpr int F_BM = 256, F_BN = 256;          // contraction tile: output rows x sextets
constexpr int F_THREADS = 512;                 // 8 waves (2 per SIMD), wave tile 128 rows x 64 sextets
constexpr int F_ST = 4 * 2 * 256 * 16;         // one k-step (16 channels) of Wh, Wl, Vh, Vl: 32 KB
constexpr int F_NST = 4;                       // ring of stages, filled three k-steps ahead by LDS-DMA
constexpr size_t F_SMEM = (size_t)F_NST * F_ST;
constexpr size_t F_SMEM_ALL = F_SMEM + 2 * 256 * sizeof(int);   // + the exponent table of the unscale
static_assert(TSPN_WINO63_GM > 0 && TSPN_WINO63_GM < 256, "the contraction's GM argument carries the tail split and the piece form above bit 7");
constexpr size_t F_PARK_PER_TILE = (size_t)7 * F_THREADS * 128 * sizeof(float);   // points 0..6 of a tile, fp32

__device__ __forceinline__ double wino63_u(int j, double g0, double g1, double g2) {
  switch (j) {
    case 0: return g0;
    case 1: return -2.0 / 9.0 * (g0 + g1 + g2);
    case 2: return -2.0 / 9.0 * (g0 - g1 + g2);
    case 3: return g0 / 90.0 + g1 / 45.0 + 2.0 * g2 / 45.0;
    case 4: return g0 / 90.0 - g1 / 45.0 + 2.0 * g2 / 45.0;
    case 5: return (32.0 * g0 + 16.0 * g1 + 8.0 * g2) / 45.0;
    case 6: return (32.0 * g0 - 16.0 * g1 + 8.0 * g2) / 45.0;
    default: return g2;
  }
}

// Split weights: one thread per (point j, row m) -- the row's scale needs all of its Cp channels.  Runs once per weight
// version.  U_j = G g in float64 from the raw taps, scaled exactly, hi = fp16(u), lo = fp16(u - hi) (u - hi exact in
// float64).
__global__ void pack_wino63_frag_kernel(const float* __restrict__ W, int64_t M, int64_t Cin, int64_t split,
                                        int16_t* __restrict__ out) {
  const int64_t Mp = split ? 2 * M : M, Cp = split ? split : Cin;
  const int64_t ncg = Cp / 8;
  const int64_t o = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (o >= NJ * Mp) return;
  const int j = (int)(o / Mp);
  const int64_t m = o - j * Mp;
  const float* g = (split && m >= M) ? W + ((m - M) * Cin + split) * 3 : W + (m * Cin) * 3;
  double mx = 0.0;
  for (int64_t c = 0; c < Cp; ++c) {
    const double u = fabs(wino63_u(j, g[3 * c], g[3 * c + 1], g[3 * c + 2]));
    mx = (u > mx || u != u) ? u : mx;      // NaN-propagating
  }
  const int e = split_exponent(mx);
  int16_t* pj = out + (int64_t)j * (2 * ncg + 1) * Mp * 8;
  for (int64_t cg = 0; cg < ncg; ++cg) {
    f16x8 hi, lo;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int64_t c = 8 * cg + i;
      const double u = ldexp(wino63_u(j, g[3 * c], g[3 * c + 1], g[3 * c + 2]), e);
      const _Float16 h = (_Float16)(float)u;
      hi[i] = h;
      lo[i] = (_Float16)(float)(u - (double)(float)h);
    }
    *reinterpret_cast<f16x8*>(pj + (cg * Mp + m) * 8) = hi;
    *reinterpret_cast<f16x8*>(pj + ((ncg + cg) * Mp + m) * 8) = lo;
  }
  *reinterpret_cast<int4*>(pj + (2 * ncg * Mp + m) * 8) = int4{e, 0, 0, 0};   // the whole slot: no undefined bytes
}

// Split input transform: V = B^T d by the functions the fp32 form uses, then one scale per (sextet, point) column over
// ALL Cin channels, so a workgroup owns whole columns: 8 sextets x all channels; thread = (sextet s = tid & 7, channel
// group slot tid >> 3 of 32), 8 channels per group.  Pass 1 takes the column maxima (and the guard's hot-sextet key),
// pass 2 recomputes V (the x lines are in L2 by then) and writes the hi / lo halves: for each (j, channel group) the
// 8 sextets of the workgroup are one 128-byte run.
__global__ __launch_bounds__(256) void wino63_input_transform_kernel(
    const float* __restrict__ x, _Float16* __restrict__ Vh, int* __restrict__ Ve, int T, int Cin, int nq,
    int64_t nsext, int64_t nsp2, int64_t ncols, unsigned long long* __restrict__ hot) {
  __shared__ float red[4][8][NJ];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int s = tid & 7, cgs = tid >> 3;
  const int64_t S = (int64_t)blockIdx.x * 8 + s;        // < nsp2 by construction of the grid
  const bool ok = S < nsext;
  const int64_t b = ok ? S / nq : 0;
  const int q = ok ? (int)(S - b * nq) : 0;
  const int ncg = Cin >> 3;
  auto transform = [&](int cg, f32x4 (&V)[2][8], bool want_max, float& xmax) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      f32x4 d[8];
      wino63_load_sextet(x, b, q, T, Cin, ok, 8 * cg + 4 * h, d);
      if (want_max) wino63_absmax_own_frames(d, xmax);
      wino63_bt(d, V[h]);
    }
  };
  // ---- pass 1: column maxima (NaN-propagating), hot-sextet key
  float cmax[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) cmax[j] = 0.f;
  float xm = 0.f;
  for (int cg = cgs; cg < ncg; cg += 32) {
    f32x4 V[2][8];
    transform(cg, V, hot != nullptr, xm);
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int h = 0; h < 2; ++h)
        cmax[j] = wino63_absmax4(cmax[j], V[h][j]);
  }
  if (hot)                                                         // uniform
    wino63_hot_publish(hot, ((unsigned long long)__float_as_uint(xm) << 32) | (unsigned)(ok ? S : 0),
                       blockIdx.x * 4 + wave);
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    float m = cmax[j];
#pragma unroll
    for (int o = 8; o < 64; o <<= 1) m = __builtin_elementwise_maximum(m, __shfl_xor(m, o, 64));
    if (lane < 8) red[wave][lane][j] = m;
  }
  __syncthreads();
  int ecol[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const float m = __builtin_elementwise_maximum(__builtin_elementwise_maximum(red[0][s][j], red[1][s][j]),
                                                  __builtin_elementwise_maximum(red[2][s][j], red[3][s][j]));
    ecol[j] = split_exponent((double)m);
  }
  if (cgs == 0) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) Ve[(int64_t)j * nsp2 + S] = ecol[j];
  }
  // ---- pass 2: scaled hi / lo halves
  for (int cg = cgs; cg < ncg; cg += 32) {
    f32x4 V[2][8];
    transform(cg, V, false, xm);
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
}

// Split contraction.  Workgroup = 256 rows x 256 sextets, ALL 8 points one after another: per point a GEMM over the
// Cin channels, k-step = 16 channels, acc += Wh.Vh + Wh.Vl + Wl.Vh (24 MFMAs per wave and k-step).  The operands of a
// k-step (Wh, Wl, Vh, Vl: 4 x 8 KB, [2 channel groups][256][16 B], a lane's fragment = one ds_read_b128) go into a ring
// of 4 LDS stages by LDS-DMA three k-steps ahead, with a counted vmcnt and one bare s_barrier per k-step (the ring of
// conv3_bf16_big_kernel).  At the end of a point the accumulator is unscaled and, for points 0..6, parked in the
// workspace (each lane reads back exactly what it wrote: no synchronisation, deterministic); after point 7 the lane
// reads its 7 parked tiles back, applies the inverse transform and the bias and writes y as the fp32 form does.
//
// The tile body, for 256 rows x 64 WN sextets.  The 8 waves are 8 / WN over the rows x WN over the sextets, a wave tile
// is 32 WN rows x 64 sextets (WN x 2 accumulators of 32 x 32):
//   WN = 4  the full tile: 2 x 4 waves of 128 x 64
//   WN = 2  half a tile (tail split by 2): 4 x 2 waves of 64 x 64
//   WN = 1  a quarter (tail split by 4): 8 x 1 waves of 32 x 64
// The LDS image of a stage and the A fragments are the same in all three; a narrower tile fills only the first 64 WN
// sextets of each V row, so a stage is 16 + 4 WN DMA pieces of 1 KB.  An output element sees the same operands in the
// same order whichever shape computes it (a 32x32x16 MFMA result depends on the element's own row and column only),
// so y does not depend on how the launch was cut.  `sub` = which 64 WN sextets of the 256-sextet tile `tile`.
//
// The k-step is software-pipelined the way the ring of conv3_bf16_big_kernel is; its three product groups play the
// role of that kernel's three taps.  For k-step g (ring stage g & 3; fragment registers ah, al, bh, bl):
//   top of g:     ah, bh of g are already in registers
//   group ah.bh   with the reads of bl, al of g between its MFMAs
//   wait for this wave's DMA pieces of g + 1, one bare s_barrier, issue the DMA pieces of g + 3
//   group ah.bl
//   group al.bh   with the reads of ah, bh of g + 1 between its MFMAs (ah is dead after the second group; bh is live,
//                 so there are two bh sets, alternated over an unroll by two: nk = Cin / 16 is even)
// The order of the products of an output element is what it was (per k-step hh, hl, lh; k ascending; points 0 .. 7).
// The ring runs on across the points; at a point's end the unscale, the parking stores and the zeroing sit between
// the third group and the next k-step's first, with that k-step's ah, bh already in registers.
//   The barrier of k-step g, B(g), orders both directions of the ring:
//   * stage (g + 3) & 3 = (g - 1) & 3 is refilled only after B(g).  Its last reads are al, bl of g - 1 (group 1 of
//     g - 1) and ah, bh of g (group 3 of g - 1); every wave has USED ah, bh of g in group 1 of g before it reaches
//     B(g), and LDS reads return in order, so all of them are complete.
//   * a wave reads stage g + 1 only after B(g), and reaches B(g) only after vmcnt says its own pieces of g + 1 landed.
//   The counted wait in front of B(g): the wave's DMA queue holds, oldest first, its pieces of g + 1 (issued in k-step
//   g - 2) and of g + 2 (issued in k-step g - 1); VMEM returns in order, so "at most n outstanding" with n = this
//   wave's pieces per stage means g + 1 has landed while g + 2 may still fly: vmcnt(n), and vmcnt(0) for the last two
//   k-steps, behind which nothing was issued.  Before the loop: three stages issued, vmcnt(2 n) lands stage 0.  The
//   parking stores and the loads of the unscale are younger than every piece in flight when they issue, so they only
//   make a counted wait stricter.
//   The two waves of a SIMD (w and w + 4) issue their pieces at different points of the k-step where the tile is the
//   full one: wm == 0 right behind the barrier, the other behind the second group.
//   The unscale keeps its own __syncthreads() (8 per tile, each drains the DMA queue once): ordering the exponent
//   table by B(g) instead needs its global loads in front of the pieces of g + 2, a k-step earlier, for 8 of 1024
//   k-steps.
//
// DMA pieces, BUF = true: buffer loads (one SGPR descriptor per operand based at the current point's slab of Wp / Vh,
// a fixed 32-bit lane offset per piece, a scalar offset that advances per k-step; the descriptors are re-based at a
// point's start) -- the launcher picks it when a point's slab of either operand is below 2 GB.  BUF = false: 64-bit
// pointers per lane, advanced per k-step.  Both land the same bytes in LDS.
#ifndef TSPN_WINO63_F16X3_STAGGER
#define TSPN_WINO63_F16X3_STAGGER 1
#endif
template <int WN, bool BUF>
__device__ __forceinline__ void wino63_f16x3_tile(
    char* smem_raw, const _Float16* __restrict__ Vh, const int* __restrict__ Ve, const int16_t* __restrict__ Wp,
    const float* __restrict__ bias, float* __restrict__ y, float* __restrict__ park, int Cin, int T, int M, int nq,
    int64_t nsext, int64_t nsp2, int tile_m, int tile_n, int tiles_n, int sub, int relu, int ldy, int vec2) {
  constexpr int MI = WN;                       // 32-row blocks of a wave: 256 rows / (8 / WN waves) / 32
  constexpr int BN = 64 * WN;                  // sextets of this tile
  constexpr int NP = 16 + 4 * WN;              // DMA pieces per stage: 16 of W, 4 WN of V
  constexpr int PW = (NP + 7) / 8;             // pieces per wave, at most
  constexpr bool EVEN = NP % 8 == 0;           // every wave issues PW pieces (else PW or PW - 1, by wave)
  constexpr bool STAGGER = TSPN_WINO63_F16X3_STAGGER && WN == 4;
  const int m0 = tile_m * F_BM;
  const int64_t S0 = (int64_t)tile_n * F_BN + sub * BN;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int li = lane & 31, kh = lane >> 5;
  const int ncg = Cin >> 3, nk = Cin >> 4;
  const int G = NJ * nk;                             // k-steps of the whole workgroup (8 points): even, >= 16

  // DMA pieces of a stage (1 KB each), numbered p: p < 16 is W: region p >> 3 (Wh, Wl), channel group (p >> 2) & 1, rows
  // 64 (p & 3) + lane; p >= 16 is V, v = p - 16: region 2 + v / (2 WN) (Vh, Vl), channel group (v / WN) & 1, sextets
  // 64 (v % WN) + lane.  Wave w issues pieces [w NP / 8, (w + 1) NP / 8).  A lane's element offset in the point's slab
  // at k-step 0 (rows < M, sextets < nsp2 always: M % 256 == 0, nsp2 % 256 == 0), and the strides per k-step / point.
  const int p0 = wave * NP / 8;
  const int npw = EVEN ? PW : (wave + 1) * NP / 8 - p0;      // wave-uniform
  const int16_t* src[PW];                                    // pointer form: the lane's source at the next k-step to issue
  unsigned voff[PW];                                         // buffer form: the lane's byte offset from that k-step's base
  int ldst[PW];                                              // byte offset of the piece in its stage
#pragma unroll
  for (int i = 0; i < PW; ++i) {
    const int p = min(p0 + i, NP - 1);
    int64_t el;
    if (p < 16) {
      const int region = p >> 3, cgi = (p >> 2) & 1, r = 64 * (p & 3) + lane;
      el = (((int64_t)region * ncg + cgi) * M + m0 + r) * 8;
      src[i] = Wp + el;
      ldst[i] = p * 1024;
    } else {
      const int v = p - 16;
      const int region = v / (2 * WN), cgi = (v / WN) & 1, r = 64 * (v % WN) + lane;
      el = (((int64_t)region * ncg + cgi) * nsp2 + S0 + r) * 8;
      src[i] = reinterpret_cast<const int16_t*>(Vh) + el;
      ldst[i] = (2 + region) * 8192 + cgi * 4096 + (v % WN) * 1024;
    }
    voff[i] = (unsigned)(el * 2);
  }
  // The next k-step to issue (wave-uniform): k-step ik of its point, into stage ist.  Buffer form: wbase / vbase are
  // that k-step's 16 channels in the point's slab of Wp / Vh, and the descriptors are made from them at the issue, so
  // the advance per k-step and the re-basing at a point's start are one scalar 64-bit add per operand.  (No range to
  // check: every row and sextet of a tile exists; the descriptor is the unbounded one, the lane offsets stay below the
  // slab's 2 GB.)
  int ik = 0, ist = 0;
  const char* wbase = reinterpret_cast<const char*>(Wp);
  const char* vbase = reinterpret_cast<const char*>(Vh);
  auto issue = [&]() {
    char* dst = smem_raw + ist * F_ST;
#pragma unroll
    for (int i = 0; i < PW; ++i)
      if (EVEN || i < npw) {
        if (BUF) bglds16(buffer_rsrc_unbounded(p0 + i < 16 ? wbase : vbase), voff[i], 0, dst + ldst[i]);   // wave-uniform choice
        else glds16(src[i], dst + ldst[i]);
      }
    ist = (ist + 1) & 3;
    // bytes to the next k-step: 16 channels on, or from a point's last k-step to the next point's first (W: over the
    // rest of the hi half, the lo half and the exponent slots; V: over the rest of the hi half and the lo half)
    const bool wrap = ++ik == nk;
    if (wrap) ik = 0;
    const int64_t dw = (int64_t)M * (wrap ? 32 * nk + 48 : 32), dv = nsp2 * (wrap ? 32 * nk + 32 : 32);
    if (BUF) {
      wbase += dw;
      vbase += dv;
    } else {
#pragma unroll
      for (int i = 0; i < PW; ++i) src[i] = reinterpret_cast<const int16_t*>(reinterpret_cast<const char*>(src[i]) + (p0 + i < 16 ? dw : dv));
    }
  };
  // all but the youngest `ahead` stages of this wave have landed (a wave's VMEM returns in order)
  auto wait_stages = [&](auto ahead_tag) {
    constexpr int AHEAD = decltype(ahead_tag)::value;
    if (EVEN || npw == PW) wait_vmcnt<AHEAD * PW>(); else wait_vmcnt<AHEAD * (PW - 1)>();
  };

  f32x16 acc[MI][2];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[mi][ni][e] = 0.f;

  // this lane's parking slots: [tile][point 0..6][32 f32x4 registers][512 lanes] (one 1 KB store per wave and register);
  // a narrower tile has 8 WN registers per point and takes the slots 8 WN sub .. of its 256-sextet tile
  float* my_park = park + (int64_t)(tile_m * tiles_n + tile_n) * (F_PARK_PER_TILE / sizeof(float)) +
                   (int64_t)sub * (8 * MI) * F_THREADS * 4 + tid * 4;
  // unscale the accumulator of point j: 2^-(e_row + e_col), exact.  The tile's 256 row and 64 WN column exponents go
  // through LDS behind the ring (one load per thread instead of 64 per lane).
  int* etab = reinterpret_cast<int*>(smem_raw + F_SMEM);        // [256 rows][256 columns]
  auto unscale = [&](int j) {
    if (tid < F_BM)
      etab[tid] = reinterpret_cast<const int*>(Wp + (int64_t)j * (2 * ncg + 1) * M * 8 + (int64_t)2 * ncg * M * 8)[(int64_t)(m0 + tid) * 4];
    else if (tid - F_BM < BN)
      etab[tid] = Ve[(int64_t)j * nsp2 + S0 + tid - F_BM];
    __syncthreads();
    int ec[2];
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) ec[ni] = etab[F_BM + wn * 64 + ni * 32 + li];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int r = etab[wm * (32 * MI) + mi * 32 + (e & 3) + 8 * (e >> 2) + 4 * kh];
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) acc[mi][ni][e] = ldexpf(acc[mi][ni][e], -(r + ec[ni]));
      }
  };

  f16x8 ah[MI], al[MI], bh[2][2], bl[2];            // bh[set]: the set of k-step g is g & 1
  const int a_off = (kh * 256 + wm * (32 * MI) + li) * 16, b_off = (kh * 256 + wn * 64 + li) * 16;
  auto read_hi = [&](int st, f16x8 (&bhn)[2]) {
    const char* s = smem_raw + st * F_ST;
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) ah[mi] = *reinterpret_cast<const f16x8*>(s + a_off + mi * 512);
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) bhn[ni] = *reinterpret_cast<const f16x8*>(s + 16384 + b_off + ni * 512);
  };
  auto read_lo = [&](int st) {                       // bl first: the second group needs it, al only the third
    const char* s = smem_raw + st * F_ST;
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) bl[ni] = *reinterpret_cast<const f16x8*>(s + 24576 + b_off + ni * 512);
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) al[mi] = *reinterpret_cast<const f16x8*>(s + 8192 + a_off + mi * 512);
  };
  auto group = [&](const f16x8 (&a)[MI], const f16x8 (&b)[2]) {
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
  };
  auto point_end = [&](int j) {
    unscale(j);
    if (j < NJ - 1) {
      // (these stores are younger than every DMA piece in flight, so the counted waits only get stricter)
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
          for (int eq = 0; eq < 4; ++eq) {
            const f32x4 v = {acc[mi][ni][4 * eq], acc[mi][ni][4 * eq + 1], acc[mi][ni][4 * eq + 2], acc[mi][ni][4 * eq + 3]};
            *reinterpret_cast<f32x4*>(my_park + ((int64_t)j * 32 + (mi * 2 + ni) * 4 + eq) * F_THREADS * 4) = v;
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[mi][ni][4 * eq + e] = 0.f;
          }
    }
    __builtin_amdgcn_sched_barrier(0);
  };
  // one k-step; STEADY: k-steps g + 1 .. g + 3 exist (no conditions inside, so the interleave hints see one block)
  auto kstep = [&](int g, f16x8 (&bc)[2], f16x8 (&bn)[2], auto steady_tag) {
    constexpr bool STEADY = decltype(steady_tag)::value;
    // n MFMAs, then r fragment reads (the full tile: 8 MFMAs and 6 reads per interleaved group)
#define TSPN_MR(NM, NR)                                \
  __builtin_amdgcn_sched_group_barrier(0x008, NM, 0);  \
  __builtin_amdgcn_sched_group_barrier(0x100, NR, 0);
    group(ah, bc);
    read_lo(g & 3);
    if (WN == 4) { TSPN_MR(1, 1) TSPN_MR(1, 1) TSPN_MR(1, 1) TSPN_MR(1, 1) TSPN_MR(1, 1) TSPN_MR(1, 1) TSPN_MR(2, 0) }
    __builtin_amdgcn_sched_barrier(0);
    if (STEADY || g + 2 < G) wait_stages(std::integral_constant<int, 1>{});   // g + 2 may still fly; g + 1 has landed
    else wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();                    // B(g): stage g + 1 landed for every wave; stage g - 1 is read out
    __builtin_amdgcn_sched_barrier(0);
    const bool more = STEADY || g + 3 < G;
    if (more && (!STAGGER || wm == 0)) issue();      // k-step g + 3 into stage (g - 1) & 3
    __builtin_amdgcn_sched_barrier(0);
    group(ah, bl);
    __builtin_amdgcn_sched_barrier(0);
    if (STAGGER && more && wm != 0) issue();
    __builtin_amdgcn_sched_barrier(0);
    group(al, bc);
    if (STEADY || g + 1 < G) read_hi((g + 1) & 3, bn);
    if (WN == 4 && STEADY) { TSPN_MR(2, 1) TSPN_MR(1, 1) TSPN_MR(1, 1) TSPN_MR(1, 1) TSPN_MR(1, 1) TSPN_MR(1, 1) TSPN_MR(1, 0) }
#undef TSPN_MR
    __builtin_amdgcn_sched_barrier(0);
  };

  issue();
  issue();
  issue();
  wait_stages(std::integral_constant<int, 2>{});
  __builtin_amdgcn_s_barrier();                      // stage 0 landed for every wave
  __builtin_amdgcn_sched_barrier(0);
  read_hi(0, bh[0]);
  int g = 0, kc = 0, jc = 0;                         // k-step, its index in its point (even here), its point
  auto pair = [&](auto steady_tag) {
    kstep(g, bh[0], bh[1], steady_tag);
    kstep(g + 1, bh[1], bh[0], steady_tag);
    g += 2;
    kc += 2;
    if (kc == nk) {                                  // nk is even: a point ends behind an odd k-step only
      point_end(jc);
      kc = 0;
      ++jc;
    }
  };
  while (g + 4 < G) pair(std::true_type{});
  while (g < G) pair(std::false_type{});

  // ---- inverse transform + bias + store: acc holds M7; M0..M6 come back from the parking area (this lane's own
  // stores, complete before they are read)
  wait_vmcnt<0>();
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const int64_t Sx = S0 + wn * 64 + ni * 32 + li;
    const bool col_ok = Sx < nsext;
    const int64_t b = col_ok ? Sx / nq : 0;
    const int q = col_ok ? (int)(Sx - b * nq) : 0;
    const int t = 6 * q;
    float* ycol = y + (b * M) * (int64_t)ldy + t;
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int eq = 0; eq < 4; ++eq) {
        f32x4 P[NJ - 1];
#pragma unroll
        for (int j = 0; j < NJ - 1; ++j)
          P[j] = *reinterpret_cast<const f32x4*>(my_park + ((int64_t)j * 32 + (mi * 2 + ni) * 4 + eq) * F_THREADS * 4);
        if (!col_ok) continue;
#pragma unroll
        for (int e4 = 0; e4 < 4; ++e4) {
          const int e = 4 * eq + e4;
          const int m = m0 + wm * (32 * MI) + mi * 32 + (e & 3) + 8 * (e >> 2) + 4 * kh;
          const float p12 = P[1][e4] + P[2][e4], m12 = P[1][e4] - P[2][e4];
          const float p34 = P[3][e4] + P[4][e4], m34 = P[3][e4] - P[4][e4];
          const float p56 = P[5][e4] + P[6][e4], m56 = P[5][e4] - P[6][e4];
          float o[6];
          o[0] = P[0][e4] + p12 + p34 + p56;
          o[1] = m12 + 2.f * m34 + 0.5f * m56;
          o[2] = p12 + 4.f * p34 + 0.25f * p56;
          o[3] = m12 + 8.f * m34 + 0.125f * m56;
          o[4] = p12 + 16.f * p34 + 0.0625f * p56;
          o[5] = m12 + 32.f * m34 + 0.03125f * m56 + acc[mi][ni][e];
          if (bias != nullptr) {
            const float bb = bias[m];
#pragma unroll
            for (int i = 0; i < 6; ++i) o[i] += bb;
          }
          if (relu) {
#pragma unroll
            for (int i = 0; i < 6; ++i) o[i] = tspn::relu_f32(o[i]);
          }
          float* dst = ycol + (int64_t)m * ldy;
          if (vec2) {
            *reinterpret_cast<f32x2*>(dst) = f32x2{o[0], o[1]};
            *reinterpret_cast<f32x2*>(dst + 2) = f32x2{o[2], o[3]};
            *reinterpret_cast<f32x2*>(dst + 4) = f32x2{o[4], o[5]};
          } else {
#pragma unroll
            for (int i = 0; i < 6; ++i)
              if (t + i < T) dst[i] = o[i];
          }
        }
      }
  }
}

// The launch.  tiles_m x tiles_n tiles of 256 x 256, numbered in groups of GM row tiles x all sextet tiles.
// `GM`: bits 0..7 the row tiles per group; bits 8..15 the tail split f (0 or 1: none); bit 16 the piece form (1 = buffer
// loads, 0 = 64-bit pointers).  With f = 2 or 4 the LAST
// R = (gridDim.x - tiles) / (f - 1) tiles of that numbering are each cut into f tiles of 256 x 256 / f (sub-tiles), so
// that the last, partly filled round of the launch keeps f times as many CUs busy:
//   blocks [0, tiles - R)       one full tile each, XCD remap over these blocks
//   blocks [tiles - R, grid)    R f sub-tiles, after every full tile in block order (the dispatcher hands them to CUs as
//                               they come free); XCD remap over these blocks, f consecutive logical ids = one tile, so
//                               the sub-tiles of a tile share an XCD (its W rows in L2) wherever the XCD's range of
//                               ids is a multiple of f -- always at R % 8 == 0 -- and at most 7 tiles straddle two
// Both remaps are bijections, so every tile and sub-tile is computed exactly once.  A sub-tile parks into its own
// share of its tile's parking area; all other arguments mean what they meant without the split.
__global__ __launch_bounds__(F_THREADS, 1) void conv3_wino63_kernel(
    const _Float16* __restrict__ Vh, const int* __restrict__ Ve, const int16_t* __restrict__ Wp,
    const float* __restrict__ bias, float* __restrict__ y, float* __restrict__ park, int Cin, int T, int M, int nq,
    int64_t nsext, int64_t nsp2, int tiles_m, int tiles_n, int relu, int ldy, int GM, int vec2) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];

  const int f = max((GM >> 8) & 0xff, 1);
  const bool buf = (GM >> 16) & 1;
  GM &= 0xff;
  const int tiles = tiles_m * tiles_n;
  const int nsplit = f > 1 ? ((int)gridDim.x - tiles) / (f - 1) : 0;     // R
  const int nfull = tiles - nsplit;
  const int bid = blockIdx.x;
  int wg, sub = 0;
  if (bid < nfull) {
    wg = xcd_remap(bid, nfull);
  } else {
    const int s = xcd_remap(bid - nfull, nsplit * f);
    wg = nfull + s / f;
    sub = s - (s / f) * f;
  }
  int tile_m, tile_n;
  grouped_tile(wg, GM, tiles_m, tiles_n, tile_m, tile_n);
  auto tile = [&](auto wn_tag, auto buf_tag) {
    wino63_f16x3_tile<decltype(wn_tag)::value, decltype(buf_tag)::value>(
        smem_raw, Vh, Ve, Wp, bias, y, park, Cin, T, M, nq, nsext, nsp2, tile_m, tile_n, tiles_n, sub, relu, ldy, vec2);
  };
  auto shape = [&](auto buf_tag) {
    if (bid < nfull) tile(std::integral_constant<int, 4>{}, buf_tag);
    else if (f == 2) tile(std::integral_constant<int, 2>{}, buf_tag);
    else tile(std::integral_constant<int, 1>{}, buf_tag);
  };
  if (buf) shape(std::true_type{}); else shape(std::false_type{});
}

int64_t padded_sextets(int64_t B, int64_t T) { return tspn::ceil_div(B * tspn::ceil_div(T, 6), SWG) * SWG; }
int64_t padded_sextets_f16x3(int64_t B, int64_t T) { return tspn::ceil_div(B * tspn::ceil_div(T, 6), F_BN) * F_BN; }

// workspace of the split form: [split V | column exponents | parking area], each 256-byte aligned
struct F16x3Layout {
  size_t v, e, park, total;
};
F16x3Layout f16x3_layout(int64_t B, int64_t T, int64_t Cin, int64_t M) {
  F16x3Layout L{};
  const size_t nsp2 = (size_t)padded_sextets_f16x3(B, T);
  L.v = 0;
  L.e = tspn::align_up((size_t)NJ * 2 * Cin * nsp2 * sizeof(_Float16), 256);
  L.park = L.e + tspn::align_up((size_t)NJ * nsp2 * sizeof(int), 256);
  L.total = L.park + (size_t)tspn::ceil_div(M, F_BM) * (nsp2 / F_BN) * F_PARK_PER_TILE;
  return L;
}

int check_common(const char* what, int64_t B, int64_t T, int64_t Cin, int64_t M, int64_t ldy) {
  TSPN_REQUIRE(B >= 0 && Cin > 0 && T > 0 && M > 0 && ldy >= T && ldy < (1 << 24), TSPN_EINVAL,
               "%s: bad sizes B=%lld T=%lld Cin=%lld M=%lld ldy=%lld", what, (long long)B, (long long)T,
               (long long)Cin, (long long)M, (long long)ldy);
  TSPN_REQUIRE(tspn::wino63_supported(Cin, M), TSPN_EUNSUPPORTED,
               "%s: needs Cin %% 32 == 0, M %% 32 == 0 (Cin=%lld M=%lld)", what, (long long)Cin, (long long)M);
  TSPN_REQUIRE(Cin < (1 << 24) && T < (1 << 24) && M < (1 << 24), TSPN_EUNSUPPORTED, "%s: dimension too large", what);
  return TSPN_OK;
}

}  // namespace

bool tspn::wino63_supported(int64_t Cin, int64_t M) { return Cin > 0 && M > 0 && Cin % 32 == 0 && M % 32 == 0; }

size_t tspn::wino63_workspace_bytes(int64_t B, int64_t T, int64_t Cin) {
  if (B <= 0 || T <= 0 || Cin <= 0 || Cin % 32 != 0) return 0;     // Cin % 32 != 0: refused by the entries
  return (size_t)(Cin / 4) * NJ * (size_t)padded_sextets(B, T) * 4 * sizeof(float);
}

extern "C" size_t tspn_conv3_tc_wino63_workspace_bytes(int64_t B, int64_t T, int64_t Cin) {
  return tspn::wino63_workspace_bytes(B, T, Cin);
}

extern "C" int tspn_pack_conv3_wino63_frag_f32(const float* W, int64_t M, int64_t Cin, int64_t split, float* frag,
                                               void* stream) {
  TSPN_REQUIRE(W && frag, TSPN_EINVAL, "tspn_pack_conv3_wino63_frag_f32: null pointer");
  TSPN_REQUIRE(M > 0 && Cin > 0 && split >= 0, TSPN_EINVAL, "tspn_pack_conv3_wino63_frag_f32: bad sizes");
  TSPN_REQUIRE(split == 0 || Cin == 2 * split, TSPN_EINVAL,
               "tspn_pack_conv3_wino63_frag_f32: split=%lld requires Cin == 2*split (Cin=%lld)", (long long)split,
               (long long)Cin);
  const int64_t Mp = split ? 2 * M : M, Cp = split ? split : Cin;
  TSPN_REQUIRE(Cp % KC == 0 && Mp % 32 == 0, TSPN_EUNSUPPORTED,
               "tspn_pack_conv3_wino63_frag_f32: needs (packed) Cin %% 8 == 0 and M %% 32 == 0 (Cin=%lld M=%lld)",
               (long long)Cp, (long long)Mp);
  const int64_t total = NJ * Cp * Mp;
  const int blocks = (int)std::min<int64_t>(tspn::ceil_div(total, 256), 8192);
  hipLaunchKernelGGL(pack_wino63_frag_kernel, dim3(blocks), dim3(256), 0, TSPN_STREAM(stream), W, M, Cin, split, frag);
  return tspn::check_launch("tspn_pack_conv3_wino63_frag_f32");
}

// step 1: V = B^T d of x [B, T, Cin] into `workspace` (HBM-bound)
int tspn::wino63_input_transform(const float* x, int64_t B, int64_t T, int64_t Cin, void* workspace,
                                 size_t workspace_bytes, void* stream, uint64_t* hot) {
  const char* what = "tspn_conv3_tc_wino63_f32(input transform)";
  if (int rc = check_common(what, B, T, Cin, 32, T)) return rc;
  if (B == 0) return TSPN_OK;
  TSPN_REQUIRE(x && tspn::aligned16(x), TSPN_EINVAL, "%s: x must be a 16-byte aligned pointer", what);
  const size_t need = tspn::wino63_workspace_bytes(B, T, Cin);
  TSPN_REQUIRE(workspace && workspace_bytes >= need, TSPN_EWORKSPACE, "%s: workspace %zu < %zu bytes", what,
               workspace_bytes, need);
  TSPN_REQUIRE(tspn::aligned16(workspace), TSPN_EINVAL, "%s: workspace must be 16-byte aligned",
               what);
  const int64_t nq = tspn::ceil_div(T, 6);
  const int64_t nsext = B * nq, nsp = padded_sextets(B, T);
  TSPN_REQUIRE(nsp / 32 < (1LL << 31) && Cin / 32 < 65536, TSPN_EUNSUPPORTED, "%s: grid too large", what);
  hipLaunchKernelGGL(wino63_input_transform_kernel, dim3((unsigned)(nsp / 32), (unsigned)(Cin / 32)), dim3(256), 0,
                     TSPN_STREAM(stream), x, static_cast<float*>(workspace), (int)T, (int)Cin, (int)nq, nsext, nsp,
                     B * T, reinterpret_cast<unsigned long long*>(hot));
  return tspn::check_launch(what);
}

// 0 = buffer-load pieces where the operands allow (default), 1 = 64-bit pointer pieces everywhere; governs the fp32
// contraction (its V pieces) and the split-fp16 one (all of its pieces)
static std::atomic<int> g_piece_form{0};

// step 2: the MFMA kernel on the transformed input
int tspn::wino63_contract(const void* workspace, int64_t B, int64_t T, int64_t Cin, const float* frag, int64_t M,
                          const float* bias, int relu, float* y, int64_t ldy, void* stream) {
  const char* what = "tspn_conv3_tc_wino63_f32";
  if (int rc = check_common(what, B, T, Cin, M, ldy)) return rc;
  if (B == 0) return TSPN_OK;
  TSPN_REQUIRE(workspace && frag && y, TSPN_EINVAL, "%s: null pointer", what);
  TSPN_REQUIRE(tspn::aligned16(frag) && (reinterpret_cast<uintptr_t>(y) & 3) == 0,
               TSPN_EUNSUPPORTED, "%s: frag must be 16-byte aligned", what);
  const int64_t nq = tspn::ceil_div(T, 6);
  const int64_t nsext = B * nq, nsp = padded_sextets(B, T);
  const int64_t tiles_m = tspn::ceil_div(M, BM), tiles_n = nsp / SWG;
  TSPN_REQUIRE(tiles_m * tiles_n < (1LL << 31), TSPN_EUNSUPPORTED, "%s: grid too large", what);
  const int vec2 = (ldy % 2 == 0) && (ldy >= 6 * nq) && ((reinterpret_cast<uintptr_t>(y) & 7) == 0);
  // buffer-load form of the V pieces where every byte offset into the workspace fits 32 bits
#ifndef TSPN_WINO63_BUFV
#define TSPN_WINO63_BUFV 1
#endif
  // (tspn_conv3_tc_wino63_set_piece_form(1) forces the pointer form: tests compare the two)
  const bool bufv = TSPN_WINO63_BUFV && tspn::wino63_workspace_bytes(B, T, Cin) < (1ull << 32) &&   /* offsets are unsigned 32-bit */
                    g_piece_form.load(std::memory_order_relaxed) == 0;
  static tspn::LdsLimit lds[2];   // 128 KB of dynamic LDS: above the 64 KB default limit
  auto launch = [&](auto kern, tspn::LdsLimit& lim) {
    if (int rc = lim.ensure(reinterpret_cast<const void*>(kern), SMEM_BYTES, what)) return rc;
    hipLaunchKernelGGL(kern, dim3((unsigned)(tiles_m * tiles_n)), dim3(THREADS), SMEM_BYTES, TSPN_STREAM(stream),
                       static_cast<const float*>(workspace), frag, bias, y, (int)Cin, (int)T, (int)M, (int)nq, nsext, nsp,
                       (int)tiles_m, (int)tiles_n, relu, (int)ldy, TSPN_WINO63_GM, vec2);
    return tspn::check_launch(what);
  };
  return bufv ? launch(conv3_wino63_kernel<true>, lds[1]) : launch(conv3_wino63_kernel<false>, lds[0]);
}

int tspn::conv3_tc_wino63(const float* x, int64_t B, int64_t T, int64_t Cin, const float* frag, int64_t M,
                          const float* bias, int relu, float* y, int64_t ldy, void* workspace,
                          size_t workspace_bytes, void* stream) {
  if (int rc = check_common("tspn_conv3_tc_wino63_f32", B, T, Cin, M, ldy)) return rc;
  if (int rc = tspn::wino63_input_transform(x, B, T, Cin, workspace, workspace_bytes, stream)) return rc;
  return tspn::wino63_contract(workspace, B, T, Cin, frag, M, bias, relu, y, ldy, stream);
}

extern "C" int tspn_conv3_tc_wino63_set_piece_form(int form) {
  TSPN_REQUIRE(form == 0 || form == 1, TSPN_EINVAL, "tspn_conv3_tc_wino63_set_piece_form: form must be 0 or 1");
  return g_piece_form.exchange(form, std::memory_order_relaxed);
}

extern "C" int tspn_conv3_tc_wino63_f32(const float* x, int64_t B, int64_t T, int64_t Cin, const float* frag,
                                        int64_t M, const float* bias, int relu, float* y, void* workspace,
                                        size_t workspace_bytes, void* stream) {
  return tspn::conv3_tc_wino63(x, B, T, Cin, frag, M, bias, relu, y, T, workspace, workspace_bytes, stream);
}

// ---------------------------------------------------------------------------------------------------------------
// Split-fp16 form (TSPN_CONV_WINOGRAD63_F16X3)
bool tspn::wino63_f16x3_supported(int64_t Cin, int64_t M) {
  return Cin > 0 && M > 0 && Cin % 32 == 0 && M % F_BM == 0 && Cin < (1 << 24) && M < (1 << 24);
}

size_t tspn::wino63_f16x3_workspace_bytes(int64_t B, int64_t T, int64_t Cin, int64_t M) {
  if (B <= 0 || T <= 0 || !tspn::wino63_f16x3_supported(Cin, M)) return 0;     // what the entries refuse
  return f16x3_layout(B, T, Cin, M).total;
}

extern "C" size_t tspn_conv3_tc_wino63_f16x3_workspace_bytes(int64_t B, int64_t T, int64_t Cin, int64_t M) {
  return tspn::wino63_f16x3_workspace_bytes(B, T, Cin, M);
}

extern "C" size_t tspn_pack_conv3_wino63_f16x3_elements(int64_t M, int64_t Cin, int64_t split) {
  if (M <= 0 || Cin <= 0 || split < 0 || (split && Cin != 2 * split)) return 0;
  const int64_t Mp = split ? 2 * M : M, Cp = split ? split : Cin;
  return (size_t)NJ * (2 * (Cp / 8) + 1) * Mp * 8;
}

extern "C" int tspn_pack_conv3_wino63_f16x3(const float* W, int64_t M, int64_t Cin, int64_t split, int16_t* packed,
                                            void* stream) {
  const char* what = "tspn_pack_conv3_wino63_f16x3";
  TSPN_REQUIRE(W && packed, TSPN_EINVAL, "%s: null pointer", what);
  TSPN_REQUIRE(M > 0 && Cin > 0 && split >= 0, TSPN_EINVAL, "%s: bad sizes", what);
  TSPN_REQUIRE(split == 0 || Cin == 2 * split, TSPN_EINVAL, "%s: split=%lld requires Cin == 2*split (Cin=%lld)", what,
               (long long)split, (long long)Cin);
  TSPN_REQUIRE(tspn::aligned16(packed), TSPN_EINVAL, "%s: packed must be 16-byte aligned", what);
  const int64_t Mp = split ? 2 * M : M, Cp = split ? split : Cin;
  TSPN_REQUIRE(tspn::wino63_f16x3_supported(Cp, Mp), TSPN_EUNSUPPORTED,
               "%s: needs (packed) Cin %% 32 == 0 and M %% 256 == 0 (Cin=%lld M=%lld)", what, (long long)Cp, (long long)Mp);
  void (*kern)(const float*, int64_t, int64_t, int64_t, int16_t*) = pack_wino63_frag_kernel;
  hipLaunchKernelGGL(kern, dim3((unsigned)tspn::ceil_div(NJ * Mp, 256)), dim3(256), 0, TSPN_STREAM(stream), W, M, Cin,
                     split, packed);
  return tspn::check_launch(what);
}

// step 1 of the split form: V = B^T d, split and scaled, into the workspace (+ the guard's hot-sextet report)
int tspn::wino63_f16x3_input_transform(const float* x, int64_t B, int64_t T, int64_t Cin, int64_t M, void* workspace,
                                       size_t workspace_bytes, void* stream, uint64_t* hot, bool fused_in, float* fbar,
                                       int stages) {
  const char* what = "tspn_conv3_tc_wino63_f16x3(input transform)";
  if (int rc = check_common(what, B, T, Cin, 32, T)) return rc;
  TSPN_REQUIRE(tspn::wino63_f16x3_supported(Cin, M), TSPN_EUNSUPPORTED,
               "%s: needs Cin %% 32 == 0 and M %% 256 == 0 (Cin=%lld M=%lld)", what, (long long)Cin, (long long)M);
  if (B == 0) return TSPN_OK;
  TSPN_REQUIRE(x && tspn::aligned16(x), TSPN_EINVAL, "%s: x must be a 16-byte aligned pointer", what);
  const F16x3Layout L = f16x3_layout(B, T, Cin, M);
  TSPN_REQUIRE(workspace && workspace_bytes >= L.total, TSPN_EWORKSPACE, "%s: workspace %zu < %zu bytes", what,
               workspace_bytes, L.total);
  TSPN_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, TSPN_EINVAL, "%s: workspace must be 256-byte aligned",
               what);
  const int64_t nq = tspn::ceil_div(T, 6);
  const int64_t nsext = B * nq, nsp2 = padded_sextets_f16x3(B, T);
  TSPN_REQUIRE(nsp2 / 8 < (1LL << 31), TSPN_EUNSUPPORTED, "%s: grid too large", what);
  char* ws = static_cast<char*>(workspace);
  if (fused_in)
    return tspn::input_f16x3(x, B, T, Cin, nsp2, reinterpret_cast<_Float16*>(ws + L.v), reinterpret_cast<int*>(ws + L.e), fbar,
                             hot, stream, stages);
  void (*kern)(const float*, _Float16*, int*, int, int, int, int64_t, int64_t, int64_t, unsigned long long*) =
      wino63_input_transform_kernel;
  hipLaunchKernelGGL(kern, dim3((unsigned)(nsp2 / 8)), dim3(256), 0, TSPN_STREAM(stream), x,
                     reinterpret_cast<_Float16*>(ws + L.v), reinterpret_cast<int*>(ws + L.e), (int)T, (int)Cin, (int)nq,
                     nsext, nsp2, B * T, reinterpret_cast<unsigned long long*>(hot));
  return tspn::check_launch(what);
}

// 1 = cut the tiles of the last, partly filled round of the split contraction into sub-tiles (default), 0 = whole tiles only
static std::atomic<int> g_tail_split{1};

extern "C" int tspn_conv3_tc_wino63_f16x3_set_tail_split(int on) {
  TSPN_REQUIRE(on == 0 || on == 1, TSPN_EINVAL, "tspn_conv3_tc_wino63_f16x3_set_tail_split: on must be 0 or 1");
  return g_tail_split.exchange(on, std::memory_order_relaxed);
}

// CUs of the current device (0 if unknown), asked once per device ordinal
static int device_cus() {
  constexpr int kMaxDevices = 64;
  static std::atomic<int> cached[kMaxDevices] = {};
  int dev = -1, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  const bool tracked = dev >= 0 && dev < kMaxDevices;
  if (tracked && (cus = cached[dev].load(std::memory_order_relaxed)) > 0) return cus;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) return 0;
  if (tracked) cached[dev].store(cus, std::memory_order_relaxed);
  return cus;
}

// ---- which input kernels run ahead of the split contraction
// The fused form (inputf16/tspn_input_f16x3.hip) takes the column maxima and the temporal mean in ONE pass over x, one
// workgroup of Cin / 4 threads per tracklet, and splits in a second; the two-pass kernel above is one workgroup per 8
// sextets, whatever Cin, and leaves the mean to a third pass (tspn_temporal_mean_f32).  The fused form is taken where its
// scan workgroups are large enough to keep a CU's loads in flight (Cin >= 1024: four waves) and numerous enough to fill the
// chip: at least one tracklet per TWO CUs (profiles/r31/README.md has the measured crossover).  A pure function of
// (NT, T, Cin, CUs); 1 = fused.
extern "C" int tspn_conv3_tc_wino63_f16x3_input_form(int64_t NT, int64_t T, int64_t Cin, int cus) {
  if (NT <= 0 || cus <= 0 || !tspn::input_f16x3_supported(T, Cin)) return 0;
  return Cin >= 1024 && 2 * NT >= cus;
}

// 0 = by tspn_conv3_tc_wino63_f16x3_input_form (default), 1 = the two-pass transform (and the mean kernel) everywhere,
// 2 = the fused kernels wherever they support the shape
static std::atomic<int> g_input_form{0};

extern "C" int tspn_conv3_tc_wino63_f16x3_set_input_form(int form) {
  TSPN_REQUIRE(form >= 0 && form <= 2, TSPN_EINVAL, "tspn_conv3_tc_wino63_f16x3_set_input_form: form must be 0, 1 or 2");
  return g_input_form.exchange(form, std::memory_order_relaxed);
}

bool tspn::wino63_f16x3_fused_input(int64_t B, int64_t T, int64_t Cin) {
  const int form = g_input_form.load(std::memory_order_relaxed);
  if (form == 1 || B <= 0) return false;
  if (form == 2) return tspn::input_f16x3_supported(T, Cin);
  return tspn_conv3_tc_wino63_f16x3_input_form(B, T, Cin, device_cus()) != 0;
}

// The tail split of a launch of `tiles` workgroups (one per CU at a time): R = tiles % CUs tiles are left for the last
// round; when they fill at most half of the CUs, each is cut into f = min(4, CUs / R) sub-tiles.  Returns f (1: no split).
static int tail_split_factor(int64_t tiles, int cus, int64_t* R) {
  *R = 0;
  if (cus <= 0 || g_tail_split.load(std::memory_order_relaxed) == 0) return 1;
  const int64_t r = tiles % cus;
  if (r == 0) return 1;
  const int64_t f = std::min<int64_t>(4, cus / r);
  if (f < 2) return 1;
  *R = r;
  return f == 3 ? 2 : (int)f;     // the kernel has the shapes 256 / 2 and 256 / 4
}

// step 2 of the split form: the f16 MFMA contraction + inverse transform
int tspn::wino63_f16x3_contract(void* workspace, size_t workspace_bytes, int64_t B, int64_t T, int64_t Cin,
                                const int16_t* packed, int64_t M, const float* bias, int relu, float* y, int64_t ldy,
                                void* stream) {
  const char* what = "tspn_conv3_tc_wino63_f16x3";
  if (int rc = check_common(what, B, T, Cin, M, ldy)) return rc;
  TSPN_REQUIRE(tspn::wino63_f16x3_supported(Cin, M), TSPN_EUNSUPPORTED,
               "%s: needs Cin %% 32 == 0 and M %% 256 == 0 (Cin=%lld M=%lld)", what, (long long)Cin, (long long)M);
  if (B == 0) return TSPN_OK;
  TSPN_REQUIRE(workspace && packed && y, TSPN_EINVAL, "%s: null pointer", what);
  TSPN_REQUIRE(tspn::aligned16(packed) && (reinterpret_cast<uintptr_t>(y) & 3) == 0,
               TSPN_EUNSUPPORTED, "%s: packed weights must be 16-byte aligned", what);
  const F16x3Layout L = f16x3_layout(B, T, Cin, M);
  TSPN_REQUIRE(workspace_bytes >= L.total, TSPN_EWORKSPACE, "%s: workspace %zu < %zu bytes", what, workspace_bytes,
               L.total);
  const int64_t nq = tspn::ceil_div(T, 6);
  const int64_t nsext = B * nq, nsp2 = padded_sextets_f16x3(B, T);
  const int64_t tiles_m = M / F_BM, tiles_n = nsp2 / F_BN;
  TSPN_REQUIRE(tiles_m * tiles_n < (1LL << 29), TSPN_EUNSUPPORTED, "%s: grid too large", what);
  const int vec2 = (ldy % 2 == 0) && (ldy >= 6 * nq) && ((reinterpret_cast<uintptr_t>(y) & 7) == 0);
  // the last round: R tiles as R f sub-tiles behind the full ones (see the kernel)
  int64_t R = 0;
  const int f = tail_split_factor(tiles_m * tiles_n, device_cus(), &R);
  const int64_t grid = tiles_m * tiles_n + R * (f - 1);
  // buffer-load pieces where the hi + lo halves of one point's slab, of the weights and of the split input, stay below
  // 2 GB (a descriptor per operand and point, 32-bit offsets inside it); tspn_conv3_tc_wino63_set_piece_form(1)
  // forces the pointer form
  const int64_t slab = 4 * Cin * std::max<int64_t>(M, nsp2);
  const int buf = slab < (1LL << 31) && g_piece_form.load(std::memory_order_relaxed) == 0;
  char* ws = static_cast<char*>(workspace);
  static tspn::LdsLimit lds;     // 128 KB of dynamic LDS
  void (*kern)(const _Float16*, const int*, const int16_t*, const float*, float*, float*, int, int, int, int, int64_t,
               int64_t, int, int, int, int, int, int) = conv3_wino63_kernel;
  if (int rc = lds.ensure(reinterpret_cast<const void*>(kern), F_SMEM_ALL, what)) return rc;
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(F_THREADS), F_SMEM_ALL, TSPN_STREAM(stream),
                     reinterpret_cast<const _Float16*>(ws + L.v), reinterpret_cast<const int*>(ws + L.e), packed, bias, y,
                     reinterpret_cast<float*>(ws + L.park), (int)Cin, (int)T, (int)M, (int)nq, nsext, nsp2, (int)tiles_m,
                     (int)tiles_n, relu, (int)ldy, TSPN_WINO63_GM | (f << 8) | (buf << 16), vec2);
  return tspn::check_launch(what);
}

extern "C" int tspn_conv3_tc_wino63_f16x3(const float* x, int64_t B, int64_t T, int64_t Cin, const int16_t* packed,
                                          int64_t M, const float* bias, int relu, float* y, void* workspace,
                                          size_t workspace_bytes, void* stream) {
  // every refusal of the contraction before the transform is launched: a refused call launches nothing
  const char* what = "tspn_conv3_tc_wino63_f16x3";
  if (int rc = check_common(what, B, T, Cin, M, T)) return rc;
  TSPN_REQUIRE(tspn::wino63_f16x3_supported(Cin, M), TSPN_EUNSUPPORTED,
               "%s: needs Cin %% 32 == 0 and M %% 256 == 0 (Cin=%lld M=%lld)", what, (long long)Cin, (long long)M);
  if (B > 0) {
    TSPN_REQUIRE(workspace && packed && y, TSPN_EINVAL, "%s: null pointer", what);
    TSPN_REQUIRE(tspn::aligned16(packed) && (reinterpret_cast<uintptr_t>(y) & 3) == 0,
                 TSPN_EUNSUPPORTED, "%s: packed weights must be 16-byte aligned", what);
  }
  if (int rc = tspn::wino63_f16x3_input_transform(x, B, T, Cin, M, workspace, workspace_bytes, stream, nullptr,
                                                  tspn::wino63_f16x3_fused_input(B, T, Cin)))
    return rc;
  return tspn::wino63_f16x3_contract(workspace, workspace_bytes, B, T, Cin, packed, M, bias, relu, y, T, stream);
}

// The input side alone (tests, A/B timing): split input + column exponents into the head of `split_input`, a buffer of the
// conv entry's size and layout, the temporal mean into `fbar` [B, Cin] (may be null), the hot-sextet keys into `hot_slots`
// (TSPN_CONV_CHECK_HOT_SLOTS slots 256 bytes apart, zeroed by the caller; may be null).  Runs the kernels the conv entry and
// the fused pass would run for the shape (tspn_conv3_tc_wino63_f16x3_set_input_form).
extern "C" int tspn_conv3_tc_wino63_f16x3_input(const float* x, int64_t B, int64_t T, int64_t Cin, int64_t M, void* split_input,
                                                size_t split_input_bytes, float* fbar, uint64_t* hot_slots, void* stream) {
  const char* what = "tspn_conv3_tc_wino63_f16x3_input";
  if (int rc = check_common(what, B, T, Cin, 32, T)) return rc;
  const bool fused_in = tspn::wino63_f16x3_fused_input(B, T, Cin);
  if (int rc = tspn::wino63_f16x3_input_transform(x, B, T, Cin, M, split_input, split_input_bytes, stream, hot_slots, fused_in, fbar))
    return rc;
  if (fbar != nullptr && !fused_in) return tspn_temporal_mean_f32(x, B, T, Cin, 1, fbar, stream);
  return TSPN_OK;
}
