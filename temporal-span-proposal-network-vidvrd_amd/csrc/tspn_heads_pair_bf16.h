// The bf16 pair stage's tile: staging, k-loop and epilogue walk of ONE workgroup tile (2 NW subject slots x OB object
// slots x 16 frames), shared by heads_pairgrid_bf16_kernel (tspn_bf16.hip: slot = tracklet, the canonical pair table)
// and heads_pairlist_bf16_kernel (pairlist/tspn_pairlist_bf16.hip: slot = rank in a video's subject / object list, an
// arbitrary pair table).  The two differ only in the slot -> tracklet map of the staged rows (`row_trk`) and in what
// is done with a finished (subject slot, object slot) accumulator (`emit`); channel order, fragment positions and the
// single accumulator per slot pair are the same, so the same (s, o) gives the same bits in both.
// Everything is force-inlined into its kernel (-fno-gpu-rdc: no device symbols across translation units).
#pragma once
#include "tspn_common.h"
#include "tspn_device.h"

namespace tspn_dev {

constexpr int HP_FB = 16;
constexpr int HP_KC = 32;
constexpr int HP_ROW = HP_FB * HP_KC * 4;  // 2048 B

__device__ __forceinline__ unsigned relu_pack(float a, float b) {
  // ReLU in fp32 with the NaN-propagating maximum (F.relu(NaN) = NaN; -0 -> +0; two v_maximum3_f32), then one rounding to
  // bf16.  The packed int16 maximum on the bf16 pair this replaces zeroed a NaN whose sign bit is set (a negative int16).
  const f32x2 s = {tspn::relu_f32(a), tspn::relu_f32(b)};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(s, bf16x2));
}

// bytes of dynamic LDS of a tile with 2 NW + OB = 4 NW staged rows: two stages of rows + the k-step's head weights
constexpr size_t heads_pair_tile_lds(int rows) { return 2 * ((size_t)rows * HP_ROW + 1024); }

// NW waves; tile = 2 NW subject slots x OB object slots x 16 frames (frames t0 ..), wave w owns SW subject slots.
// <4, 8>: 8 x 8 pairs, 32 KB per stage, 2 workgroups/CU (small N).  <8, 16>: 16 x 16 pairs, 64 KB per
// stage, 1 workgroup/CU -- half the bytes streamed from L2 per activation, which is what bounds the
// kernel (ablation at the config-3 shape, 8 x 8: 4.5 ms, without the DMA stream 2.2, without the
// VALU work still 4.5).
// `Map` holds the two places where the kernels differ, as static functions of a small context `Ctx` that travels by
// value (plain scalars in registers: nothing for the optimiser to look through):
//   Map::row_trk(ctx, r)  tracklet (local to video b, inside [0, N)) of staged row r: r < 2 NW a subject slot (U half
//               of y), else object slot r - 2 NW (V half)
//   Map::emit(ctx, s_slot, o_slot, t, hg, acc, bias)   lane (frame t = t0 + lane % 16, head group hg = lane / 16) holds
//               heads 4 hg .. 4 hg + 3 of frame t of the tile's slot pair (s_slot, o_slot) in `acc`, their biases in
//               `bias`; called for every slot pair the wave owns, compile-time unrolled, t may be >= T
template <int NW, int OB, int SW, class Map, class Ctx>
__device__ __forceinline__ void heads_pair_tile_bf16(const float* __restrict__ y, int64_t ldm, int b, int N,
                                                     int C, int T, const __bf16* __restrict__ Whp,
                                                     const float* __restrict__ bh, int H, int t0, const Ctx ctx) {
  constexpr int SBLK = 2 * NW;
  constexpr int WS = SBLK / SW, WO = NW / WS, OW = OB / WO;   // waves along subjects / objects, objects per wave
  static_assert(WS * WO == NW && OW * WO == OB, "wave tiling");
  constexpr int ROWS = SBLK + OB;
  constexpr int ST = ROWS * HP_ROW + 1024;  // + the k-step's slice of the head weights (one piece)
  static_assert(ROWS == 4 * NW, "each wave stages 4 rows");
  extern __shared__ __attribute__((aligned(16))) char smem[];   // heads_pair_tile_lds(ROWS) bytes, the kernel's only LDS

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int f = lane & 15, kg = lane >> 4;
  const int ws = wave % WS, wo = wave / WS;      // this wave's subject slots SW ws .., object slots OW wo ..

  // DMA sources: wave w stages rows 4w .. 4w+3 (2 pieces each); row r < SBLK: subject slot r
  // (U half, channels [0,C)), else object slot r - SBLK (V half, channels [C,2C))
  // LDS image of a row: two pieces of 8 frames; inside a piece position = 16 X + slot with
  //   slot = (f & 7) + 8 ((q >> 1) & 1),  X = 2 (q >> 2) + (q & 1)      (q = 16-byte channel quad 0..7)
  // so that (a) one DMA piece fetches 8 complete 128-byte lines of y (8 frames x 32 channels) and
  // (b) the fragment read of lane (f, kg) for quad 2 kg + r sits at slot (f & 7) + 8 (kg & 1): the
  // four 16-lane groups of a ds_read_b128 each cover all 16 slots -- conflict-free.
  // (buffer loads: descriptor = this video's rows of y, a fixed 32-bit lane offset per piece, one scalar offset that
  // advances 128 bytes per k-step -- cheaper to issue beside MFMAs than global_load_lds with eight 64-bit pointers per
  // lane, and eight registers and sixteen vector adds per k-step less; tools/probes/lds_dma_issue_probe.hip)
  const __amdgpu_buffer_rsrc_t rsrc_y = buffer_rsrc(y + (int64_t)b * N * T * ldm, (int)(unsigned)((int64_t)N * T * ldm * 4));
  unsigned voff[8];
  {
    const int fq = lane & 7;
    const int q = (lane >> 5) * 4 + ((lane >> 3) & 1) * 2 + ((lane >> 4) & 1);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int r = wave * 4 + (i >> 1), j = i & 1;
      const int trk = Map::row_trk(ctx, r);
      const int t = min(t0 + 8 * j + fq, T - 1);
      voff[i] = (unsigned)((((int64_t)trk * T + t) * ldm + (r < SBLK ? 0 : C) + 4 * q) * 4);
    }
  }
  const __amdgpu_buffer_rsrc_t rsrc_w = buffer_rsrc(Whp, C * 32);
  int y_soff = 0, w_soff = 0;
  auto stage = [&](int buf) {
    char* dst = smem + buf * ST + wave * 4 * HP_ROW;
#pragma unroll
    for (int i = 0; i < 8; ++i)
      bglds16(rsrc_y, voff[i], y_soff, dst + i * 1024);
    y_soff += HP_KC * 4;
    // head weights of the k-step, [4 kg][16 h][8 ch] bf16 = the packed layout itself; staged through
    // LDS as well so that no register-returning global load (whose wait the compiler would place at the
    // top of the loop, serialising the whole DMA queue with the compute) is left in the loop
    if (wave == 0) {
      bglds16(rsrc_w, lane * 16, w_soff, smem + buf * ST + ROWS * HP_ROW);
      w_soff += 1024;
    }
  };

  f32x4 acc[SW][OW];
#pragma unroll
  for (int s = 0; s < SW; ++s)
#pragma unroll
    for (int o = 0; o < OW; ++o) acc[s][o] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = C / HP_KC;
  // fragment of lane (f, kg): quads 2 kg (here) and 2 kg + 1 (256 bytes further)
  const int frag_off = (64 * (f >> 3) + 32 * (kg >> 1) + 8 * (kg & 1) + (f & 7)) * 16;
  stage(0);
  __builtin_amdgcn_s_waitcnt(0x0070);                 // vmcnt(0) lgkmcnt(0)
  __builtin_amdgcn_s_barrier();

  for (int k = 0; k < nk; ++k) {
    const int buf = k & 1;
    if (k + 1 < nk) stage(buf ^ 1);
    __builtin_amdgcn_sched_barrier(0);
    const bf16x8 wfrag = *reinterpret_cast<const bf16x8*>(smem + buf * ST + ROWS * HP_ROW + lane * 16);
    const char* base = smem + buf * ST + frag_off;
    f32x4 u[SW][2];
#pragma unroll
    for (int s = 0; s < SW; ++s) {
      u[s][0] = *reinterpret_cast<const f32x4*>(base + (SW * ws + s) * HP_ROW);
      u[s][1] = *reinterpret_cast<const f32x4*>(base + (SW * ws + s) * HP_ROW + 256);
    }
    // V fragments are read two objects ahead of their use (LDS latency off the critical path).  The
    // reads and their counted waits are written out: left to itself the compiler issues every
    // fragment read right before its first use and waits for it at once (32 exposed LDS round trips
    // per k-step).  LDS returns in order, so "lgkmcnt(n)" = all but the newest n reads have landed.
    const unsigned vaddr = (unsigned)(size_t)(__attribute__((address_space(3))) const char*)(base + (SBLK + OW * wo) * HP_ROW);
    f32x4 vq[3][2];
#define TSPN_VREAD(slot, o)                                                                             \
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(vq[slot][0]) : "v"(vaddr), "n"((o) * HP_ROW)); \
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(vq[slot][1]) : "v"(vaddr), "n"((o) * HP_ROW + 256));
    TSPN_VREAD(0, 0)
    TSPN_VREAD(1, 1)
#pragma unroll
    for (int o = 0; o < OW; ++o) {
      if (o + 2 < OW) {
        TSPN_VREAD((o + 2) % 3, o + 2)
        asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(vq[o % 3][0]), "+v"(vq[o % 3][1]));
      } else if (o + 1 < OW) {
        asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(vq[o % 3][0]), "+v"(vq[o % 3][1]));
      } else {
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(vq[o % 3][0]), "+v"(vq[o % 3][1]));
      }
      const f32x4 v0 = vq[o % 3][0], v1 = vq[o % 3][1];
#pragma unroll
      for (int s = 0; s < SW; ++s) {
        const f32x4 a0 = u[s][0] + v0, a1 = u[s][1] + v1;
        u32x4 pk = {relu_pack(a0[0], a0[1]), relu_pack(a0[2], a0[3]), relu_pack(a1[0], a1[1]),
                    relu_pack(a1[2], a1[3])};
        acc[s][o] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wfrag, __builtin_bit_cast(bf16x8, pk),
                                                             acc[s][o], 0, 0, 0);
      }
    }
#undef TSPN_VREAD
    __builtin_amdgcn_s_waitcnt(0x0070);               // vmcnt(0) lgkmcnt(0): the next k-step is in LDS
    __builtin_amdgcn_s_barrier();
  }

  // epilogue: lane = (frame f, head group hg): heads 4 hg .. 4 hg + 3
  const int t = t0 + f;
  const int hg = lane >> 4;
  float bias[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) bias[r] = (4 * hg + r < H) ? bh[4 * hg + r] : 0.f;
#pragma unroll
  for (int s = 0; s < SW; ++s) {
#pragma unroll
    for (int o = 0; o < OW; ++o)
      Map::emit(ctx, SW * ws + s, OW * wo + o, t, hg, acc[s][o], f32x4{bias[0], bias[1], bias[2], bias[3]});
  }
}

}  // namespace tspn_dev
