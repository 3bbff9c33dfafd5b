// Pair-list stage of the bf16-operand path: the pair stage of tspn_bf16.hip for an ARBITRARY [P,2] pair table
// (a proposal filter's subset, a PPN top-k, training samples with repeated rows) at the cost of the tiles the
// table touches.
//
// The grid kernel gets its speed from 16 U rows and 16 V rows serving 256 pairs; a list form keeps that reuse by
// scoring, per video, the grid (distinct subjects that occur) x (distinct objects that occur) and handing each
// finished slot pair to every table row that names it:
//   pair_plan_lists_kernel   per video: the ascending lists of the subjects / objects that occur, their counts and
//                            the tracklet -> rank maps;
//   pair_plan_link_kernel    one pass over the table: next[p] = atomicExch(&head[b][rank s][rank o], p) -- a chain per
//                            slot pair through every row that names it (duplicates included), in no particular order;
//   heads_pairlist_bf16_kernel  the tile of tspn_heads_pair_bf16.h on the compacted slots: a workgroup whose tile has no
//                            chain returns at once; the epilogue walks each slot pair's chain and stores its 16 heads x
//                            16 frames to every row on it.
// A row whose ids lie outside [0, B N) or in two different videos is on no chain: nothing is read or written for it and
// its output row is left as it was.
#include <algorithm>
#include <cstdlib>

#include "tspn_common.h"
#include "tspn_device.h"
#include "tspn_heads_pair_bf16.h"

namespace {

using namespace tspn_dev;

constexpr int PL_MAX_N = 2048;       // a video's presence flags and ranks live in LDS
constexpr int PL_THREADS = 1024;

// the video of a row, or -1 for a row that is skipped
__device__ __forceinline__ int row_video(int64_t s, int64_t o, int64_t NT, int N) {
  if (s < 0 || o < 0 || s >= NT || o >= NT) return -1;
  const int64_t bs = s / N, bo = o / N;
  return bs == bo ? (int)bs : -1;
}

// One workgroup per video b.  flags -> exclusive ranks -> lists.  s_list / o_list [B][Np] (slots past the count hold 0),
// counts [B][2], rank_ws [B][2][N] (the rank of a tracklet that occurs, -1 otherwise).
__global__ __launch_bounds__(PL_THREADS) void pair_plan_lists_kernel(const int64_t* __restrict__ pairs, int P, int B,
                                                                     int N, int Np, int* __restrict__ s_list,
                                                                     int* __restrict__ o_list, int* __restrict__ counts,
                                                                     int* __restrict__ rank_ws) {
  __shared__ int flag[2][PL_MAX_N];
  __shared__ int wave_sum[PL_THREADS / 64];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int64_t NT = (int64_t)B * N;
  for (int i = tid; i < 2 * PL_MAX_N; i += PL_THREADS) (&flag[0][0])[i] = 0;
  __syncthreads();
  for (int p = tid; p < P; p += PL_THREADS) {
    const int64_t s = pairs[2 * (int64_t)p], o = pairs[2 * (int64_t)p + 1];
    if (row_video(s, o, NT, N) == b) {
      flag[0][(int)(s - (int64_t)b * N)] = 1;     // every writer stores the same value
      flag[1][(int)(o - (int64_t)b * N)] = 1;
    }
  }
  __syncthreads();
  for (int side = 0; side < 2; ++side) {
    int* list = (side ? o_list : s_list) + (int64_t)b * Np;
    int* rank = rank_ws + ((int64_t)b * 2 + side) * N;
    // thread t owns tracklets 2t, 2t + 1 (N <= 2048 = 2 * PL_THREADS)
    const int i0 = 2 * tid, i1 = 2 * tid + 1;
    const int f0 = i0 < N ? flag[side][i0] : 0, f1 = i1 < N ? flag[side][i1] : 0;
    int incl = f0 + f1;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int up = __shfl_up(incl, d, 64);
      if ((tid & 63) >= d) incl += up;
    }
    if ((tid & 63) == 63) wave_sum[tid >> 6] = incl;
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < PL_THREADS / 64; ++w) {
      const int v = wave_sum[w];
      before += w < (tid >> 6) ? v : 0;
      total += v;
    }
    const int r0 = before + incl - f0 - f1, r1 = r0 + f0;
    if (i0 < N) rank[i0] = f0 ? r0 : -1;
    if (i1 < N) rank[i1] = f1 ? r1 : -1;
    if (f0) list[r0] = i0;
    if (f1) list[r1] = i1;
    for (int i = total + tid; i < Np; i += PL_THREADS) list[i] = 0;
    if (tid == 0) counts[2 * b + side] = total;
    __syncthreads();                              // wave_sum is reused by the other side
  }
}

// head [B][Np][Np] was set to -1 by the launcher; next [P]
__global__ __launch_bounds__(256) void pair_plan_link_kernel(const int64_t* __restrict__ pairs, int P, int B, int N, int Np,
                                                             const int* __restrict__ rank_ws, int* __restrict__ head,
                                                             int* __restrict__ next) {
  const int64_t NT = (int64_t)B * N;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < P; p += gridDim.x * 256) {
    const int64_t s = pairs[2 * (int64_t)p], o = pairs[2 * (int64_t)p + 1];
    const int b = row_video(s, o, NT, N);
    int nx = -1;
    if (b >= 0) {
      const int i = rank_ws[((int64_t)b * 2 + 0) * N + (int)(s - (int64_t)b * N)];
      const int j = rank_ws[((int64_t)b * 2 + 1) * N + (int)(o - (int64_t)b * N)];
      if (i >= 0 && j >= 0 && i < Np && j < Np)   // always true for a plan built from this table
        nx = atomicExch(&head[((int64_t)b * Np + i) * Np + j], p);
    }
    next[p] = nx;
  }
}

struct PairListCtx {
  int N, T, H, P, Np, sb, ob, ns, no;
  const int* __restrict__ sl;       // this video's subject / object lists
  const int* __restrict__ ol;
  const int* __restrict__ htile;    // head entry of the tile's slot pair (0, 0)
  const int* __restrict__ next;
  float* __restrict__ out;
};
// an arbitrary table on the tile of tspn_heads_pair_bf16.h: slot i of the subject axis is tracklet s_list[b][i], slot j
// of the object axis o_list[b][j]
template <int SBLK, int OB>
struct PairListMap {
  static __device__ __forceinline__ int row_trk(const PairListCtx c, int r) {
    // slots past the lists' ends stage a listed tracklet again (their accumulators have no chain)
    const int si = max(min(c.sb * SBLK + r, c.ns - 1), 0), oi = max(min(c.ob * OB + r - SBLK, c.no - 1), 0);
    const int trk = r < SBLK ? c.sl[si] : c.ol[oi];
    return max(min(trk, c.N - 1), 0);
  }
  // every row on the slot pair's chain gets the 16 heads x 16 frames; no s == o skip (that belongs to the canonical
  // table).  The walk is wave-uniform (scalar loads) and bounded: a chain has at most P rows.
  static __device__ __forceinline__ void emit(const PairListCtx c, int s_slot, int o_slot, int t, int hg, f32x4 acc,
                                              f32x4 bias) {
    int p = __builtin_amdgcn_readfirstlane(c.htile[s_slot * c.Np + o_slot]);
    for (int n = 0; n < c.P && (unsigned)p < (unsigned)c.P; ++n) {
      if (t < c.T) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int h = 4 * hg + r;
          if (h < c.H) c.out[((int64_t)p * c.H + h) * c.T + t] = acc[r] + bias[r];
        }
      }
      p = __builtin_amdgcn_readfirstlane(c.next[p]);
    }
  }
};

// The tile of heads_pairgrid_bf16_kernel over a video's compacted subject / object slots: same template forms, same
// grid, same xcd_remap.
template <int NW, int OB, int SW>
__global__ __launch_bounds__(NW * 64, NW == 4 ? 2 : 1) void heads_pairlist_bf16_kernel(
    const float* __restrict__ y, int64_t ldm, int B, int N, int C, int T,
    const __bf16* __restrict__ Whp, const float* __restrict__ bh, int H, float* __restrict__ out, int P, int Np,
    const int* __restrict__ s_list, const int* __restrict__ o_list, const int* __restrict__ counts,
    const int* __restrict__ head, const int* __restrict__ next, int nsb, int nob, int nfb) {
  constexpr int SBLK = 2 * NW;

  int wg = xcd_remap(blockIdx.x, gridDim.x);
  const int ob = wg % nob;
  wg /= nob;
  const int sb = wg % nsb;
  wg /= nsb;
  const int fb = wg % nfb;
  const int b = wg / nfb;

  // this tile's chains (Np is a multiple of 16 >= N: every slot of every tile has an entry).  Each wave looks at the
  // whole tile, so all of them take the same way and an empty tile ends before any barrier or DMA.
  const int* htile = head + ((int64_t)b * Np + sb * SBLK) * Np + ob * OB;
  {
    const int lane = threadIdx.x & 63;
    bool any = false;
#pragma unroll
    for (int e = lane; e < SBLK * OB; e += 64) any |= htile[(e / OB) * Np + e % OB] >= 0;
    if (__builtin_amdgcn_ballot_w64(any) == 0) return;
  }
  heads_pair_tile_bf16<NW, OB, SW, PairListMap<SBLK, OB>>(
      y, ldm, b, N, C, T, Whp, bh, H, fb * HP_FB,
      PairListCtx{N, T, H, P, Np, sb, ob, counts[2 * b], counts[2 * b + 1], s_list + (int64_t)b * Np,
                  o_list + (int64_t)b * Np, htile, next, out});
}

struct PlanLayout {
  size_t s_list, o_list, counts, head, next, rank, total;
};
int64_t plan_np(int64_t N) { return (N + 15) / 16 * 16; }
PlanLayout plan_layout(int64_t B, int64_t N, int64_t P) {
  PlanLayout L{};
  const size_t Np = (size_t)plan_np(N);
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t at = off;
    off += tspn::align_up(bytes, 256);
    return at;
  };
  L.s_list = take((size_t)B * Np * 4);
  L.o_list = take((size_t)B * Np * 4);
  L.counts = take((size_t)B * 2 * 4);
  L.head = take((size_t)B * Np * Np * 4);
  L.next = take((size_t)P * 4);
  L.rank = take((size_t)B * 2 * (size_t)N * 4);
  L.total = off;
  return L;
}

}  // namespace

extern "C" int tspn_pair_plan_i32(const int64_t* pairs, int64_t P, int64_t B, int64_t N, int32_t* s_list, int32_t* o_list,
                                  int32_t* counts, int32_t* head, int32_t* next, int32_t* rank_ws, void* stream) {
  TSPN_REQUIRE(P >= 0 && B >= 0 && N >= 0, TSPN_EINVAL, "tspn_pair_plan_i32: bad sizes P=%lld B=%lld N=%lld", (long long)P,
               (long long)B, (long long)N);
  TSPN_REQUIRE(N <= PL_MAX_N && P < (1LL << 31) && B < (1 << 20), TSPN_EUNSUPPORTED,
               "tspn_pair_plan_i32: needs N <= %d, P < 2^31, B < 2^20 (N=%lld P=%lld B=%lld)", PL_MAX_N, (long long)N,
               (long long)P, (long long)B);
  if (B == 0 || N == 0) return TSPN_OK;
  TSPN_REQUIRE(s_list && o_list && counts && head && rank_ws && (P == 0 || (pairs && next)), TSPN_EINVAL,
               "tspn_pair_plan_i32: null pointer");
  const int64_t Np = plan_np(N);
  hipStream_t s = TSPN_STREAM(stream);
  if (hipMemsetAsync(head, 0xff, (size_t)B * Np * Np * 4, s) != hipSuccess)       // every chain empty: -1
    return tspn::fail(TSPN_ELAUNCH, "tspn_pair_plan_i32: clearing the chain heads failed");
  hipLaunchKernelGGL(pair_plan_lists_kernel, dim3((unsigned)B), dim3(PL_THREADS), 0, s, pairs, (int)P, (int)B, (int)N, (int)Np,
                     s_list, o_list, counts, rank_ws);
  if (P > 0) {
    const int blocks = (int)std::min<int64_t>(tspn::ceil_div(P, 256), 4096);
    hipLaunchKernelGGL(pair_plan_link_kernel, dim3(blocks), dim3(256), 0, s, pairs, (int)P, (int)B, (int)N, (int)Np, rank_ws, head,
                       next);
  }
  return tspn::check_launch("tspn_pair_plan_i32");
}

extern "C" size_t tspn_heads_pairlist_bf16_workspace_bytes(int64_t B, int64_t N, int64_t P) {
  if (B <= 0 || N <= 0 || P < 0 || N > PL_MAX_N || P >= (1LL << 31)) return 0;
  return plan_layout(B, N, P).total;
}

extern "C" int tspn_heads_pairlist_bf16(const float* y, int64_t ldm, int64_t B, int64_t N, int64_t C, int64_t T,
                                        const int64_t* pairs, int64_t P, const uint16_t* head_packed, const float* head_b,
                                        int64_t H, float* out, void* workspace, size_t workspace_bytes, void* stream) {
  TSPN_REQUIRE(B >= 0 && N >= 0 && P >= 0 && C > 0 && T > 0 && H > 0 && H <= 16 && ldm > 0, TSPN_EINVAL,
               "tspn_heads_pairlist_bf16: bad sizes B=%lld N=%lld P=%lld C=%lld T=%lld H=%lld ldm=%lld", (long long)B,
               (long long)N, (long long)P, (long long)C, (long long)T, (long long)H, (long long)ldm);
  TSPN_REQUIRE(N <= PL_MAX_N && P < (1LL << 31), TSPN_EUNSUPPORTED,
               "tspn_heads_pairlist_bf16: needs N <= %d and P < 2^31 (N=%lld P=%lld)", PL_MAX_N, (long long)N, (long long)P);
  TSPN_REQUIRE(ldm >= 2 * C, TSPN_EUNSUPPORTED, "tspn_heads_pairlist_bf16: rows of y hold ldm=%lld < 2C=%lld floats",
               (long long)ldm, (long long)(2 * C));
  if (B == 0 || N == 0 || P == 0) return TSPN_OK;
  TSPN_REQUIRE(y && pairs && head_packed && head_b && out && workspace, TSPN_EINVAL, "tspn_heads_pairlist_bf16: null pointer");
  TSPN_REQUIRE(C % HP_KC == 0 && ldm % 4 == 0 && tspn::aligned16(y) && tspn::aligned16(head_packed), TSPN_EUNSUPPORTED,
               "tspn_heads_pairlist_bf16: needs C %% 32 == 0, ldm %% 4 == 0, 16-byte aligned y / weights");
  const bool big = N > 12;
  const int64_t sblk = big ? 16 : 8;
  const int64_t nsb = tspn::ceil_div(N, sblk), nfb = tspn::ceil_div(T, HP_FB);
  const int64_t grid = B * nsb * nsb * nfb;
  TSPN_REQUIRE(grid < (1LL << 31) && T < (1 << 24) && C < (1 << 24) && N * T * ldm * 4 < (1LL << 31) && B < (1 << 20),
               TSPN_EUNSUPPORTED, "tspn_heads_pairlist_bf16: problem too large (a video's projections must stay below 2 GB)");
  const PlanLayout L = plan_layout(B, N, P);
  TSPN_REQUIRE(workspace_bytes >= L.total, TSPN_EWORKSPACE, "tspn_heads_pairlist_bf16: workspace %zu < %zu bytes",
               workspace_bytes, L.total);
  TSPN_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, TSPN_EINVAL,
               "tspn_heads_pairlist_bf16: workspace must be 256-byte aligned");
  char* ws = static_cast<char*>(workspace);
  int32_t* s_list = reinterpret_cast<int32_t*>(ws + L.s_list);
  int32_t* o_list = reinterpret_cast<int32_t*>(ws + L.o_list);
  int32_t* counts = reinterpret_cast<int32_t*>(ws + L.counts);
  int32_t* head = reinterpret_cast<int32_t*>(ws + L.head);
  int32_t* next = reinterpret_cast<int32_t*>(ws + L.next);
  if (int rc = tspn_pair_plan_i32(pairs, P, B, N, s_list, o_list, counts, head, next, reinterpret_cast<int32_t*>(ws + L.rank),
                                  stream))
    return rc;
  const int Np = (int)plan_np(N);
  const size_t smem = heads_pair_tile_lds((int)(2 * sblk));
  static tspn::LdsLimit lds[2];
  if (int rc = big ? lds[1].ensure(reinterpret_cast<const void*>(heads_pairlist_bf16_kernel<8, 16, 2>), smem,
                                   "tspn_heads_pairlist_bf16")
                   : lds[0].ensure(reinterpret_cast<const void*>(heads_pairlist_bf16_kernel<4, 8, 2>), smem,
                                   "tspn_heads_pairlist_bf16"))
    return rc;
  if (big)
    hipLaunchKernelGGL((heads_pairlist_bf16_kernel<8, 16, 2>), dim3((unsigned)grid), dim3(512), smem, TSPN_STREAM(stream), y,
                       ldm, (int)B, (int)N, (int)C, (int)T, reinterpret_cast<const __bf16*>(head_packed), head_b, (int)H, out,
                       (int)P, Np, s_list, o_list, counts, head, next, (int)nsb, (int)nsb, (int)nfb);
  else
    hipLaunchKernelGGL((heads_pairlist_bf16_kernel<4, 8, 2>), dim3((unsigned)grid), dim3(256), smem, TSPN_STREAM(stream), y,
                       ldm, (int)B, (int)N, (int)C, (int)T, reinterpret_cast<const __bf16*>(head_packed), head_b, (int)H, out,
                       (int)P, Np, s_list, o_list, counts, head, next, (int)nsb, (int)nsb, (int)nfb);
  return tspn::check_launch("tspn_heads_pairlist_bf16");
}
