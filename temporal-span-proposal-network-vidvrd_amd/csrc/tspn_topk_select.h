// The one home of selection ("Top-k ties" and "Selection": larger tspn::order_key first, lower index on ties,
// key 0 below every real key).  Users:
//   bitonic_sort_desc    ppn_kernel (tspn_ppn.hip), decode_spans_kernel (tspn_spans.hip), select_topk_sorted below
//   wave_row_topk        pair_topk_kernel (tspn_decode.hip), span_row_topk_kernel (relations/tspn_span_relations.hip),
//                        span_row_topk_q_kernel (spanbf16/tspn_span_bf16.hip)
//   select_topk_sorted   segment_topk_kernel (tspn_decode.hip), segment_span_topk_kernel
//                        (relations/tspn_span_relations.hip): exact top-M of Q keyed candidates by one workgroup, in
//                        torch's stable descending order; box_nms_select_kernel (detect/tspn_detect.hip) runs the same
//                        body at MAXM = kSelectMaxMBig
//   argmax_first         the class labels of both segment kernels
#pragma once
#include "tspn_common.h"

namespace tspn {

// Padding of a sort or of an arg-max seed: real keys are never 0 (tspn::order_key), so padding sorts last, and among
// padding the index is irrelevant.
constexpr unsigned kPadKey = 0u;
constexpr int kPadIdx = 0x7fffffff;

// Bitonic sort of n2 (a power of two) pairs (key[i], idx[i]) in LDS into key_before order.  All THREADS threads of the
// workgroup call it, after a barrier that made the arrays visible; one barrier per (k, j) step (none when n2 == 1), and
// on return, after the last of them, the arrays are sorted.
template <int THREADS>
__device__ __forceinline__ void bitonic_sort_desc(unsigned* key, int* idx, int n2) {
  const int tid = threadIdx.x;
  for (int k = 2; k <= n2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < n2; i += THREADS) {
        const int l = i ^ j;
        if (l > i) {
          const unsigned ki = key[i], kl = key[l];
          const int ii = idx[i], il = idx[l];
          const bool fwd = (i & k) == 0;
          const bool swap = fwd ? key_before(kl, il, ki, ii) : key_before(ki, ii, kl, il);
          if (swap) {
            key[i] = kl;
            key[l] = ki;
            idx[i] = il;
            idx[l] = ii;
          }
        }
      }
      __syncthreads();
    }
  }
}

constexpr int kRowTopkVPT = 4;                      // values a lane holds in registers
constexpr int kRowTopkMaxK = 64 * kRowTopkVPT;

// The R best of a row of K <= kRowTopkMaxK values by one wave, in key_before order.  Lane `lane` holds value
// k = lane + 64 i in v[i] (anything where k >= K).  R rounds of a lane-local best over the unused slots followed by a
// wave arg-max; R <= K and every real value has a key > 0, so each round selects an unused k < K.  emit(r, value, k)
// runs on the lane that owns the winner of round r only, with the value as loaded (NaN payloads kept).
template <class Emit>
__device__ __forceinline__ void wave_row_topk(const float (&v)[kRowTopkVPT], int K, int R, int lane, Emit emit) {
  unsigned kv[kRowTopkVPT];
#pragma unroll
  for (int i = 0; i < kRowTopkVPT; ++i) kv[i] = order_key(v[i]);
  unsigned used = 0;
  for (int r = 0; r < R; ++r) {
    unsigned bk = kPadKey;
    int bi = kPadIdx;
#pragma unroll
    for (int i = 0; i < kRowTopkVPT; ++i) {
      const int k = lane + 64 * i;
      if (k < K && !((used >> i) & 1u) && key_before(kv[i], k, bk, bi)) {
        bk = kv[i];
        bi = k;
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned ok = __shfl_xor(bk, off);
      const int oi = __shfl_xor(bi, off);
      if (key_before(ok, oi, bk, bi)) {
        bk = ok;
        bi = oi;
      }
    }
    if ((bi & 63) == lane && bi < K) {
      float bv = v[0];
#pragma unroll
      for (int i = 1; i < kRowTopkVPT; ++i)
        if ((bi >> 6) == i) bv = v[i];
      used |= 1u << (bi >> 6);
      emit(r, bv, bi);
    }
  }
}

constexpr int kSelectThreads = 1024;   // the workgroup size select_topk_sorted expects
constexpr int kSelectMaxM = 1024;
constexpr int kSelectMaxMBig = 8192;   // the box NMS's capacity (detect/tspn_detect.hip): 64 KB of pairs, dynamic LDS

template <int MAXM>
struct SelectLdsT {
  unsigned hist[256];
  unsigned prefix, need, count;
  unsigned kk[MAXM];
  int ki[MAXM];
};
using SelectLds = SelectLdsT<kSelectMaxM>;
using SelectLdsBig = SelectLdsT<kSelectMaxMBig>;

// Called by all kSelectThreads threads of a workgroup.  key(i), i in [0, Q): the order key of candidate i (larger first,
// lower i first on ties); at least M <= MAXM candidates have a key > 0.  Exact radix select of the M-th largest
// key (4 x 8-bit histograms), index-select among the candidates that tie with it, compaction into LDS and a bitonic
// sort: on return, after a barrier, L.ki[r] is the flat index of the r-th best candidate and L.kk[r] its key, r < M.
template <int MAXM, class KeyFn>
__device__ __forceinline__ void select_topk_sorted(SelectLdsT<MAXM>& L, KeyFn key, int Q, int M) {
  const int tid = threadIdx.x;
  // ---- exact M-th largest key by 4 radix passes (most significant byte first)
  if (tid == 0) {
    L.prefix = 0;
    L.need = (unsigned)M;
  }
  __syncthreads();
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    if (tid < 256) L.hist[tid] = 0;
    __syncthreads();
    const unsigned prefix = L.prefix;
    const unsigned himask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
    for (int i = tid; i < Q; i += kSelectThreads) {
      const unsigned k = key(i);
      if ((k & himask) == prefix) atomicAdd(&L.hist[(k >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      unsigned need = L.need, acc = 0;
      int b = 255;
      for (; b >= 0; --b) {
        if (acc + L.hist[b] >= need) break;
        acc += L.hist[b];
      }
      L.prefix = prefix | ((unsigned)b << shift);
      L.need = need - acc;  // how many we still need inside bucket b
    }
    __syncthreads();
  }
  const unsigned kth = L.prefix;        // key of the M-th largest candidate
  const unsigned ties_needed = L.need;  // of the candidates equal to it, the lowest indices win
  __syncthreads();  // everyone has read prefix / need before they are reused below
  // ---- among ties: the `ties_needed`-th smallest flat index (4 byte-wide passes, lowest first)
  if (tid == 0) {
    L.prefix = 0;
    L.need = ties_needed;
  }
  __syncthreads();
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    if (tid < 256) L.hist[tid] = 0;
    __syncthreads();
    const unsigned prefix = L.prefix;
    const unsigned himask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
    for (int i = tid; i < Q; i += kSelectThreads) {
      if (key(i) == kth && (((unsigned)i) & himask) == prefix)
        atomicAdd(&L.hist[(((unsigned)i) >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      unsigned need = L.need, acc = 0;
      int b = 0;
      for (; b < 256; ++b) {
        if (acc + L.hist[b] >= need) break;
        acc += L.hist[b];
      }
      L.prefix = prefix | ((unsigned)b << shift);
      L.need = need - acc;
    }
    __syncthreads();
  }
  const unsigned last_tie_idx = L.prefix;  // ties with index <= this are selected

  // ---- compaction of the M winners into LDS (unordered), then bitonic sort
  if (tid == 0) L.count = 0;
  __syncthreads();
  for (int i = tid; i < Q; i += kSelectThreads) {
    const unsigned k = key(i);
    if (k > kth || (k == kth && (unsigned)i <= last_tie_idx)) {
      const unsigned slot = atomicAdd(&L.count, 1u);
      if (slot < (unsigned)MAXM) {
        L.kk[slot] = k;
        L.ki[slot] = i;
      }
    }
  }
  __syncthreads();
  const int m2 = (int)next_pow2(M);
  for (int i = tid; i < m2; i += kSelectThreads)
    if (i >= M) {
      L.kk[i] = kPadKey;
      L.ki[i] = kPadIdx;
    }
  __syncthreads();
  bitonic_sort_desc<kSelectThreads>(L.kk, L.ki, m2);
}

// torch.argmax over n values: the first NaN, else the first maximum
__device__ inline int argmax_first(const float* p, int n) {
  unsigned bk = order_key(p[0]);
  int bi = 0;
  for (int i = 1; i < n; ++i) {
    const unsigned k = order_key(p[i]);
    if (k > bk) {
      bk = k;
      bi = i;
    }
  }
  return bi;
}

}  // namespace tspn
