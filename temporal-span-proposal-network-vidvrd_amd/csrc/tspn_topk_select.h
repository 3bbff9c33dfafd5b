// Exact top-M of Q keyed candidates by one workgroup, in torch's stable descending order: shared by
// segment_topk_kernel (tspn_decode.hip) and segment_span_topk_kernel (relations/tspn_span_relations.hip).
#pragma once
#include "tspn_common.h"

namespace tspn {

constexpr int kSelectThreads = 1024;   // the workgroup size select_topk_sorted expects
constexpr int kSelectMaxM = 1024;

struct SelectLds {
  unsigned hist[256];
  unsigned prefix, need, count;
  unsigned kk[kSelectMaxM];
  int ki[kSelectMaxM];
};

// Called by all kSelectThreads threads of a workgroup.  key(i), i in [0, Q): the order key of candidate i (larger first,
// lower i first on ties); at least M <= kSelectMaxM candidates have a key > 0.  Exact radix select of the M-th largest
// key (4 x 8-bit histograms), index-select among the candidates that tie with it, compaction into LDS and a bitonic
// sort: on return, after a barrier, L.ki[r] is the flat index of the r-th best candidate and L.kk[r] its key, r < M.
template <class KeyFn>
__device__ __forceinline__ void select_topk_sorted(SelectLds& L, KeyFn key, int Q, int M) {
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
      if (slot < (unsigned)kSelectMaxM) {
        L.kk[slot] = k;
        L.ki[slot] = i;
      }
    }
  }
  __syncthreads();
  int m2 = 1;
  while (m2 < M) m2 <<= 1;
  for (int i = tid; i < m2; i += kSelectThreads)
    if (i >= M) {
      L.kk[i] = 0u;                                  // below every real key
      L.ki[i] = 0x7fffffff;
    }
  __syncthreads();
  for (int k = 2; k <= m2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < m2; i += kSelectThreads) {
        const int l = i ^ j;
        if (l > i) {
          const unsigned vi = L.kk[i], vl = L.kk[l];
          const int ii = L.ki[i], il = L.ki[l];
          const bool fwd = (i & k) == 0;
          const bool swap = fwd ? key_before(vl, il, vi, ii) : key_before(vi, ii, vl, il);
          if (swap) {
            L.kk[i] = vl;
            L.kk[l] = vi;
            L.ki[i] = il;
            L.ki[l] = ii;
          }
        }
      }
      __syncthreads();
    }
  }
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
