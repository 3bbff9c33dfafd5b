// A balanced mini-batch of span anchors for the span losses (gfx950): the mask tspn_span_loss_f32 takes, selected on the
// device from the labels of tspn_span_anchor_labels.
//
// Semantics (DESIGN.md 2 "span anchor sampling").  label int8 [n]: >= 1 positive, 0 negative, < 0 never selected.
//   word(i) = splitmix64(stream_key + i * 0x9E3779B97F4A7C15)   (the words of hashrng.bits), key(i) = word(i) >> (64 - key_bits)
//   the anchors of a class are ordered by (key, i) ascending; n_pos, n_neg = the class sizes,
//   sel_pos = min(n_pos, want_pos), sel_neg = min(n_neg, batch - sel_pos);
//   mask[i] = 1 for the sel_pos first positives and the sel_neg first negatives, 0 elsewhere (every element written);
//   counts = (n_pos, n_neg, sel_pos, sel_neg).
// Everything is wrapping 64-bit integer arithmetic; the quotas never leave the device.
//
// A radix select over 8-bit digits, most significant first, R = ceil(key_bits / 8) rounds; a chunk is CHUNK consecutive
// anchors, one workgroup, thread t holding the 16 anchors 16 t .. 16 t + 15 of it:
//   span_sample_hist_kernel     round r, one workgroup per chunk: the keys again, and of the anchors whose digits above
//                               round r equal the class's prefix (all of them in round 0) a histogram of digit r, both
//                               classes, in LDS (LDS integer adds: the sum does not depend on the order); stored whole to
//                               hist[chunk].
//   span_sample_select_kernel   one workgroup, one thread per (class, bin): the thread adds its bin of every chunk in chunk
//                               order; an inclusive prefix over the class's 256 bins (round 0: its last value is the class
//                               size, from which every thread forms the quotas; thread 0 writes counts) finds the one bin
//                               that holds the class's last selected anchor; that bin's thread appends its digit to the
//                               prefix and takes the anchors in the bins below off the remaining rank.  After round R - 1
//                               the prefix is the threshold key and the remaining rank is how many threshold-equal anchors
//                               are taken.
//   span_sample_offsets_kernel  one workgroup: the threshold-equal anchors of a chunk are bin (threshold & 255) of its
//                               last histogram; an exclusive prefix over the chunks, in chunk order, gives each chunk the
//                               rank of its first one.
//   span_sample_write_kernel    one workgroup per chunk: mask = key < threshold, or key == threshold and (chunk offset +
//                               rank inside the chunk) < remaining; the rank inside the chunk is an index-ordered
//                               workgroup prefix (lanes by shuffles, waves through LDS), never arrival order.
// partials uint32: [STATE] state, [2 nchunks] chunk offsets, [512 nchunks] histograms; every word is written by the
// call before the call reads it.
#include "tspn_common.h"

namespace {

constexpr int THREADS = 256;
constexpr int PER_THREAD = 16;                    // one 16-byte load of labels, one 16-byte store of mask
constexpr int CHUNK = THREADS * PER_THREAD;       // 4096 anchors per workgroup
constexpr int BINS = 256;                         // 8-bit digits
constexpr int SELECT_THREADS = 2 * BINS;          // one thread per (class, bin)
constexpr int STATE = 8;
// the state words
constexpr int ST_PREFIX = 0;                      // [2] the digits found so far; after the last round the threshold key
constexpr int ST_REMAIN = 2;                      // [2] the rank (1-based) still to find among the anchors under the prefix
constexpr int ST_SEL = 4;                         // [2] sel_pos, sel_neg
constexpr int ST_SIZE = 6;                        // [2] n_pos, n_neg

constexpr uint64_t GOLDEN = 0x9E3779B97F4A7C15ull;

__device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
  z += GOLDEN;
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}

__device__ __forceinline__ uint64_t anchor_key(uint64_t stream_key, int64_t i, int key_bits) {
  return splitmix64(stream_key + (uint64_t)i * GOLDEN) >> (64 - key_bits);
}

// 0 positive, 1 negative, -1 neither
__device__ __forceinline__ int anchor_class(int l) { return l >= 1 ? 0 : (l == 0 ? 1 : -1); }

struct Labels16 {
  int8_t v[PER_THREAD];
};

// the thread's 16 labels from `base` on; the elements from n on read as ignored
__device__ __forceinline__ Labels16 load_labels(const int8_t* __restrict__ label, int64_t base, int64_t n, bool aligned) {
  Labels16 l;
  if (aligned && base + PER_THREAD <= n) {
    const int4 q = *reinterpret_cast<const int4*>(label + base);
    const int w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < PER_THREAD; ++j) l.v[j] = (int8_t)(w[j >> 2] >> (8 * (j & 3)));
  } else {
#pragma unroll
    for (int j = 0; j < PER_THREAD; ++j) l.v[j] = base + j < n ? label[base + j] : (int8_t)-1;
  }
  return l;
}

// exclusive prefix of (a, b) over the workgroup's THREADS threads in thread order; `lds_wave` holds 2 * THREADS / 64 words
__device__ __forceinline__ void block_exclusive_scan2(unsigned& a, unsigned& b, unsigned* lds_wave) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned ia = a, ib = b;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned ua = __shfl_up(ia, o, 64), ub = __shfl_up(ib, o, 64);
    if (lane >= o) {
      ia += ua;
      ib += ub;
    }
  }
  if (lane == 63) {
    lds_wave[2 * wave] = ia;
    lds_wave[2 * wave + 1] = ib;
  }
  __syncthreads();
  unsigned ba = 0, bb = 0;
#pragma unroll
  for (int w = 0; w < THREADS / 64; ++w) {
    if (w < wave) {
      ba += lds_wave[2 * w];
      bb += lds_wave[2 * w + 1];
    }
  }
  a = ba + ia - a;
  b = bb + ib - b;
}

__global__ __launch_bounds__(THREADS) void span_sample_hist_kernel(const int8_t* __restrict__ label, int64_t n,
                                                                   uint64_t stream_key, int key_bits, int round, int shift,
                                                                   bool aligned, const unsigned* __restrict__ state,
                                                                   unsigned* __restrict__ hist) {
  __shared__ unsigned lds_hist[2 * BINS];
  lds_hist[threadIdx.x] = 0;
  lds_hist[threadIdx.x + THREADS] = 0;
  uint64_t prefix[2] = {0, 0};
  if (round > 0) {                                          // round 0 reads no state: nothing has written it yet
    prefix[0] = state[ST_PREFIX];
    prefix[1] = state[ST_PREFIX + 1];
  }
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * CHUNK + (int64_t)threadIdx.x * PER_THREAD;
  const Labels16 l = load_labels(label, base, n, aligned);
#pragma unroll
  for (int j = 0; j < PER_THREAD; ++j) {
    const int c = anchor_class(l.v[j]);
    if (c >= 0) {
      const uint64_t key = anchor_key(stream_key, base + j, key_bits);
      if (round == 0 || (key >> (shift + 8)) == (c ? prefix[1] : prefix[0]))
        atomicAdd(&lds_hist[c * BINS + (int)((key >> shift) & 255)], 1u);
    }
  }
  __syncthreads();
  unsigned* out = hist + (int64_t)blockIdx.x * (2 * BINS);
  out[threadIdx.x] = lds_hist[threadIdx.x];
  out[threadIdx.x + THREADS] = lds_hist[threadIdx.x + THREADS];
}

__global__ __launch_bounds__(SELECT_THREADS) void span_sample_select_kernel(const unsigned* __restrict__ hist,
                                                                            int64_t nchunks, int round, int64_t batch,
                                                                            int64_t want_pos, unsigned* __restrict__ state,
                                                                            int64_t* __restrict__ counts) {
  __shared__ unsigned lds_wave[SELECT_THREADS / 64];
  const int c = threadIdx.x >> 8, digit = threadIdx.x & (BINS - 1);      // the thread's class and bin
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, first = c * (BINS / 64);   // `first`: the class's first wave
  unsigned prefix = 0, remain = 0;
  if (round > 0) {                                           // read before any thread of this launch writes them
    prefix = state[ST_PREFIX + c];
    remain = state[ST_REMAIN + c];
  }
  unsigned total = 0;                                        // < 2^31: a bin holds at most n anchors
  int64_t k = 0;
  for (; k + 8 <= nchunks; k += 8) {                         // eight loads in flight: the walk is bound by their latency
    unsigned v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = hist[(k + u) * (2 * BINS) + threadIdx.x];
#pragma unroll
    for (int u = 0; u < 8; ++u) total += v[u];
  }
  for (; k < nchunks; ++k) total += hist[k * (2 * BINS) + threadIdx.x];
  // through = the class's anchors in the bins 0 .. digit: lanes by shuffles, the class's four waves through LDS
  unsigned through = total;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned up = __shfl_up(through, o, 64);
    if (lane >= o) through += up;
  }
  if (lane == 63) lds_wave[wave] = through;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < BINS / 64; ++w)
    if (first + w < wave) through += lds_wave[first + w];
  if (round == 0) {                                          // the class sizes and the quotas, the same in every thread
    int64_t size[2] = {0, 0};
#pragma unroll
    for (int w = 0; w < BINS / 64; ++w) {
      size[0] += lds_wave[w];
      size[1] += lds_wave[BINS / 64 + w];
    }
    const int64_t sel_pos = size[0] < want_pos ? size[0] : want_pos;
    const int64_t room = batch - sel_pos;
    const int64_t sel_neg = size[1] < room ? size[1] : room;
    remain = (unsigned)(c ? sel_neg : sel_pos);              // <= n < 2^31
    if (threadIdx.x == 0) {
      counts[0] = size[0];
      counts[1] = size[1];
      counts[2] = sel_pos;
      counts[3] = sel_neg;
      if (nchunks > 0) {                                     // n == 0: there is no state to keep
        state[ST_SEL] = (unsigned)sel_pos;
        state[ST_SEL + 1] = (unsigned)sel_neg;
        state[ST_SIZE] = (unsigned)size[0];
        state[ST_SIZE + 1] = (unsigned)size[1];
      }
    }
  }
  if (nchunks == 0) return;
  // the remain-th anchor under the prefix (it exists: remain <= the class's anchors under the prefix) lies in exactly one
  // bin; a class that selects nothing keeps digit 0
  const unsigned below = through - total;
  if (remain > 0 ? (below < remain && remain <= through) : digit == 0) {
    state[ST_PREFIX + c] = (prefix << 8) | (unsigned)digit;
    state[ST_REMAIN + c] = remain > 0 ? remain - below : 0;
  }
}

__global__ __launch_bounds__(THREADS) void span_sample_offsets_kernel(const unsigned* __restrict__ hist, int64_t nchunks,
                                                                      const unsigned* __restrict__ state,
                                                                      unsigned* __restrict__ offsets) {
  __shared__ unsigned lds_wave[2 * THREADS / 64];
  const int d0 = (int)(state[ST_PREFIX] & 255), d1 = (int)(state[ST_PREFIX + 1] & 255);
  const int64_t per = (nchunks + THREADS - 1) / THREADS;     // consecutive chunks of a thread
  const int64_t lo = threadIdx.x * per, hi = lo + per < nchunks ? lo + per : nchunks;
  unsigned a = 0, b = 0;
  for (int64_t c = lo; c < hi; ++c) {
    a += hist[c * (2 * BINS) + d0];
    b += hist[c * (2 * BINS) + BINS + d1];
  }
  block_exclusive_scan2(a, b, lds_wave);
  for (int64_t c = lo; c < hi; ++c) {
    offsets[2 * c] = a;
    offsets[2 * c + 1] = b;
    a += hist[c * (2 * BINS) + d0];
    b += hist[c * (2 * BINS) + BINS + d1];
  }
}

__global__ __launch_bounds__(THREADS) void span_sample_write_kernel(const int8_t* __restrict__ label, int64_t n,
                                                                    uint64_t stream_key, int key_bits, bool aligned,
                                                                    const unsigned* __restrict__ state,
                                                                    const unsigned* __restrict__ offsets,
                                                                    uint8_t* __restrict__ mask) {
  __shared__ unsigned lds_wave[2 * THREADS / 64];
  const uint64_t thr[2] = {state[ST_PREFIX], state[ST_PREFIX + 1]};
  const unsigned take[2] = {state[ST_REMAIN], state[ST_REMAIN + 1]};
  const bool on[2] = {state[ST_SEL] > 0, state[ST_SEL + 1] > 0};
  const int64_t base = (int64_t)blockIdx.x * CHUNK + (int64_t)threadIdx.x * PER_THREAD;
  const Labels16 l = load_labels(label, base, n, aligned);
  unsigned below = 0, equal = 0, neg = 0;                    // bit j: anchor j is under / on its class's threshold, is negative
#pragma unroll
  for (int j = 0; j < PER_THREAD; ++j) {
    const int c = anchor_class(l.v[j]);
    if (c >= 0 && (c ? on[1] : on[0])) {
      const uint64_t key = anchor_key(stream_key, base + j, key_bits);
      const uint64_t t = c ? thr[1] : thr[0];
      below |= (unsigned)(key < t) << j;
      equal |= (unsigned)(key == t) << j;
      neg |= (unsigned)c << j;
    }
  }
  unsigned rank[2] = {(unsigned)__popc(equal & ~neg), (unsigned)__popc(equal & neg)};
  block_exclusive_scan2(rank[0], rank[1], lds_wave);
  rank[0] += offsets[2 * (int64_t)blockIdx.x];
  rank[1] += offsets[2 * (int64_t)blockIdx.x + 1];
  unsigned w[4] = {0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < PER_THREAD; ++j) {
    const bool c = neg >> j & 1;
    unsigned m = below >> j & 1;
    if (equal >> j & 1) {
      m = c ? rank[1] < take[1] : rank[0] < take[0];
      rank[0] += !c;
      rank[1] += c;
    }
    w[j >> 2] |= m << (8 * (j & 3));
  }
  if (aligned && base + PER_THREAD <= n) {
    *reinterpret_cast<uint4*>(mask + base) = make_uint4(w[0], w[1], w[2], w[3]);
  } else {
#pragma unroll
    for (int j = 0; j < PER_THREAD; ++j)
      if (base + j < n) mask[base + j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
  }
}

// 0 for an n the entry refuses
int64_t chunks_of(int64_t n) { return n < 0 || n >= (1LL << 31) ? -1 : tspn::ceil_div(n, CHUNK); }

}  // namespace

extern "C" int64_t tspn_span_anchor_sample_partials(int64_t n) {
  const int64_t nchunks = chunks_of(n);
  return nchunks < 0 ? 0 : STATE + nchunks * (2 + 2 * BINS);
}

extern "C" int tspn_span_anchor_sample(const int8_t* label, int64_t n, uint64_t stream_key, int key_bits, int64_t batch,
                                       int64_t want_pos, uint32_t* partials, int64_t* counts, uint8_t* mask, void* stream) {
  const char* who = "tspn_span_anchor_sample";
  TSPN_REQUIRE(n >= 0, TSPN_EINVAL, "%s: bad size n=%lld", who, (long long)n);
  TSPN_REQUIRE(n < (1LL << 31), TSPN_EUNSUPPORTED, "%s: n=%lld anchors (needs < 2^31)", who, (long long)n);
  TSPN_REQUIRE(key_bits >= 1 && key_bits <= 32, TSPN_EINVAL, "%s: key_bits=%d outside [1, 32]", who, key_bits);
  TSPN_REQUIRE(batch >= 0, TSPN_EINVAL, "%s: bad batch=%lld", who, (long long)batch);
  TSPN_REQUIRE(want_pos >= 0 && want_pos <= batch, TSPN_EINVAL, "%s: want_pos=%lld outside [0, batch=%lld]", who,
               (long long)want_pos, (long long)batch);
  TSPN_REQUIRE(counts && (n == 0 || (label && partials && mask)), TSPN_EINVAL, "%s: null pointer", who);
  TSPN_REQUIRE((reinterpret_cast<uintptr_t>(counts) & 7) == 0 && (reinterpret_cast<uintptr_t>(partials) & 3) == 0,
               TSPN_EUNSUPPORTED, "%s: unaligned pointer (counts needs 8 bytes, partials 4)", who);
  const int64_t nchunks = chunks_of(n);
  unsigned* state = partials;
  unsigned* offsets = partials + STATE;
  unsigned* hist = offsets + 2 * nchunks;
  // the 16-byte forms of the label load and the mask store, where both pointers allow them
  const bool aligned = tspn::all_aligned16(label, mask);
  const int rounds = (key_bits + 7) / 8;
  hipStream_t s = TSPN_STREAM(stream);
  if (n == 0) {                                             // only what writes counts = 0
    hipLaunchKernelGGL(span_sample_select_kernel, dim3(1), dim3(SELECT_THREADS), 0, s, hist, nchunks, 0, batch, want_pos,
                       state, counts);
    return tspn::check_launch(who);
  }
  for (int r = 0; r < rounds; ++r) {
    const int shift = 8 * (rounds - 1 - r);
    hipLaunchKernelGGL(span_sample_hist_kernel, dim3((unsigned)nchunks), dim3(THREADS), 0, s, label, n, stream_key, key_bits,
                       r, shift, aligned, state, hist);
    hipLaunchKernelGGL(span_sample_select_kernel, dim3(1), dim3(SELECT_THREADS), 0, s, hist, nchunks, r, batch, want_pos,
                       state, counts);
  }
  hipLaunchKernelGGL(span_sample_offsets_kernel, dim3(1), dim3(THREADS), 0, s, hist, nchunks, state, offsets);
  hipLaunchKernelGGL(span_sample_write_kernel, dim3((unsigned)nchunks), dim3(THREADS), 0, s, label, n, stream_key, key_bits,
                     aligned, state, offsets, mask);
  return tspn::check_launch(who);
}
