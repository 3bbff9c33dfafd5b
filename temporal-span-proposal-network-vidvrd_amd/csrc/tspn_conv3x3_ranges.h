// The 3x3 of the bf16 bottleneck tails as LINEAR RANGES (gfx950 only), shared by tspn_bottleneck_bf16.hip,
// tspn_tail_io_bf16.hip and tspn_bottleneck_pipe_bf16.hip: the tile constants the three agree on and the tap mask.
//
// A tile is BN consecutive pixels of a channels-last [npix][CM] bf16 map.  Tap (a, b) of pixel n is pixel
// n + (a - 1) W + (b - 1), so ONE staged range -- pixels n0 + (a - 1) W - 1 .. + 129 of a 64-channel part -- serves the
// three taps (a, 0..2) of the whole tile at slot offsets 0..2.  A range runs across row and image boundaries; the taps
// that fall off the image are zeroed at the fragment read, by the lane's tap mask.
//
// What is NOT here: the staging of a range (lane offset, four pieces at 2 p SLP 16, the side piece for slots 128, 129).
// The three kernels write the same pixel arithmetic, but bottleneck_bf16_kernel issues the side piece from wave 0 alone,
// tail_io_bf16_kernel from every io wave with a guard per main piece (its vmcnt(10) waits count exactly those pieces),
// and team A of the pipe kernel stages with per-lane pointers and a zero page instead of a buffer descriptor.  Even the
// offset computation alone, moved into a function, changed the register allocation of all three instances of
// bottleneck_bf16_kernel (+2 to +4 VGPRs at 248 of 256), so each kernel keeps its staging in its own file.
#pragma once
#include <cstdint>

#include "tspn_device.h"

namespace tspn_dev {

constexpr int BN = 128;                 // pixels per tile
constexpr int KC = 64;                  // channels per chunk
constexpr int SLP = 132;                // padded pixel slots per channel group (130 used by a range)
constexpr int B_ST = 8 * SLP * 16;      // bytes per range stage = per 64 channels of the h2 image
constexpr unsigned OOB = 0x80000000u;   // beyond every unbounded descriptor: the piece arrives as zeros

// TapMask{npix, H, W}(n): the 9-bit mask of the taps (bit 3 a + b) of pixel n that lie inside its H x W image; 0 for
// n >= npix.  The members are REFERENCES to the kernel's own arguments, which must outlive the object: build it from
// the named arguments (`const TapMask tap_mask{npix, H, W};`), never from a temporary.  It holds references, as the
// kernels' lambdas did, because that form compiles to the instructions the kernels had (profiles/r14/README.md).
struct TapMask {
  const int64_t& npix;
  const int& H;
  const int& W;
  __device__ unsigned operator()(int64_t n) const {
    unsigned m = 0;
    const bool okn = n < npix;
    const int64_t nc = okn ? n : 0;
    const int64_t nb = nc / ((int64_t)H * W);
    const int r = (int)(nc - nb * H * W);
    const int oh = r / W, ow = r - oh * W;
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b)
        if (okn && oh - 1 + a >= 0 && oh - 1 + a < H && ow - 1 + b >= 0 && ow - 1 + b < W) m |= 1u << (a * 3 + b);
    return m;
  }
};

}  // namespace tspn_dev
