// Device-side vocabulary shared by the MFMA kernel files (gfx950 only): vector types, the global-to-LDS DMA pieces in
// their pointer and buffer forms, buffer descriptors, the inline-asm fragment loads with their counted waits, and the
// workgroup-to-tile maps.  One
// definition each; a kernel file pulls them in with `using namespace tspn_dev;` inside its anonymous namespace.  What
// belongs to ONE kernel's plan (tile constants, LDS counters, role barriers, packed-math helpers) stays in its file.
// Everything here is force-inlined: -fno-gpu-rdc gives no device symbols across translation units.
#pragma once
#include <hip/hip_runtime.h>

namespace tspn_dev {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// ---- global -> LDS DMA, pointer form (global_load_lds_dwordx4 / _dword): each lane names its own 16 (4) source bytes,
// the wave's pieces land at `l` + 16 (4) * lane.  AUX = the cache policy bits of the instruction.
template <int AUX = 0>
__device__ __forceinline__ void glds16(const void* g, void* l) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                   (__attribute__((address_space(3))) void*)l, 16, 0, AUX);
}
__device__ __forceinline__ void glds4(const void* g, void* l) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                   (__attribute__((address_space(3))) void*)l, 4, 0, 0);
}

// ---- buffer descriptors.  The flags word (dword 3 of the descriptor) selects DATA_FORMAT = 32 bit and nothing else: no
// swizzle, no stride, no index -- a raw buffer whose range check is `byte offset < bytes`.  A load beyond the range returns
// zeros (into LDS too), a store beyond it is dropped: that is how the kernels pad.  `bytes` is the descriptor's
// num_records as the builtin takes it (an int carrying an unsigned 32-bit count).
constexpr int kBufferFlags = 0x00020000;
constexpr int kBufferUnbounded = 0x7fffffff;   // 2^31 - 1: every offset with the top bit set is out of range
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_rsrc(const void* p, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes, kBufferFlags);
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_rsrc_unbounded(const void* p) {
  return buffer_rsrc(p, kBufferUnbounded);
}

// ---- global -> LDS DMA, buffer form (buffer_load_dwordx4 ... offen lds): one SGPR descriptor, the lane's 32-bit byte
// offset `voff`, a wave-uniform byte offset `soff`; the wave's pieces land at `l` + 16 * lane.
// (The builtin takes the LDS address BEFORE the offsets.  Where a kernel's schedule was tuned with the raw builtin, the call site
// names the address on the line before the call, so that the address arithmetic is still emitted first.)
__device__ __forceinline__ void bglds16(__amdgpu_buffer_rsrc_t rsrc, unsigned voff, int soff, void* l) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)l, 16, (int)voff, soff, 0, 0);
}

// ---- fragment loads straight into MFMA operand registers.  They are inline asm (a 13-bit immediate offset on a
// wave-uniform base, issued exactly where the kernel's schedule wants them), so the compiler does not see them as
// asynchronous: every use of their destination registers is preceded by a counted wait that is tied to those
// registers by "+v", which keeps the use behind the wait and the wait behind the load.  A copy or a spill that the
// compiler put between a load and its wait would capture stale data, hence NO_SPILL_KERNELS in build.py.
template <int OFF>
__device__ __forceinline__ void load_wfrag(f32x4& dst, unsigned lane_off, const char* base) {
  asm volatile("global_load_dwordx4 %0, %1, %2 offset:%3" : "=v"(dst) : "v"(lane_off), "s"(base), "n"(OFF) : "memory");
}
template <int VM>
__device__ __forceinline__ void wait_w(f32x4& r) {
  asm volatile("s_waitcnt vmcnt(%1)" : "+v"(r) : "n"(VM));
}
template <int VM>
__device__ __forceinline__ void wait_w(f32x4& r0, f32x4& r1) {
  asm volatile("s_waitcnt vmcnt(%2)" : "+v"(r0), "+v"(r1) : "n"(VM));
}
// the plain counted wait, for the LDS-DMA rings (no destination registers to tie it to)
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// ---- workgroup -> tile maps.
// bijective XCD remap of `n` workgroups: the hardware deals consecutive block ids round the 8 XCDs, this gives XCD x a
// contiguous range of the logical ids (which therefore share its L2)
__device__ __forceinline__ int xcd_remap(int id, int n) {
  const int q8 = n >> 3, r8 = n & 7, xcd = id & 7;
  return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (id >> 3);
}
// Grouped tile numbering of a tiles_m x tiles_n grid: groups of GM weight panels (row tiles) x all column tiles, the
// row tile running fastest inside a group, so that the workgroups resident on one XCD (consecutive `wg` after
// xcd_remap) share a few weight panels and column panels in its L2.  The last group holds tiles_m % GM row tiles when
// that is not zero.
__device__ __forceinline__ void grouped_tile(int wg, int GM, int tiles_m, int tiles_n, int& tile_m, int& tile_n) {
  const int group_sz = GM * tiles_n;
  const int group = wg / group_sz;
  const int first_m = group * GM;
  const int gm = min(GM, tiles_m - first_m);
  const int in_group = wg - group * group_sz;
  tile_m = first_m + in_group % gm;
  tile_n = in_group / gm;
}

// Pair-stage map: workgroup -> (group = (video, frame block), subject block sb, object block ob).  The nsb * nob
// workgroups of one group read the same tracklet rows and walk the channels in step, so they are placed on ONE XCD
// (ids congruent mod 8 share an XCD) and dispatched back to back: each row chunk then comes from HBM once and from that
// XCD's L2 for the other blocks.  The grid is rounded up to whole rounds of 8 groups: a kernel returns where the
// group number is >= its ngroups (uniform per workgroup, before any barrier).
__device__ __forceinline__ int64_t pair_stage_group(int id, int nsb, int nob, int& sb, int& ob) {
  const int per_group = nsb * nob;
  const int xcd = id & 7, k = id >> 3;
  const int member = k % per_group;
  sb = member / nob;
  ob = member - sb * nob;
  return (int64_t)(k / per_group) * 8 + xcd;
}

}  // namespace tspn_dev
