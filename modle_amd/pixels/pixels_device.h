// pixels_device.h -- the device primitives the kernels of libmodle_pixels.so share (private, like pixels_context.h):
// the wave scan and the wave reductions, the 128-bit add, one pass of a summed-area table in LDS, and the grid
// folded into y.  One copy each, so that a change of an instruction sequence has one place and one set of kernels
// to time.  wave64 throughout; every shuffle is called by whole waves.
//
// What is not here, and why: csrc/wave_hip.h of the simulator has DPP sequences for some of these, but is built
// with other flags; the accumulators of modle_stripes.hip and modle_scc.hip, the butterfly of modle_marginals.hip,
// the column-chunk loops of modle_insulation.hip and modle_profiles.hip and the tile loaders of modle_dots.hip and
// modle_scc.hip say at their place what keeps them apart.
#ifndef MODLE_PIXELS_DEVICE_H
#define MODLE_PIXELS_DEVICE_H
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

namespace modle_pixels_device {

using u64 = unsigned long long;

// the inclusive scan of x over the wave; `lane` is the caller's threadIdx.x & 63
__device__ __forceinline__ u64 wave_scan(u64 x, unsigned lane) {
#pragma unroll
  for (unsigned s = 1; s < 64; s *= 2) {
    const u64 y = __shfl_up(x, s);
    if (lane >= s) x += y;
  }
  return x;
}

// the last lane's x in every lane: after wave_scan, the wave's total
__device__ __forceinline__ u64 wave_last(u64 x) { return __shfl(x, 63); }

// The reductions leave their result in lane 0 (the other lanes hold partial results).
__device__ __forceinline__ u64 wave_sum(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  return v;
}

__device__ __forceinline__ unsigned wave_max(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_down(v, o));
  return v;
}

__device__ __forceinline__ u64 wave_min(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, static_cast<u64>(__shfl_down(v, o)));
  return v;
}

// (hi, lo) += (x_hi, x_lo): the carry of the low word is counted in the high one
__device__ __forceinline__ void add128(u64& lo, u64& hi, u64 x_lo, u64 x_hi) {
  lo += x_lo;
  hi += x_hi + (lo < x_lo ? 1u : 0u);
}

// One pass of a summed-area table in LDS, called by a whole workgroup of kThreads: `nlines` lines of `nelem`
// elements, element e of line l at base[l * line_stride + e * se], where cell (0, 0) of the tile is A[1][1] of a
// table of pitch kPitch.  A line goes to min(kThreads / nlines, kMaxSeg) threads, which scan their segments in
// place, read the totals of the segments before theirs and add them.  nlines <= kThreads.  Ends with a barrier.
// kMaxLines, where given: the caller's nlines never exceed it, and it leaves every line kMaxSeg threads (checked
// here), so the segments of a line are a constant (modle_dots.hip; with their number read at run time its kernels
// took 0.8 - 2.3 % longer on the chr1-shaped band, profiles/shared_device/timing_vs_parent.txt).
template <unsigned kThreads, int kPitch, int kMaxSeg, int kMaxLines = 0>
__device__ __forceinline__ void sat_scan_pass(u64* sat, int nlines, int nelem, int line_stride, int se) {
  static_assert(kMaxLines == 0 || static_cast<int>(kThreads) / kMaxLines >= kMaxSeg, "kMaxSeg threads for every line");
  const int t = static_cast<int>(threadIdx.x);
  const int segs = kMaxLines != 0 ? kMaxSeg : min(static_cast<int>(kThreads) / nlines, kMaxSeg);
  const int line = t % nlines, seg = t / nlines;
  const int L = (nelem + segs - 1) / segs;
  const bool active = seg < segs;
  u64* base = sat + kPitch + 1 + line * line_stride;
  const int e0 = min(nelem, seg * L), e1 = min(nelem, e0 + L);
  if (active) {
    u64 acc = 0;
    for (int e = e0; e < e1; ++e) {
      acc += base[e * se];
      base[e * se] = acc;
    }
  }
  __syncthreads();
  u64 off = 0;
  if (active)
    for (int s = 1; s <= seg; ++s) {
      const int end = min(nelem, s * L);  // one past the last element of segment s - 1
      if (end > min(nelem, (s - 1) * L)) off += base[(end - 1) * se];
    }
  __syncthreads();
  if (active && seg > 0)
    for (int e = e0; e < e1; ++e) base[e * se] += off;
  __syncthreads();
}

// A grid folded into y: a grid's x holds kGridX workgroups, those beyond go to y (no loop strides by the grid).
// grid_of(groups) launches at least `groups` workgroups, and group_id() numbers them; a kernel leaves those at or
// beyond `groups` idle.  (grid_of is hidden, like the helpers of pixels_context.h.)
constexpr unsigned kGridX = 1u << 20;

__device__ __forceinline__ u64 group_id() { return static_cast<u64>(blockIdx.y) * gridDim.x + blockIdx.x; }

__attribute__((visibility("hidden")))
inline dim3 grid_of(uint64_t groups) {
  const uint64_t x = std::min<uint64_t>(groups, kGridX);
  return dim3(static_cast<unsigned>(x), static_cast<unsigned>((groups + x - 1) / x));
}

}  // namespace modle_pixels_device

#endif
