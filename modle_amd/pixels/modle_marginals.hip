// modle_marginals.hip -- the marginals of a band matrix, summed on the MI355X
// (include/modle_pixels.h: modle_pixels_marginals / _marginals_to_host / _coarse_marginals_to_host).
//
// One streaming kernel reads every pixel word once, the way it lies in memory, and feeds three 64-bit
// sums from that one read: the diagonal sums diag_sum[d], and the two halves of the coverage of the
// symmetric matrix, the column part (pixel (i, j) counted for bin j) and the row part (counted for bin
// i = j - d, the diagonal pixel left out: it is in the column part already).
//
// The tile is pixels_count's: kCols columns x kDepth band words, kDepth threads, thread dd owns
// d = d0 + dd in every column of the tile, so a wave reads 256 contiguous bytes per column, kUnroll
// columns in flight.
//   diag_sum   the thread's own register over the tile's columns: no cross-lane work, one 64-bit
//              add per thread and tile, 64 contiguous words per wave instruction;
//   row part   cn + dn - 1 64-bit LDS slots, slot = jj + dn - 1 - dd as in pixels_count: the 64
//              lanes of one column hit 64 different slots, a zero word adds nothing;
//   column     kUnroll = 4 columns are reduced over the wave together: after the exchange over 32 and
//   part       over 16 lanes every group of 16 lanes holds one column's partial sums, four more steps
//              finish all four (7 64-bit exchanges per four columns, not 24), and lanes 0, 16, 32, 48
//              add one column each to its LDS slot: four adds per slot and tile, one per wave.  A wave
//              whose four words per lane are all zero skips the reduction.
// The tile's slots are flushed to coverage[] once.  min_diag masks by index; words with d > j (the
// left-edge triangle), d >= nrows or j >= ncols are never addressed.  Integer adds commute, so the
// result does not depend on the launch geometry or on the order of the atomics.
//
// The kernel accumulates into words of the context (8-byte aligned, cleared here on the same
// stream); the caller's arrays are then written whole by a copy, so they need only be 4-byte aligned
// and need not be cleared.
#include <hip/hip_runtime.h>

#include <limits>

#include "modle_pixels.h"
#include "pixels_context.h"

namespace {

constexpr unsigned kCols = 64;     // columns of one tile
constexpr unsigned kDepth = 256;   // band words (d) of one tile = threads of a workgroup
constexpr unsigned kUnroll = 4;    // columns in flight, reduced together
static_assert(kCols % kUnroll == 0 && kDepth % 64 == 0, "whole groups of columns, whole waves");

// (not a reduction of pixels_device.h: those leave their result in lane 0, and here every lane of a group of 16
// needs it, four columns at a time)
__device__ __forceinline__ unsigned long long xor_lanes(unsigned long long x, int mask) {
  return __shfl_xor(x, mask);
}

__global__ __launch_bounds__(kDepth) void pixels_marginals(const uint32_t* __restrict__ band, uint64_t nrows,
                                                           uint64_t ncols, uint64_t min_diag,
                                                           unsigned long long* __restrict__ diag_sum,
                                                           unsigned long long* __restrict__ coverage) {
  __shared__ unsigned long long row_slots[kCols + kDepth - 1];
  __shared__ unsigned long long col_slots[kCols];
  const uint64_t j0 = static_cast<uint64_t>(blockIdx.x) * kCols;
  const uint64_t d0 = static_cast<uint64_t>(blockIdx.y) * kDepth;
  const unsigned cn = static_cast<unsigned>(min(static_cast<uint64_t>(kCols), ncols - j0));
  const unsigned dn = static_cast<unsigned>(min(static_cast<uint64_t>(kDepth), nrows - d0));
  const unsigned nslots = cn + dn - 1;
  const unsigned dd = threadIdx.x, lane = threadIdx.x & 63;
  const uint64_t d = d0 + dd;
  const bool want_cov = coverage != nullptr;  // (the same in every thread)
  if (want_cov) {
    for (unsigned s = dd; s < nslots; s += kDepth) row_slots[s] = 0;
    if (dd < kCols) col_slots[dd] = 0;
    __syncthreads();
  }
  const bool in_col = d >= min_diag;                                // counted for bin j
  const bool in_row = d >= (min_diag > 1 ? min_diag : uint64_t{1});  // counted for bin j - d
  const bool up32 = (lane & 32) != 0, up16 = (lane & 16) != 0;
  // after the two exchanges a group of 16 lanes holds the column (lane bit 4) * 2 + (lane bit 5)
  const unsigned my_col = ((lane >> 4) & 1) * 2 + (lane >> 5);

  unsigned long long diag = 0;
  for (unsigned jj = 0; jj < cn; jj += kUnroll) {
    uint32_t v[kUnroll];
#pragma unroll
    for (unsigned u = 0; u < kUnroll; ++u) {
      const uint64_t j = j0 + jj + u;
      v[u] = (jj + u < cn && dd < dn && d <= j) ? band[j * nrows + d] : 0u;
    }
#pragma unroll
    for (unsigned u = 0; u < kUnroll; ++u) diag += v[u];
    if (!want_cov) continue;
#pragma unroll
    for (unsigned u = 0; u < kUnroll; ++u)
      if (in_row && v[u] != 0) atomicAdd(&row_slots[jj + u + (dn - 1 - dd)], static_cast<unsigned long long>(v[u]));
    const unsigned long long c0 = in_col ? v[0] : 0u, c1 = in_col ? v[1] : 0u;
    const unsigned long long c2 = in_col ? v[2] : 0u, c3 = in_col ? v[3] : 0u;
    if (__ballot((c0 | c1 | c2 | c3) != 0) == 0) continue;  // (the same in every lane of the wave)
    // lanes 0..31 keep column 0 (2) and hand over column 1 (3); lanes 32..63 the other way round
    const unsigned long long x01 = (up32 ? c1 : c0) + xor_lanes(up32 ? c0 : c1, 32);
    const unsigned long long x23 = (up32 ? c3 : c2) + xor_lanes(up32 ? c2 : c3, 32);
    // lanes with bit 4 clear keep the pair's first column, the others the second
    unsigned long long y = (up16 ? x23 : x01) + xor_lanes(up16 ? x01 : x23, 16);
    y += xor_lanes(y, 8);
    y += xor_lanes(y, 4);
    y += xor_lanes(y, 2);
    y += xor_lanes(y, 1);
    // (a column beyond cn has only zero words: y == 0)
    if ((lane & 15) == 0 && y != 0) atomicAdd(&col_slots[jj + my_col], y);
  }
  // 64 contiguous 64-bit words per wave instruction
  if (diag_sum != nullptr && dd < dn && diag != 0) atomicAdd(&diag_sum[d], diag);
  if (!want_cov) return;
  __syncthreads();
  // row of slot s: j0 - (d0 + dn - 1) + s; the slots of rows below 0 belong to no pixel and hold 0
  const int64_t row0 = static_cast<int64_t>(j0) - static_cast<int64_t>(d0 + dn - 1);
  for (unsigned s = dd; s < nslots; s += kDepth) {
    const unsigned long long c = row_slots[s];
    const int64_t row = row0 + static_cast<int64_t>(s);
    if (c != 0 && row >= 0) atomicAdd(&coverage[row], c);
  }
  if (dd < cn) {
    const unsigned long long c = col_slots[dd];
    if (c != 0) atomicAdd(&coverage[j0 + dd], c);
  }
}

using modle_pixels_detail::set_err;

// Clears the context's nrows + ncols sums (diag_sum first, then coverage) and enqueues the kernel;
// a part that is not wanted is neither cleared nor summed.
int marginals_impl(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows, uint64_t ncols,
                   uint64_t min_diag, bool want_diag, bool want_cov, hipStream_t stream, char* err,
                   size_t errlen) {
  PIX_TRY(hipSetDevice(h->device));
  const int rc = h->marginals.ensure(nrows + ncols, err, errlen);
  if (rc != MODLE_PIXELS_OK) return rc;
  auto* sums = reinterpret_cast<unsigned long long*>(h->marginals.dev);
  if (want_diag) PIX_TRY(hipMemsetAsync(sums, 0, nrows * 8, stream));
  if (want_cov) PIX_TRY(hipMemsetAsync(sums + nrows, 0, ncols * 8, stream));
  const dim3 grid(static_cast<unsigned>((ncols + kCols - 1) / kCols),
                  static_cast<unsigned>((nrows + kDepth - 1) / kDepth));
  hipLaunchKernelGGL(pixels_marginals, grid, dim3(kDepth), 0, stream, d_band, nrows, ncols, min_diag,
                     want_diag ? sums : nullptr, want_cov ? sums + nrows : nullptr);
  PIX_TRY(hipGetLastError());
  return MODLE_PIXELS_OK;
}

// modle_pixels_marginals_to_host (`cs` null) and modle_pixels_coarse_marginals_to_host under their `name`: the
// band resolved, marginals_impl, the copy to the pinned mirror, the wait
int marginals_one_call(const char* name, const modle_pixels_detail::CoarseSpec* cs, modle_pixels_handle* h,
                       const uint32_t* d_band, uint64_t nrows, uint64_t ncols, uint64_t min_diag,
                       const uint64_t** diag_sum, const uint64_t** coverage, void* stream, char* err, size_t errlen) {
  const bool want_diag = diag_sum != nullptr, want_cov = coverage != nullptr;
  if (want_diag) *diag_sum = nullptr;
  if (want_cov) *coverage = nullptr;
  modle_pixels_detail::BandView v;
  if (h == nullptr || (!want_diag && !want_cov) || !modle_pixels_detail::view_shape(d_band, nrows, ncols, cs, &v)) {
    set_err(err, errlen, std::string(name) + ": invalid argument (" + (cs != nullptr ? "factor >= 2, " : "") +
                             "0 < nrows <= ncols, an output)");
    return MODLE_PIXELS_ERR_ARG;
  }
  const hipStream_t st = static_cast<hipStream_t>(stream);
  int rc = modle_pixels_detail::resolve_band(h, d_band, nrows, ncols, cs, &v, st, err, errlen);
  if (rc == MODLE_PIXELS_OK) rc = marginals_impl(h, v.d, v.nrows, v.ncols, min_diag, want_diag, want_cov, st, err, errlen);
  if (rc != MODLE_PIXELS_OK) return rc;
  const uint64_t* dev = h->marginals.dev;
  uint64_t* host = h->marginals.host;
  if (want_diag) PIX_TRY(hipMemcpyAsync(host, dev, v.nrows * 8, hipMemcpyDeviceToHost, st));
  if (want_cov) PIX_TRY(hipMemcpyAsync(host + v.nrows, dev + v.nrows, v.ncols * 8, hipMemcpyDeviceToHost, st));
  PIX_TRY(hipStreamSynchronize(st));
  if (want_diag) *diag_sum = host;
  if (want_cov) *coverage = host + v.nrows;
  return MODLE_PIXELS_OK;
}

}  // namespace

extern "C" int modle_pixels_marginals(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                                      uint64_t ncols, uint64_t min_diag, uint64_t* d_diag_sum,
                                      uint64_t* d_coverage, void* stream, char* err, size_t errlen) {
  if (h == nullptr || d_band == nullptr || nrows == 0 || modle_pixels_detail::bad_shape(nrows, ncols) ||
      (d_diag_sum == nullptr && d_coverage == nullptr) ||
      ((reinterpret_cast<uintptr_t>(d_diag_sum) | reinterpret_cast<uintptr_t>(d_coverage)) & 3) != 0) {
    set_err(err, errlen, "modle_pixels_marginals: invalid argument (0 < nrows <= ncols, an output)");
    return MODLE_PIXELS_ERR_ARG;
  }
  const uint64_t nb = modle_pixels_detail::band_bytes(nrows, ncols);
  // (not any_overlap: the header holds the outputs apart from the band only, not from each other)
  if (modle_pixels_detail::overlap(d_diag_sum, nrows * 8, d_band, nb) ||
      modle_pixels_detail::overlap(d_coverage, ncols * 8, d_band, nb)) {
    set_err(err, errlen, "modle_pixels_marginals: an output overlaps the band");
    return MODLE_PIXELS_ERR_ARG;
  }
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const int rc = marginals_impl(h, d_band, nrows, ncols, min_diag, d_diag_sum != nullptr, d_coverage != nullptr,
                                st, err, errlen);
  if (rc != MODLE_PIXELS_OK) return rc;
  const uint64_t* dev = h->marginals.dev;
  if (d_diag_sum != nullptr) PIX_TRY(hipMemcpyAsync(d_diag_sum, dev, nrows * 8, hipMemcpyDeviceToDevice, st));
  if (d_coverage != nullptr)
    PIX_TRY(hipMemcpyAsync(d_coverage, dev + nrows, ncols * 8, hipMemcpyDeviceToDevice, st));
  return MODLE_PIXELS_OK;
}

extern "C" int modle_pixels_marginals_to_host(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                                              uint64_t ncols, uint64_t min_diag, const uint64_t** diag_sum,
                                              const uint64_t** coverage, void* stream, char* err,
                                              size_t errlen) {
  return marginals_one_call("modle_pixels_marginals_to_host", nullptr, h, d_band, nrows, ncols, min_diag, diag_sum,
                            coverage, stream, err, errlen);
}

extern "C" int modle_pixels_coarse_marginals_to_host(modle_pixels_handle* h, const uint32_t* d_band,
                                                     uint64_t nrows, uint64_t ncols, uint64_t factor,
                                                     uint64_t first_bin, uint64_t min_diag,
                                                     const uint64_t** diag_sum, const uint64_t** coverage,
                                                     void* stream, char* err, size_t errlen) {
  const modle_pixels_detail::CoarseSpec cs{factor, first_bin};
  return marginals_one_call("modle_pixels_coarse_marginals_to_host", &cs, h, d_band, nrows, ncols, min_diag, diag_sum,
                            coverage, stream, err, errlen);
}
