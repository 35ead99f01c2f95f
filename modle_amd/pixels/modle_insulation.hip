// modle_insulation.hip -- the insulation sums of a band matrix, formed on the MI355X
// (include/modle_pixels.h: modle_pixels_insulation / _insulation_to_host / _coarse_insulation_to_host,
// and the host-only modle_pixels_insulation_n_valid).
//
// ins_sum[k][b] is the sum of the pixels (a, c) with b - w_k + 1 <= a <= b <= c <= b + w_k - 1 and
// c - a >= min_diag.  In band coordinates column j = b + t (0 <= t < w) gives bin b the contiguous words
// d in [max(t, min_diag), min(t + w - 1, j)]: with the exclusive prefix sums P_j of the column that is
// P_j[min(t + w - 1, j) + 1] - P_j[max(t, min_diag)], and one prefix serves every window of the call.
//
// The kernel is output-stationary.  A workgroup of four waves owns the 64 bins b0 .. b0 + 63 for all
// windows; lane i of every wave stands for bin b0 + i and keeps that bin's sums, one per window, in
// registers.  The waves take the columns j = b0 .. min(b0 + 62 + wmax, ncols - 1) in turn.  Of a column
// a wave reads only the words some window still needs, d <= min(j - b0, w - 1) + w - 1 over the windows
// with w > j - b0 - 63, in memory order (64 lanes, 256 contiguous bytes per load, four loads in
// flight), forms their 64-bit prefix sums with a wave scan carried across the chunks and leaves them in
// its own LDS row of 2 * wmax words.  Then every lane takes, per window, the two words of the row that
// bound its bin's span of this column (t = j - b0 - lane; lanes with t < 0 or t >= w sit out) and adds
// their difference to its register: one lane per bin, so there are no atomics, in LDS or in memory.
// At the end the four waves' registers meet in LDS (the rows are free by then) and every output word
// out[k][b] is stored once, by one lane, with a plain store: nothing is cleared beforehand and nothing
// depends on the launch geometry.  min_diag masks by index; words with d > j (the left-edge triangle),
// d >= nrows or j >= ncols are never addressed (2 * wmax - 1 <= nrows is checked by the host).
//
// LDS: max(4 rows * 2 * wmax, 4 waves * n_windows * 64) 64-bit words, dynamic: 64 KiB at the cap of
// 1024 bins (two workgroups = 8 waves on a CU's 160 KiB), 19 KiB at 300 bins (eight workgroups).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "modle_pixels.h"
#include "pixels_context.h"
#include "pixels_device.h"

namespace {

using modle_pixels_device::wave_last;
using modle_pixels_device::wave_scan;

constexpr unsigned kBins = 64;    // bins of one workgroup = lanes of a wave
constexpr unsigned kWaves = 4;    // waves of a workgroup, each with an LDS row of its own
constexpr unsigned kUnroll = 4;   // chunks of 64 words in flight
constexpr unsigned kMaxWindows = MODLE_PIXELS_MAX_WINDOWS;
static_assert(kMaxWindows == 8, "the kernel unrolls its windows into 8 registers");

struct Windows {
  uint32_t w[kMaxWindows];
};

// what orders a wave's LDS stores and loads of its own row for the compiler; the LDS itself serves
// the instructions of one wave in order
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(kBins * kWaves) void pixels_insulation(const uint32_t* __restrict__ band, uint64_t nrows,
                                                                    uint64_t ncols, Windows win, unsigned nw,
                                                                    unsigned wmax, unsigned min_diag,
                                                                    unsigned long long* __restrict__ out) {
  extern __shared__ unsigned long long lds[];
  const unsigned lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint64_t b0 = static_cast<uint64_t>(blockIdx.x) * kBins;
  unsigned long long* row = lds + static_cast<size_t>(wv) * (2 * wmax);  // P[0 .. 2 * wmax - 1]
  unsigned long long acc[kMaxWindows];
#pragma unroll
  for (unsigned k = 0; k < kMaxWindows; ++k) acc[k] = 0;

  // columns b0 + jj, jj < jn (at most 63 + wmax)
  const unsigned jn = static_cast<unsigned>(min(static_cast<uint64_t>(kBins - 1 + wmax), ncols - b0));
  for (unsigned jj = wv; jj < jn; jj += kWaves) {  // (the same in every lane of the wave)
    const uint64_t j = b0 + jj;
    // the bins of this workgroup that column j serves have t = jj - lane in [tmin, jj]
    const unsigned tmin = jj > kBins - 1 ? jj - (kBins - 1) : 0;
    unsigned top = 0;  // the deepest word a window still needs (wmax always does: tmin < wmax)
#pragma unroll
    for (unsigned k = 0; k < kMaxWindows; ++k)
      if (k < nw && win.w[k] > tmin) top = max(top, min(jj, win.w[k] - 1) + win.w[k] - 1);
    const unsigned dn = static_cast<unsigned>(min(static_cast<uint64_t>(top), j)) + 1;  // words d < dn <= 2 * wmax - 1
    const uint32_t* col = band + j * nrows;

    wave_sync();  // the row's readers of the column before are done
    if (lane == 0) row[0] = 0;
    unsigned long long carry = 0;
    // (modle_profiles.hip has a loop like this one; only the scan inside is shared: there the prefix is picked
    // at cut points by a shuffle, here every word of it goes to the LDS row)
    for (unsigned c0 = 0; c0 < dn; c0 += kUnroll * 64) {
      uint32_t v[kUnroll];
#pragma unroll
      for (unsigned u = 0; u < kUnroll; ++u) {
        const unsigned d = c0 + u * 64 + lane;
        v[u] = d < dn ? col[d] : 0u;
      }
#pragma unroll
      for (unsigned u = 0; u < kUnroll; ++u) {
        if (c0 + u * 64 >= dn) break;  // (the same in every lane)
        const unsigned long long x = wave_scan(v[u], lane);
        const unsigned d = c0 + u * 64 + lane;
        if (d < dn) row[d + 1] = carry + x;
        carry += wave_last(x);
      }
    }
    wave_sync();  // the row is whole

    const int t = static_cast<int>(jj) - static_cast<int>(lane);  // bin b0 + lane
#pragma unroll
    for (unsigned k = 0; k < kMaxWindows; ++k) {
      if (k >= nw) break;
      const unsigned w = win.w[k];
      if (t < 0 || static_cast<unsigned>(t) >= w) continue;
      const unsigned lo = max(static_cast<unsigned>(t), min_diag);
      const unsigned hi = static_cast<unsigned>(min(static_cast<uint64_t>(t + w - 1), j));  // < dn
      if (lo <= hi) acc[k] += row[hi + 1] - row[lo];
    }
  }

  // the four waves' sums meet in LDS; every output word is stored once
  __syncthreads();
#pragma unroll
  for (unsigned k = 0; k < kMaxWindows; ++k)
    if (k < nw) lds[(wv * nw + k) * kBins + lane] = acc[k];
  __syncthreads();
  for (unsigned s = threadIdx.x; s < nw * kBins; s += kBins * kWaves) {
    const uint64_t b = b0 + (s & (kBins - 1));
    if (b >= ncols) continue;
    unsigned long long sum = 0;
#pragma unroll
    for (unsigned x = 0; x < kWaves; ++x) sum += lds[x * nw * kBins + s];
    out[static_cast<uint64_t>(s / kBins) * ncols + b] = sum;
  }
}

using modle_pixels_detail::set_err;

// the windows the kernel accepts on a band of `nrows`: the whole diamond lies in the band
bool bad_windows(const uint64_t* windows, uint64_t n_windows, uint64_t nrows) {
  if (windows == nullptr || n_windows == 0 || n_windows > kMaxWindows) return true;
  for (uint64_t k = 0; k < n_windows; ++k)
    if (windows[k] == 0 || windows[k] > MODLE_PIXELS_MAX_WINDOW || 2 * windows[k] - 1 > nrows) return true;
  return false;
}

constexpr const char* kRule =
    "(0 < nrows <= ncols, 1..8 windows with 2 * w - 1 <= nrows and w <= 1024, an 8-byte aligned output)";

// enqueues the kernel on checked arguments
int insulation_impl(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows, uint64_t ncols,
                    const uint64_t* windows, uint64_t n_windows, uint64_t min_diag, uint64_t* d_out,
                    hipStream_t stream, char* err, size_t errlen) {
  PIX_TRY(hipSetDevice(h->device));
  Windows win{};
  unsigned wmax = 0;
  for (uint64_t k = 0; k < n_windows; ++k) {
    win.w[k] = static_cast<uint32_t>(windows[k]);
    wmax = std::max(wmax, win.w[k]);
  }
  const unsigned nw = static_cast<unsigned>(n_windows);
  const size_t words = std::max<size_t>(size_t{kWaves} * 2 * wmax, size_t{kWaves} * nw * kBins);
  // (a min_diag beyond every span masks everything, like any larger one)
  const unsigned md = static_cast<unsigned>(std::min<uint64_t>(min_diag, 2 * uint64_t{wmax}));
  const dim3 grid(static_cast<unsigned>((ncols + kBins - 1) / kBins));
  hipLaunchKernelGGL(pixels_insulation, grid, dim3(kBins * kWaves), words * 8, stream, d_band, nrows, ncols, win,
                     nw, wmax, md, reinterpret_cast<unsigned long long*>(d_out));
  PIX_TRY(hipGetLastError());
  return MODLE_PIXELS_OK;
}

// modle_pixels_insulation_to_host (`cs` null) and modle_pixels_coarse_insulation_to_host under their `name`: the
// band resolved, insulation_impl into the sums of the context, their copy to the pinned mirror, the wait
int insulation_one_call(const char* name, const modle_pixels_detail::CoarseSpec* cs, modle_pixels_handle* h,
                        const uint32_t* d_band, uint64_t nrows, uint64_t ncols, const uint64_t* windows,
                        uint64_t n_windows, uint64_t min_diag, const uint64_t** ins_sum, void* stream, char* err,
                        size_t errlen) {
  if (ins_sum != nullptr) *ins_sum = nullptr;
  modle_pixels_detail::BandView v;
  if (h == nullptr || ins_sum == nullptr || !modle_pixels_detail::view_shape(d_band, nrows, ncols, cs, &v) ||
      bad_windows(windows, n_windows, v.nrows)) {
    set_err(err, errlen, modle_pixels_detail::refusal(name, cs, kRule));
    return MODLE_PIXELS_ERR_ARG;
  }
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const int rc = modle_pixels_detail::resolve_band(h, d_band, nrows, ncols, cs, &v, st, err, errlen);
  if (rc != MODLE_PIXELS_OK) return rc;
  return modle_pixels_detail::sums_to_host(h, n_windows * v.ncols, ins_sum, st, err, errlen, [&](uint64_t* d_out) {
    return insulation_impl(h, v.d, v.nrows, v.ncols, windows, n_windows, min_diag, d_out, st, err, errlen);
  });
}

}  // namespace

extern "C" int modle_pixels_insulation_n_valid(uint64_t ncols, uint64_t window, uint64_t min_diag,
                                               uint64_t* n_valid) {
  if (n_valid == nullptr || window == 0 || window > MODLE_PIXELS_MAX_WINDOW) return MODLE_PIXELS_ERR_ARG;
  for (uint64_t b = 0; b < ncols; ++b) {
    const uint64_t na = std::min(window, b + 1), nc = std::min(window, ncols - b);
    uint64_t cut = 0;  // the pairs (p, q), p < na, q < nc, with p + q < min_diag
    for (uint64_t p = 0; p < na && p < min_diag; ++p) cut += std::min(nc, min_diag - p);
    n_valid[b] = na * nc - cut;
  }
  return MODLE_PIXELS_OK;
}

extern "C" int modle_pixels_insulation(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                                       uint64_t ncols, const uint64_t* windows, uint64_t n_windows,
                                       uint64_t min_diag, uint64_t* d_out, uint64_t out_words, void* stream,
                                       char* err, size_t errlen) {
  if (h == nullptr || d_band == nullptr || d_out == nullptr || nrows == 0 ||
      modle_pixels_detail::bad_shape(nrows, ncols) || bad_windows(windows, n_windows, nrows) ||
      out_words < n_windows * ncols || (reinterpret_cast<uintptr_t>(d_out) & 7) != 0) {
    set_err(err, errlen, std::string("modle_pixels_insulation: invalid argument ") + kRule);
    return MODLE_PIXELS_ERR_ARG;
  }
  if (modle_pixels_detail::overlap(d_out, n_windows * ncols * 8, d_band,
                                   modle_pixels_detail::band_bytes(nrows, ncols))) {
    set_err(err, errlen, "modle_pixels_insulation: the output overlaps the band");
    return MODLE_PIXELS_ERR_ARG;
  }
  return insulation_impl(h, d_band, nrows, ncols, windows, n_windows, min_diag, d_out,
                         static_cast<hipStream_t>(stream), err, errlen);
}

extern "C" int modle_pixels_insulation_to_host(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                                               uint64_t ncols, const uint64_t* windows, uint64_t n_windows,
                                               uint64_t min_diag, const uint64_t** ins_sum, void* stream,
                                               char* err, size_t errlen) {
  return insulation_one_call("modle_pixels_insulation_to_host", nullptr, h, d_band, nrows, ncols, windows, n_windows,
                             min_diag, ins_sum, stream, err, errlen);
}

extern "C" int modle_pixels_coarse_insulation_to_host(modle_pixels_handle* h, const uint32_t* d_band,
                                                      uint64_t nrows, uint64_t ncols, uint64_t factor,
                                                      uint64_t first_bin, const uint64_t* windows,
                                                      uint64_t n_windows, uint64_t min_diag,
                                                      const uint64_t** ins_sum, void* stream, char* err,
                                                      size_t errlen) {
  const modle_pixels_detail::CoarseSpec cs{factor, first_bin};
  return insulation_one_call("modle_pixels_coarse_insulation_to_host", &cs, h, d_band, nrows, ncols, windows,
                             n_windows, min_diag, ins_sum, stream, err, errlen);
}
