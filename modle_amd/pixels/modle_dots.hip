// modle_dots.hip -- dot calling on a band matrix: the four HiCCUPS neighbourhood sums of every pixel
// and the candidate decision, formed on the MI355X (include/modle_pixels.h: modle_pixels_dots /
// _dots_to_host / _coarse_dots_to_host).
//
// The kernel is output-stationary.  A workgroup of sixteen waves owns the 64 x 64 block of pixels
// (i, j), i0 <= i < i0 + 64, j0 <= j < j0 + 64, in (row, column) coordinates of the symmetric matrix;
// the grid is (column block, D) with i0 = j0 - 64 D, D = 0 .. (nrows + 62) / 64, so that every word
// band[j * nrows + d] -- the left-edge triangle (i < 0) included -- belongs to exactly one block and
// is stored exactly once by it, with a plain store: O_k and obs at a valid pixel, 0 elsewhere.  Only
// the trailing word of d_cand is left to a hipMemsetAsync of the host.  A block without a valid
// pixel stores its zeros and reads nothing.
//
// A block with valid pixels loads its S x S tile, S = 64 + 2 w, of the matrix (cells that are no
// pixels of the band count 0; no valid pixel's square holds one) into LDS as 64-bit words: matrix
// column c over the rows r is one contiguous span of band words with a descending address, so a wave
// reads it with the lanes reversed, 256 contiguous bytes per load, kUnroll loads in flight.  The tile
// becomes a summed-area table A[r + 1][c + 1] = sum of the cells (<= r, <= c), with a zero row and
// column in front: first along r, then along c.  Each pass gives a line to kSeg threads, which scan
// their segments in place, read the totals of the segments before theirs and add them.  The pitch of
// 105 words is odd: lanes on consecutive lines of either pass, a stride of 1 or of 105 64-bit words,
// fall on distinct banks.  Then every lane forms the four sums of its pixels as differences of twelve
// rectangles, decides -- (double)obs >= __dmul_rn((double)O_k, scale[k][d]) for every k and obs >=
// min_count; the only floating point on the device -- and stores.  A wave takes a column of the block
// with the lanes reversed, so its 64 words of d_cand and of each plane of d_sums are contiguous.
//
// LDS: 105 * 105 * 8 = 88 200 bytes, static, whatever w is: one workgroup (16 waves) per CU.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "modle_pixels.h"
#include "pixels_context.h"

namespace {

constexpr int kT = 64;                                   // the block is kT x kT pixels
constexpr int kMaxW = MODLE_PIXELS_MAX_DOT_WINDOW;       // 20
constexpr int kPitch = kT + 2 * kMaxW + 1;               // 105 64-bit words, odd
constexpr unsigned kDotThreads = 1024;                   // 16 waves
constexpr int kDotWaves = kDotThreads / 64;
constexpr int kUnroll = 4;                               // loads a wave keeps in flight
constexpr int kSeg = 8;                                  // threads per line of a scan pass
static_assert(kPitch % 2 == 1, "an odd pitch keeps both passes free of bank conflicts");
static_assert(kSeg * (kT + 2 * kMaxW) <= static_cast<int>(kDotThreads), "a thread per segment");

typedef unsigned long long u64;

// one pass of the summed-area table: line l < S (threads l + S * seg), elements base[e * se], e < S
__device__ __forceinline__ void scan_pass(u64* sat, int S, int line_stride, int se) {
  const int t = static_cast<int>(threadIdx.x);
  const int line = t % S, seg = t / S;
  const int L = (S + kSeg - 1) / kSeg;
  const bool active = seg < kSeg;
  u64* base = sat + kPitch + 1 + line * line_stride;  // cell (0, 0) of the tile is A[1][1]
  const int e0 = min(S, seg * L), e1 = min(S, e0 + L);
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
      const int end = min(S, s * L);  // one past the last element of segment s - 1
      if (end > min(S, (s - 1) * L)) off += base[(end - 1) * se];
    }
  __syncthreads();
  if (active && seg > 0)
    for (int e = e0; e < e1; ++e) base[e * se] += off;
  __syncthreads();
}

__global__ __launch_bounds__(kDotThreads) void pixels_dots(const uint32_t* __restrict__ band, int64_t nrows,
                                                           int64_t ncols, int w, int p, int64_t dlo, int64_t dhi,
                                                           u64 min_count, const double* __restrict__ scale,
                                                           uint32_t* __restrict__ cand, u64* __restrict__ sums) {
  __shared__ u64 sat[kPitch * kPitch];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t j0 = static_cast<int64_t>(blockIdx.x) * kT;
  const int64_t i0 = j0 - static_cast<int64_t>(blockIdx.y) * kT;  // (negative: the left-edge triangle)
  const int64_t dt = j0 - i0;
  const int S = kT + 2 * w;
  // whether the block holds a valid pixel (the same in every lane)
  const bool any = dt + (kT - 1) >= dlo && dt - (kT - 1) <= dhi && i0 + (kT - 1) >= w && j0 + w < ncols;

  if (any) {
    for (int t = threadIdx.x; t <= S; t += kDotThreads) {
      sat[t] = 0;
      sat[t * kPitch] = 0;
    }
    // tile cell (r, c) is matrix cell (i0 - w + r, j0 - w + c); lane <-> r descending, d ascending
    const int nchunk = (S + 63) / 64;
    const int items = S * nchunk;
    for (int it0 = wv * kUnroll; it0 < items; it0 += kDotWaves * kUnroll) {
      uint32_t v[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int it = it0 + u;
        const int c = it / nchunk, r = S - 1 - ((it % nchunk) * 64 + lane);
        const int64_t R = i0 - w + r, Cc = j0 - w + c, d = Cc - R;
        v[u] = (it < items && r >= 0 && R >= 0 && Cc < ncols && d >= 0 && d < nrows) ? band[Cc * nrows + d] : 0u;
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int it = it0 + u;
        const int c = it / nchunk, r = S - 1 - ((it % nchunk) * 64 + lane);
        if (it < items && r >= 0) sat[(r + 1) * kPitch + (c + 1)] = v[u];
      }
    }
    __syncthreads();
    scan_pass(sat, S, 1, kPitch);  // along r, a line per c
    scan_pass(sat, S, kPitch, 1);  // along c, a line per r
  }

  const uint64_t plane = static_cast<uint64_t>(nrows) * static_cast<uint64_t>(ncols);
  // the sum of the tile cells [ra, rb] x [ca, cb]; an empty range (rb == ra - 1, cb == ca - 1) gives 0
  auto rect = [&](int ra, int rb, int ca, int cb) -> u64 {
    return sat[(rb + 1) * kPitch + (cb + 1)] - sat[ra * kPitch + (cb + 1)] - sat[(rb + 1) * kPitch + ca] +
           sat[ra * kPitch + ca];
  };
  for (int jj = wv; jj < kT; jj += kDotWaves) {
    const int ii = kT - 1 - lane;
    const int64_t i = i0 + ii, j = j0 + jj, d = j - i;
    if (j >= ncols || d < 0 || d >= nrows) continue;  // no word of the band
    const uint64_t word = static_cast<uint64_t>(j) * static_cast<uint64_t>(nrows) + static_cast<uint64_t>(d);
    u64 o0 = 0, o1 = 0, o2 = 0, o3 = 0;
    uint32_t keep = 0;
    if (any && i >= w && j + w < ncols && d >= dlo && d <= dhi) {
      const int r = w + ii, c = w + jj;
      o0 = rect(r - w, r + w, c - w, c + w) - rect(r - p, r + p, c - p, c + p) - rect(r, r, c - w, c - p - 1) -
           rect(r, r, c + p + 1, c + w) - rect(r - w, r - p - 1, c, c) - rect(r + p + 1, r + w, c, c);
      o1 = rect(r + 1, r + w, c - w, c - 1) - rect(r + 1, r + p, c - p, c - 1);
      o2 = rect(r - 1, r + 1, c - w, c - p - 1) + rect(r - 1, r + 1, c + p + 1, c + w);
      o3 = rect(r - w, r - p - 1, c - 1, c + 1) + rect(r + p + 1, r + w, c - 1, c + 1);
      if (cand != nullptr) {
        const uint32_t obs = static_cast<uint32_t>(rect(r, r, c, c));
        const double x = static_cast<double>(obs);
        const bool is = obs >= min_count && x >= __dmul_rn(static_cast<double>(o0), scale[d]) &&
                        x >= __dmul_rn(static_cast<double>(o1), scale[nrows + d]) &&
                        x >= __dmul_rn(static_cast<double>(o2), scale[2 * nrows + d]) &&
                        x >= __dmul_rn(static_cast<double>(o3), scale[3 * nrows + d]);
        keep = is ? obs : 0u;
      }
    }
    if (cand != nullptr) cand[word] = keep;
    if (sums != nullptr) {
      sums[word] = o0;
      sums[plane + word] = o1;
      sums[2 * plane + word] = o2;
      sums[3 * plane + word] = o3;
    }
  }
}

using modle_pixels_detail::bad_pixel_outputs;
using modle_pixels_detail::overlap;
using modle_pixels_detail::set_err;

constexpr const char* kRule =
    "(0 < nrows <= ncols, 0 <= p < w <= 20, 4 * w + 1 + min_diag <= nrows, min_count >= 1, a scale table "
    "without NaN or negative entries at the valid diagonals (it may be null without d_cand), at least one output, "
    "d_sums 8-byte aligned)";

// what the arguments alone refuse (no pointer to device memory is looked at)
bool bad_dots(uint64_t nrows, uint64_t ncols, uint64_t w, uint64_t p, uint64_t min_diag, uint64_t min_count,
              const double* scale, bool need_scale) {
  if (nrows == 0 || modle_pixels_detail::bad_shape(nrows, ncols) || (need_scale && scale == nullptr) || w == 0 ||
      w > MODLE_PIXELS_MAX_DOT_WINDOW || p >= w || min_count == 0 || min_diag > nrows || 4 * w + 1 + min_diag > nrows ||
      (nrows + kT - 2) / kT + 1 > 65535)
    return true;
  for (uint64_t k = 0; k < 4 && scale != nullptr; ++k)
    for (uint64_t d = 2 * w + min_diag; d + 2 * w < nrows; ++d) {
      const double s = scale[k * nrows + d];
      if (std::isnan(s) || s < 0.0) return true;
    }
  return false;
}

// enqueues the table's copy, the clearing of the trailing word and the kernel on checked arguments
int dots_impl(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows, uint64_t ncols, uint64_t w, uint64_t p,
              uint64_t min_diag, uint64_t min_count, const double* scale, uint32_t* d_cand, uint64_t* d_sums,
              hipStream_t stream, char* err, size_t errlen) {
  PIX_TRY(hipSetDevice(h->device));
  const uint64_t dlo = 2 * w + min_diag, dhi = nrows - 1 - 2 * w;  // dlo <= dhi by the acceptance rule
  if (d_cand != nullptr) {
    // the pinned copy of the table may still feed the copy of the call before
    if (h->dot_scale_copied == nullptr)
      PIX_TRY(hipEventCreateWithFlags(&h->dot_scale_copied, hipEventDisableTiming));
    else
      PIX_TRY(hipEventSynchronize(h->dot_scale_copied));
    const int rc = h->dot_scale.ensure(4 * nrows, err, errlen);
    if (rc != MODLE_PIXELS_OK) return rc;
    for (uint64_t k = 0; k < 4; ++k)
      for (uint64_t d = 0; d < nrows; ++d)
        h->dot_scale.host[k * nrows + d] = (d >= dlo && d <= dhi) ? scale[k * nrows + d] : 0.0;
    PIX_TRY(hipMemcpyAsync(h->dot_scale.dev, h->dot_scale.host, 4 * nrows * sizeof(double), hipMemcpyHostToDevice,
                           stream));
    PIX_TRY(hipEventRecord(h->dot_scale_copied, stream));
    PIX_TRY(hipMemsetAsync(d_cand + nrows * ncols, 0, 4, stream));  // the trailing word: no block owns it
  }
  const dim3 grid(static_cast<unsigned>((ncols + kT - 1) / kT), static_cast<unsigned>((nrows + kT - 2) / kT + 1));
  hipLaunchKernelGGL(pixels_dots, grid, dim3(kDotThreads), 0, stream, d_band, static_cast<int64_t>(nrows),
                     static_cast<int64_t>(ncols), static_cast<int>(w), static_cast<int>(p), static_cast<int64_t>(dlo),
                     static_cast<int64_t>(dhi), static_cast<u64>(min_count),
                     d_cand != nullptr ? h->dot_scale.dev : nullptr, d_cand, reinterpret_cast<u64*>(d_sums));
  PIX_TRY(hipGetLastError());
  return MODLE_PIXELS_OK;
}

// the candidates of the band `d_band` into the scratch band of the context, then count / scan / extract
int dots_to_host(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows, uint64_t ncols, uint64_t w,
                 uint64_t p, uint64_t min_diag, uint64_t min_count, const double* scale, int64_t bin_offset,
                 const int64_t** bin1, const int64_t** bin2, const int32_t** count, const int64_t** bin1_offset,
                 modle_pixels_stats* stats, hipStream_t stream, char* err, size_t errlen) {
  PIX_TRY(hipSetDevice(h->device));
  int rc = h->dot_cand.ensure(nrows * ncols + 1, err, errlen);
  if (rc != MODLE_PIXELS_OK) return rc;
  rc = dots_impl(h, d_band, nrows, ncols, w, p, min_diag, min_count, scale, h->dot_cand.dev, nullptr, stream, err,
                 errlen);
  if (rc != MODLE_PIXELS_OK) return rc;
  return modle_pixels_detail::to_host(h, h->dot_cand.dev, nrows, ncols, bin_offset, bin1, bin2, count, bin1_offset,
                                      stats, stream, err, errlen);
}

}  // namespace

extern "C" int modle_pixels_dots(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows, uint64_t ncols,
                                 uint64_t w, uint64_t p, uint64_t min_diag, uint64_t min_count, const double* scale,
                                 uint32_t* d_cand, uint64_t* d_sums, void* stream, char* err, size_t errlen) {
  if (h == nullptr || d_band == nullptr || (d_cand == nullptr && d_sums == nullptr) ||
      (reinterpret_cast<uintptr_t>(d_sums) & 7) != 0 || bad_dots(nrows, ncols, w, p, min_diag, min_count, scale, d_cand != nullptr)) {
    set_err(err, errlen, std::string("modle_pixels_dots: invalid argument ") + kRule);
    return MODLE_PIXELS_ERR_ARG;
  }
  const uint64_t nb = modle_pixels_detail::band_bytes(nrows, ncols), ns = nrows * ncols * 32;
  if ((d_cand != nullptr && overlap(d_cand, nb, d_band, nb)) || (d_sums != nullptr && overlap(d_sums, ns, d_band, nb)) ||
      (d_cand != nullptr && d_sums != nullptr && overlap(d_cand, nb, d_sums, ns))) {
    set_err(err, errlen, "modle_pixels_dots: an output overlaps the band or the other output");
    return MODLE_PIXELS_ERR_ARG;
  }
  return dots_impl(h, d_band, nrows, ncols, w, p, min_diag, min_count, scale, d_cand, d_sums,
                   static_cast<hipStream_t>(stream), err, errlen);
}

extern "C" int modle_pixels_dots_to_host(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                                         uint64_t ncols, uint64_t w, uint64_t p, uint64_t min_diag,
                                         uint64_t min_count, const double* scale, int64_t bin_offset,
                                         const int64_t** bin1, const int64_t** bin2, const int32_t** count,
                                         const int64_t** bin1_offset, modle_pixels_stats* stats, void* stream,
                                         char* err, size_t errlen) {
  if (h == nullptr || d_band == nullptr || bad_pixel_outputs(bin1, bin2, count, bin1_offset, stats, bin_offset) ||
      bad_dots(nrows, ncols, w, p, min_diag, min_count, scale, true)) {
    set_err(err, errlen, std::string("modle_pixels_dots_to_host: invalid argument ") + kRule);
    return MODLE_PIXELS_ERR_ARG;
  }
  return dots_to_host(h, d_band, nrows, ncols, w, p, min_diag, min_count, scale, bin_offset, bin1, bin2, count,
                      bin1_offset, stats, static_cast<hipStream_t>(stream), err, errlen);
}

extern "C" int modle_pixels_coarse_dots_to_host(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                                                uint64_t ncols, uint64_t factor, uint64_t first_bin, uint64_t w,
                                                uint64_t p, uint64_t min_diag, uint64_t min_count,
                                                const double* scale, int64_t bin_offset, const int64_t** bin1,
                                                const int64_t** bin2, const int32_t** count,
                                                const int64_t** bin1_offset, modle_pixels_stats* stats,
                                                void* stream, char* err, size_t errlen) {
  uint64_t nr = 0, nc = 0;
  // (modle_pixels_coarse_shape refuses what modle_pixels_coarsen refuses of shape and factor)
  if (h == nullptr || d_band == nullptr || bad_pixel_outputs(bin1, bin2, count, bin1_offset, stats, bin_offset) ||
      modle_pixels_coarse_shape(nrows, ncols, factor, first_bin, &nr, &nc) != MODLE_PIXELS_OK ||
      bad_dots(nr, nc, w, p, min_diag, min_count, scale, true)) {
    set_err(err, errlen, std::string("modle_pixels_coarse_dots_to_host: invalid argument (factor >= 2; of the "
                                     "coarse band:) ") + kRule);
    return MODLE_PIXELS_ERR_ARG;
  }
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const int rc = modle_pixels_detail::coarsen_to_scratch(h, d_band, nrows, ncols, factor, first_bin, nr, nc, st, err,
                                                         errlen);
  if (rc != MODLE_PIXELS_OK) return rc;
  return dots_to_host(h, h->coarse.dev, nr, nc, w, p, min_diag, min_count, scale, bin_offset, bin1, bin2, count,
                      bin1_offset, stats, st, err, errlen);
}
