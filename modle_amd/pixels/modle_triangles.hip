// modle_triangles.hip -- the triangle sums of every window on the diagonal, formed on the MI355X
// (include/modle_pixels.h: modle_pixels_triangles / _triangles_to_host / _coarse_triangles_to_host, and the
// host-only modle_pixels_triangle_cells).
//
// For start s < ncols and k < W = max_width the library writes
//   T[k][s] = sum of M(a, c) over s <= a <= c < min(s + k + 1, ncols), c - a >= d0
// into out[W][ncols]: the upper triangle of the window of k + 1 bins that starts at bin s, what every
// dynamic-programming domain caller scores.  With the prefix of band column j,
//   P(j, k) = sum over d0 <= d <= k of band[j * nrows + d]     (contiguous words; 0 for j >= ncols),
// the window of k + 1 bins is the window of k bins and the part of column s + k above row s:
//   T[k][s] = T[k - 1][s] + P(s + k, k).
// So T is the prefix along k of the column prefixes read along matrix rows, and two kernels form it in the
// output itself, both output-stationary: a word has one owner, nothing is cleared beforehand, there are no
// atomics, no scratch memory, and no result depends on the launch.
//
//   columns  a workgroup of one wave owns the 64 columns c0 .. c0 + 63 and walks the depth in chunks of 64
//            diagonals.  Of every column it reads the chunk's 64 contiguous words, one per lane (8 loads in
//            flight), into a 64 x 64 tile of LDS; then lane l stands for column c0 + l, adds the tile's row l
//            word by word to the column's running prefix, which it keeps in a register from chunk to chunk,
//            and stores P(c, d) at out[d][c - d]: for one d the 64 lanes store 64 consecutive words.  The
//            columns ncols .. ncols + W - 2 do not exist; their owners store the zeros of the windows that the
//            chromosome's end clips, so that every word of the output has exactly one writer here.  The
//            words d > c (the left-edge triangle), d < d0 and d >= W are never addressed.
//   walk     one lane per start s walks k upwards in place, out[k][s] += out[k - 1][s], 16 loads in flight;
//            neighbouring lanes are on neighbouring words.  A word is read and then stored by the same lane.
//
// Traffic: the band once, the table written, read and written again.
//
// LDS of `columns`: the tile is 64 rows of 65 uint32 (16.25 KiB, static).  A row is written by ds_write_b32 at
// 64 consecutive words and read down a column at a stride of 65 words: bank (65 l + r) mod 32 = (l + r) mod 32
// is different for the 32 lanes of either half, so neither side has a bank conflict.  (An 8-byte tile of
// prefixes turned after a wave scan would need a stride that is odd in 8-byte units and twice the LDS.)  Nine
// workgroups = nine waves fit a CU's 160 KiB; a chr1-sized band (49 792 columns) has 788 workgroups, three to a
// CU.  `walk` uses no LDS.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "modle_pixels.h"
#include "pixels_context.h"
#include "pixels_device.h"

namespace {

using modle_pixels_device::grid_of;
using modle_pixels_device::group_id;
using modle_pixels_device::u64;

constexpr unsigned kCols = 64;         // columns of a workgroup of `columns` = lanes of its wave
constexpr unsigned kStride = kCols + 1;  // words of a tile row
constexpr unsigned kLoads = 8;         // loads in flight per lane of `columns`
constexpr unsigned kWalk = 16;         // loads in flight per lane of `walk`
constexpr u64 kMaxWidth = MODLE_PIXELS_MAX_TRIANGLE_WIDTH;
// W (W + 1) / 2 pixels below 2^32 stay below 2^64
static_assert(kMaxWidth * (kMaxWidth + 1) / 2 <= 0xFFFFFFFFFFFFFFFFull / 0xFFFFFFFFull, "the sums must not wrap");

// out[d][c - d] = P(c, d) for the columns c of the workgroup, 0 <= c - d < ncols, d < W
__global__ __launch_bounds__(kCols) void triangles_columns(const uint32_t* __restrict__ band, u64 nrows, u64 ncols,
                                                           unsigned W, unsigned d0, u64 groups,
                                                           u64* __restrict__ out) {
  __shared__ uint32_t tile[kCols * kStride];  // [column][diagonal of the chunk]
  const unsigned lane = threadIdx.x;
  const u64 g = group_id();
  if (g >= groups) return;  // (the same in every lane)
  const u64 c0 = g * kCols;
  const u64 c = c0 + lane;  // the column this lane keeps the prefix of
  u64 run = 0;
  for (unsigned k0 = 0; k0 < W; k0 += kCols) {  // (the same in every lane)
    const unsigned d = k0 + lane;
    if (k0 + kCols > d0) {  // a chunk below d0 holds zeros only: nothing is read
#pragma unroll 1
      for (unsigned i0 = 0; i0 < kCols; i0 += kLoads) {
        uint32_t v[kLoads];
#pragma unroll
        for (unsigned u = 0; u < kLoads; ++u) {
          const u64 j = c0 + i0 + u;
          // a pixel of the band: j < ncols, d <= j, d < W <= nrows
          const bool ok = j < ncols && d >= d0 && d < W && d <= j;
          v[u] = ok ? band[j * nrows + d] : 0u;
        }
#pragma unroll
        for (unsigned u = 0; u < kLoads; ++u) tile[(i0 + u) * kStride + lane] = v[u];
      }
    }
    __syncthreads();
    const unsigned top = min(kCols, W - k0);
    if (k0 + kCols > d0) {
#pragma unroll 4
      for (unsigned r = 0; r < top; ++r) {
        run += tile[lane * kStride + r];
        const u64 s = c - (k0 + r);  // (wraps below 0: not < ncols)
        if (s < ncols) out[static_cast<u64>(k0 + r) * ncols + s] = run;
      }
    } else {
      for (unsigned r = 0; r < top; ++r) {
        const u64 s = c - (k0 + r);
        if (s < ncols) out[static_cast<u64>(k0 + r) * ncols + s] = 0;
      }
    }
    __syncthreads();
  }
}

// out[k][s] += out[k - 1][s], k upwards
__global__ __launch_bounds__(64) void triangles_walk(u64 ncols, unsigned W, u64 groups, u64* __restrict__ out) {
  const u64 g = group_id();
  if (g >= groups) return;
  const u64 s = g * 64 + threadIdx.x;
  if (s >= ncols) return;
  u64 run = 0;
  for (unsigned k0 = 0; k0 < W; k0 += kWalk) {
    u64 v[kWalk];
#pragma unroll
    for (unsigned u = 0; u < kWalk; ++u) v[u] = k0 + u < W ? out[static_cast<u64>(k0 + u) * ncols + s] : 0;
#pragma unroll
    for (unsigned u = 0; u < kWalk; ++u) {
      run += v[u];
      if (k0 + u < W) out[static_cast<u64>(k0 + u) * ncols + s] = run;
    }
  }
}

using modle_pixels_detail::set_err;

constexpr const char* kRule =
    "(no null pointer, 0 < nrows <= ncols, 1 <= max_width <= nrows, max_width <= 65535 "
    "(MODLE_PIXELS_MAX_TRIANGLE_WIDTH), out_words >= max_width * ncols, an 8-byte aligned output)";

// what every entry point refuses of the width on a band of `nrows`
bool bad_width(uint64_t nrows, uint64_t max_width) {
  return max_width == 0 || max_width > nrows || max_width > kMaxWidth;
}

// enqueues the kernels on checked arguments
int triangles_impl(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows, uint64_t ncols, uint64_t max_width,
                   uint64_t min_diag, uint64_t* d_out, hipStream_t stream, char* err, size_t errlen) {
  PIX_TRY(hipSetDevice(h->device));
  const unsigned W = static_cast<unsigned>(max_width);
  const unsigned d0 = static_cast<unsigned>(std::min<uint64_t>(min_diag, max_width));  // (d0 >= W: zeros, like W)
  u64* out = reinterpret_cast<u64*>(d_out);
  const uint64_t col_groups = (ncols + W - 1 + kCols - 1) / kCols;  // the columns 0 .. ncols + W - 2
  hipLaunchKernelGGL(triangles_columns, grid_of(col_groups), dim3(kCols), 0, stream, d_band, nrows, ncols, W, d0,
                     col_groups, out);
  PIX_TRY(hipGetLastError());
  const uint64_t walk_groups = (ncols + 63) / 64;
  hipLaunchKernelGGL(triangles_walk, grid_of(walk_groups), dim3(64), 0, stream, ncols, W, walk_groups, out);
  PIX_TRY(hipGetLastError());
  return MODLE_PIXELS_OK;
}

// modle_pixels_triangles_to_host (`cs` null) and modle_pixels_coarse_triangles_to_host under their `name`: the
// band resolved, triangles_impl into the sums of the context, their copy to the pinned mirror, the wait
int triangles_one_call(const char* name, const modle_pixels_detail::CoarseSpec* cs, modle_pixels_handle* h,
                       const uint32_t* d_band, uint64_t nrows, uint64_t ncols, uint64_t max_width, uint64_t min_diag,
                       const uint64_t** table, void* stream, char* err, size_t errlen) {
  if (table != nullptr) *table = nullptr;
  modle_pixels_detail::BandView v;
  if (h == nullptr || table == nullptr || !modle_pixels_detail::view_shape(d_band, nrows, ncols, cs, &v) ||
      bad_width(v.nrows, max_width)) {
    set_err(err, errlen, modle_pixels_detail::refusal(name, cs, kRule));
    return MODLE_PIXELS_ERR_ARG;
  }
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const int rc = modle_pixels_detail::resolve_band(h, d_band, nrows, ncols, cs, &v, st, err, errlen);
  if (rc != MODLE_PIXELS_OK) return rc;
  return modle_pixels_detail::sums_to_host(h, max_width * v.ncols, table, st, err, errlen, [&](uint64_t* d_out) {
    return triangles_impl(h, v.d, v.nrows, v.ncols, max_width, min_diag, d_out, st, err, errlen);
  });
}

}  // namespace

extern "C" int modle_pixels_triangle_cells(uint64_t ncols, uint64_t max_width, uint64_t min_diag, uint64_t* cells) {
  if (cells == nullptr || max_width == 0 || max_width > kMaxWidth) return MODLE_PIXELS_ERR_ARG;
  for (uint64_t k = 0; k < max_width; ++k)
    for (uint64_t s = 0; s < ncols; ++s) {
      const uint64_t w = std::min(k + 1, ncols - s);
      cells[k * ncols + s] = w <= min_diag ? 0 : (w - min_diag) * (w - min_diag + 1) / 2;
    }
  return MODLE_PIXELS_OK;
}

extern "C" int modle_pixels_triangles(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows, uint64_t ncols,
                                      uint64_t max_width, uint64_t min_diag, uint64_t* d_out, uint64_t out_words,
                                      void* stream, char* err, size_t errlen) {
  if (h == nullptr || d_band == nullptr || d_out == nullptr || nrows == 0 ||
      modle_pixels_detail::bad_shape(nrows, ncols) || bad_width(nrows, max_width) ||
      out_words < max_width * ncols || (reinterpret_cast<uintptr_t>(d_out) & 7) != 0) {
    set_err(err, errlen, std::string("modle_pixels_triangles: invalid argument ") + kRule);
    return MODLE_PIXELS_ERR_ARG;
  }
  if (modle_pixels_detail::any_overlap({{d_out, max_width * ncols * 8}},
                                       {{d_band, modle_pixels_detail::band_bytes(nrows, ncols)}})) {
    set_err(err, errlen, "modle_pixels_triangles: the output overlaps the band");
    return MODLE_PIXELS_ERR_ARG;
  }
  return triangles_impl(h, d_band, nrows, ncols, max_width, min_diag, d_out, static_cast<hipStream_t>(stream), err,
                        errlen);
}

extern "C" int modle_pixels_triangles_to_host(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                                              uint64_t ncols, uint64_t max_width, uint64_t min_diag,
                                              const uint64_t** table, void* stream, char* err, size_t errlen) {
  return triangles_one_call("modle_pixels_triangles_to_host", nullptr, h, d_band, nrows, ncols, max_width, min_diag,
                            table, stream, err, errlen);
}

extern "C" int modle_pixels_coarse_triangles_to_host(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                                                     uint64_t ncols, uint64_t factor, uint64_t first_bin,
                                                     uint64_t max_width, uint64_t min_diag, const uint64_t** table,
                                                     void* stream, char* err, size_t errlen) {
  const modle_pixels_detail::CoarseSpec cs{factor, first_bin};
  return triangles_one_call("modle_pixels_coarse_triangles_to_host", &cs, h, d_band, nrows, ncols, max_width,
                            min_diag, table, stream, err, errlen);
}
