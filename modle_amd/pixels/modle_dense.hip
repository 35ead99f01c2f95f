// modle_dense.hip -- square regions of a band matrix, unpacked on the MI355X
// (include/modle_pixels.h: modle_pixels_tiles_fit / _dense_tiles / _dense_to_host).
//
// Tile t of a run covers the bins lo = first + t * step .. lo + size - 1; its output is the symmetric
// size x size matrix out[t][r][c] = band[max(a, b) * nrows + |a - b|] (a = lo + r, b = lo + c) where
// |a - b| < nrows, and 0 elsewhere.  The kernel is output-stationary: one workgroup of four waves
// owns, within one tile, one pair of 64 x 64 blocks (R, C), R <= C, and writes out[R-block][C-block]
// and its mirror out[C-block][R-block].  Dense column b over the rows a = a0 .. a0 + 63 is ONE
// contiguous span of the band, band[b * nrows + (b - a)], with a descending address for ascending a:
// a wave reads it with the lanes mapped in reverse (256 contiguous bytes per load, kLoadUnroll
// columns in flight) into a 64 x 65-word LDS tile.  The pad of one word per row makes the row-wise
// pass (the upper block) and the column-wise pass (the mirror, at a stride of 65 words) free of bank
// conflicts.  A diagonal block (R == C) is composed symmetric in LDS -- every word read goes to
// (r, c) and (c, r) -- and written once.  A block whose smallest d is already >= nrows is written as
// zeros without a read.  The band (d < nrows), the diagonal (d >= 0) and the tile's edge (size % 64)
// are masked by index; a >= 0 keeps d <= b, so the words that are no pixels are never addressed.
// Every output word is written exactly once, as part of a whole row of its block: no atomics, no
// pre-zeroing, and nothing depends on the launch geometry.  All offsets are 64-bit.
#include <hip/hip_runtime.h>

#include <limits>

#include "modle_pixels.h"
#include "pixels_context.h"

namespace {

constexpr int kBlock = 64;             // a block of the output is kBlock x kBlock words
constexpr int kPitch = kBlock + 1;     // LDS row pitch, words
constexpr unsigned kDenseThreads = 256;  // 4 waves
constexpr int kWaves = kDenseThreads / 64;
constexpr int kLoadUnroll = 4;         // dense columns a wave keeps in flight

// block pair p = C * (C + 1) / 2 + R, R <= C
__device__ __forceinline__ void block_pair(int64_t p, int64_t* R, int64_t* C) {
  int64_t c = static_cast<int64_t>((sqrt(8.0 * static_cast<double>(p) + 1.0) - 1.0) * 0.5);
  while (c * (c + 1) / 2 > p) --c;
  while ((c + 1) * (c + 2) / 2 <= p) ++c;
  *C = c;
  *R = p - c * (c + 1) / 2;
}

__global__ __launch_bounds__(kDenseThreads) void pixels_dense(const uint32_t* __restrict__ band, int64_t nrows,
                                                              int64_t first, int64_t size, int64_t step,
                                                              int64_t pairs, uint32_t* __restrict__ out) {
  __shared__ uint32_t tile[kBlock * kPitch];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t t = static_cast<int64_t>(blockIdx.x) / pairs;
  int64_t R, C;
  block_pair(static_cast<int64_t>(blockIdx.x) % pairs, &R, &C);
  const int64_t lo = first + t * step;
  const int64_t r0 = R * kBlock, c0 = C * kBlock;              // the upper block's corner within the tile
  const int nr = static_cast<int>(min(static_cast<int64_t>(kBlock), size - r0));  // its rows and columns
  const int nc = static_cast<int>(min(static_cast<int64_t>(kBlock), size - c0));
  uint32_t* const tile_out = out + t * size * size;
  uint32_t* const upper = tile_out + r0 * size + c0;   // out[t][r0 + r][c0 + c] = upper[r * size + c]
  uint32_t* const mirror = tile_out + c0 * size + r0;  // out[t][c0 + c][r0 + r] = mirror[c * size + r]
  const bool diagonal = R == C;

  // smallest d of the block: column c0, row r0 + 63
  if (c0 - (r0 + kBlock - 1) >= nrows) {  // (the same in every lane; never a diagonal block)
    for (int r = wave; r < nr; r += kWaves)
      if (lane < nc) upper[r * size + lane] = 0u;
    for (int c = wave; c < nc; c += kWaves)
      if (lane < nr) mirror[c * size + lane] = 0u;
    return;
  }

  // dense column c of the block, rows r = 63 - lane: d = (c0 + c) - (r0 + r), ascending with the lane
  const int r = kBlock - 1 - lane;
  const int64_t d_lane = c0 - r0 - r;  // d of this lane in column 0
  for (int cc = wave * kLoadUnroll; cc < kBlock; cc += kWaves * kLoadUnroll) {
    uint32_t v[kLoadUnroll];
#pragma unroll
    for (int u = 0; u < kLoadUnroll; ++u) {
      const int c = cc + u;
      const int64_t d = d_lane + c;
      v[u] = (c < nc && r < nr && d >= 0 && d < nrows) ? band[(lo + c0 + c) * nrows + d] : 0u;
    }
#pragma unroll
    for (int u = 0; u < kLoadUnroll; ++u) {
      const int c = cc + u;
      if (!diagonal) {
        tile[r * kPitch + c] = v[u];
      } else if (r <= c) {  // the upper triangle and its reflection: together every word of the tile
        tile[r * kPitch + c] = v[u];
        tile[c * kPitch + r] = v[u];
      }
    }
  }
  __syncthreads();
  // whole rows of the upper block: lane = column
  for (int rr = wave; rr < nr; rr += kWaves)
    if (lane < nc) upper[rr * size + lane] = tile[rr * kPitch + lane];
  if (diagonal) return;
  // whole rows of the mirrored block: lane = row of the upper block, LDS read at a stride of kPitch
  for (int c = wave; c < nc; c += kWaves)
    if (lane < nr) mirror[c * size + lane] = tile[lane * kPitch + c];
}

int tiles_fit(uint64_t ncols, uint64_t first, uint64_t size, uint64_t step, uint64_t* max_count) {
  if (max_count == nullptr || size == 0 || step == 0 || first > ncols || size > ncols - first)
    return MODLE_PIXELS_ERR_ARG;
  *max_count = (ncols - first - size) / step + 1;
  return MODLE_PIXELS_OK;
}

// the argument checks of modle_pixels_dense_tiles that need no pointer; *words = count * size * size
int check_run(uint64_t nrows, uint64_t ncols, uint64_t first, uint64_t size, uint64_t step, uint64_t count,
              uint64_t* words, const char** why) {
  uint64_t fit = 0, sq = 0;
  *why = "invalid argument (0 < nrows <= ncols, size > 0, step > 0, first + size <= ncols)";
  constexpr uint64_t kMaxBytes = static_cast<uint64_t>(std::numeric_limits<int64_t>::max());
  if (nrows == 0 || nrows > ncols || ncols > kMaxBytes / 8 / nrows ||
      tiles_fit(ncols, first, size, step, &fit) != MODLE_PIXELS_OK)
    return MODLE_PIXELS_ERR_ARG;
  *why = "count is 0 or larger than the number of tiles that fit (modle_pixels_tiles_fit)";
  if (count == 0 || count > fit) return MODLE_PIXELS_ERR_ARG;
  *why = "count * size * size does not fit 63 bits";
  if (__builtin_mul_overflow(size, size, &sq) || __builtin_mul_overflow(sq, count, words) ||
      *words > kMaxBytes / 4)
    return MODLE_PIXELS_ERR_ARG;
  return MODLE_PIXELS_OK;
}

int dense_impl(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows, uint64_t first, uint64_t size,
               uint64_t step, uint64_t count, uint32_t* d_out, hipStream_t stream, char* err, size_t errlen) {
  const uint64_t nb = (size + kBlock - 1) / kBlock;
  const uint64_t pairs = nb * (nb + 1) / 2;  // (size * size fits 61 bits: no overflow)
  if (pairs > static_cast<uint64_t>(std::numeric_limits<int32_t>::max()) / count) {
    modle_pixels_detail::set_err(err, errlen, "modle_pixels_dense_tiles: the run is too large for one launch");
    return MODLE_PIXELS_ERR_ARG;
  }
  PIX_TRY(hipSetDevice(h->device));
  hipLaunchKernelGGL(pixels_dense, dim3(static_cast<unsigned>(pairs * count)), dim3(kDenseThreads), 0, stream,
                     d_band, static_cast<int64_t>(nrows), static_cast<int64_t>(first), static_cast<int64_t>(size),
                     static_cast<int64_t>(step), static_cast<int64_t>(pairs), d_out);
  PIX_TRY(hipGetLastError());
  return MODLE_PIXELS_OK;
}

}  // namespace

extern "C" int modle_pixels_tiles_fit(uint64_t ncols, uint64_t first, uint64_t size, uint64_t step,
                                      uint64_t* max_count) {
  return tiles_fit(ncols, first, size, step, max_count);
}

extern "C" int modle_pixels_dense_tiles(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                                        uint64_t ncols, uint64_t first, uint64_t size, uint64_t step,
                                        uint64_t count, uint32_t* d_out, uint64_t out_words, void* stream,
                                        char* err, size_t errlen) {
  using modle_pixels_detail::set_err;
  if (h == nullptr || d_band == nullptr || d_out == nullptr) {
    set_err(err, errlen, "modle_pixels_dense_tiles: null pointer");
    return MODLE_PIXELS_ERR_ARG;
  }
  uint64_t words = 0;
  const char* why = nullptr;
  if (check_run(nrows, ncols, first, size, step, count, &words, &why) != MODLE_PIXELS_OK) {
    set_err(err, errlen, std::string("modle_pixels_dense_tiles: ") + why);
    return MODLE_PIXELS_ERR_ARG;
  }
  if (out_words < words) {
    set_err(err, errlen, "modle_pixels_dense_tiles: out_words is smaller than count * size * size");
    return MODLE_PIXELS_ERR_ARG;
  }
  if (modle_pixels_detail::overlap(d_out, words * 4, d_band, modle_pixels_detail::band_bytes(nrows, ncols))) {
    set_err(err, errlen, "modle_pixels_dense_tiles: d_out overlaps the band");
    return MODLE_PIXELS_ERR_ARG;
  }
  return dense_impl(h, d_band, nrows, first, size, step, count, d_out, static_cast<hipStream_t>(stream), err,
                    errlen);
}

extern "C" int modle_pixels_dense_to_host(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                                          uint64_t ncols, uint64_t lo, uint64_t hi, const uint32_t** dense,
                                          void* stream, char* err, size_t errlen) {
  using modle_pixels_detail::set_err;
  if (dense != nullptr) *dense = nullptr;
  uint64_t words = 0;
  const char* why = "null pointer, or lo >= hi";
  if (h == nullptr || d_band == nullptr || dense == nullptr || lo >= hi ||
      check_run(nrows, ncols, lo, hi - lo, 1, 1, &words, &why) != MODLE_PIXELS_OK) {
    set_err(err, errlen, std::string("modle_pixels_dense_to_host: ") + why);
    return MODLE_PIXELS_ERR_ARG;
  }
  const hipStream_t st = static_cast<hipStream_t>(stream);
  PIX_TRY(hipSetDevice(h->device));
  int rc = h->dense.ensure(words, err, errlen);
  if (rc != MODLE_PIXELS_OK) return rc;
  rc = dense_impl(h, d_band, nrows, lo, hi - lo, 1, 1, h->dense.dev, st, err, errlen);
  if (rc != MODLE_PIXELS_OK) return rc;
  PIX_TRY(hipMemcpyAsync(h->dense.host, h->dense.dev, words * 4, hipMemcpyDeviceToHost, st));
  PIX_TRY(hipStreamSynchronize(st));
  *dense = h->dense.host;
  return MODLE_PIXELS_OK;
}
