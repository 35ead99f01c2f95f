// modle_band.hip -- sorted pixels scattered into a band matrix on the MI355X, the inverse of modle_pixels_extract
// (include/modle_pixels.h: modle_pixels_band_check / _band_fill / _band_from_host, and the host-only
// modle_pixels_band_classify).
//
//   band_check  one pass over the list, a grid-stride loop: every lane classes its pixel (in / beyond / outside),
//               compares it with its predecessor (the order), looks at the sign of its count and adds to the
//               reductions, which meet per wave through shuffles and per grid through integer atomics on a dozen
//               words of the context (sums and minima of integers: the result does not depend on the order).
//   band_rows   one lane per row start: a binary search of i + bin_offset in bin1.  It reads inside the n entries
//               whatever they hold, so a list that is not sorted costs no more than a sorted one.
//   band_fill   output-stationary, no atomics.  A workgroup owns a tile of kBandCols columns times kBandDiags
//               diagonals of the band and clears it in LDS.  The tile is crossed by the kBandCols + kBandDiags - 1
//               matrix rows i = j - d.  One lane per row clamps the row's start and end to [0, n] and searches
//               bin2 for the first entry at or beyond the tile's first column in that row.  Then one wave per row
//               reads the at most kBandCols entries from there (a coalesced read of bin2 and of count; the reads
//               of eight rows are in flight together: waiting for every row on its own cost 1.7 x), derives (i, j)
//               anew from the row and the entry's bin2, and places the count in LDS when (j, j - i) lies in the
//               tile: consecutive j of a row are kBandDiags + 1 words apart, which is free of bank conflicts.  At last the tile goes out: a column's diagonals are consecutive words, so a wave
//               stores 256 contiguous bytes.  What is stored is the tile clipped to the band and nothing else; what
//               is read is clamped; a list that breaks the order can give a wrong band, never a wild access.
//
// Only vector loads / stores, and atomics in band_check alone; no floating point; wave64 throughout.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "modle_pixels.h"
#include "pixels_context.h"
#include "pixels_device.h"

namespace {

using modle_pixels_device::u64;
using modle_pixels_device::wave_max;
using modle_pixels_device::wave_min;
using modle_pixels_device::wave_sum;

constexpr unsigned kBandCols = MODLE_PIXELS_BAND_TILE_COLS;    // columns of a tile of band_fill
constexpr unsigned kBandDiags = MODLE_PIXELS_BAND_TILE_DIAGS;  // diagonals of a tile
constexpr unsigned kBandRows = kBandCols + kBandDiags - 1;     // matrix rows that cross a tile
constexpr unsigned kFillThreads = 256;
constexpr unsigned kCheckThreads = 256;
constexpr unsigned kCheckGroups = MODLE_BAND_CHECK_GROUPS;  // workgroups of band_check at most: 1024 (pixels_context.h)
constexpr unsigned kFillMaxY = MODLE_BAND_FILL_MAX_Y;       // gridDim.y of band_fill at most: 65535
static_assert(kBandCols % 64 == 0 && kBandDiags % 64 == 0, "a wave stores within one column of a full tile");
static_assert(kBandCols * kBandDiags * 4 <= 32 * 1024, "several workgroups per CU");
static_assert(kBandCols == 64, "a wave reads a row's entries inside the tile in one step");

// the words of the context band_check reduces into
enum : unsigned { kNIn, kSumIn, kNnzIn, kNBeyond, kSumBeyond, kNOutside, kSumOutside, kMaxCount, kBadOrder, kBadSign, kWords };
constexpr u64 kNone = ~u64{0};

// `id` - `off` when it is not negative: the difference of two int64 fits 64 unsigned bits exactly then, and
// everything after is unsigned and cannot wrap (modle_pixels_pileup's rule)
__host__ __device__ inline bool rel(int64_t id, int64_t off, uint64_t* out) {
  if (id < off) return false;
  *out = static_cast<uint64_t>(id) - static_cast<uint64_t>(off);
  return true;
}

// The class of a pixel, for any int64 input; (i, j) are set for MODLE_PIXELS_BAND_IN and _BEYOND.
__host__ __device__ inline unsigned band_class(uint64_t nrows, uint64_t ncols, int64_t off, int64_t bin1, int64_t bin2,
                                               uint64_t* i_out, uint64_t* j_out) {
  uint64_t i = 0, j = 0;
  if (!rel(bin1, off, &i) || !rel(bin2, off, &j) || i > j || j >= ncols) return MODLE_PIXELS_BAND_OUTSIDE;
  *i_out = i, *j_out = j;
  return j - i < nrows ? MODLE_PIXELS_BAND_IN : MODLE_PIXELS_BAND_BEYOND;
}

// id >= x + off, without forming the sum
__device__ inline bool at_or_beyond(int64_t id, int64_t off, uint64_t x) {
  uint64_t r = 0;
  return rel(id, off, &r) && r >= x;
}

__global__ __launch_bounds__(kCheckThreads) void band_check(const int64_t* __restrict__ bin1,
                                                            const int64_t* __restrict__ bin2,
                                                            const int32_t* __restrict__ count, uint64_t n, uint64_t nrows,
                                                            uint64_t ncols, int64_t off, u64* __restrict__ words) {
  u64 acc[7] = {0, 0, 0, 0, 0, 0, 0};
  unsigned mx = 0;
  u64 bad_order = kNone, bad_sign = kNone;
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kCheckThreads;
  for (uint64_t t = static_cast<uint64_t>(blockIdx.x) * kCheckThreads + threadIdx.x; t < n; t += stride) {
    const int64_t b1 = bin1[t], b2 = bin2[t];
    const int32_t c = count[t];
    if (t != 0) {
      const int64_t p1 = bin1[t - 1], p2 = bin2[t - 1];
      if (!(p1 < b1 || (p1 == b1 && p2 < b2))) bad_order = min(bad_order, static_cast<u64>(t));
    }
    if (c < 0) bad_sign = min(bad_sign, static_cast<u64>(t));
    const u64 v = c < 0 ? 0 : static_cast<u64>(c);  // (a negative count enters no sum)
    uint64_t i = 0, j = 0;
    const unsigned cls = band_class(nrows, ncols, off, b1, b2, &i, &j);
    if (cls == MODLE_PIXELS_BAND_IN) {
      acc[kNIn] += 1, acc[kSumIn] += v, acc[kNnzIn] += v != 0;
      mx = max(mx, static_cast<unsigned>(v));
    } else if (cls == MODLE_PIXELS_BAND_BEYOND) {
      acc[kNBeyond] += 1, acc[kSumBeyond] += v;
    } else {
      acc[kNOutside] += 1, acc[kSumOutside] += v;
    }
  }
#pragma unroll
  for (unsigned k = 0; k < 7; ++k) {
    const u64 s = wave_sum(acc[k]);
    if ((threadIdx.x & 63) == 0 && s != 0) atomicAdd(&words[k], s);
  }
  mx = wave_max(mx);
  bad_order = wave_min(bad_order);
  bad_sign = wave_min(bad_sign);
  if ((threadIdx.x & 63) == 0) {
    if (mx != 0) atomicMax(&words[kMaxCount], static_cast<u64>(mx));
    if (bad_order != kNone) atomicMin(&words[kBadOrder], bad_order);
    if (bad_sign != kNone) atomicMin(&words[kBadSign], bad_sign);
  }
}

// row_start[i] = the first index whose bin1 >= i + off, 0 <= i <= ncols
__global__ __launch_bounds__(256) void band_rows(const int64_t* __restrict__ bin1, uint64_t n, uint64_t ncols,
                                                 int64_t off, int64_t* __restrict__ row_start) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i > ncols) return;
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (at_or_beyond(bin1[mid], off, i)) hi = mid; else lo = mid + 1;
  }
  row_start[i] = static_cast<int64_t>(lo);
}

__global__ __launch_bounds__(kFillThreads) void band_fill(const int64_t* __restrict__ bin2,
                                                          const int32_t* __restrict__ count, uint64_t n, uint64_t nrows,
                                                          uint64_t ncols, int64_t off,
                                                          const int64_t* __restrict__ row_start,
                                                          uint32_t* __restrict__ out) {
  __shared__ uint32_t tile[kBandCols * kBandDiags];  // tile[jj * kBandDiags + dd]
  __shared__ uint32_t seg_lo[kBandRows], seg_hi[kBandRows];  // (n < 2^31: an index fits 32 bits)
  const unsigned tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint64_t j0 = static_cast<uint64_t>(blockIdx.x) * kBandCols;
  const unsigned cn = static_cast<unsigned>(min(static_cast<uint64_t>(kBandCols), ncols - j0));
  // (the grid's y is capped at kFillMaxY: a workgroup takes every gridDim.y-th tile of its columns)
  for (uint64_t d0 = static_cast<uint64_t>(blockIdx.y) * kBandDiags; d0 < nrows;
       d0 += static_cast<uint64_t>(gridDim.y) * kBandDiags) {
  const unsigned dn = static_cast<unsigned>(min(static_cast<uint64_t>(kBandDiags), nrows - d0));
  for (unsigned q = tid; q < kBandCols * kBandDiags; q += kFillThreads) tile[q] = 0;

  // slot r stands for the row i = j0 + cn - 1 - d0 - r, from the tile's last column on its first diagonal down
  // to its first column on its last diagonal; rows below 0 (the left-edge triangle) have no entries
  const uint64_t top = j0 + cn - 1;  // i + d0 of slot 0
  const unsigned nslots = cn + dn - 1;
  for (unsigned r = tid; r < nslots; r += kFillThreads) {
    uint32_t lo = 0, hi = 0;
    if (top >= d0 + r) {
      const uint64_t i = top - d0 - r;  // < ncols
      const int64_t s = row_start[i], e = row_start[i + 1];
      const uint64_t sc = s < 0 ? 0 : min(static_cast<uint64_t>(s), n);
      const uint64_t ec = e < 0 ? 0 : min(static_cast<uint64_t>(e), n);
      const uint64_t jlo = max(j0, i + d0);  // the row's first column inside the tile
      uint64_t a = sc, b = max(sc, ec);
      hi = static_cast<uint32_t>(b);
      while (a < b) {
        const uint64_t mid = a + (b - a) / 2;
        if (at_or_beyond(bin2[mid], off, jlo)) b = mid; else a = mid + 1;
      }
      lo = static_cast<uint32_t>(a);
      hi = min(hi, lo + kBandCols);  // a row has at most kBandCols entries inside the tile
    }
    seg_lo[r] = lo, seg_hi[r] = hi;
  }
  __syncthreads();

  // a wave takes every fourth row, kRowsInFlight of them at a time: lane l reads entry lo + l of each (a row
  // has at most kBandCols == 64 entries inside the tile), all loads are issued before the first is used
  constexpr unsigned kWaves = kFillThreads / 64, kRowsInFlight = 8;
  for (unsigned r0 = wv; r0 < nslots; r0 += kWaves * kRowsInFlight) {  // (the same in every lane of a wave)
    int64_t b2[kRowsInFlight];
    uint32_t cnt[kRowsInFlight];
    bool have[kRowsInFlight];
#pragma unroll
    for (unsigned u = 0; u < kRowsInFlight; ++u) {
      const unsigned r = r0 + kWaves * u;
      const uint32_t idx = (r < nslots ? seg_lo[r] : 0u) + lane;
      have[u] = r < nslots && idx < seg_hi[r];
      b2[u] = have[u] ? bin2[idx] : 0;
      cnt[u] = have[u] ? static_cast<uint32_t>(count[idx]) : 0u;
    }
#pragma unroll
    for (unsigned u = 0; u < kRowsInFlight; ++u) {
      const unsigned r = r0 + kWaves * u;
      uint64_t j = 0;
      if (!have[u] || !rel(b2[u], off, &j)) continue;
      const uint64_t i = top - d0 - r;  // (an entry only where the row exists)
      if (j < j0 || j >= j0 + cn || j < i) continue;
      const uint64_t d = j - i;
      if (d < d0 || d >= d0 + dn) continue;
      tile[static_cast<unsigned>(j - j0) * kBandDiags + static_cast<unsigned>(d - d0)] = cnt[u];
    }
  }
  __syncthreads();

  // the tile clipped to the band: column j0 + jj, words d0 .. d0 + dn - 1
  if (dn == kBandDiags) {
    for (unsigned q = tid; q < cn * kBandDiags; q += kFillThreads) {
      const unsigned jj = q / kBandDiags, dd = q % kBandDiags;
      out[(j0 + jj) * nrows + d0 + dd] = tile[q];
    }
  } else {
    for (unsigned q = tid; q < cn * dn; q += kFillThreads) {
      const unsigned jj = q / dn, dd = q - jj * dn;
      out[(j0 + jj) * nrows + d0 + dd] = tile[jj * kBandDiags + dd];
    }
  }
  __syncthreads();  // the tile and the segments are free for the next one
  }
  if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) out[nrows * ncols] = 0;  // the trailing word
}

using modle_pixels_detail::bad_shape;
using modle_pixels_detail::any_overlap;
using modle_pixels_detail::set_err;

bool misaligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) != 0; }

// what check and fill refuse of the numbers alone
bool bad_band(uint64_t nrows, uint64_t ncols, uint64_t n) { return bad_shape(nrows, ncols) || n >= (uint64_t{1} << 31); }

int check_impl(modle_pixels_handle* h, const int64_t* d_bin1, const int64_t* d_bin2, const int32_t* d_count, uint64_t n,
               uint64_t nrows, uint64_t ncols, int64_t bin_offset, int64_t* d_row_start, modle_pixels_band_stats* stats,
               hipStream_t stream, char* err, size_t errlen) {
  PIX_TRY(hipSetDevice(h->device));
  const int rc = h->band_words.ensure(kWords, err, errlen, /*room=*/false);
  if (rc != MODLE_PIXELS_OK) return rc;
  u64* words = reinterpret_cast<u64*>(h->band_words.dev);
  PIX_TRY(hipMemsetAsync(words, 0, kBadOrder * 8, stream));
  PIX_TRY(hipMemsetAsync(words + kBadOrder, 0xFF, 2 * 8, stream));
  if (n != 0) {
    const unsigned groups = static_cast<unsigned>(std::min<uint64_t>(kCheckGroups, (n + kCheckThreads - 1) / kCheckThreads));
    hipLaunchKernelGGL(band_check, dim3(groups), dim3(kCheckThreads), 0, stream, d_bin1, d_bin2, d_count, n, nrows, ncols,
                       bin_offset, words);
    PIX_TRY(hipGetLastError());
  }
  if (d_row_start != nullptr) {
    hipLaunchKernelGGL(band_rows, dim3(static_cast<unsigned>(ncols / 256 + 1)), dim3(256), 0, stream, d_bin1, n, ncols,
                       bin_offset, d_row_start);
    PIX_TRY(hipGetLastError());
  }
  PIX_TRY(hipMemcpyAsync(h->band_words.host, words, kWords * 8, hipMemcpyDeviceToHost, stream));
  PIX_TRY(hipStreamSynchronize(stream));
  const uint64_t* w = h->band_words.host;
  stats->n_in = w[kNIn], stats->sum_in = w[kSumIn], stats->nnz_in = w[kNnzIn];
  stats->n_beyond = w[kNBeyond], stats->sum_beyond = w[kSumBeyond];
  stats->n_outside = w[kNOutside], stats->sum_outside = w[kSumOutside];
  stats->max_count = static_cast<uint32_t>(w[kMaxCount]);
  stats->reserved_ = 0;
  stats->first_bad = -1;
  const uint64_t bo = w[kBadOrder], bs = w[kBadSign];
  if (bo != kNone && bo <= bs) {
    stats->first_bad = static_cast<int64_t>(bo);
    set_err(err, errlen, "modle_pixels_band_check: pixel " + std::to_string(bo) +
                             " is not after its predecessor in (bin1, bin2): the list is not sorted or holds a duplicate");
    return MODLE_PIXELS_ERR_ORDER;
  }
  if (bs != kNone) {
    stats->first_bad = static_cast<int64_t>(bs);
    set_err(err, errlen, "modle_pixels_band_check: pixel " + std::to_string(bs) + " has a negative count");
    return MODLE_PIXELS_ERR_RANGE;
  }
  return MODLE_PIXELS_OK;
}

int fill_impl(modle_pixels_handle* h, const int64_t* d_bin2, const int32_t* d_count, uint64_t n, uint64_t nrows,
              uint64_t ncols, int64_t bin_offset, const int64_t* d_row_start, uint32_t* d_out, hipStream_t stream,
              char* err, size_t errlen) {
  PIX_TRY(hipSetDevice(h->device));
  if (ncols == 0) {  // (then nrows == 0: the trailing word is all there is)
    PIX_TRY(hipMemsetAsync(d_out, 0, 4, stream));
    return MODLE_PIXELS_OK;
  }
  const dim3 grid(static_cast<unsigned>((ncols + kBandCols - 1) / kBandCols),
                  static_cast<unsigned>(std::min<uint64_t>(kFillMaxY, (nrows + kBandDiags - 1) / kBandDiags)));
  hipLaunchKernelGGL(band_fill, grid, dim3(kFillThreads), 0, stream, d_bin2, d_count, n, nrows, ncols, bin_offset,
                     d_row_start, d_out);
  PIX_TRY(hipGetLastError());
  return MODLE_PIXELS_OK;
}

}  // namespace

extern "C" int modle_pixels_band_classify(uint64_t nrows, uint64_t ncols, int64_t bin_offset, const int64_t* bin1,
                                          const int64_t* bin2, uint64_t n, uint8_t* cls) {
  if (bad_band(nrows, ncols, n) || (n != 0 && (bin1 == nullptr || bin2 == nullptr || cls == nullptr)))
    return MODLE_PIXELS_ERR_ARG;
  for (uint64_t t = 0; t < n; ++t) {
    uint64_t i = 0, j = 0;
    cls[t] = static_cast<uint8_t>(band_class(nrows, ncols, bin_offset, bin1[t], bin2[t], &i, &j));
  }
  return MODLE_PIXELS_OK;
}

extern "C" int modle_pixels_band_check(modle_pixels_handle* h, const int64_t* d_bin1, const int64_t* d_bin2,
                                       const int32_t* d_count, uint64_t n, uint64_t nrows, uint64_t ncols,
                                       int64_t bin_offset, int64_t* d_row_start, modle_pixels_band_stats* stats,
                                       void* stream, char* err, size_t errlen) {
  if (h == nullptr || stats == nullptr || bad_band(nrows, ncols, n) ||
      (n != 0 && (d_bin1 == nullptr || d_bin2 == nullptr || d_count == nullptr)) || misaligned8(d_bin1) ||
      misaligned8(d_bin2) || misaligned8(d_row_start) || (reinterpret_cast<uintptr_t>(d_count) & 3) != 0) {
    set_err(err, errlen, "modle_pixels_band_check: invalid argument (0 < nrows <= ncols, or both 0; n < 2^31; pixel "
                         "arrays unless n == 0; 8-byte aligned int64 arrays)");
    return MODLE_PIXELS_ERR_ARG;
  }
  if (any_overlap({{d_row_start, (ncols + 1) * 8}}, {{d_bin1, n * 8}, {d_bin2, n * 8}, {d_count, n * 4}})) {
    set_err(err, errlen, "modle_pixels_band_check: d_row_start overlaps the pixels");
    return MODLE_PIXELS_ERR_ARG;
  }
  return check_impl(h, d_bin1, d_bin2, d_count, n, nrows, ncols, bin_offset, d_row_start, stats,
                    static_cast<hipStream_t>(stream), err, errlen);
}

extern "C" int modle_pixels_band_fill(modle_pixels_handle* h, const int64_t* d_bin2, const int32_t* d_count, uint64_t n,
                                      uint64_t nrows, uint64_t ncols, int64_t bin_offset, const int64_t* d_row_start,
                                      uint32_t* d_out, uint64_t out_words, void* stream, char* err, size_t errlen) {
  if (h == nullptr || d_out == nullptr || d_row_start == nullptr || bad_band(nrows, ncols, n) ||
      (n != 0 && (d_bin2 == nullptr || d_count == nullptr)) || out_words < nrows * ncols + 1 || misaligned8(d_bin2) ||
      misaligned8(d_row_start) || (reinterpret_cast<uintptr_t>(d_count) & 3) != 0 ||
      (reinterpret_cast<uintptr_t>(d_out) & 3) != 0) {
    set_err(err, errlen, "modle_pixels_band_fill: invalid argument (0 < nrows <= ncols, or both 0; n < 2^31; pixel "
                         "arrays unless n == 0; 8-byte aligned int64 arrays; out_words >= nrows * ncols + 1)");
    return MODLE_PIXELS_ERR_ARG;
  }
  const uint64_t nb = modle_pixels_detail::band_bytes(nrows, ncols);
  if (any_overlap({{d_out, nb}}, {{d_bin2, n * 8}, {d_count, n * 4}, {d_row_start, (ncols + 1) * 8}})) {
    set_err(err, errlen, "modle_pixels_band_fill: d_out overlaps an input");
    return MODLE_PIXELS_ERR_ARG;
  }
  return fill_impl(h, d_bin2, d_count, n, nrows, ncols, bin_offset, d_row_start, d_out, static_cast<hipStream_t>(stream),
                   err, errlen);
}

extern "C" int modle_pixels_band_from_host(modle_pixels_handle* h, const int64_t* bin1, const int64_t* bin2,
                                           const int32_t* count, uint64_t n, uint64_t nrows, uint64_t ncols,
                                           int64_t bin_offset, uint32_t* d_out, uint64_t out_words,
                                           modle_pixels_band_stats* stats, void* stream, char* err, size_t errlen) {
  if (h == nullptr || stats == nullptr || d_out == nullptr || bad_band(nrows, ncols, n) ||
      (n != 0 && (bin1 == nullptr || bin2 == nullptr || count == nullptr)) || out_words < nrows * ncols + 1 ||
      (reinterpret_cast<uintptr_t>(d_out) & 3) != 0) {
    set_err(err, errlen, "modle_pixels_band_from_host: invalid argument (0 < nrows <= ncols, or both 0; n < 2^31; pixel "
                         "arrays unless n == 0; out_words >= nrows * ncols + 1)");
    return MODLE_PIXELS_ERR_ARG;
  }
  const hipStream_t st = static_cast<hipStream_t>(stream);
  PIX_TRY(hipSetDevice(h->device));
  int rc = h->band_bin1.ensure(n, err, errlen);
  if (rc == MODLE_PIXELS_OK) rc = h->band_bin2.ensure(n, err, errlen);
  if (rc == MODLE_PIXELS_OK) rc = h->band_count.ensure(n, err, errlen);
  if (rc == MODLE_PIXELS_OK) rc = h->band_rows.ensure(ncols + 1, err, errlen);
  if (rc != MODLE_PIXELS_OK) return rc;
  const uint64_t nb = modle_pixels_detail::band_bytes(nrows, ncols);
  if (any_overlap({{d_out, nb}}, {{h->band_bin1.dev, n * 8}, {h->band_bin2.dev, n * 8}, {h->band_count.dev, n * 4},
                                  {h->band_rows.dev, (ncols + 1) * 8}})) {
    set_err(err, errlen, "modle_pixels_band_from_host: d_out overlaps the scratch of the context");
    return MODLE_PIXELS_ERR_ARG;
  }
  if (n != 0) {
    PIX_TRY(hipMemcpyAsync(h->band_bin1.dev, bin1, n * 8, hipMemcpyHostToDevice, st));
    PIX_TRY(hipMemcpyAsync(h->band_bin2.dev, bin2, n * 8, hipMemcpyHostToDevice, st));
    PIX_TRY(hipMemcpyAsync(h->band_count.dev, count, n * 4, hipMemcpyHostToDevice, st));
  }
  rc = check_impl(h, h->band_bin1.dev, h->band_bin2.dev, h->band_count.dev, n, nrows, ncols, bin_offset, h->band_rows.dev,
                  stats, st, err, errlen);
  if (rc != MODLE_PIXELS_OK) return rc;
  rc = fill_impl(h, h->band_bin2.dev, h->band_count.dev, n, nrows, ncols, bin_offset, h->band_rows.dev, d_out, st, err,
                 errlen);
  if (rc != MODLE_PIXELS_OK) return rc;
  PIX_TRY(hipStreamSynchronize(st));
  return MODLE_PIXELS_OK;
}
