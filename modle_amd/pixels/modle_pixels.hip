// modle_pixels.hip -- sparse cooler pixels from a dense band matrix on the MI355X
// (include/modle_pixels.h).  Three kernels:
//
//   pixels_count    reads the band the way it lies in memory (d contiguous within a column, so a
//                   wave reads 256 contiguous bytes), counts the non-zero pixels per row in LDS
//                   counters, adds them to the global row counts, and reduces sum and max;
//   pixels_scan     one workgroup: exclusive scan of the row counts -> bin1_offset, nnz;
//   pixels_extract  one wave per 16 consecutive rows.  A row's pixels are nrows + 1 words apart,
//                   but pixel (i, d) and pixel (i - 1, d + 1) are neighbours in memory: lane
//                   (r, c) of a wave reads row i0 + r at d = t - r with t = 4 * step + c, so the 16
//                   lanes of one c read 16 contiguous words of column i0 + t.  The ranks within a
//                   row come from a ballot masked to the row's four lanes, the running base of a
//                   row from the popcount of the same mask.
//
// Only vector loads / stores and atomics; wave64 throughout.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <limits>
#include <new>
#include <string>

#include "modle_pixels.h"
#include "pixels_context.h"
#include "pixels_device.h"

namespace {

using modle_pixels_device::wave_max;
using modle_pixels_device::wave_scan;
using modle_pixels_device::wave_sum;

constexpr unsigned kCountCols = 64;     // columns of one pixels_count tile
constexpr unsigned kCountDepth = 256;  // band words (d) of one pixels_count tile
constexpr unsigned kCountThreads = 256;
constexpr unsigned kScanThreads = MODLE_PIXELS_SCAN_THREADS;  // 1024 (pixels_context.h)
constexpr unsigned kExtractThreads = 256;  // 4 waves
constexpr unsigned kRowsPerWave = 16;
constexpr unsigned kRowsPerBlock = kRowsPerWave * (kExtractThreads / 64);

// Tile (bx, by): columns [j0, j0 + cn), band words [d0, d0 + dn).  Its pixels belong to the rows
// j - d, a range of cn + dn - 1 rows: slot = (j - j0) + (d0 + dn - 1 - d).
__global__ __launch_bounds__(kCountThreads) void pixels_count(const uint32_t* __restrict__ band,
                                                              uint64_t nrows, uint64_t ncols,
                                                              unsigned long long* __restrict__ row_count,
                                                              DeviceStats* __restrict__ stats) {
  __shared__ unsigned int slots[kCountCols + kCountDepth - 1];
  const uint64_t j0 = static_cast<uint64_t>(blockIdx.x) * kCountCols;
  const uint64_t d0 = static_cast<uint64_t>(blockIdx.y) * kCountDepth;
  const unsigned cn = static_cast<unsigned>(min(static_cast<uint64_t>(kCountCols), ncols - j0));
  const unsigned dn = static_cast<unsigned>(min(static_cast<uint64_t>(kCountDepth), nrows - d0));
  const unsigned nslots = cn + dn - 1;
  for (unsigned s = threadIdx.x; s < nslots; s += kCountThreads) slots[s] = 0;
  __syncthreads();

  unsigned long long sum = 0;
  unsigned int mx = 0;
  for (unsigned jj = 0; jj < cn; ++jj) {
    const uint64_t j = j0 + jj;
    const uint32_t* col = band + j * nrows;
    for (unsigned dd = threadIdx.x; dd < dn; dd += kCountThreads) {
      const uint64_t d = d0 + dd;
      if (d > j) break;  // left-edge triangle: no pixel (and none further down this column)
      const uint32_t v = col[d];
      sum += v;
      mx = max(mx, v);
      if (v != 0) atomicAdd(&slots[jj + (dn - 1 - dd)], 1u);
    }
  }
  __syncthreads();
  // row of slot s: j0 - (d0 + dn - 1) + s; slots of rows below 0 hold nothing
  const int64_t row0 = static_cast<int64_t>(j0) - static_cast<int64_t>(d0 + dn - 1);
  for (unsigned s = threadIdx.x; s < nslots; s += kCountThreads) {
    const unsigned int c = slots[s];
    if (c != 0) atomicAdd(&row_count[row0 + static_cast<int64_t>(s)], static_cast<unsigned long long>(c));
  }
  sum = wave_sum(sum);
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) {
    if (sum != 0) atomicAdd(&stats->sum, sum);
    if (mx != 0) atomicMax(&stats->max_count, mx);
  }
}

// In place: offsets[i] = sum of the counts of the rows below i; offsets[ncols] = nnz.
__global__ __launch_bounds__(kScanThreads) void pixels_scan(unsigned long long* __restrict__ offsets,
                                                            uint64_t ncols,
                                                            DeviceStats* __restrict__ stats) {
  __shared__ unsigned long long wave_total[kScanThreads / 64];
  const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long carry = 0;
  for (uint64_t base = 0; base < ncols; base += kScanThreads) {
    const uint64_t idx = base + threadIdx.x;
    const unsigned long long v = idx < ncols ? offsets[idx] : 0;
    const unsigned long long x = wave_scan(v, lane);
    if (lane == 63) wave_total[wave] = x;
    __syncthreads();
    unsigned long long before = 0, total = 0;
    for (unsigned w = 0; w < kScanThreads / 64; ++w) {
      const unsigned long long s = wave_total[w];
      if (w < wave) before += s;
      total += s;
    }
    if (idx < ncols) offsets[idx] = carry + before + x - v;
    carry += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    offsets[ncols] = carry;
    stats->nnz = carry;
  }
}

__global__ __launch_bounds__(kExtractThreads) void pixels_extract(
    const uint32_t* __restrict__ band, uint64_t nrows, uint64_t ncols, int64_t bin_offset,
    const int64_t* __restrict__ offsets, int64_t* __restrict__ bin1, int64_t* __restrict__ bin2,
    int32_t* __restrict__ count, uint64_t nnz) {
  const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned r = lane & (kRowsPerWave - 1), c = lane >> 4;
  const uint64_t i = (static_cast<uint64_t>(blockIdx.x) * (kExtractThreads / 64) + wave) * kRowsPerWave + r;
  uint64_t len = 0, base = 0;  // pixels of row i: d < len; a row beyond the matrix has none
  if (i < ncols) {
    len = ncols - i < nrows ? ncols - i : nrows;
    base = static_cast<uint64_t>(offsets[i]);
  }
  const unsigned long long row_lanes = 0x0001000100010001ULL << r;  // lanes (r, 0..3)
  const unsigned long long below = (1ULL << lane) - 1;
  const int64_t id1 = bin_offset + static_cast<int64_t>(i);
  // t runs over [0, nrows - 1 + 15], kUnroll steps at a time: the loads of a group are issued
  // together (a step beyond the last has no pixel); the trip count is the same for every wave
  constexpr unsigned kUnroll = 4;
  const uint64_t steps = (nrows + kRowsPerWave - 1 + 3) / 4;
  for (uint64_t s0 = 0; s0 < steps; s0 += kUnroll) {
    uint32_t v[kUnroll];
#pragma unroll
    for (unsigned u = 0; u < kUnroll; ++u) {
      const uint64_t t = 4 * (s0 + u) + c;
      const uint64_t d = t - r;
      v[u] = (i < ncols && t >= r && d < len) ? band[(i + d) * nrows + d] : 0u;
    }
#pragma unroll
    for (unsigned u = 0; u < kUnroll; ++u) {
      const uint64_t d = 4 * (s0 + u) + c - r;
      const unsigned long long mine = __ballot(v[u] != 0) & row_lanes;
      if (v[u] != 0) {
        const uint64_t pos = base + __popcll(mine & below);
        if (pos < nnz) {
          bin1[pos] = id1;
          bin2[pos] = id1 + static_cast<int64_t>(d);
          count[pos] = static_cast<int32_t>(v[u]);
        }
      }
      base += __popcll(mine);
    }
  }
}

}  // namespace

namespace modle_pixels_detail {

void set_err(char* err, size_t errlen, const std::string& msg) {
  if (err != nullptr && errlen != 0) std::snprintf(err, errlen, "%s", msg.c_str());
}

bool bad_shape(uint64_t nrows, uint64_t ncols) {
  // (the last two: the grid of pixels_count, x < 2^31 and y < 2^16 blocks)
  return nrows > ncols || (nrows == 0) != (ncols == 0) ||
         ncols > static_cast<uint64_t>(std::numeric_limits<int32_t>::max()) * kCountCols ||
         nrows > 65535ull * kCountDepth;
}

}  // namespace modle_pixels_detail

namespace {

using modle_pixels_detail::bad_shape;
using modle_pixels_detail::set_err;

// the pixel arrays of the one-call form, sized by nnz
int reserve_pixels(modle_pixels_handle* h, uint64_t nnz, char* err, size_t errlen) {
  int rc = h->bin1.ensure(nnz, err, errlen);
  if (rc == MODLE_PIXELS_OK) rc = h->bin2.ensure(nnz, err, errlen);
  if (rc == MODLE_PIXELS_OK) rc = h->count.ensure(nnz, err, errlen);
  return rc;
}

int count_impl(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows, uint64_t ncols,
               int64_t* d_bin1_offset, modle_pixels_stats* stats, hipStream_t stream, char* err,
               size_t errlen) {
  PIX_TRY(hipSetDevice(h->device));
  PIX_TRY(hipMemsetAsync(h->d_stats, 0, sizeof(DeviceStats), stream));
  PIX_TRY(hipMemsetAsync(d_bin1_offset, 0, (ncols + 1) * 8, stream));
  auto* offsets = reinterpret_cast<unsigned long long*>(d_bin1_offset);
  if (ncols != 0) {
    const dim3 grid(static_cast<unsigned>((ncols + kCountCols - 1) / kCountCols),
                    static_cast<unsigned>((nrows + kCountDepth - 1) / kCountDepth));
    hipLaunchKernelGGL(pixels_count, grid, dim3(kCountThreads), 0, stream, d_band, nrows, ncols, offsets,
                       h->d_stats);
    PIX_TRY(hipGetLastError());
    hipLaunchKernelGGL(pixels_scan, dim3(1), dim3(kScanThreads), 0, stream, offsets, ncols, h->d_stats);
    PIX_TRY(hipGetLastError());
  }
  PIX_TRY(hipMemcpyAsync(h->h_stats, h->d_stats, sizeof(DeviceStats), hipMemcpyDeviceToHost, stream));
  PIX_TRY(hipStreamSynchronize(stream));
  stats->nnz = h->h_stats->nnz;
  stats->sum = h->h_stats->sum;
  stats->max_count = h->h_stats->max_count;
  stats->reserved_ = 0;
  if (stats->max_count > static_cast<uint32_t>(std::numeric_limits<int32_t>::max())) {
    set_err(err, errlen, "modle_pixels: a count does not fit the int32 pixel type");
    return MODLE_PIXELS_ERR_RANGE;
  }
  return MODLE_PIXELS_OK;
}

int extract_impl(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows, uint64_t ncols,
                 int64_t bin_offset, const int64_t* d_bin1_offset, int64_t* d_bin1, int64_t* d_bin2,
                 int32_t* d_count, uint64_t nnz, hipStream_t stream, char* err, size_t errlen) {
  PIX_TRY(hipSetDevice(h->device));
  if (nnz == 0 || ncols == 0) return MODLE_PIXELS_OK;
  const dim3 grid(static_cast<unsigned>((ncols + kRowsPerBlock - 1) / kRowsPerBlock));
  hipLaunchKernelGGL(pixels_extract, grid, dim3(kExtractThreads), 0, stream, d_band, nrows, ncols, bin_offset,
                     d_bin1_offset, d_bin1, d_bin2, d_count, nnz);
  PIX_TRY(hipGetLastError());
  return MODLE_PIXELS_OK;
}

}  // namespace

extern "C" void modle_pixels_build_caps(uint64_t caps[4]) {
  if (caps == nullptr) return;
  caps[0] = MODLE_STRIPES_MAX_GRID;
  caps[1] = MODLE_BAND_FILL_MAX_Y;
  caps[2] = MODLE_BAND_CHECK_GROUPS;
  caps[3] = kScanThreads;
}

extern "C" int modle_pixels_create(int device, modle_pixels_handle** out, char* err, size_t errlen) {
  if (out == nullptr || device < 0) {
    set_err(err, errlen, "modle_pixels_create: invalid argument");
    return MODLE_PIXELS_ERR_ARG;
  }
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device >= ndev) {
    set_err(err, errlen, "modle_pixels_create: no such HIP device (there is no CPU fallback)");
    return MODLE_PIXELS_ERR_DEVICE;
  }
  PIX_TRY(hipSetDevice(device));
  auto* h = new (std::nothrow) modle_pixels_handle;
  if (h == nullptr) {
    set_err(err, errlen, "modle_pixels_create: out of memory");
    return MODLE_PIXELS_ERR_DEVICE;
  }
  h->device = device;
  if (hipMalloc(reinterpret_cast<void**>(&h->d_stats), sizeof(DeviceStats)) != hipSuccess ||
      hipHostMalloc(reinterpret_cast<void**>(&h->h_stats), sizeof(DeviceStats), hipHostMallocDefault) !=
          hipSuccess) {
    set_err(err, errlen, "modle_pixels_create: cannot allocate the statistics words");
    modle_pixels_destroy(h);
    return MODLE_PIXELS_ERR_DEVICE;
  }
  *out = h;
  return MODLE_PIXELS_OK;
}

extern "C" void modle_pixels_destroy(modle_pixels_handle* h) {
  if (h == nullptr) return;
  (void)hipSetDevice(h->device);
  (void)hipFree(h->d_stats);
  (void)hipHostFree(h->h_stats);
  if (h->dot_scale_copied != nullptr) (void)hipEventDestroy(h->dot_scale_copied);
  if (h->dot_lam_copied != nullptr) (void)hipEventDestroy(h->dot_lam_copied);
  delete h;  // (releases every buffer of the context)
}

extern "C" int modle_pixels_count(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                                  uint64_t ncols, int64_t* d_bin1_offset, modle_pixels_stats* stats,
                                  void* stream, char* err, size_t errlen) {
  if (h == nullptr || stats == nullptr || (d_band == nullptr && ncols != 0) || bad_shape(nrows, ncols)) {
    set_err(err, errlen, "modle_pixels_count: invalid argument (0 < nrows <= ncols, or both 0)");
    return MODLE_PIXELS_ERR_ARG;
  }
  if (d_bin1_offset == nullptr) {  // statistics only: the index goes to the context's own array
    PIX_TRY(hipSetDevice(h->device));
    const int rc = h->offsets.ensure(ncols + 1, err, errlen, /*room=*/false);
    if (rc != MODLE_PIXELS_OK) return rc;
    d_bin1_offset = h->offsets.dev;
  }
  return count_impl(h, d_band, nrows, ncols, d_bin1_offset, stats, static_cast<hipStream_t>(stream), err,
                    errlen);
}

extern "C" int modle_pixels_extract(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                                    uint64_t ncols, int64_t bin_offset, const int64_t* d_bin1_offset,
                                    int64_t* d_bin1, int64_t* d_bin2, int32_t* d_count, uint64_t nnz,
                                    void* stream, char* err, size_t errlen) {
  if (h == nullptr || d_bin1_offset == nullptr || (d_band == nullptr && ncols != 0) ||
      bad_shape(nrows, ncols) || bin_offset < 0 ||
      (nnz != 0 && (d_bin1 == nullptr || d_bin2 == nullptr || d_count == nullptr))) {
    set_err(err, errlen, "modle_pixels_extract: invalid argument");
    return MODLE_PIXELS_ERR_ARG;
  }
  return extract_impl(h, d_band, nrows, ncols, bin_offset, d_bin1_offset, d_bin1, d_bin2, d_count, nnz,
                      static_cast<hipStream_t>(stream), err, errlen);
}

extern "C" int modle_pixels_to_host(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                                    uint64_t ncols, int64_t bin_offset, const int64_t** bin1,
                                    const int64_t** bin2, const int32_t** count,
                                    const int64_t** bin1_offset, modle_pixels_stats* stats, void* stream,
                                    char* err, size_t errlen) {
  return modle_pixels_detail::pixels_one_call("modle_pixels_to_host", nullptr, h, d_band, nrows, ncols, bin_offset, bin1,
                                              bin2, count, bin1_offset, stats, stream, err, errlen);
}

int modle_pixels_detail::pixels_one_call(const char* name, const CoarseSpec* cs, modle_pixels_handle* h,
                                         const uint32_t* d_band, uint64_t nrows, uint64_t ncols, int64_t bin_offset,
                                         const int64_t** bin1, const int64_t** bin2, const int32_t** count,
                                         const int64_t** bin1_offset, modle_pixels_stats* stats, void* stream,
                                         char* err, size_t errlen) {
  BandView v;
  if (h == nullptr || bad_pixel_outputs(bin1, bin2, count, bin1_offset, stats, bin_offset) ||
      !view_shape(d_band, nrows, ncols, cs, &v, /*empty_ok=*/true)) {
    set_err(err, errlen, std::string(name) + ": invalid argument " +
                             (cs != nullptr ? "(factor >= 2, 0 < nrows <= ncols)" : "(0 < nrows <= ncols, or both 0)"));
    return MODLE_PIXELS_ERR_ARG;
  }
  *bin1 = *bin2 = nullptr;  // (before the coarsening, which may fail)
  *count = nullptr;
  *bin1_offset = nullptr;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const int rc = resolve_band(h, d_band, nrows, ncols, cs, &v, st, err, errlen);
  if (rc != MODLE_PIXELS_OK) return rc;
  return to_host(h, v.d, v.nrows, v.ncols, bin_offset, bin1, bin2, count, bin1_offset, stats, st, err, errlen);
}

int modle_pixels_detail::to_host(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows, uint64_t ncols,
                                 int64_t bin_offset, const int64_t** bin1, const int64_t** bin2,
                                 const int32_t** count, const int64_t** bin1_offset,
                                 modle_pixels_stats* stats, hipStream_t st, char* err, size_t errlen) {
  *bin1 = *bin2 = nullptr;
  *count = nullptr;
  *bin1_offset = nullptr;
  PIX_TRY(hipSetDevice(h->device));
  int rc = h->offsets.ensure(ncols + 1, err, errlen, /*room=*/false);
  if (rc != MODLE_PIXELS_OK) return rc;
  rc = count_impl(h, d_band, nrows, ncols, h->offsets.dev, stats, st, err, errlen);
  if (rc != MODLE_PIXELS_OK) return rc;
  rc = reserve_pixels(h, stats->nnz, err, errlen);
  if (rc != MODLE_PIXELS_OK) return rc;
  rc = extract_impl(h, d_band, nrows, ncols, bin_offset, h->offsets.dev, h->bin1.dev, h->bin2.dev, h->count.dev,
                    stats->nnz, st, err, errlen);
  if (rc != MODLE_PIXELS_OK) return rc;
  PIX_TRY(hipMemcpyAsync(h->offsets.host, h->offsets.dev, (ncols + 1) * 8, hipMemcpyDeviceToHost, st));
  if (stats->nnz != 0) {
    PIX_TRY(hipMemcpyAsync(h->bin1.host, h->bin1.dev, stats->nnz * 8, hipMemcpyDeviceToHost, st));
    PIX_TRY(hipMemcpyAsync(h->bin2.host, h->bin2.dev, stats->nnz * 8, hipMemcpyDeviceToHost, st));
    PIX_TRY(hipMemcpyAsync(h->count.host, h->count.dev, stats->nnz * 4, hipMemcpyDeviceToHost, st));
  }
  PIX_TRY(hipStreamSynchronize(st));
  *bin1_offset = h->offsets.host;
  if (stats->nnz != 0) {
    *bin1 = h->bin1.host;
    *bin2 = h->bin2.host;
    *count = h->count.host;
  }
  return MODLE_PIXELS_OK;
}
