// modle_rescale.hip -- rescaled pileups of a band matrix, summed on the MI355X (include/modle_pixels.h:
// modle_pixels_rescale / _rescale_to_host / _coarse_rescale_to_host / _rescale_groups, and the host-only
// modle_pixels_rescale_accepts).
//
// A window [s, e) of width W = e - s is cut into R blocks: block u holds the x with floor(x R / W) == u, that
// is lo(u) <= x < lo(u + 1) with lo(u) = ceil(u W / R).  Cell (u, v) of the pile is the sum of M(s + x, s + y)
// over block u times block v, M the symmetric matrix of the band; only the T = R (R + 1) / 2 cells u <= v are
// formed and the sum kernel mirrors them.  For u < v every (x, y) has x < y and is the word
//     band[(s + y) * nrows + (y - x)]:
// for a fixed y the block u is a run of consecutive words of one band column, and the lanes of a wave, which
// run along u, read neighbouring runs of it.  For u == v the pixels above the diagonal are summed, doubled,
// and the diagonal ones added once: the block read through the symmetry.
//
// The kernel is output-stationary.  Workgroup g of G takes the windows g, g + G, ...: a strided share, so that
// a list sorted by width still spreads.  Every lane reads the window (a broadcast) and judges it; an accepted
// one has its R + 1 block edges formed in LDS, then lane l sums the cells q = l, l + 1024, ... in registers
// and adds them to the workgroup's partial pile and partial area, which live in LDS (8 + 4 bytes per cell: the
// area of a workgroup is below 2^32 by the refusal below).  A cell belongs to one lane for the whole kernel, so
// the LDS words need no atomics.  At the end every workgroup stores its T partial sums, T partial areas and
// its count of accepted windows into the context's scratch with plain stores, and a second kernel adds the
// partials per cell and stores pile, area and n_used: one lane per output word, nothing cleared beforehand.
// The grid is capped at MODLE_RESCALE_MAX_GROUPS workgroups.  A rejected window is never turned into an
// address; an accepted one lies in the band, so no word that is no pixel is read.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "modle_pixels.h"
#include "pixels_context.h"
#include "pixels_device.h"

namespace {

using modle_pixels_device::u64;

constexpr unsigned kLanes = 1024;                         // lanes of a workgroup of pixels_rescale
constexpr unsigned kMaxR = MODLE_PIXELS_MAX_RESCALE;      // grid side at most
constexpr unsigned kMaxCells = kMaxR * (kMaxR + 1) / 2;   // cells u <= v at most
constexpr unsigned kMaxGroups = MODLE_RESCALE_MAX_GROUPS; // workgroups at most
constexpr unsigned kSumCells = 64;                        // cells of a workgroup of pixels_rescale_sum, 4 lanes each
static_assert(kMaxR <= 255, "a cell's (u, v) is packed into 16 bits");
static_assert(kMaxCells * 14 + (kMaxR + 1) * 8 <= 160 * 1024, "the partial pile, area and cells fit the LDS of a CU");

// The acceptance rule, for any int64 input: s = start - off and e = end - off are formed only once they are
// known to be non-negative; then the differences fit 64 unsigned bits exactly, and everything after is
// unsigned and cannot wrap.
__host__ __device__ inline bool rescale_accept(uint64_t nrows, uint64_t ncols, uint64_t R, int64_t off, int64_t start,
                                               int64_t end, uint64_t* s_out, uint64_t* w_out) {
  if (start < off || end < off) return false;  // s < 0, or e < 0 <= s
  const uint64_t s = static_cast<uint64_t>(start) - static_cast<uint64_t>(off);
  const uint64_t e = static_cast<uint64_t>(end) - static_cast<uint64_t>(off);
  if (s >= e || e > ncols) return false;
  *s_out = s, *w_out = e - s;
  return R <= e - s && e - s <= nrows;
}

__global__ __launch_bounds__(kLanes) void pixels_rescale(const uint32_t* __restrict__ band, uint64_t nrows,
                                                         uint64_t ncols, unsigned R, int64_t bin_offset,
                                                         const int64_t* __restrict__ start,
                                                         const int64_t* __restrict__ end, uint64_t n,
                                                         u64* __restrict__ partial, u64* __restrict__ counts) {
  __shared__ u64 spile[kMaxCells];       // the workgroup's partial pile, cell q = v (v + 1) / 2 + u
  __shared__ u64 slo[kMaxR + 1];         // the block edges of the window at hand
  __shared__ uint32_t sarea[kMaxCells];  // its partial area
  __shared__ uint16_t scell[kMaxCells];  // u | v << 8 of cell q
  const unsigned tid = threadIdx.x;
  const unsigned T = R * (R + 1) / 2;

  for (unsigned q = tid; q < T; q += kLanes) {
    // v is the largest with v (v + 1) / 2 <= q: the root of a float (8 q + 1 < 2^17 is exact), put right by one
    // step either way
    unsigned v = static_cast<unsigned>((sqrtf(static_cast<float>(8 * q + 1)) - 1.0f) * 0.5f);
    while (v * (v + 1) / 2 > q) --v;
    while ((v + 1) * (v + 2) / 2 <= q) ++v;
    const unsigned u = q - v * (v + 1) / 2;
    scell[q] = static_cast<uint16_t>(u | (v << 8));
    spile[q] = 0;
    sarea[q] = 0;
  }

  u64 n_used = 0;
  for (uint64_t t = blockIdx.x; t < n; t += gridDim.x) {  // (the same in every lane, and so is all that is judged)
    uint64_t s = 0, W = 0;
    if (!rescale_accept(nrows, ncols, R, bin_offset, start[t], end[t], &s, &W)) continue;
    ++n_used;
    __syncthreads();  // the edges of the window before are read
    if (tid <= R) slo[tid] = (tid * W + (R - 1)) / R;  // ceil(u W / R): u <= 128 and W <= nrows < 2^48, no wrap
    __syncthreads();

    for (unsigned q = tid; q < T; q += kLanes) {
      const unsigned uv = scell[q], u = uv & 255u, v = uv >> 8;
      const uint64_t x0 = slo[u], x1 = slo[u + 1], y0 = slo[v], y1 = slo[v + 1];
      u64 sum = 0;
      if (u != v) {
        for (uint64_t y = y0; y < y1; ++y) {
          const uint32_t* col = band + (s + y) * nrows;  // x1 <= y0: the block u lies above the diagonal
          const uint64_t d1 = y - x0;
#pragma unroll 4
          for (uint64_t d = y - x1 + 1; d <= d1; ++d) sum += col[d];
        }
      } else {
        u64 diag = 0;
        for (uint64_t y = y0; y < y1; ++y) {
          const uint32_t* col = band + (s + y) * nrows;
          const uint64_t d1 = y - x0;
#pragma unroll 4
          for (uint64_t d = 1; d <= d1; ++d) sum += col[d];
          diag += col[0];
        }
        sum = 2 * sum + diag;
      }
      spile[q] += sum;
      sarea[q] += static_cast<uint32_t>((x1 - x0) * (y1 - y0));
    }
  }

  u64* mine = partial + static_cast<uint64_t>(blockIdx.x) * (2 * T);
  for (unsigned q = tid; q < T; q += kLanes) {
    mine[q] = spile[q];
    mine[T + q] = sarea[q];
  }
  if (tid == 0) counts[blockIdx.x] = n_used;
}

// A workgroup owns kSumCells output words c = r * R + col of the R x R grid (c == R * R stands for the counts of
// accepted windows); four lanes share a word, each adding every fourth workgroup's partial of the cell
// (min, max), meet in LDS, and one of them stores pile[c] and area[c]: the mirror image is another word's work.
__global__ __launch_bounds__(4 * kSumCells) void pixels_rescale_sum(const u64* __restrict__ partial,
                                                                    const u64* __restrict__ counts, unsigned groups,
                                                                    unsigned R, u64* __restrict__ pile,
                                                                    u64* __restrict__ area, u64* __restrict__ n_used) {
  __shared__ u64 part[2][4 * kSumCells];
  const unsigned RR = R * R, T = R * (R + 1) / 2;
  const unsigned cell = threadIdx.x % kSumCells, slice = threadIdx.x / kSumCells;
  const unsigned c = blockIdx.x * kSumCells + cell;
  u64 sum = 0, ar = 0;
  if (c < RR) {
    const unsigned r = c / R, k = c - r * R, u = r < k ? r : k, v = r < k ? k : r;
    const unsigned q = v * (v + 1) / 2 + u;
#pragma unroll 4
    for (unsigned g = slice; g < groups; g += 4) {
      const u64* p = partial + static_cast<uint64_t>(g) * (2 * T);
      sum += p[q];
      ar += p[T + q];
    }
  } else if (c == RR) {
    for (unsigned g = slice; g < groups; g += 4) sum += counts[g];
  }
  part[0][threadIdx.x] = sum;
  part[1][threadIdx.x] = ar;
  __syncthreads();
  if (slice != 0) return;
  sum = part[0][cell] + part[0][kSumCells + cell] + part[0][2 * kSumCells + cell] + part[0][3 * kSumCells + cell];
  ar = part[1][cell] + part[1][kSumCells + cell] + part[1][2 * kSumCells + cell] + part[1][3 * kSumCells + cell];
  if (c < RR) {
    pile[c] = sum;
    if (area != nullptr) area[c] = ar;
  } else if (c == RR && n_used != nullptr) {
    *n_used = sum;
  }
}

using modle_pixels_detail::set_err;

constexpr const char* kRule =
    "(0 < nrows <= ncols, 1 <= size <= 128, n < 2^31, n * ceil(nrows / size)^2 < 2^32, windows unless n == 0, "
    "8-byte aligned outputs that overlap neither the band nor the windows)";

// what the numbers alone refuse
bool bad_rescale(uint64_t nrows, uint64_t ncols, uint64_t R, uint64_t n) {
  if (nrows == 0 || modle_pixels_detail::bad_shape(nrows, ncols) || R == 0 || R > kMaxR || n >= (uint64_t{1} << 31))
    return true;
  const uint64_t side = std::min(nrows, ncols), c = side / R + (side % R != 0 ? 1 : 0);  // ceil, without a sum
  if (n == 0) return false;
  // c < 2^16 and n < 2^31: the product fits 63 bits
  return c >= (uint64_t{1} << 16) || n * c * c >= (uint64_t{1} << 32);
}

// enqueues the two kernels on checked arguments; the windows and the outputs are device arrays
int rescale_impl(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows, uint64_t ncols, uint64_t R,
                 int64_t bin_offset, const int64_t* d_start, const int64_t* d_end, uint64_t n, uint64_t* d_pile,
                 uint64_t* d_area, uint64_t* d_n_used, hipStream_t stream, char* err, size_t errlen) {
  PIX_TRY(hipSetDevice(h->device));
  const unsigned r = static_cast<unsigned>(R), RR = r * r, T = r * (r + 1) / 2;
  // a window is W * W / 2 loads, walked by one workgroup: one workgroup per window until the cap binds
  const uint64_t groups = std::min<uint64_t>(kMaxGroups, n);
  const int rc = h->rescale_partial.ensure(groups * (2 * T + 1), err, errlen);
  if (rc != MODLE_PIXELS_OK) return rc;
  u64* partial = reinterpret_cast<u64*>(h->rescale_partial.dev);
  u64* counts = partial + groups * (2 * T);
  if (groups != 0) {
    hipLaunchKernelGGL(pixels_rescale, dim3(static_cast<unsigned>(groups)), dim3(kLanes), 0, stream, d_band, nrows,
                       ncols, r, bin_offset, d_start, d_end, n, partial, counts);
    PIX_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(pixels_rescale_sum, dim3(RR / kSumCells + 1), dim3(4 * kSumCells), 0, stream, partial, counts,
                     static_cast<unsigned>(groups), r, reinterpret_cast<u64*>(d_pile), reinterpret_cast<u64*>(d_area),
                     reinterpret_cast<u64*>(d_n_used));
  PIX_TRY(hipGetLastError());
  return MODLE_PIXELS_OK;
}

// modle_pixels_rescale_to_host (`cs` null) and modle_pixels_coarse_rescale_to_host under their `name`: the band
// resolved, the host windows up, rescale_impl into the sums of the context, their copy to the pinned mirror, the wait
int rescale_one_call(const char* name, const modle_pixels_detail::CoarseSpec* cs, modle_pixels_handle* h,
                     const uint32_t* d_band, uint64_t nrows, uint64_t ncols, uint64_t R, int64_t bin_offset,
                     const int64_t* start, const int64_t* end, uint64_t n, const uint64_t** pile, const uint64_t** area,
                     const uint64_t** n_used, void* stream, char* err, size_t errlen) {
  if (pile != nullptr) *pile = nullptr;
  if (area != nullptr) *area = nullptr;
  if (n_used != nullptr) *n_used = nullptr;
  modle_pixels_detail::BandView v;
  if (h == nullptr || pile == nullptr || area == nullptr || n_used == nullptr ||
      !modle_pixels_detail::view_shape(d_band, nrows, ncols, cs, &v) || bad_rescale(v.nrows, v.ncols, R, n) ||
      (n != 0 && (start == nullptr || end == nullptr))) {
    set_err(err, errlen, modle_pixels_detail::refusal(name, cs, kRule));
    return MODLE_PIXELS_ERR_ARG;
  }
  const hipStream_t st = static_cast<hipStream_t>(stream);
  int rc = modle_pixels_detail::resolve_band(h, d_band, nrows, ncols, cs, &v, st, err, errlen);
  if (rc != MODLE_PIXELS_OK) return rc;
  const uint64_t RR = R * R;
  rc = modle_pixels_detail::sums_to_host(h, 2 * RR + 1, pile, st, err, errlen, [&](uint64_t* d_out) {
    const int64_t* d[2];
    const int up = modle_pixels_detail::upload_lists(h, start, end, n, d, st, err, errlen);
    if (up != MODLE_PIXELS_OK) return up;
    return rescale_impl(h, v.d, v.nrows, v.ncols, R, bin_offset, d[0], d[1], n, d_out, d_out + RR, d_out + 2 * RR, st,
                        err, errlen);
  });
  if (rc != MODLE_PIXELS_OK) return rc;
  *area = *pile + RR;
  *n_used = *pile + 2 * RR;
  return MODLE_PIXELS_OK;
}

}  // namespace

extern "C" uint64_t modle_pixels_rescale_groups(void) { return kMaxGroups; }

extern "C" int modle_pixels_rescale_accepts(uint64_t nrows, uint64_t ncols, uint64_t size, int64_t bin_offset,
                                            const int64_t* start, const int64_t* end, uint64_t n, uint8_t* accept) {
  if (bad_rescale(nrows, ncols, size, n) || (n != 0 && (start == nullptr || end == nullptr || accept == nullptr)))
    return MODLE_PIXELS_ERR_ARG;
  for (uint64_t t = 0; t < n; ++t) {
    uint64_t s = 0, w = 0;
    accept[t] = rescale_accept(nrows, ncols, size, bin_offset, start[t], end[t], &s, &w) ? 1 : 0;
  }
  return MODLE_PIXELS_OK;
}

extern "C" int modle_pixels_rescale(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows, uint64_t ncols,
                                    uint64_t size, int64_t bin_offset, const int64_t* d_start, const int64_t* d_end,
                                    uint64_t n, uint64_t* d_pile, uint64_t* d_area, uint64_t* d_n_used, void* stream,
                                    char* err, size_t errlen) {
  if (h == nullptr || d_band == nullptr || d_pile == nullptr || bad_rescale(nrows, ncols, size, n) ||
      (n != 0 && (d_start == nullptr || d_end == nullptr)) || (reinterpret_cast<uintptr_t>(d_pile) & 7) != 0 ||
      (reinterpret_cast<uintptr_t>(d_area) & 7) != 0 || (reinterpret_cast<uintptr_t>(d_n_used) & 7) != 0) {
    set_err(err, errlen, std::string("modle_pixels_rescale: invalid argument ") + kRule);
    return MODLE_PIXELS_ERR_ARG;
  }
  const uint64_t nb = modle_pixels_detail::band_bytes(nrows, ncols), np = size * size * 8;
  if (modle_pixels_detail::any_overlap({{d_pile, np}, {d_area, np}, {d_n_used, 8}},
                                       {{d_band, nb}, {d_start, n * 8}, {d_end, n * 8}})) {
    set_err(err, errlen, "modle_pixels_rescale: an output overlaps the band, the windows or another output");
    return MODLE_PIXELS_ERR_ARG;
  }
  return rescale_impl(h, d_band, nrows, ncols, size, bin_offset, d_start, d_end, n, d_pile, d_area, d_n_used,
                      static_cast<hipStream_t>(stream), err, errlen);
}

extern "C" int modle_pixels_rescale_to_host(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                                            uint64_t ncols, uint64_t size, int64_t bin_offset, const int64_t* start,
                                            const int64_t* end, uint64_t n, const uint64_t** pile,
                                            const uint64_t** area, const uint64_t** n_used, void* stream, char* err,
                                            size_t errlen) {
  return rescale_one_call("modle_pixels_rescale_to_host", nullptr, h, d_band, nrows, ncols, size, bin_offset, start, end,
                          n, pile, area, n_used, stream, err, errlen);
}

extern "C" int modle_pixels_coarse_rescale_to_host(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                                                   uint64_t ncols, uint64_t factor, uint64_t first_bin, uint64_t size,
                                                   int64_t bin_offset, const int64_t* start, const int64_t* end,
                                                   uint64_t n, const uint64_t** pile, const uint64_t** area,
                                                   const uint64_t** n_used, void* stream, char* err, size_t errlen) {
  const modle_pixels_detail::CoarseSpec cs{factor, first_bin};
  return rescale_one_call("modle_pixels_coarse_rescale_to_host", &cs, h, d_band, nrows, ncols, size, bin_offset, start,
                          end, n, pile, area, n_used, stream, err, errlen);
}
