// modle_pileup.hip -- pileups of a band matrix, summed on the MI355X (include/modle_pixels.h:
// modle_pixels_pileup / _pileup_to_host / _coarse_pileup_to_host, and the host-only
// modle_pixels_pileup_accepts).
//
// pile[r][c] is the sum over the accepted anchors (a, b) of M(a - f + r, b - f + c), M the symmetric
// matrix of the band.  With d = b - a and e = d + c - r the cell is the word
//     e >= 0:  band[(b - f + c) * nrows + e]        (on or above the diagonal)
//     e <  0:  band[(a - f + r) * nrows - e]        (below it: read through the symmetry)
// so for a fixed window column c the S cells are consecutive words of one band column, descending in r:
// lanes run fastest over r, and the lanes of one window column share cache lines.
//
// The kernel is output-stationary.  A workgroup of 256 lanes takes a contiguous chunk of the anchors (an
// equal share, of at least 8 while there are that many) in batches of 256: every lane loads and judges one anchor, the accepted ones are packed into LDS (ballot
// and prefix count, no atomics), then all lanes walk the packed list, lane l owning the cells
// q = l + 256 k (r = q % S, c = q / S) in ceil(S * S / 256) 64-bit registers -- 1, 4 or 17 of them, a
// compile-time class per flank.  A lane whose q lies beyond the window reads cell 0 again and is not
// stored.  At the end every workgroup stores its S * S partial sums (in the lanes' order) and its count of
// accepted anchors into the context's scratch with plain stores, and a second kernel adds the partials per
// cell and stores the pile row-major: one lane per output word, nothing cleared beforehand.  The grid is capped at kPileupGroups workgroups, so the
// partials stay below 9 MiB.  Rejected anchors are never turned into an address; an accepted window
// lies in the band, so no word that is no pixel is read.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "modle_pixels.h"
#include "pixels_context.h"
#include "pixels_device.h"

namespace {

using modle_pixels_device::u64;

constexpr unsigned kBatch = 256;         // lanes of a workgroup = anchors of a batch
constexpr unsigned kPileupGroups = 256;  // workgroups at most: MODLE_PIXELS_PILEUP_GROUPS
constexpr unsigned kMinChunk = 8;        // anchors of a workgroup at least (while there are that many)
constexpr unsigned kSumCells = 64;       // cells of a workgroup of pixels_pileup_sum, each added up by 4 lanes
static_assert(kPileupGroups == MODLE_PIXELS_PILEUP_GROUPS, "the header states the cap");
static_assert(MODLE_PIXELS_MAX_PILEUP_FLANK == 32, "the accumulator classes end at 17 * 256 >= 65 * 65 cells");

// The acceptance rule, for any int64 input.  2 * f + 1 <= nrows <= ncols holds (the callers check it).
// a = bin1 - off and b = bin2 - off are formed only once they are known to be non-negative: then the
// differences fit 64 unsigned bits exactly, and everything after is unsigned and cannot wrap.
__host__ __device__ inline bool pileup_accept(uint64_t nrows, uint64_t ncols, uint64_t f, int64_t off, int64_t bin1,
                                              int64_t bin2, uint64_t* a_out, uint64_t* b_out) {
  if (bin1 < off || bin2 < off) return false;  // a < 0 <= f, or b < 0 <= a
  const uint64_t a = static_cast<uint64_t>(bin1) - static_cast<uint64_t>(off);
  const uint64_t b = static_cast<uint64_t>(bin2) - static_cast<uint64_t>(off);
  *a_out = a, *b_out = b;
  return a <= b && a >= f && b <= ncols - 1 - f && b - a <= nrows - 1 - 2 * f;
}

template <unsigned kAcc>
__global__ __launch_bounds__(kBatch) void pixels_pileup(const uint32_t* __restrict__ band, uint64_t nrows,
                                                        uint64_t ncols, unsigned f, int64_t bin_offset,
                                                        const int64_t* __restrict__ bin1,
                                                        const int64_t* __restrict__ bin2, uint64_t n,
                                                        u64* __restrict__ partial, u64* __restrict__ counts) {
  // anchors of a walk step in flight: 8, 16 or 34 loads per lane
  constexpr unsigned kWalk = kAcc == 1 ? 8 : kAcc <= 4 ? 4 : 2;
  __shared__ u64 sa[kBatch], sb[kBatch];  // the accepted anchors of the batch, packed
  __shared__ unsigned wcount[kBatch / 64];
  const unsigned tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const unsigned S = 2 * f + 1, SS = S * S;
  const unsigned used = (SS + kBatch - 1) / kBatch;  // accumulators in use (the same in every lane)

  int cr[kAcc], rr[kAcc];  // c - f and r - f of this lane's cells
  u64 acc[kAcc];
#pragma unroll
  for (unsigned k = 0; k < kAcc; ++k) {
    const unsigned q = tid + kBatch * k;
    const unsigned c = q < SS ? q / S : 0, r = q < SS ? q - c * S : 0;
    cr[k] = static_cast<int>(c) - static_cast<int>(f);
    rr[k] = static_cast<int>(r) - static_cast<int>(f);
    acc[k] = 0;
  }

  u64 n_used = 0;
  // workgroup g of G takes the anchors [g n / G, (g + 1) n / G): contiguous, none empty for G <= n, and
  // sizes that differ by one at most (g < 2^8 and n < 2^31: the products fit)
  const uint64_t t0 = blockIdx.x * n / gridDim.x, t1 = (blockIdx.x + uint64_t{1}) * n / gridDim.x;
  for (uint64_t base = t0; base < t1; base += kBatch) {  // (the same in every lane)
    const uint64_t t = base + tid;
    uint64_t a = 0, b = 0;
    const bool ok = t < t1 && pileup_accept(nrows, ncols, f, bin_offset, bin1[t], bin2[t], &a, &b);
    const u64 mask = __ballot(ok);
    if (lane == 0) wcount[wv] = __popcll(mask);
    __syncthreads();
    unsigned before = 0, total = 0;
#pragma unroll
    for (unsigned x = 0; x < kBatch / 64; ++x) {
      before += x < wv ? wcount[x] : 0;
      total += wcount[x];
    }
    if (ok) {
      const unsigned slot = before + __popcll(mask & ((1ull << lane) - 1));
      sa[slot] = a, sb[slot] = b;
    }
    __syncthreads();
    n_used += total;

#pragma unroll kWalk
    for (unsigned s = 0; s < total; ++s) {
      const uint64_t wa = sa[s], wb = sb[s];  // (a broadcast: every lane reads the same word)
      const int64_t d = static_cast<int64_t>(wb - wa);
#pragma unroll
      for (unsigned k = 0; k < kAcc; ++k) {
        if (k < used) {  // (the same in every lane)
          const int64_t e = d + (cr[k] - rr[k]);
          const uint64_t col = e >= 0 ? wb + static_cast<int64_t>(cr[k]) : wa + static_cast<int64_t>(rr[k]);
          const uint64_t dg = static_cast<uint64_t>(e >= 0 ? e : -e);
          acc[k] += band[col * nrows + dg];
        }
      }
    }
    __syncthreads();  // the list and the counts are free for the next batch
  }

  u64* mine = partial + static_cast<uint64_t>(blockIdx.x) * SS;
#pragma unroll
  for (unsigned k = 0; k < kAcc; ++k) {
    const unsigned q = tid + kBatch * k;
    if (q < SS) mine[q] = acc[k];
  }
  if (tid == 0) counts[blockIdx.x] = n_used;
}

// The partials are in the lanes' order, q = c * S + r.  A workgroup owns kSumCells cells; four lanes share a
// cell, each adding every fourth workgroup's partial (coalesced reads, eight in flight), meet in LDS, and one
// of them stores pile[r][c], row-major.  Cell S * S stands for the counts of accepted anchors.
__global__ __launch_bounds__(4 * kSumCells) void pixels_pileup_sum(const u64* __restrict__ partial,
                                                                   const u64* __restrict__ counts, unsigned groups,
                                                                   unsigned S, u64* __restrict__ pile,
                                                                   u64* __restrict__ n_used) {
  __shared__ u64 part[4 * kSumCells];
  const unsigned SS = S * S;
  const unsigned cell = threadIdx.x % kSumCells, slice = threadIdx.x / kSumCells;
  const unsigned q = blockIdx.x * kSumCells + cell;
  u64 sum = 0;
  if (q < SS) {
#pragma unroll 8
    for (unsigned g = slice; g < groups; g += 4) sum += partial[static_cast<uint64_t>(g) * SS + q];
  } else if (q == SS) {
    for (unsigned g = slice; g < groups; g += 4) sum += counts[g];
  }
  part[threadIdx.x] = sum;
  __syncthreads();
  if (slice != 0) return;
  sum = part[cell] + part[kSumCells + cell] + part[2 * kSumCells + cell] + part[3 * kSumCells + cell];
  if (q < SS)
    pile[(q % S) * S + q / S] = sum;
  else if (q == SS && n_used != nullptr)
    *n_used = sum;
}

using modle_pixels_detail::set_err;

constexpr const char* kRule =
    "(0 < nrows <= ncols, flank <= 32, 2 * flank + 1 <= nrows, n < 2^31, anchors unless n == 0, 8-byte aligned "
    "outputs that overlap neither the band nor the anchors)";

// what the numbers alone refuse
bool bad_pileup(uint64_t nrows, uint64_t ncols, uint64_t f, uint64_t n) {
  return nrows == 0 || modle_pixels_detail::bad_shape(nrows, ncols) || f > MODLE_PIXELS_MAX_PILEUP_FLANK ||
         2 * f + 1 > nrows || n >= (uint64_t{1} << 31);
}

// enqueues the two kernels on checked arguments; the anchors and the outputs are device arrays
int pileup_impl(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows, uint64_t ncols, uint64_t f,
                int64_t bin_offset, const int64_t* d_bin1, const int64_t* d_bin2, uint64_t n, uint64_t* d_pile,
                uint64_t* d_n_used, hipStream_t stream, char* err, size_t errlen) {
  PIX_TRY(hipSetDevice(h->device));
  const unsigned S = 2 * static_cast<unsigned>(f) + 1, SS = S * S;
  // one workgroup per kMinChunk anchors until the cap binds: few anchors still spread over the device (the walk
  // of a workgroup is serial in its anchors), many leave every workgroup several batches
  const uint64_t groups = std::min<uint64_t>(kPileupGroups, (n + kMinChunk - 1) / kMinChunk);
  const int rc = h->pile_partial.ensure(groups * (SS + 1), err, errlen);
  if (rc != MODLE_PIXELS_OK) return rc;
  u64* partial = reinterpret_cast<u64*>(h->pile_partial.dev);
  u64* counts = partial + groups * SS;
  if (groups != 0) {
    const dim3 grid(static_cast<unsigned>(groups)), block(kBatch);
    const unsigned ff = static_cast<unsigned>(f);
    if (SS <= kBatch)
      hipLaunchKernelGGL(pixels_pileup<1>, grid, block, 0, stream, d_band, nrows, ncols, ff, bin_offset, d_bin1, d_bin2,
                         n, partial, counts);
    else if (SS <= 4 * kBatch)
      hipLaunchKernelGGL(pixels_pileup<4>, grid, block, 0, stream, d_band, nrows, ncols, ff, bin_offset, d_bin1, d_bin2,
                         n, partial, counts);
    else
      hipLaunchKernelGGL(pixels_pileup<17>, grid, block, 0, stream, d_band, nrows, ncols, ff, bin_offset, d_bin1,
                         d_bin2, n, partial, counts);
    PIX_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(pixels_pileup_sum, dim3(SS / kSumCells + 1), dim3(4 * kSumCells), 0, stream, partial, counts,
                     static_cast<unsigned>(groups), S, reinterpret_cast<u64*>(d_pile),
                     reinterpret_cast<u64*>(d_n_used));
  PIX_TRY(hipGetLastError());
  return MODLE_PIXELS_OK;
}

// modle_pixels_pileup_to_host (`cs` null) and modle_pixels_coarse_pileup_to_host under their `name`: the band
// resolved, the host anchors up, pileup_impl into the sums of the context, their copy to the pinned mirror, the wait
int pileup_one_call(const char* name, const modle_pixels_detail::CoarseSpec* cs, modle_pixels_handle* h,
                    const uint32_t* d_band, uint64_t nrows, uint64_t ncols, uint64_t f, int64_t bin_offset,
                    const int64_t* bin1, const int64_t* bin2, uint64_t n, const uint64_t** pile, const uint64_t** n_used,
                    void* stream, char* err, size_t errlen) {
  if (pile != nullptr) *pile = nullptr;
  if (n_used != nullptr) *n_used = nullptr;
  modle_pixels_detail::BandView v;
  if (h == nullptr || pile == nullptr || n_used == nullptr ||
      !modle_pixels_detail::view_shape(d_band, nrows, ncols, cs, &v) || bad_pileup(v.nrows, v.ncols, f, n) ||
      (n != 0 && (bin1 == nullptr || bin2 == nullptr))) {
    set_err(err, errlen, modle_pixels_detail::refusal(name, cs, kRule));
    return MODLE_PIXELS_ERR_ARG;
  }
  const hipStream_t st = static_cast<hipStream_t>(stream);
  int rc = modle_pixels_detail::resolve_band(h, d_band, nrows, ncols, cs, &v, st, err, errlen);
  if (rc != MODLE_PIXELS_OK) return rc;
  const uint64_t SS = (2 * f + 1) * (2 * f + 1);
  rc = modle_pixels_detail::sums_to_host(h, SS + 1, pile, st, err, errlen, [&](uint64_t* d_out) {
    const int64_t* d[2];
    const int up = modle_pixels_detail::upload_lists(h, bin1, bin2, n, d, st, err, errlen);
    if (up != MODLE_PIXELS_OK) return up;
    return pileup_impl(h, v.d, v.nrows, v.ncols, f, bin_offset, d[0], d[1], n, d_out, d_out + SS, st, err, errlen);
  });
  if (rc == MODLE_PIXELS_OK) *n_used = *pile + SS;
  return rc;
}

}  // namespace

extern "C" int modle_pixels_pileup_accepts(uint64_t nrows, uint64_t ncols, uint64_t flank, int64_t bin_offset,
                                           const int64_t* bin1, const int64_t* bin2, uint64_t n, uint8_t* accept) {
  if (bad_pileup(nrows, ncols, flank, n) || (n != 0 && (bin1 == nullptr || bin2 == nullptr || accept == nullptr)))
    return MODLE_PIXELS_ERR_ARG;
  for (uint64_t t = 0; t < n; ++t) {
    uint64_t a = 0, b = 0;
    accept[t] = pileup_accept(nrows, ncols, flank, bin_offset, bin1[t], bin2[t], &a, &b) ? 1 : 0;
  }
  return MODLE_PIXELS_OK;
}

extern "C" int modle_pixels_pileup(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows, uint64_t ncols,
                                   uint64_t flank, int64_t bin_offset, const int64_t* d_bin1, const int64_t* d_bin2,
                                   uint64_t n, uint64_t* d_pile, uint64_t* d_n_used, void* stream, char* err,
                                   size_t errlen) {
  if (h == nullptr || d_band == nullptr || d_pile == nullptr || bad_pileup(nrows, ncols, flank, n) ||
      (n != 0 && (d_bin1 == nullptr || d_bin2 == nullptr)) || (reinterpret_cast<uintptr_t>(d_pile) & 7) != 0 ||
      (reinterpret_cast<uintptr_t>(d_n_used) & 7) != 0) {
    set_err(err, errlen, std::string("modle_pixels_pileup: invalid argument ") + kRule);
    return MODLE_PIXELS_ERR_ARG;
  }
  const uint64_t nb = modle_pixels_detail::band_bytes(nrows, ncols), np = (2 * flank + 1) * (2 * flank + 1) * 8;
  if (modle_pixels_detail::any_overlap({{d_pile, np}, {d_n_used, 8}}, {{d_band, nb}, {d_bin1, n * 8}, {d_bin2, n * 8}})) {
    set_err(err, errlen, "modle_pixels_pileup: an output overlaps the band, the anchors or the other output");
    return MODLE_PIXELS_ERR_ARG;
  }
  return pileup_impl(h, d_band, nrows, ncols, flank, bin_offset, d_bin1, d_bin2, n, d_pile, d_n_used,
                     static_cast<hipStream_t>(stream), err, errlen);
}

extern "C" int modle_pixels_pileup_to_host(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                                           uint64_t ncols, uint64_t flank, int64_t bin_offset, const int64_t* bin1,
                                           const int64_t* bin2, uint64_t n, const uint64_t** pile,
                                           const uint64_t** n_used, void* stream, char* err, size_t errlen) {
  return pileup_one_call("modle_pixels_pileup_to_host", nullptr, h, d_band, nrows, ncols, flank, bin_offset, bin1, bin2,
                         n, pile, n_used, stream, err, errlen);
}

extern "C" int modle_pixels_coarse_pileup_to_host(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                                                  uint64_t ncols, uint64_t factor, uint64_t first_bin, uint64_t flank,
                                                  int64_t bin_offset, const int64_t* bin1, const int64_t* bin2,
                                                  uint64_t n, const uint64_t** pile, const uint64_t** n_used,
                                                  void* stream, char* err, size_t errlen) {
  const modle_pixels_detail::CoarseSpec cs{factor, first_bin};
  return pileup_one_call("modle_pixels_coarse_pileup_to_host", &cs, h, d_band, nrows, ncols, flank, bin_offset, bin1,
                         bin2, n, pile, n_used, stream, err, errlen);
}
