// modle_coarsen.hip -- a band matrix at `factor` times the bin size, summed on the MI355X
// (include/modle_pixels.h: modle_pixels_coarse_shape / _coarsen / _coarse_to_host).
//
// With k = factor and p = first_bin % k, fine column j belongs to coarse column (j + p) / k.  The
// kernel is output-stationary: one wave owns kCoarseCols consecutive coarse columns J and, in each,
// a run of 64 band words D = J - I, one per lane.  Coarse column J is made of the fine columns
// j = J * k - p + jj, jj < k.  In fine column j the words that belong to output D are the k words
// d = D * k + jj - (k - 1) .. D * k + jj (from i = j - d and (i + p) / k = J - D), so the words the
// 64 outputs of a wave need from one fine column are ONE contiguous span of 64 * k words.  The
// wave reads that span the way it lies in memory (a wave reads 256 contiguous bytes), kChunk words
// at a time, into LDS, and every lane then sums its own k words from there in 64 bits.  Words
// with d < 0 (the lower triangle of a diagonal block), d > j (left of the matrix), d >= nrows or
// j outside [0, ncols) are masked by index and never read.  Every output word is written exactly
// once, by one lane: no atomics, and the result does not depend on the launch geometry.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <limits>

#include "modle_pixels.h"
#include "pixels_context.h"

namespace {

constexpr unsigned kWave = 64;         // one wave per workgroup: its LDS tile is its own
constexpr unsigned kChunk = 1024;      // words of a span staged at a time
constexpr unsigned kCoarseCols = 4;    // coarse columns of one wave
constexpr unsigned kLoadUnroll = 4;    // loads issued together
constexpr uint64_t kMaxFactor = 1ull << 32;

// LDS index of span word e: one pad word per 32, so that lanes that read at a stride of k words
// (lane l reads e = l * k + t) spread over the banks also when k is even
__device__ __forceinline__ unsigned pad(unsigned e) { return e + (e >> 5); }

__global__ __launch_bounds__(kWave) void pixels_coarsen(const uint32_t* __restrict__ band, int64_t nrows,
                                                        int64_t ncols, int64_t k, int64_t p,
                                                        uint32_t* __restrict__ out, int64_t nrows_out,
                                                        int64_t ncols_out, int64_t d_blocks) {
  __shared__ uint32_t tile[kChunk + kChunk / 32];
  const int64_t lane = threadIdx.x;
  const int64_t col_group = static_cast<int64_t>(blockIdx.x) / d_blocks;
  const int64_t D0 = (static_cast<int64_t>(blockIdx.x) % d_blocks) * kWave;
  const int64_t n_out = min(static_cast<int64_t>(kWave), nrows_out - D0);  // outputs of this wave per column
  const int64_t span = n_out * k;
  const int64_t D = D0 + lane;
  if (blockIdx.x == 0 && lane == 0) out[nrows_out * ncols_out] = 0;  // the trailing word

  const int64_t J_end = min((col_group + 1) * static_cast<int64_t>(kCoarseCols), ncols_out);
  for (int64_t J = col_group * kCoarseCols; J < J_end; ++J) {
    unsigned long long acc = 0;
    for (int64_t jj = 0; jj < k; ++jj) {
      const int64_t j = J * k - p + jj;
      if (j < 0 || j >= ncols) continue;            // (the same in every lane)
      const int64_t d_max = min(nrows - 1, j);      // pixels of column j: 0 <= d <= d_max
      const int64_t d_first = D0 * k + jj - (k - 1);  // d of span word 0
      const uint32_t* col = band + j * nrows;
      for (int64_t c0 = 0; c0 < span; c0 += kChunk) {
        const int64_t len = min(static_cast<int64_t>(kChunk), span - c0);
        const int64_t d0 = d_first + c0;
        if (d0 > d_max) break;               // nothing but masked words from here on
        if (d0 + len - 1 < 0) continue;
        for (int64_t e0 = 0; e0 < len; e0 += kLoadUnroll * kWave) {
          uint32_t v[kLoadUnroll];
#pragma unroll
          for (unsigned u = 0; u < kLoadUnroll; ++u) {
            const int64_t e = e0 + u * kWave + lane, d = d0 + e;
            v[u] = (e < len && d >= 0 && d <= d_max) ? col[d] : 0u;
          }
#pragma unroll
          for (unsigned u = 0; u < kLoadUnroll; ++u) {
            const int64_t e = e0 + u * kWave + lane;
            if (e < len) tile[pad(static_cast<unsigned>(e))] = v[u];
          }
        }
        __syncthreads();
        // this lane's words are span words [lane * k, lane * k + k); the part within the chunk
        const int64_t lo = max(lane * k, c0), hi = min(lane * k + k, c0 + len);
        for (int64_t e = lo; e < hi; ++e) acc += tile[pad(static_cast<unsigned>(e - c0))];
        __syncthreads();
      }
      acc = min(acc, 0xFFFFFFFFull);  // saturation is monotone: the sum stays far from 2^64
    }
    // D > J: the left-edge triangle, no pixel (its words were all masked: acc == 0)
    if (D < nrows_out) out[J * nrows_out + D] = static_cast<uint32_t>(acc);
  }
}

int bad_coarsen_args(uint64_t nrows, uint64_t ncols, uint64_t factor) {
  return factor < 2 || factor > kMaxFactor || nrows == 0 || nrows > ncols ||
         modle_pixels_detail::bad_shape(nrows, ncols);
}

void coarse_shape(uint64_t nrows, uint64_t ncols, uint64_t k, uint64_t first_bin, uint64_t* nrows_out,
                  uint64_t* ncols_out) {
  const uint64_t p = first_bin % k;
  *ncols_out = (p + ncols + k - 1) / k;
  *nrows_out = std::min(*ncols_out, (nrows - 1 + k - 1) / k + 1);
}

int coarsen_impl(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows, uint64_t ncols,
                 uint64_t factor, uint64_t first_bin, uint32_t* d_out, uint64_t nrows_out,
                 uint64_t ncols_out, hipStream_t stream, char* err, size_t errlen) {
  const uint64_t d_blocks = (nrows_out + kWave - 1) / kWave;
  const uint64_t blocks = d_blocks * ((ncols_out + kCoarseCols - 1) / kCoarseCols);
  if (blocks > static_cast<uint64_t>(std::numeric_limits<int32_t>::max())) {
    modle_pixels_detail::set_err(err, errlen, "modle_pixels_coarsen: the band is too large for one launch");
    return MODLE_PIXELS_ERR_ARG;
  }
  PIX_TRY(hipSetDevice(h->device));
  hipLaunchKernelGGL(pixels_coarsen, dim3(static_cast<unsigned>(blocks)), dim3(kWave), 0, stream, d_band,
                     static_cast<int64_t>(nrows), static_cast<int64_t>(ncols), static_cast<int64_t>(factor),
                     static_cast<int64_t>(first_bin % factor), d_out, static_cast<int64_t>(nrows_out),
                     static_cast<int64_t>(ncols_out), static_cast<int64_t>(d_blocks));
  PIX_TRY(hipGetLastError());
  return MODLE_PIXELS_OK;
}

}  // namespace

bool modle_pixels_detail::view_shape(const uint32_t* d_band, uint64_t nrows, uint64_t ncols, const CoarseSpec* cs,
                                     BandView* v, bool empty_ok) {
  *v = BandView{d_band, nrows, ncols};
  if (cs != nullptr)
    return d_band != nullptr &&
           modle_pixels_coarse_shape(nrows, ncols, cs->factor, cs->first_bin, &v->nrows, &v->ncols) == MODLE_PIXELS_OK;
  if (empty_ok ? d_band == nullptr && ncols != 0 : d_band == nullptr || nrows == 0) return false;
  return !bad_shape(nrows, ncols);
}

int modle_pixels_detail::resolve_band(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows, uint64_t ncols,
                                      const CoarseSpec* cs, BandView* v, hipStream_t stream, char* err,
                                      size_t errlen) {
  if (cs == nullptr) return MODLE_PIXELS_OK;
  PIX_TRY(hipSetDevice(h->device));
  const int rc = h->coarse.ensure(v->nrows * v->ncols + 1, err, errlen);
  if (rc != MODLE_PIXELS_OK) return rc;
  v->d = h->coarse.dev;
  return coarsen_impl(h, d_band, nrows, ncols, cs->factor, cs->first_bin, h->coarse.dev, v->nrows, v->ncols, stream,
                      err, errlen);
}

std::string modle_pixels_detail::refusal(const char* name, const CoarseSpec* cs, const char* rule) {
  return std::string(name) + ": invalid argument " + (cs != nullptr ? "(factor >= 2; of the coarse band:) " : "") + rule;
}

extern "C" int modle_pixels_coarse_shape(uint64_t nrows, uint64_t ncols, uint64_t factor, uint64_t first_bin,
                                         uint64_t* nrows_out, uint64_t* ncols_out) {
  if (nrows_out == nullptr || ncols_out == nullptr || bad_coarsen_args(nrows, ncols, factor))
    return MODLE_PIXELS_ERR_ARG;
  coarse_shape(nrows, ncols, factor, first_bin, nrows_out, ncols_out);
  return MODLE_PIXELS_OK;
}

extern "C" int modle_pixels_coarsen(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                                    uint64_t ncols, uint64_t factor, uint64_t first_bin, uint32_t* d_out,
                                    uint64_t out_words, void* stream, char* err, size_t errlen) {
  if (h == nullptr || d_band == nullptr || d_out == nullptr || bad_coarsen_args(nrows, ncols, factor)) {
    modle_pixels_detail::set_err(err, errlen,
                                 "modle_pixels_coarsen: invalid argument (factor >= 2, 0 < nrows <= ncols)");
    return MODLE_PIXELS_ERR_ARG;
  }
  uint64_t nr = 0, nc = 0;
  coarse_shape(nrows, ncols, factor, first_bin, &nr, &nc);
  if (out_words < nr * nc + 1) {
    modle_pixels_detail::set_err(err, errlen, "modle_pixels_coarsen: out_words is smaller than the coarse band");
    return MODLE_PIXELS_ERR_ARG;
  }
  return coarsen_impl(h, d_band, nrows, ncols, factor, first_bin, d_out, nr, nc,
                      static_cast<hipStream_t>(stream), err, errlen);
}

extern "C" int modle_pixels_coarse_to_host(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                                           uint64_t ncols, uint64_t factor, uint64_t first_bin,
                                           int64_t bin_offset, const int64_t** bin1, const int64_t** bin2,
                                           const int32_t** count, const int64_t** bin1_offset,
                                           modle_pixels_stats* stats, void* stream, char* err,
                                           size_t errlen) {
  const modle_pixels_detail::CoarseSpec cs{factor, first_bin};
  return modle_pixels_detail::pixels_one_call("modle_pixels_coarse_to_host", &cs, h, d_band, nrows, ncols, bin_offset,
                                              bin1, bin2, count, bin1_offset, stats, stream, err, errlen);
}
