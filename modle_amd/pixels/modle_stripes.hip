// modle_stripes.hip -- two band matrices compared stripe by stripe, on the MI355X
// (include/modle_pixels.h: modle_pixels_stripes / _stripes_to_host / _stripes_rows).
//
// For bin c the vertical stripe is v[i] = M(c - i, c) = band[c * nrows + i], i <= c, and the horizontal
// stripe h[i] = M(c, c + i) = band[(c + i) * nrows + i], c + i < ncols; both have nrows entries, zeros where
// the matrix ends.  Per direction and bin the library writes the integer sums a correlation or a distance of
// the two stripes is made of; pixels.stripe_scores states the scores on the host.  Three kernels, all
// output-stationary -- a stripe has one owner, nothing is cleared beforehand, there are no atomics and every
// output word is stored once, with a plain store:
//
//   vertical moments    a wave owns a stripe: its words are contiguous, the lanes take them 64 at a time
//                       (four loads in flight) and the sums meet in a wave reduction;
//   horizontal moments  a workgroup owns the 64 stripes c0 .. c0 + 63 and lane l of every wave stands for
//                       stripe c0 + l.  Of column j = c0 + jj of the band the words i = jj - l, 64 contiguous
//                       ones, belong to these stripes, one per lane: a wave reads them in one load and every
//                       lane adds its own.  The four waves take the columns in turn and meet in LDS.  So every
//                       pixel word is read once, in memory order, without a sheared copy of the band;
//   ranks               a workgroup owns one stripe of one direction: both stripes go to LDS padded with the
//                       largest key to a power of two, a bitonic network sorts them there, and every lane
//                       finds #less and #equal of its entries, read again from the band, by a lower- and an
//                       upper-bound search over the first nrows sorted keys.  (A padding key that equals a
//                       count of 0xFFFFFFFF is no trouble: equal keys are interchangeable.)
//
// The second moments are 128-bit sums in two words: a product of two uint32 fits 64 bits, the carry of the
// low word is counted in the high one.  Every index is a function of nrows and ncols alone: the words with
// i > j (the left-edge triangle) and the trailing word are never addressed, whatever the bands hold.
//
// LDS: ranks 2 * P * 4 bytes for P = nrows rounded up to a power of two, 32 KiB at the cap of 4096 (five
// workgroups = 20 waves on a CU's 160 KiB); horizontal moments 3 waves * 9 or 18 rows * 64 words: 13.5 / 27 KiB.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "modle_pixels.h"
#include "pixels_context.h"
#include "pixels_device.h"

namespace {

using modle_pixels_device::add128;
using modle_pixels_device::u64;
using modle_pixels_device::wave_sum;

constexpr unsigned kBins = 64;      // stripes of a workgroup of the horizontal kernel = lanes of a wave
constexpr unsigned kWaves = 4;      // waves of a workgroup
constexpr unsigned kUnroll = 4;     // loads in flight per lane
constexpr unsigned kMomRows = 9;    // n, Sa, Sb, Saa, Sbb, Sab (the last three in two words)
constexpr unsigned kRankRows = 3;   // Raa, Rbb, Rab
// workgroups of a launch, 2^20 (pixels_context.h); the kernels stride over what is beyond
constexpr unsigned kMaxGrid = MODLE_STRIPES_MAX_GRID;
constexpr uint64_t kAll = MODLE_PIXELS_STRIPES_MOMENTS | MODLE_PIXELS_STRIPES_MASKED | MODLE_PIXELS_STRIPES_RANKS;

// the nine words of a stripe pair, in the order of the output rows
// (Acc of modle_scc.hip is not merged with this: either layout is its pinned output rows, 9 and 11 words, and n is
// counted differently; only add128 underneath is shared)
struct Mom {
  u64 w[kMomRows];
};

__device__ __forceinline__ void mom_zero(Mom& m) {
#pragma unroll
  for (unsigned k = 0; k < kMomRows; ++k) m.w[k] = 0;
}

// one entry (a, b) of the pair; n is counted by the caller
__device__ __forceinline__ void mom_add(Mom& m, uint32_t a, uint32_t b) {
  m.w[1] += a;
  m.w[2] += b;
  add128(m.w[3], m.w[4], static_cast<u64>(a) * a, 0);
  add128(m.w[5], m.w[6], static_cast<u64>(b) * b, 0);
  add128(m.w[7], m.w[8], static_cast<u64>(a) * b, 0);
}

__device__ __forceinline__ void mom_merge(Mom& m, const Mom& o) {
  m.w[0] += o.w[0];
  m.w[1] += o.w[1];
  m.w[2] += o.w[2];
  add128(m.w[3], m.w[4], o.w[3], o.w[4]);
  add128(m.w[5], m.w[6], o.w[5], o.w[6]);
  add128(m.w[7], m.w[8], o.w[7], o.w[8]);
}

// The sums a kernel keeps per stripe: over all entries (kWhat & 1) and over those where both are non-zero
// (kWhat & 2).  The set that is not asked for is never touched and costs no register.
template <unsigned kWhat>
struct Acc {
  static constexpr unsigned kSets = (kWhat & 1 ? 1 : 0) + (kWhat & 2 ? 1 : 0);
  Mom plain, masked;
  __device__ __forceinline__ void zero() {
    if (kWhat & 1) mom_zero(plain);
    if (kWhat & 2) mom_zero(masked);
  }
  // (an entry of the zero padding adds nothing to either set)
  __device__ __forceinline__ void add(uint32_t a, uint32_t b) {
    if (kWhat & 1) mom_add(plain, a, b);
    if (kWhat & 2) {
      const bool both = a != 0 && b != 0;
      mom_add(masked, both ? a : 0u, both ? b : 0u);
      masked.w[0] += both ? 1u : 0u;
    }
  }
  __device__ __forceinline__ void merge(const Acc& o) {
    if (kWhat & 1) mom_merge(plain, o.plain);
    if (kWhat & 2) mom_merge(masked, o.masked);
  }
  // set s < kSets, in the order of the output blocks
  __device__ __forceinline__ Mom& set(unsigned s) { return (kWhat & 1) && s == 0 ? plain : masked; }
  // the rows of stripe c of one direction; the padding counts among the n of the unmasked sums
  __device__ __forceinline__ void store(u64* __restrict__ out, u64 ncols, u64 c, u64 nrows) {
    if (kWhat & 1) plain.w[0] = nrows;
#pragma unroll
    for (unsigned s = 0; s < kSets; ++s)
#pragma unroll
      for (unsigned k = 0; k < kMomRows; ++k) out[(s * kMomRows + k) * ncols + c] = set(s).w[k];
  }
};

template <unsigned kWhat>
__global__ __launch_bounds__(64 * kWaves) void stripes_vertical(const uint32_t* __restrict__ ref,
                                                                const uint32_t* __restrict__ tgt, u64 nrows,
                                                                u64 ncols, u64* __restrict__ out) {
  const unsigned lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (u64 c = static_cast<u64>(blockIdx.x) * kWaves + wv; c < ncols; c += static_cast<u64>(gridDim.x) * kWaves) {
    const unsigned len = static_cast<unsigned>(min(c + 1, nrows));  // the words i <= c: the others are no pixels
    const uint32_t* a = ref + c * nrows;
    const uint32_t* b = tgt + c * nrows;
    Acc<kWhat> acc;
    acc.zero();
    for (unsigned i0 = 0; i0 < len; i0 += kUnroll * 64) {
      uint32_t va[kUnroll], vb[kUnroll];
#pragma unroll
      for (unsigned u = 0; u < kUnroll; ++u) {
        const unsigned i = i0 + u * 64 + lane;
        va[u] = i < len ? a[i] : 0u;
        vb[u] = i < len ? b[i] : 0u;
      }
#pragma unroll
      for (unsigned u = 0; u < kUnroll; ++u) acc.add(va[u], vb[u]);
    }
    // (not pixels_device.h's wave_sum: the words of a 128-bit sum merge with a carry, so a step shifts the whole
    // struct, word by word, and merges it)
#pragma unroll
    for (unsigned s = 32; s > 0; s >>= 1) {
      Acc<kWhat> o;
#pragma unroll
      for (unsigned t = 0; t < Acc<kWhat>::kSets; ++t)
#pragma unroll
        for (unsigned k = 0; k < kMomRows; ++k) o.set(t).w[k] = __shfl_down(acc.set(t).w[k], s);
      acc.merge(o);
    }
    if (lane == 0) acc.store(out, ncols, c, nrows);
  }
}

template <unsigned kWhat>
__global__ __launch_bounds__(kBins * kWaves) void stripes_horizontal(const uint32_t* __restrict__ ref,
                                                                     const uint32_t* __restrict__ tgt, u64 nrows,
                                                                     u64 ncols, u64* __restrict__ out) {
  constexpr unsigned kWords = Acc<kWhat>::kSets * kMomRows;
  __shared__ u64 lds[(kWaves - 1) * kWords * kBins];
  const unsigned lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (u64 c0 = static_cast<u64>(blockIdx.x) * kBins; c0 < ncols; c0 += static_cast<u64>(gridDim.x) * kBins) {
    Acc<kWhat> acc;
    acc.zero();
    // the columns c0 + jj, jj < jn, hold the words of these stripes; stripe c0 + lane has i = jj - lane there
    const u64 jn = min(kBins - 1 + nrows, ncols - c0);
    for (u64 jj0 = wv; jj0 < jn; jj0 += kWaves * kUnroll) {  // (the same in every lane of the wave)
      uint32_t va[kUnroll], vb[kUnroll];
#pragma unroll
      for (unsigned u = 0; u < kUnroll; ++u) {
        const u64 jj = jj0 + u * kWaves;
        // 0 <= i < nrows and j < ncols: a pixel (i <= j as lane <= c0 + lane) of the stripe c0 + lane <= j
        const bool ok = jj < jn && jj >= lane && jj - lane < nrows;
        const u64 at = (c0 + jj) * nrows + (jj - lane);
        va[u] = ok ? ref[at] : 0u;
        vb[u] = ok ? tgt[at] : 0u;
      }
#pragma unroll
      for (unsigned u = 0; u < kUnroll; ++u) acc.add(va[u], vb[u]);
    }
    // the four waves' sums meet in LDS; wave 0 stores every output word once
    if (wv != 0) {
#pragma unroll
      for (unsigned s = 0; s < Acc<kWhat>::kSets; ++s)
#pragma unroll
        for (unsigned k = 0; k < kMomRows; ++k)
          lds[((wv - 1) * kWords + s * kMomRows + k) * kBins + lane] = acc.set(s).w[k];
    }
    __syncthreads();
    if (wv == 0) {
#pragma unroll
      for (unsigned x = 0; x < kWaves - 1; ++x) {
        Acc<kWhat> o;
#pragma unroll
        for (unsigned s = 0; s < Acc<kWhat>::kSets; ++s)
#pragma unroll
          for (unsigned k = 0; k < kMomRows; ++k) o.set(s).w[k] = lds[(x * kWords + s * kMomRows + k) * kBins + lane];
        acc.merge(o);
      }
      if (c0 + lane < ncols) acc.store(out, ncols, c0 + lane, nrows);
    }
    __syncthreads();  // the rows are free for the next group of stripes
  }
}

// entry i < nrows of the stripe of bin c: direction 0 vertical, 1 horizontal
__device__ __forceinline__ uint32_t stripe_word(const uint32_t* __restrict__ band, u64 nrows, u64 ncols,
                                                unsigned dir, u64 c, unsigned i) {
  if (dir == 0) return i <= c ? band[c * nrows + i] : 0u;
  return c + i < ncols ? band[(c + i) * nrows + i] : 0u;
}

// #{y < x} + #{y <= x} + 1 over the n sorted keys: the doubled average rank of x
__device__ __forceinline__ unsigned rank2(const uint32_t* keys, unsigned n, uint32_t x) {
  unsigned lo = 0, hi = n;  // the first key >= x
  while (lo < hi) {
    const unsigned mid = (lo + hi) >> 1;
    if (keys[mid] < x) lo = mid + 1; else hi = mid;
  }
  const unsigned less = lo;
  hi = n;  // the first key > x (not before `less`)
  while (lo < hi) {
    const unsigned mid = (lo + hi) >> 1;
    if (keys[mid] <= x) lo = mid + 1; else hi = mid;
  }
  return less + lo + 1;
}

// pow2: nrows rounded up to a power of two, at most MODLE_PIXELS_MAX_STRIPE; `out` is the first rank row
// of direction 0 and `dir_words` the words from one direction to the next
__global__ __launch_bounds__(64 * kWaves) void stripes_ranks(const uint32_t* __restrict__ ref,
                                                             const uint32_t* __restrict__ tgt, u64 nrows, u64 ncols,
                                                             unsigned pow2, u64* __restrict__ out, u64 dir_words) {
  extern __shared__ uint32_t keys[];  // the sorted stripe of ref, then of tgt: pow2 words each
  __shared__ u64 part[kWaves][kRankRows];
  uint32_t* ka = keys;
  uint32_t* kb = keys + pow2;
  const unsigned n = static_cast<unsigned>(nrows), tid = threadIdx.x, dir = blockIdx.y;
  for (u64 c = blockIdx.x; c < ncols; c += gridDim.x) {  // (the same in every thread of the workgroup)
    for (unsigned i = tid; i < pow2; i += 64 * kWaves) {
      ka[i] = i < n ? stripe_word(ref, nrows, ncols, dir, c, i) : 0xFFFFFFFFu;
      kb[i] = i < n ? stripe_word(tgt, nrows, ncols, dir, c, i) : 0xFFFFFFFFu;
    }
    __syncthreads();
    for (unsigned k = 2; k <= pow2; k <<= 1)
      for (unsigned j = k >> 1; j > 0; j >>= 1) {
        for (unsigned t = tid; t < pow2 / 2; t += 64 * kWaves) {
          const unsigned lo = 2 * t - (t & (j - 1)), hi = lo + j;  // lo has bit j clear; hi < pow2
          const bool up = (lo & k) == 0;
          const uint32_t xa = ka[lo], ya = ka[hi], xb = kb[lo], yb = kb[hi];
          if ((xa > ya) == up) ka[lo] = ya, ka[hi] = xa;
          if ((xb > yb) == up) kb[lo] = yb, kb[hi] = xb;
        }
        __syncthreads();
      }
    u64 r[kRankRows] = {0, 0, 0};
    for (unsigned i = tid; i < n; i += 64 * kWaves) {
      const u64 ra = rank2(ka, n, stripe_word(ref, nrows, ncols, dir, c, i));
      const u64 rb = rank2(kb, n, stripe_word(tgt, nrows, ncols, dir, c, i));
      r[0] += ra * ra;  // (below 2^27 each, at most 4096 of them)
      r[1] += rb * rb;
      r[2] += ra * rb;
    }
#pragma unroll
    for (unsigned k = 0; k < kRankRows; ++k) r[k] = wave_sum(r[k]);
    if ((tid & 63) == 0)
#pragma unroll
      for (unsigned k = 0; k < kRankRows; ++k) part[tid >> 6][k] = r[k];
    __syncthreads();
    if (tid < kRankRows) {
      u64 sum = 0;
#pragma unroll
      for (unsigned x = 0; x < kWaves; ++x) sum += part[x][tid];
      out[dir * dir_words + tid * ncols + c] = sum;
    }
    __syncthreads();  // the keys and the partial sums are free for the next stripe
  }
}

using modle_pixels_detail::set_err;

int rows_of(uint64_t what) {
  return (what & MODLE_PIXELS_STRIPES_MOMENTS ? kMomRows : 0) + (what & MODLE_PIXELS_STRIPES_MASKED ? kMomRows : 0) +
         (what & MODLE_PIXELS_STRIPES_RANKS ? kRankRows : 0);
}

// what both entry points refuse of the shape and the mask
bool bad_request(uint64_t nrows, uint64_t ncols, uint64_t what) {
  return nrows == 0 || modle_pixels_detail::bad_shape(nrows, ncols) || what == 0 || (what & ~kAll) != 0 ||
         ((what & MODLE_PIXELS_STRIPES_RANKS) != 0 && nrows > MODLE_PIXELS_MAX_STRIPE);
}

constexpr const char* kRule =
    "(0 < nrows <= ncols, `what` a non-empty mask of MOMENTS 1, MASKED 2, RANKS 4, RANKS with nrows <= 4096 only, "
    "out_words == 2 * rows * ncols, an 8-byte aligned output)";

template <unsigned kWhat>
void launch_moments(const uint32_t* d_ref, const uint32_t* d_tgt, uint64_t nrows, uint64_t ncols, u64* out,
                    uint64_t dir_words, hipStream_t stream) {
  const unsigned gv = static_cast<unsigned>(std::min<uint64_t>((ncols + kWaves - 1) / kWaves, kMaxGrid));
  const unsigned gh = static_cast<unsigned>(std::min<uint64_t>((ncols + kBins - 1) / kBins, kMaxGrid));
  hipLaunchKernelGGL(stripes_vertical<kWhat>, dim3(gv), dim3(64 * kWaves), 0, stream, d_ref, d_tgt, nrows, ncols, out);
  hipLaunchKernelGGL(stripes_horizontal<kWhat>, dim3(gh), dim3(kBins * kWaves), 0, stream, d_ref, d_tgt, nrows, ncols,
                     out + dir_words);
}

// enqueues the kernels on checked arguments
int stripes_impl(modle_pixels_handle* h, const uint32_t* d_ref, const uint32_t* d_tgt, uint64_t nrows,
                 uint64_t ncols, uint64_t what, uint64_t* d_out, hipStream_t stream, char* err, size_t errlen) {
  PIX_TRY(hipSetDevice(h->device));
  u64* out = reinterpret_cast<u64*>(d_out);
  const uint64_t dir_words = static_cast<uint64_t>(rows_of(what)) * ncols;
  switch (what & (MODLE_PIXELS_STRIPES_MOMENTS | MODLE_PIXELS_STRIPES_MASKED)) {
    case 1: launch_moments<1>(d_ref, d_tgt, nrows, ncols, out, dir_words, stream); break;
    case 2: launch_moments<2>(d_ref, d_tgt, nrows, ncols, out, dir_words, stream); break;
    case 3: launch_moments<3>(d_ref, d_tgt, nrows, ncols, out, dir_words, stream); break;
    default: break;
  }
  PIX_TRY(hipGetLastError());
  if (what & MODLE_PIXELS_STRIPES_RANKS) {
    unsigned pow2 = 1;
    while (pow2 < nrows) pow2 *= 2;
    const dim3 grid(static_cast<unsigned>(std::min<uint64_t>(ncols, kMaxGrid)), 2);
    hipLaunchKernelGGL(stripes_ranks, grid, dim3(64 * kWaves), size_t{2} * pow2 * sizeof(uint32_t), stream, d_ref,
                       d_tgt, nrows, ncols, pow2, out + (dir_words - uint64_t{kRankRows} * ncols), dir_words);
    PIX_TRY(hipGetLastError());
  }
  return MODLE_PIXELS_OK;
}

}  // namespace

extern "C" int modle_pixels_stripes_rows(uint64_t what) {
  return what == 0 || (what & ~kAll) != 0 ? MODLE_PIXELS_ERR_ARG : rows_of(what);
}

extern "C" int modle_pixels_stripes(modle_pixels_handle* h, const uint32_t* d_ref, const uint32_t* d_tgt,
                                    uint64_t nrows, uint64_t ncols, uint64_t what, uint64_t* d_out,
                                    uint64_t out_words, void* stream, char* err, size_t errlen) {
  if (h == nullptr || d_ref == nullptr || d_tgt == nullptr || d_out == nullptr || bad_request(nrows, ncols, what) ||
      out_words != 2 * static_cast<uint64_t>(rows_of(what)) * ncols || (reinterpret_cast<uintptr_t>(d_out) & 7) != 0) {
    set_err(err, errlen, std::string("modle_pixels_stripes: invalid argument ") + kRule);
    return MODLE_PIXELS_ERR_ARG;
  }
  const uint64_t band = modle_pixels_detail::band_bytes(nrows, ncols);
  if (modle_pixels_detail::any_overlap({{d_out, out_words * 8}}, {{d_ref, band}, {d_tgt, band}})) {
    set_err(err, errlen, "modle_pixels_stripes: the output overlaps a band");
    return MODLE_PIXELS_ERR_ARG;
  }
  return stripes_impl(h, d_ref, d_tgt, nrows, ncols, what, d_out, static_cast<hipStream_t>(stream), err, errlen);
}

extern "C" int modle_pixels_stripes_to_host(modle_pixels_handle* h, const uint32_t* d_ref, const uint32_t* d_tgt,
                                            uint64_t nrows, uint64_t ncols, uint64_t what, const uint64_t** rows,
                                            void* stream, char* err, size_t errlen) {
  if (rows != nullptr) *rows = nullptr;
  if (h == nullptr || d_ref == nullptr || d_tgt == nullptr || rows == nullptr || bad_request(nrows, ncols, what)) {
    set_err(err, errlen, std::string("modle_pixels_stripes_to_host: invalid argument ") + kRule);
    return MODLE_PIXELS_ERR_ARG;
  }
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const uint64_t words = 2 * static_cast<uint64_t>(rows_of(what)) * ncols;
  return modle_pixels_detail::sums_to_host(h, words, rows, st, err, errlen, [&](uint64_t* d_out) {
    return stripes_impl(h, d_ref, d_tgt, nrows, ncols, what, d_out, st, err, errlen);
  });
}
