// modle_sample.hip -- binomial thinning of a band matrix on the MI355X (include/modle_pixels.h:
// modle_pixels_sample / _sample_to_host, and the host-only modle_pixels_sample_pixels).
//
// Trial t of pixel (I, J) is kept when word t & 3 of philox4x32_10((I, J, t >> 2, salt), seed) is below the
// threshold: the result of a pixel is a pure function of (I, J, n, threshold, seed, salt), so the kernel is
// free in how it spreads the Philox blocks (four trials each) over its lanes.
//
// One lane per word of the band, in memory order: a wave reads 64 contiguous words (256 B) per load and a
// lane has kIters loads in flight.  (j, d) of a lane's words come from one division per workgroup and one
// 32-bit division per lane; from word to word the lane walks the columns (d += 256 mod nrows, a carry into
// j).  The words that are no pixels (d > j, the trailing word) are not loaded and give 0.
//
// The work per word is as skewed as the distance decay: the lane at d = 0 holds hundreds of trials, the
// lane at d = 50 one or none.  Two tiers:
//   tier 1  a lane draws the first kTier1 blocks (MODLE_PIXELS_SAMPLE_TIER1_TRIALS trials) of its own pixel;
//   tier 2  the pixels with more trials, found with a ballot, are taken by the whole wave one after the
//           other: (I, J, n) are read from the owner lane, lane l takes the blocks kTier1 + l + 64 m, the
//           comparisons are counted over the wave (ballots and scalar population counts: the reduction) and
//           the owner lane adds the sum to its word.
// A pixel is never spread over several waves (profiles/sample/sample_vs_torch.txt).  Every word of an output
// is stored once, by its lane, with a plain store; nothing is cleared beforehand, there are no atomics and
// no LDS, and nothing depends on the launch geometry.
#include <hip/hip_runtime.h>

#include "modle_pixels.h"
#include "pixels_context.h"

namespace {

using u32 = uint32_t;  // (64-bit words are uint64_t here: the short name of pixels_device.h is unsigned long long)

constexpr unsigned kThreads = 256;  // lanes of a workgroup
constexpr unsigned kIters = 8;      // words of a lane: 2048 contiguous words per workgroup
#ifndef MODLE_SAMPLE_TIER1_BLOCKS   // (the measurement builds the other boundaries; 0xFFFFFFFF: one tier)
#define MODLE_SAMPLE_TIER1_BLOCKS (MODLE_PIXELS_SAMPLE_TIER1_TRIALS / 4)
#endif
constexpr u32 kTier1 = MODLE_SAMPLE_TIER1_BLOCKS;
static_assert(MODLE_PIXELS_SAMPLE_TIER1_TRIALS % 4 == 0, "tier 1 ends at a Philox block");

// Philox4x32-10 (Salmon et al., SC'11): the arithmetic of modle_amd/csrc/sim_rng.h's round function
__host__ __device__ inline void philox4x32_10(u32 c0, u32 c1, u32 c2, u32 c3, u32 k0, u32 k1, u32 out[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = static_cast<uint64_t>(0xD2511F53u) * c0;
    const uint64_t p1 = static_cast<uint64_t>(0xCD9E8D57u) * c2;
    const u32 n0 = static_cast<u32>(p1 >> 32) ^ c1 ^ k0;
    const u32 n1 = static_cast<u32>(p1);
    const u32 n2 = static_cast<u32>(p0 >> 32) ^ c3 ^ k1;
    const u32 n3 = static_cast<u32>(p0);
    c0 = n0;
    c1 = n1;
    c2 = n2;
    c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0;
  out[1] = c1;
  out[2] = c2;
  out[3] = c3;
}

// what one generator is keyed by, and the threshold below 2^32 (0 and 2^32 take the short paths)
struct Draw {
  u32 k0, k1, salt, thr;
};

// the kept ones of the trials 4 * blk .. 4 * blk + 3 that are below n (blk < ceil(n / 4))
__host__ __device__ inline u32 kept_in_block(const Draw& g, u32 I, u32 J, u32 blk, u32 n) {
  u32 w[4];
  philox4x32_10(I, J, blk, g.salt, g.k0, g.k1, w);
  const u32 left = n - 4 * blk;  // >= 1
  return (w[0] < g.thr) + (left > 1 && w[1] < g.thr) + (left > 2 && w[2] < g.thr) + (left > 3 && w[3] < g.thr);
}

enum Mode : int { kDrawMode = 0, kKeepNone = 1, kKeepAll = 2 };

// the kept ones of the trials of the blocks first .. nblk - 1 of pixel (I, J) with n trials, drawn by the
// whole wave (every argument is the same in every lane): lane l takes the blocks first + l + 64 m, and the
// four comparisons of a round are counted over the wave by ballots, in scalar registers -- the reduction
// costs no cross-lane traffic
__device__ __forceinline__ u32 wave_kept(const Draw& g, u32 I, u32 J, u32 n, u32 first, u32 nblk, unsigned lane) {
  u32 total = 0;
  for (u32 b0 = first; b0 < nblk; b0 += 64) {  // (nblk <= 2^30: b0 + 64 cannot wrap)
    const u32 b = b0 + lane;
    u32 w[4];
    philox4x32_10(I, J, b, g.salt, g.k0, g.k1, w);
    const u32 left = b < nblk ? n - 4 * b : 0u;  // the trials of the lane's block; none beyond the last block
    total += __popcll(__ballot(left > 0 && w[0] < g.thr)) + __popcll(__ballot(left > 1 && w[1] < g.thr)) +
             __popcll(__ballot(left > 2 && w[2] < g.thr)) + __popcll(__ballot(left > 3 && w[3] < g.thr));
  }
  return total;
}

// the kept trials of the lane's pixel (I, J) with n trials (n == 0: a word that gives 0); every lane of the
// wave calls it
__device__ __forceinline__ u32 sample_word(const Draw& g, u32 I, u32 J, u32 n, unsigned lane) {
  const u32 nblk = (n >> 2) + ((n & 3) != 0);
  u32 kept = 0;
  const u32 own = nblk < kTier1 ? nblk : kTier1;
  for (u32 b = 0; b < own; ++b) kept += kept_in_block(g, I, J, b, n);
  unsigned long long todo = __ballot(nblk > kTier1);
  while (todo != 0) {  // (the same in every lane)
    const int src = __builtin_amdgcn_readfirstlane(__ffsll(todo) - 1);
    todo &= todo - 1;
    const u32 pI = __builtin_amdgcn_readlane(I, src), pJ = __builtin_amdgcn_readlane(J, src),
              pn = __builtin_amdgcn_readlane(n, src);
    const u32 more = wave_kept(g, pI, pJ, pn, kTier1, (pn >> 2) + ((pn & 3) != 0), lane);
    if (static_cast<int>(lane) == src) kept += more;
  }
  return kept;
}

__global__ __launch_bounds__(kThreads) void pixels_sample(const u32* __restrict__ band, u32 nrows, uint64_t words,
                                                          u32 id0, Draw g, int mode, u32 step_j, u32 step_d,
                                                          u32* __restrict__ kept_out, u32* __restrict__ rest_out) {
  const unsigned lane = threadIdx.x & 63;
  const uint64_t base = static_cast<uint64_t>(blockIdx.x) * (kThreads * kIters);
  // word base + threadIdx.x is (j, d); `words` = nrows * ncols is the trailing word
  const uint64_t jb = base / nrows;  // (the same in every lane)
  const u32 x = static_cast<u32>(base - jb * nrows) + threadIdx.x;  // < 2^24 + 256
  const u32 q = x / nrows;
  uint64_t j = jb + q;
  u32 d = x - q * nrows;

  u32 n[kIters], I[kIters], J[kIters];
  bool inside[kIters];
#pragma unroll
  for (unsigned u = 0; u < kIters; ++u) {
    const uint64_t w = base + u * kThreads + threadIdx.x;
    inside[u] = w <= words;
    const bool pixel = w < words && d <= j;
    n[u] = pixel ? band[w] : 0u;
    J[u] = id0 + static_cast<u32>(j);  // (the host has checked that the ids fit 32 bits)
    I[u] = J[u] - d;
    j += step_j;
    d += step_d;
    if (d >= nrows) d -= nrows, ++j;
  }
#pragma unroll
  for (unsigned u = 0; u < kIters; ++u) {
    if (base + u * kThreads + (threadIdx.x & ~63u) > words) break;  // (the same in every lane of the wave)
    u32 kept;
    if (mode == kDrawMode)
      kept = sample_word(g, I[u], J[u], n[u], lane);
    else
      kept = mode == kKeepAll ? n[u] : 0u;
    if (inside[u]) {
      const uint64_t w = base + u * kThreads + threadIdx.x;
      if (kept_out != nullptr) kept_out[w] = kept;
      if (rest_out != nullptr) rest_out[w] = n[u] - kept;
    }
  }
}

using modle_pixels_detail::set_err;

constexpr uint64_t kTwo32 = 1ull << 32;

Draw make_draw(uint64_t seed, u32 salt, uint64_t threshold) {
  return Draw{static_cast<u32>(seed), static_cast<u32>(seed >> 32), salt, static_cast<u32>(threshold)};
}

int mode_of(uint64_t threshold) { return threshold == 0 ? kKeepNone : threshold == kTwo32 ? kKeepAll : kDrawMode; }

constexpr const char* kRule =
    "(0 < nrows <= ncols, an output, threshold <= 2^32, a band, its stats; no output overlaps the band or the other)";

// what modle_pixels_sample refuses of shape, threshold and ids: 0, or the error code with the message set
int refuse(const char* who, uint64_t nrows, uint64_t ncols, int64_t bin_offset, uint64_t threshold, bool null_arg,
           char* err, size_t errlen) {
  if (null_arg || nrows == 0 || modle_pixels_detail::bad_shape(nrows, ncols) || threshold > kTwo32 ||
      (nrows * ncols) / (kThreads * kIters) + 1 > 0x7FFFFFFFull) {
    set_err(err, errlen, std::string(who) + ": invalid argument " + kRule);
    return MODLE_PIXELS_ERR_ARG;
  }
  if (bin_offset < 0 || static_cast<uint64_t>(bin_offset) > kTwo32 ||
      static_cast<uint64_t>(bin_offset) + ncols > kTwo32) {
    set_err(err, errlen, std::string(who) + ": the bin ids bin_offset .. bin_offset + ncols - 1 do not fit 32 bits");
    return MODLE_PIXELS_ERR_RANGE;
  }
  return MODLE_PIXELS_OK;
}

int refuse_sum(const char* who, uint64_t sum, char* err, size_t errlen) {
  if (sum <= MODLE_PIXELS_MAX_SAMPLE_TRIALS) return MODLE_PIXELS_OK;
  set_err(err, errlen, std::string(who) + ": the band holds " + std::to_string(sum) +
                           " contacts, above MODLE_PIXELS_MAX_SAMPLE_TRIALS");
  return MODLE_PIXELS_ERR_RANGE;
}

// enqueues the kernel on checked arguments
int sample_impl(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows, uint64_t ncols, int64_t bin_offset,
                uint64_t threshold, uint64_t seed, uint32_t salt, uint32_t* d_kept, uint32_t* d_rest,
                hipStream_t stream, char* err, size_t errlen) {
  PIX_TRY(hipSetDevice(h->device));
  const uint64_t words = nrows * ncols;  // and the trailing word
  const dim3 grid(static_cast<unsigned>(words / (kThreads * kIters) + 1));
  hipLaunchKernelGGL(pixels_sample, grid, dim3(kThreads), 0, stream, d_band, static_cast<u32>(nrows), words,
                     static_cast<u32>(bin_offset), make_draw(seed, salt, threshold), mode_of(threshold),
                     static_cast<u32>(kThreads / nrows), static_cast<u32>(kThreads % nrows), d_kept, d_rest);
  PIX_TRY(hipGetLastError());
  return MODLE_PIXELS_OK;
}

}  // namespace

extern "C" int modle_pixels_sample_pixels(uint64_t seed, uint32_t salt, uint64_t threshold, int64_t bin_offset,
                                          const int64_t* bin1, const int64_t* bin2, const uint32_t* count,
                                          uint64_t n, uint32_t* kept) {
  if (threshold > kTwo32 || (n != 0 && (bin1 == nullptr || bin2 == nullptr || count == nullptr || kept == nullptr)))
    return MODLE_PIXELS_ERR_ARG;
  // (in 128 bits: no int64 pair can wrap)
  for (uint64_t t = 0; t < n; ++t) {
    const __int128 a = static_cast<__int128>(bin1[t]) + bin_offset, b = static_cast<__int128>(bin2[t]) + bin_offset;
    if (a < 0 || b < 0 || a >= static_cast<__int128>(kTwo32) || b >= static_cast<__int128>(kTwo32))
      return MODLE_PIXELS_ERR_RANGE;
  }
  const Draw g = make_draw(seed, salt, threshold);
  const int mode = mode_of(threshold);
  for (uint64_t t = 0; t < n; ++t) {
    const u32 I = static_cast<u32>(bin1[t] + bin_offset), J = static_cast<u32>(bin2[t] + bin_offset), c = count[t];
    u32 k = mode == kKeepAll ? c : 0u;
    if (mode == kDrawMode)
      for (u32 b = 0; b < (c >> 2) + ((c & 3) != 0); ++b) k += kept_in_block(g, I, J, b, c);
    kept[t] = k;
  }
  return MODLE_PIXELS_OK;
}

extern "C" int modle_pixels_sample(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows, uint64_t ncols,
                                   int64_t bin_offset, uint64_t threshold, uint64_t seed, uint32_t salt,
                                   const modle_pixels_stats* stats, uint32_t* d_kept, uint32_t* d_rest, void* stream,
                                   char* err, size_t errlen) {
  int rc = refuse("modle_pixels_sample", nrows, ncols, bin_offset, threshold,
                  h == nullptr || d_band == nullptr || stats == nullptr || (d_kept == nullptr && d_rest == nullptr),
                  err, errlen);
  if (rc != MODLE_PIXELS_OK) return rc;
  const uint64_t nb = modle_pixels_detail::band_bytes(nrows, ncols);
  if (modle_pixels_detail::any_overlap({{d_kept, nb}, {d_rest, nb}}, {{d_band, nb}})) {
    set_err(err, errlen, "modle_pixels_sample: an output overlaps the band or the other output");
    return MODLE_PIXELS_ERR_ARG;
  }
  rc = refuse_sum("modle_pixels_sample", stats->sum, err, errlen);
  if (rc != MODLE_PIXELS_OK) return rc;
  return sample_impl(h, d_band, nrows, ncols, bin_offset, threshold, seed, salt, d_kept, d_rest,
                     static_cast<hipStream_t>(stream), err, errlen);
}

extern "C" int modle_pixels_sample_to_host(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                                           uint64_t ncols, int64_t bin_offset, uint64_t threshold, uint64_t seed,
                                           uint32_t salt, int which, const int64_t** bin1, const int64_t** bin2,
                                           const int32_t** count, const int64_t** bin1_offset,
                                           modle_pixels_stats* stats_out, void* stream, char* err, size_t errlen) {
  int rc = refuse("modle_pixels_sample_to_host", nrows, ncols, bin_offset, threshold,
                  // (a negative bin_offset is refuse()'s own, with the range code: 0 stands in for it here)
                  h == nullptr || d_band == nullptr ||
                      modle_pixels_detail::bad_pixel_outputs(bin1, bin2, count, bin1_offset, stats_out, 0) ||
                      (which != MODLE_PIXELS_SAMPLE_KEPT && which != MODLE_PIXELS_SAMPLE_REST),
                  err, errlen);
  if (rc != MODLE_PIXELS_OK) return rc;
  *bin1 = *bin2 = nullptr;
  *count = nullptr;
  *bin1_offset = nullptr;
  modle_pixels_stats whole{};
  rc = modle_pixels_count(h, d_band, nrows, ncols, nullptr, &whole, stream, err, errlen);
  if (rc != MODLE_PIXELS_OK) return rc;
  rc = refuse_sum("modle_pixels_sample_to_host", whole.sum, err, errlen);
  if (rc != MODLE_PIXELS_OK) return rc;
  PIX_TRY(hipSetDevice(h->device));
  GrowBuf<uint32_t>& out = which == MODLE_PIXELS_SAMPLE_KEPT ? h->sample_kept : h->sample_rest;
  rc = out.ensure(nrows * ncols + 1, err, errlen);
  if (rc != MODLE_PIXELS_OK) return rc;
  rc = sample_impl(h, d_band, nrows, ncols, bin_offset, threshold, seed, salt,
                   which == MODLE_PIXELS_SAMPLE_KEPT ? out.dev : nullptr,
                   which == MODLE_PIXELS_SAMPLE_REST ? out.dev : nullptr, static_cast<hipStream_t>(stream), err, errlen);
  if (rc != MODLE_PIXELS_OK) return rc;
  return modle_pixels_detail::to_host(h, out.dev, nrows, ncols, bin_offset, bin1, bin2, count, bin1_offset, stats_out,
                                      static_cast<hipStream_t>(stream), err, errlen);
}
