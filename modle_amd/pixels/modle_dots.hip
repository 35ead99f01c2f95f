// modle_dots.hip -- dot calling on a band matrix: the four HiCCUPS neighbourhood sums of every pixel
// and the candidate decision, formed on the MI355X (include/modle_pixels.h: modle_pixels_dots /
// _dots_to_host / _coarse_dots_to_host), and the statistical test on the same tile: the lambda-chunk histogram
// and the threshold decision (modle_pixels_dot_hist / _dot_hist_to_host / _coarse_dot_hist_to_host, modle_pixels_
// dots_fdr / _dots_fdr_to_host / _coarse_dots_fdr_to_host).
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
//
// The statistical test (modle_pixels_dot_hist* / _dots_fdr*) runs the same body -- the kernel is a template over
// what the tile feeds, so the load, the scan and the twelve rectangles cannot drift apart -- on the same grid:
//   threshold decision  lambda_k = __dmul_rn((double)O_k, lam[k][d]), its chunk by a binary search of the edges
//                       (in LDS, with the thresholds), obs against thr[k][chunk], the fold test where a scale table
//                       is given, one plain store per word as above.
//   histogram           nothing is stored per pixel.  A workgroup counts obs < 32 in a private LDS table of 4 x 64
//                       rows (k, chunk) x 32 words with LDS integer atomics -- a tile has 4 096 pixels: no word can
//                       overflow -- and keeps per row one slot for a count >= 32 (the first it meets; a compare-and-
//                       swap takes the slot), so that a band whose pixels all hold one large count stays in LDS too;
//                       any other count >= 32 is added to the table in device memory directly.  A wave whose lanes
//                       all hold one index adds their number once.  At the end the workgroup adds its non-zero LDS
//                       words to the table with 64-bit integer atomics (no partial tables, so no grid cap and no
//                       fold kernel).  Integer addition commutes: the table does not depend on the order.
// LDS of the histogram kernel: 88 200 (tile) + 32 768 (low counts) + 2 048 (slots) + 512 (edges) = 123 528, 123 536
// as allocated, of 163 840: one workgroup per CU, as for the other two (the tile alone allows no second).  The
// decision kernel: 88 200 + 512 + 1 024 (thresholds) = 89 736, 89 744 as allocated.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "modle_pixels.h"
#include "pixels_context.h"
#include "pixels_device.h"

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

using modle_pixels_device::sat_scan_pass;
using modle_pixels_device::u64;

// What the tile feeds (the template argument of the kernel): the fold decision and / or the sums
// (modle_pixels_dots), the lambda-chunk histogram (modle_pixels_dot_hist), the threshold decision
// (modle_pixels_dots_fdr).  The load, the scan and the twelve rectangles are one body for all three.
enum : int { kFold = 0, kHist = 1, kFdr = 2 };

constexpr int kMaxChunks = MODLE_PIXELS_MAX_DOT_EDGES + 1;  // 64
constexpr int kLow = 32;                                    // counts below it are counted in LDS

// what the histogram and the threshold decision read and write besides the band (device pointers)
struct ChunkTables {
  const double* lam;    // [4][nrows], 0 outside the valid diagonals
  const double* edges;  // [n_edges]
  const uint32_t* thr;  // [4][n_edges + 1]; kFdr
  u64* hist;            // [4][n_edges + 1][n_obs]; kHist
  int n_edges;
  int n_obs;
};

// the LDS beside the tile, of the kernels that use it: the edges, the thresholds, the low counts
__device__ __forceinline__ double* lds_edges() {
  __shared__ double edges[kMaxChunks];
  return edges;
}
__device__ __forceinline__ uint32_t* lds_thr() {
  __shared__ uint32_t thr[4 * kMaxChunks];
  return thr;
}
__device__ __forceinline__ uint32_t* lds_low() {
  __shared__ uint32_t low[4 * kMaxChunks * kLow];
  return low;
}
// per row (k, chunk) of the table one count of kLow or more: the index of its word in the table and how often
// the workgroup met it.  The first such count a row meets takes the slot; the others go to the table directly.
__device__ __forceinline__ uint32_t* lds_high() {
  __shared__ uint32_t high[2 * 4 * kMaxChunks];
  return high;
}
constexpr uint32_t kNoIndex = 0xFFFFFFFFu;  // (the table has at most 4 * 64 * 16384 words)

// the number of edges strictly below lambda; a NaN goes to the top chunk
__device__ __forceinline__ int chunk_of(double lambda, const double* edges, int n_edges) {
  if (lambda != lambda) return n_edges;
  int lo = 0, hi = n_edges;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (edges[mid] < lambda)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// Counts one at index `idx` for every lane with `on` (called by whole waves), through add(index, how many): the
// lanes that hold the index of the wave's first such lane are added once, by that lane, the others add one each.
// A wave of the empty far field of a band or of a constant band so adds once.
template <class F>
__device__ __forceinline__ void wave_count(bool on, unsigned idx, F add) {
  const u64 mask = __ballot(on);
  if (mask == 0) return;
  const int first = __ffsll(static_cast<unsigned long long>(mask)) - 1;
  const unsigned key = static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(idx), first));
  const bool mine = on && idx == key;
  const u64 same = __ballot(mine);
  if (static_cast<int>(threadIdx.x & 63) == first)
    add(key, static_cast<unsigned>(__popcll(same)));
  else if (on && !mine)
    add(idx, 1u);
}

template <int kMode>
__global__ __launch_bounds__(kDotThreads) void pixels_dots(const uint32_t* __restrict__ band, int64_t nrows,
                                                           int64_t ncols, int w, int p, int64_t dlo, int64_t dhi,
                                                           u64 min_count, const double* __restrict__ scale,
                                                           uint32_t* __restrict__ cand, u64* __restrict__ sums,
                                                           ChunkTables ct) {
  __shared__ u64 sat[kPitch * kPitch];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t j0 = static_cast<int64_t>(blockIdx.x) * kT;
  const int64_t i0 = j0 - static_cast<int64_t>(blockIdx.y) * kT;  // (negative: the left-edge triangle)
  const int64_t dt = j0 - i0;
  const int S = kT + 2 * w;
  // whether the block holds a valid pixel (the same in every lane)
  const bool any = dt + (kT - 1) >= dlo && dt - (kT - 1) <= dhi && i0 + (kT - 1) >= w && j0 + w < ncols;
  const int n_chunks = ct.n_edges + 1;
  if constexpr (kMode == kHist) {
    if (!any) return;  // nothing to count, and nothing else to write
  }

  if (any) {
    if constexpr (kMode != kFold)
      for (int t = threadIdx.x; t < ct.n_edges; t += kDotThreads) lds_edges()[t] = ct.edges[t];
    if constexpr (kMode == kFdr)
      for (int t = threadIdx.x; t < 4 * n_chunks; t += kDotThreads) lds_thr()[t] = ct.thr[t];
    if constexpr (kMode == kHist) {
      for (int t = threadIdx.x; t < 4 * n_chunks * kLow; t += kDotThreads) lds_low()[t] = 0;
      for (int t = threadIdx.x; t < 4 * n_chunks; t += kDotThreads) {
        lds_high()[2 * t] = kNoIndex;
        lds_high()[2 * t + 1] = 0;
      }
    }
    for (int t = threadIdx.x; t <= S; t += kDotThreads) {
      sat[t] = 0;
      sat[t * kPitch] = 0;
    }
    // tile cell (r, c) is matrix cell (i0 - w + r, j0 - w + c); lane <-> r descending, d ascending
    // (build_table of modle_scc.hip is not merged with this: its tile is a rectangle across the main diagonal,
    // loaded an item per thread; only the two scan passes are shared)
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
    // (S <= kT + 2 * kMaxW, which the pass is told: a line has kSeg segments whatever w is)
    sat_scan_pass<kDotThreads, kPitch, kSeg, kT + 2 * kMaxW>(sat, S, S, 1, kPitch);  // along r, a line per c
    sat_scan_pass<kDotThreads, kPitch, kSeg, kT + 2 * kMaxW>(sat, S, S, kPitch, 1);  // along c, a line per r
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
    const bool in_band = j < ncols && d >= 0 && d < nrows;
    if constexpr (kMode != kHist) {
      if (!in_band) continue;  // no word of the band
    }
    const uint64_t word = static_cast<uint64_t>(j) * static_cast<uint64_t>(nrows) + static_cast<uint64_t>(d);
    const bool valid = any && in_band && i >= w && j + w < ncols && d >= dlo && d <= dhi;
    u64 o[4] = {0, 0, 0, 0};
    uint32_t obs = 0;
    if (valid) {
      const int r = w + ii, c = w + jj;
      o[0] = rect(r - w, r + w, c - w, c + w) - rect(r - p, r + p, c - p, c + p) - rect(r, r, c - w, c - p - 1) -
             rect(r, r, c + p + 1, c + w) - rect(r - w, r - p - 1, c, c) - rect(r + p + 1, r + w, c, c);
      o[1] = rect(r + 1, r + w, c - w, c - 1) - rect(r + 1, r + p, c - p, c - 1);
      o[2] = rect(r - 1, r + 1, c - w, c - p - 1) + rect(r - 1, r + 1, c + p + 1, c + w);
      o[3] = rect(r - w, r - p - 1, c - 1, c + 1) + rect(r + p + 1, r + w, c - 1, c + 1);
      if (kMode != kFold || cand != nullptr) obs = static_cast<uint32_t>(rect(r, r, c, c));
    }
    if constexpr (kMode == kFold) {
      if (cand != nullptr) {
        bool is = valid && obs >= min_count;
        const double x = static_cast<double>(obs);
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (is) is = x >= __dmul_rn(static_cast<double>(o[k]), scale[k * nrows + d]);
        cand[word] = is ? obs : 0u;
      }
      if (sums != nullptr) {
        sums[word] = o[0];
        sums[plane + word] = o[1];
        sums[2 * plane + word] = o[2];
        sums[3 * plane + word] = o[3];
      }
    } else if constexpr (kMode == kFdr) {
      bool is = valid && obs >= min_count;
      const double x = static_cast<double>(obs);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (is) {
          const double od = static_cast<double>(o[k]);
          const uint32_t t = lds_thr()[k * n_chunks + chunk_of(__dmul_rn(od, ct.lam[k * nrows + d]), lds_edges(), ct.n_edges)];
          is = t != 0 && obs >= t && (scale == nullptr || x >= __dmul_rn(od, scale[k * nrows + d]));
        }
      cand[word] = is ? obs : 0u;
    } else {
      // (whole waves: a lane without a valid pixel takes part in the votes of wave_count and adds nothing)
      const uint32_t seen = min(obs, static_cast<uint32_t>(ct.n_obs - 1));
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        unsigned row = 0;
        if (valid)
          row = static_cast<unsigned>(
              k * n_chunks + chunk_of(__dmul_rn(static_cast<double>(o[k]), ct.lam[k * nrows + d]), lds_edges(), ct.n_edges));
        wave_count(valid && seen < kLow, row * kLow + seen, [](unsigned at, unsigned n) { atomicAdd(&lds_low()[at], n); });
        wave_count(valid && seen >= kLow, row * static_cast<unsigned>(ct.n_obs) + seen, [&](unsigned at, unsigned n) {
          uint32_t* slot = lds_high() + 2 * (at / static_cast<unsigned>(ct.n_obs));
          const uint32_t held = atomicCAS(&slot[0], kNoIndex, at);
          if (held == kNoIndex || held == at)
            atomicAdd(&slot[1], n);
          else
            atomicAdd(&ct.hist[at], static_cast<u64>(n));
        });
      }
    }
  }
  if constexpr (kMode == kHist) {
    __syncthreads();
    for (int t = threadIdx.x; t < 4 * n_chunks * kLow; t += kDotThreads) {
      const uint32_t v = lds_low()[t];  // (a count below kLow is below n_obs too: seen <= n_obs - 1)
      if (v != 0) atomicAdd(&ct.hist[static_cast<unsigned>(t / kLow) * static_cast<unsigned>(ct.n_obs) + t % kLow], static_cast<u64>(v));
    }
    for (int t = threadIdx.x; t < 4 * n_chunks; t += kDotThreads) {
      const uint32_t at = lds_high()[2 * t], v = lds_high()[2 * t + 1];  // (at is a word of row t, or v is 0)
      if (v != 0) atomicAdd(&ct.hist[at], static_cast<u64>(v));
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

// The scale table into the context: a pinned copy, zeroed outside the valid diagonals, and its copy to the device
// enqueued.  The pinned copy may still feed the copy of the call before: an event guards its reuse.
int stage_scale(modle_pixels_handle* h, uint64_t nrows, uint64_t w, uint64_t min_diag, const double* scale,
                hipStream_t stream, char* err, size_t errlen) {
  const uint64_t dlo = 2 * w + min_diag, dhi = nrows - 1 - 2 * w;
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
  return MODLE_PIXELS_OK;
}

// the one launch of the three kernels: the grid covers every word of the band
template <int kMode>
int launch(const uint32_t* d_band, uint64_t nrows, uint64_t ncols, uint64_t w, uint64_t p, uint64_t min_diag,
           uint64_t min_count, const double* d_scale, uint32_t* d_cand, uint64_t* d_sums, const ChunkTables& ct,
           hipStream_t stream, char* err, size_t errlen) {
  const uint64_t dlo = 2 * w + min_diag, dhi = nrows - 1 - 2 * w;  // dlo <= dhi by the acceptance rule
  const dim3 grid(static_cast<unsigned>((ncols + kT - 1) / kT), static_cast<unsigned>((nrows + kT - 2) / kT + 1));
  hipLaunchKernelGGL(pixels_dots<kMode>, grid, dim3(kDotThreads), 0, stream, d_band, static_cast<int64_t>(nrows),
                     static_cast<int64_t>(ncols), static_cast<int>(w), static_cast<int>(p), static_cast<int64_t>(dlo),
                     static_cast<int64_t>(dhi), static_cast<u64>(min_count), d_scale, d_cand,
                     reinterpret_cast<u64*>(d_sums), ct);
  PIX_TRY(hipGetLastError());
  return MODLE_PIXELS_OK;
}

// enqueues the table's copy, the clearing of the trailing word and the kernel on checked arguments
int dots_impl(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows, uint64_t ncols, uint64_t w, uint64_t p,
              uint64_t min_diag, uint64_t min_count, const double* scale, uint32_t* d_cand, uint64_t* d_sums,
              hipStream_t stream, char* err, size_t errlen) {
  PIX_TRY(hipSetDevice(h->device));
  if (d_cand != nullptr) {
    const int rc = stage_scale(h, nrows, w, min_diag, scale, stream, err, errlen);
    if (rc != MODLE_PIXELS_OK) return rc;
    PIX_TRY(hipMemsetAsync(d_cand + nrows * ncols, 0, 4, stream));  // the trailing word: no block owns it
  }
  return launch<kFold>(d_band, nrows, ncols, w, p, min_diag, min_count, d_cand != nullptr ? h->dot_scale.dev : nullptr,
                       d_cand, d_sums, ChunkTables{}, stream, err, errlen);
}

// what the histogram and the threshold decision refuse of their tables beyond bad_dots (lam goes there as the
// scale table: the same rule); `thr` is looked at only with need_thr
bool bad_chunks(const double* lam, const double* edges, uint64_t n_edges, const uint32_t* thr, bool need_thr) {
  if (lam == nullptr || edges == nullptr || (need_thr && thr == nullptr) || n_edges == 0 ||
      n_edges > MODLE_PIXELS_MAX_DOT_EDGES)
    return true;
  for (uint64_t e = 0; e < n_edges; ++e)
    if (!std::isfinite(edges[e]) || !(edges[e] > 0.0) || (e > 0 && !(edges[e] > edges[e - 1]))) return true;
  return false;
}

// The tables of the histogram and of the threshold decision into the context, on checked arguments: a pinned
// copy (lam zeroed outside the valid diagonals, like the scale table), the copy to the device enqueued, the event
// that guards the pinned copy recorded.  `thr` may be null (the histogram).
int stage_chunks(modle_pixels_handle* h, uint64_t nrows, uint64_t w, uint64_t min_diag, const double* lam,
                 const double* edges, uint64_t n_edges, const uint32_t* thr, ChunkTables* ct, hipStream_t stream,
                 char* err, size_t errlen) {
  const uint64_t dlo = 2 * w + min_diag, dhi = nrows - 1 - 2 * w;
  if (h->dot_lam_copied == nullptr)
    PIX_TRY(hipEventCreateWithFlags(&h->dot_lam_copied, hipEventDisableTiming));
  else
    PIX_TRY(hipEventSynchronize(h->dot_lam_copied));
  const uint64_t n = 4 * nrows + kMaxChunks + 2 * kMaxChunks;  // lam, edges, 4 * kMaxChunks 32-bit thresholds
  const int rc = h->dot_lam.ensure(n, err, errlen);
  if (rc != MODLE_PIXELS_OK) return rc;
  double* host = h->dot_lam.host;
  for (uint64_t k = 0; k < 4; ++k)
    for (uint64_t d = 0; d < nrows; ++d) host[k * nrows + d] = (d >= dlo && d <= dhi) ? lam[k * nrows + d] : 0.0;
  for (uint64_t e = 0; e < static_cast<uint64_t>(kMaxChunks); ++e) host[4 * nrows + e] = e < n_edges ? edges[e] : 0.0;
  uint32_t* host_thr = reinterpret_cast<uint32_t*>(host + 4 * nrows + kMaxChunks);
  for (uint64_t t = 0; t < static_cast<uint64_t>(4 * kMaxChunks); ++t)
    host_thr[t] = (thr != nullptr && t < 4 * (n_edges + 1)) ? thr[t] : 0u;
  PIX_TRY(hipMemcpyAsync(h->dot_lam.dev, host, n * sizeof(double), hipMemcpyHostToDevice, stream));
  PIX_TRY(hipEventRecord(h->dot_lam_copied, stream));
  ct->lam = h->dot_lam.dev;
  ct->edges = h->dot_lam.dev + 4 * nrows;
  ct->thr = reinterpret_cast<const uint32_t*>(h->dot_lam.dev + 4 * nrows + kMaxChunks);
  ct->n_edges = static_cast<int>(n_edges);
  return MODLE_PIXELS_OK;
}

// enqueues the histogram of the band into d_hist (adds) on checked arguments
int hist_impl(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows, uint64_t ncols, uint64_t w, uint64_t p,
              uint64_t min_diag, const double* lam, const double* edges, uint64_t n_edges, uint64_t n_obs,
              uint64_t* d_hist, hipStream_t stream, char* err, size_t errlen) {
  PIX_TRY(hipSetDevice(h->device));
  ChunkTables ct{};
  const int rc = stage_chunks(h, nrows, w, min_diag, lam, edges, n_edges, nullptr, &ct, stream, err, errlen);
  if (rc != MODLE_PIXELS_OK) return rc;
  ct.hist = reinterpret_cast<u64*>(d_hist);
  ct.n_obs = static_cast<int>(n_obs);
  return launch<kHist>(d_band, nrows, ncols, w, p, min_diag, 1, nullptr, nullptr, nullptr, ct, stream, err, errlen);
}

// enqueues the threshold decision into d_cand on checked arguments; `scale` may be null
int fdr_impl(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows, uint64_t ncols, uint64_t w, uint64_t p,
             uint64_t min_diag, uint64_t min_count, const double* lam, const double* edges, uint64_t n_edges,
             const uint32_t* thr, const double* scale, uint32_t* d_cand, hipStream_t stream, char* err,
             size_t errlen) {
  PIX_TRY(hipSetDevice(h->device));
  ChunkTables ct{};
  int rc = stage_chunks(h, nrows, w, min_diag, lam, edges, n_edges, thr, &ct, stream, err, errlen);
  if (rc != MODLE_PIXELS_OK) return rc;
  if (scale != nullptr) {
    rc = stage_scale(h, nrows, w, min_diag, scale, stream, err, errlen);
    if (rc != MODLE_PIXELS_OK) return rc;
  }
  PIX_TRY(hipMemsetAsync(d_cand + nrows * ncols, 0, 4, stream));  // the trailing word: no block owns it
  return launch<kFdr>(d_band, nrows, ncols, w, p, min_diag, min_count, scale != nullptr ? h->dot_scale.dev : nullptr,
                      d_cand, nullptr, ct, stream, err, errlen);
}

// modle_pixels_dots_to_host (`cs` null) and modle_pixels_coarse_dots_to_host under their `name`: the band resolved,
// its candidates into the scratch band of the context, then count / scan / extract
int dots_one_call(const char* name, const modle_pixels_detail::CoarseSpec* cs, modle_pixels_handle* h,
                  const uint32_t* d_band, uint64_t nrows, uint64_t ncols, uint64_t w, uint64_t p, uint64_t min_diag,
                  uint64_t min_count, const double* scale, int64_t bin_offset, const int64_t** bin1,
                  const int64_t** bin2, const int32_t** count, const int64_t** bin1_offset, modle_pixels_stats* stats,
                  void* stream, char* err, size_t errlen) {
  modle_pixels_detail::BandView v;
  if (h == nullptr || bad_pixel_outputs(bin1, bin2, count, bin1_offset, stats, bin_offset) ||
      !modle_pixels_detail::view_shape(d_band, nrows, ncols, cs, &v) ||
      bad_dots(v.nrows, v.ncols, w, p, min_diag, min_count, scale, true)) {
    set_err(err, errlen, modle_pixels_detail::refusal(name, cs, kRule));
    return MODLE_PIXELS_ERR_ARG;
  }
  const hipStream_t st = static_cast<hipStream_t>(stream);
  int rc = modle_pixels_detail::resolve_band(h, d_band, nrows, ncols, cs, &v, st, err, errlen);
  if (rc != MODLE_PIXELS_OK) return rc;
  PIX_TRY(hipSetDevice(h->device));
  rc = h->dot_cand.ensure(v.nrows * v.ncols + 1, err, errlen);
  if (rc == MODLE_PIXELS_OK)
    rc = dots_impl(h, v.d, v.nrows, v.ncols, w, p, min_diag, min_count, scale, h->dot_cand.dev, nullptr, st, err, errlen);
  if (rc != MODLE_PIXELS_OK) return rc;
  return modle_pixels_detail::to_host(h, h->dot_cand.dev, v.nrows, v.ncols, bin_offset, bin1, bin2, count, bin1_offset,
                                      stats, st, err, errlen);
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
  if (modle_pixels_detail::any_overlap({{d_cand, nb}, {d_sums, ns}}, {{d_band, nb}})) {
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
  return dots_one_call("modle_pixels_dots_to_host", nullptr, h, d_band, nrows, ncols, w, p, min_diag, min_count, scale,
                       bin_offset, bin1, bin2, count, bin1_offset, stats, stream, err, errlen);
}

extern "C" int modle_pixels_coarse_dots_to_host(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                                                uint64_t ncols, uint64_t factor, uint64_t first_bin, uint64_t w,
                                                uint64_t p, uint64_t min_diag, uint64_t min_count,
                                                const double* scale, int64_t bin_offset, const int64_t** bin1,
                                                const int64_t** bin2, const int32_t** count,
                                                const int64_t** bin1_offset, modle_pixels_stats* stats,
                                                void* stream, char* err, size_t errlen) {
  const modle_pixels_detail::CoarseSpec cs{factor, first_bin};
  return dots_one_call("modle_pixels_coarse_dots_to_host", &cs, h, d_band, nrows, ncols, w, p, min_diag, min_count,
                       scale, bin_offset, bin1, bin2, count, bin1_offset, stats, stream, err, errlen);
}

namespace {

constexpr const char* kChunkRule =
    "(of the tables: lam without NaN or negative entries at the valid diagonals, 1 <= n_edges <= 63 finite, "
    "positive, strictly increasing edges, 2 <= n_obs <= 16384, thr and an output that are not null, d_hist 8-byte "
    "aligned; of the rest:) ";

bool bad_n_obs(uint64_t n_obs) { return n_obs < 2 || n_obs > MODLE_PIXELS_MAX_DOT_OBS; }

// the refusal of the forms with tables; the coarse twins name the factor before and the coarse band behind the tables' rule
std::string chunk_refusal(const char* name, const modle_pixels_detail::CoarseSpec* cs) {
  return std::string(name) + ": invalid argument " + (cs != nullptr ? "(factor >= 2) " : "") + kChunkRule +
         (cs != nullptr ? "(of the coarse band:) " : "") + kRule;
}

// modle_pixels_dot_hist_to_host (`cs` null) and modle_pixels_coarse_dot_hist_to_host under their `name`: the band
// resolved, the table in the sums of the context zeroed, the band's histogram added, the copy to the pinned mirror, the wait
int hist_one_call(const char* name, const modle_pixels_detail::CoarseSpec* cs, modle_pixels_handle* h,
                  const uint32_t* d_band, uint64_t nrows, uint64_t ncols, uint64_t w, uint64_t p, uint64_t min_diag,
                  const double* lam, const double* edges, uint64_t n_edges, uint64_t n_obs, const uint64_t** hist,
                  void* stream, char* err, size_t errlen) {
  if (hist != nullptr) *hist = nullptr;
  modle_pixels_detail::BandView v;
  if (h == nullptr || hist == nullptr || bad_n_obs(n_obs) || bad_chunks(lam, edges, n_edges, nullptr, false) ||
      !modle_pixels_detail::view_shape(d_band, nrows, ncols, cs, &v) ||
      bad_dots(v.nrows, v.ncols, w, p, min_diag, 1, lam, true)) {
    set_err(err, errlen, chunk_refusal(name, cs));
    return MODLE_PIXELS_ERR_ARG;
  }
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const int rc = modle_pixels_detail::resolve_band(h, d_band, nrows, ncols, cs, &v, st, err, errlen);
  if (rc != MODLE_PIXELS_OK) return rc;
  const uint64_t words = 4 * (n_edges + 1) * n_obs;
  return modle_pixels_detail::sums_to_host(h, words, hist, st, err, errlen, [&](uint64_t* d_hist) {
    PIX_TRY(hipMemsetAsync(d_hist, 0, words * 8, st));  // (hist_impl adds)
    return hist_impl(h, v.d, v.nrows, v.ncols, w, p, min_diag, lam, edges, n_edges, n_obs, d_hist, st, err, errlen);
  });
}

// modle_pixels_dots_fdr_to_host (`cs` null) and modle_pixels_coarse_dots_fdr_to_host under their `name`: the band
// resolved, the threshold decision into the scratch band of the context, then count / scan / extract
int fdr_one_call(const char* name, const modle_pixels_detail::CoarseSpec* cs, modle_pixels_handle* h,
                 const uint32_t* d_band, uint64_t nrows, uint64_t ncols, uint64_t w, uint64_t p, uint64_t min_diag,
                 uint64_t min_count, const double* lam, const double* edges, uint64_t n_edges, const uint32_t* thr,
                 const double* scale, int64_t bin_offset, const int64_t** bin1, const int64_t** bin2,
                 const int32_t** count, const int64_t** bin1_offset, modle_pixels_stats* stats, void* stream, char* err,
                 size_t errlen) {
  modle_pixels_detail::BandView v;
  if (h == nullptr || bad_pixel_outputs(bin1, bin2, count, bin1_offset, stats, bin_offset) ||
      bad_chunks(lam, edges, n_edges, thr, true) || !modle_pixels_detail::view_shape(d_band, nrows, ncols, cs, &v) ||
      bad_dots(v.nrows, v.ncols, w, p, min_diag, min_count, lam, true) ||
      bad_dots(v.nrows, v.ncols, w, p, min_diag, min_count, scale, false)) {
    set_err(err, errlen, chunk_refusal(name, cs));
    return MODLE_PIXELS_ERR_ARG;
  }
  const hipStream_t st = static_cast<hipStream_t>(stream);
  int rc = modle_pixels_detail::resolve_band(h, d_band, nrows, ncols, cs, &v, st, err, errlen);
  if (rc != MODLE_PIXELS_OK) return rc;
  PIX_TRY(hipSetDevice(h->device));
  rc = h->dot_cand.ensure(v.nrows * v.ncols + 1, err, errlen);
  if (rc == MODLE_PIXELS_OK)
    rc = fdr_impl(h, v.d, v.nrows, v.ncols, w, p, min_diag, min_count, lam, edges, n_edges, thr, scale, h->dot_cand.dev,
                  st, err, errlen);
  if (rc != MODLE_PIXELS_OK) return rc;
  return modle_pixels_detail::to_host(h, h->dot_cand.dev, v.nrows, v.ncols, bin_offset, bin1, bin2, count, bin1_offset,
                                      stats, st, err, errlen);
}

}  // namespace

extern "C" int modle_pixels_dot_hist(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows, uint64_t ncols,
                                     uint64_t w, uint64_t p, uint64_t min_diag, const double* lam, const double* edges,
                                     uint64_t n_edges, uint64_t n_obs, uint64_t* d_hist, void* stream, char* err,
                                     size_t errlen) {
  if (h == nullptr || d_band == nullptr || d_hist == nullptr || (reinterpret_cast<uintptr_t>(d_hist) & 7) != 0 ||
      bad_n_obs(n_obs) || bad_chunks(lam, edges, n_edges, nullptr, false) ||
      bad_dots(nrows, ncols, w, p, min_diag, 1, lam, true)) {
    set_err(err, errlen, std::string("modle_pixels_dot_hist: invalid argument ") + kChunkRule + kRule);
    return MODLE_PIXELS_ERR_ARG;
  }
  if (overlap(d_hist, 4 * (n_edges + 1) * n_obs * 8, d_band, modle_pixels_detail::band_bytes(nrows, ncols))) {
    set_err(err, errlen, "modle_pixels_dot_hist: the table overlaps the band");
    return MODLE_PIXELS_ERR_ARG;
  }
  return hist_impl(h, d_band, nrows, ncols, w, p, min_diag, lam, edges, n_edges, n_obs, d_hist,
                   static_cast<hipStream_t>(stream), err, errlen);
}

extern "C" int modle_pixels_dot_hist_to_host(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                                             uint64_t ncols, uint64_t w, uint64_t p, uint64_t min_diag,
                                             const double* lam, const double* edges, uint64_t n_edges,
                                             uint64_t n_obs, const uint64_t** hist, void* stream, char* err,
                                             size_t errlen) {
  return hist_one_call("modle_pixels_dot_hist_to_host", nullptr, h, d_band, nrows, ncols, w, p, min_diag, lam, edges,
                       n_edges, n_obs, hist, stream, err, errlen);
}

extern "C" int modle_pixels_coarse_dot_hist_to_host(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                                                    uint64_t ncols, uint64_t factor, uint64_t first_bin, uint64_t w,
                                                    uint64_t p, uint64_t min_diag, const double* lam,
                                                    const double* edges, uint64_t n_edges, uint64_t n_obs,
                                                    const uint64_t** hist, void* stream, char* err, size_t errlen) {
  const modle_pixels_detail::CoarseSpec cs{factor, first_bin};
  return hist_one_call("modle_pixels_coarse_dot_hist_to_host", &cs, h, d_band, nrows, ncols, w, p, min_diag, lam, edges,
                       n_edges, n_obs, hist, stream, err, errlen);
}

extern "C" int modle_pixels_dots_fdr(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows, uint64_t ncols,
                                     uint64_t w, uint64_t p, uint64_t min_diag, uint64_t min_count, const double* lam,
                                     const double* edges, uint64_t n_edges, const uint32_t* thr, const double* scale,
                                     uint32_t* d_cand, void* stream, char* err, size_t errlen) {
  if (h == nullptr || d_band == nullptr || d_cand == nullptr || bad_chunks(lam, edges, n_edges, thr, true) ||
      bad_dots(nrows, ncols, w, p, min_diag, min_count, lam, true) ||
      bad_dots(nrows, ncols, w, p, min_diag, min_count, scale, false)) {
    set_err(err, errlen, std::string("modle_pixels_dots_fdr: invalid argument ") + kChunkRule + kRule);
    return MODLE_PIXELS_ERR_ARG;
  }
  const uint64_t nb = modle_pixels_detail::band_bytes(nrows, ncols);
  if (overlap(d_cand, nb, d_band, nb)) {
    set_err(err, errlen, "modle_pixels_dots_fdr: the output overlaps the band");
    return MODLE_PIXELS_ERR_ARG;
  }
  return fdr_impl(h, d_band, nrows, ncols, w, p, min_diag, min_count, lam, edges, n_edges, thr, scale, d_cand,
                  static_cast<hipStream_t>(stream), err, errlen);
}

extern "C" int modle_pixels_dots_fdr_to_host(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                                             uint64_t ncols, uint64_t w, uint64_t p, uint64_t min_diag,
                                             uint64_t min_count, const double* lam, const double* edges,
                                             uint64_t n_edges, const uint32_t* thr, const double* scale,
                                             int64_t bin_offset, const int64_t** bin1, const int64_t** bin2,
                                             const int32_t** count, const int64_t** bin1_offset,
                                             modle_pixels_stats* stats, void* stream, char* err, size_t errlen) {
  return fdr_one_call("modle_pixels_dots_fdr_to_host", nullptr, h, d_band, nrows, ncols, w, p, min_diag, min_count, lam,
                      edges, n_edges, thr, scale, bin_offset, bin1, bin2, count, bin1_offset, stats, stream, err, errlen);
}

extern "C" int modle_pixels_coarse_dots_fdr_to_host(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                                                    uint64_t ncols, uint64_t factor, uint64_t first_bin, uint64_t w,
                                                    uint64_t p, uint64_t min_diag, uint64_t min_count,
                                                    const double* lam, const double* edges, uint64_t n_edges,
                                                    const uint32_t* thr, const double* scale, int64_t bin_offset,
                                                    const int64_t** bin1, const int64_t** bin2, const int32_t** count,
                                                    const int64_t** bin1_offset, modle_pixels_stats* stats,
                                                    void* stream, char* err, size_t errlen) {
  const modle_pixels_detail::CoarseSpec cs{factor, first_bin};
  return fdr_one_call("modle_pixels_coarse_dots_fdr_to_host", &cs, h, d_band, nrows, ncols, w, p, min_diag, min_count,
                      lam, edges, n_edges, thr, scale, bin_offset, bin1, bin2, count, bin1_offset, stats, stream, err,
                      errlen);
}
