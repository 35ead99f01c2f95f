// modle_scc.hip -- two band matrices compared diagonal by diagonal, on the MI355X
// (include/modle_pixels.h: modle_pixels_scc / _scc_to_host / _scc_groups).
//
// Stratum d of the comparison holds the entries a_i = X_A(i, i + d) and b_i = X_B(i, i + d), 0 <= i < ncols - d,
// where X is the box sum of half-width h of the symmetric matrix of a band (h == 0: the band word itself).  Per
// stratum the library writes n = #{a_i != 0 or b_i != 0} and the 128-bit sums of a, b, a * a, b * b and a * b;
// pixels.scc_scores states HiCRep's stratum-adjusted correlation on the host.
//
// The strata min_diag .. max_diag are cut into strips of 64, and lane l of every wave stands for stratum d0 + l
// of its workgroup's strip from the first to the last pixel the workgroup sees: the eleven words of a stratum
// stay in that lane's registers, no sum crosses lanes, and the eight waves of a workgroup meet once, in LDS, when
// the walk is over.  A strip is walked by G <= MODLE_SCC_MAX_GROUPS workgroups, which take its tiles in turn
// and leave their sums in scratch of the context, uint64[strip][G][11][64]; scc_fold adds the G partial sums
// of every stratum with carries and stores every output word once, the zeros outside the strata included.  No
// atomics, no floating point, and no word depends on G.
//
//   h == 0  (scc_stream)  a tile is 64 columns of the band.  Of column j the words d0 .. d0 + 63 belong to the
//           strip, one per lane: a wave reads them in one load of 256 contiguous bytes, four loads in flight,
//           and the waves take the columns in turn.  Every word of the strata is read once, in memory order.
//   h > 0   (scc_smooth)  a tile is 32 rows i0 .. i0 + 31 of the matrix.  The entries of the strip in these rows
//           are the cells (i, i + d0 + l); their boxes lie in the (32 + 2h) x (95 + 2h) rectangle of the matrix
//           whose corner is (i0 - h, i0 + d0 - h).  The workgroup loads that rectangle of A into LDS as 64-bit
//           words -- cell (R, C) is band[max(R, C) * nrows + |R - C|], so a box crosses the main diagonal
//           through the symmetry; a cell outside the matrix, or on a diagonal no box of the strip reaches,
//           counts 0 and is not loaded --, turns it into a summed-area table with the two segmented scan
//           passes modle_dots.hip uses too (pixels_device.h), and every lane takes the box sums of its four rows into registers: four
//           reads each.  Then the table is rebuilt for B in the same LDS and the products are formed.  Consecutive
//           lanes read consecutive table words, and the pitch of 137 words is odd, so both scan passes and the
//           box reads are free of bank conflicts.
//
// A box sum is below 1681 * 2^32 < 2^43 and a table entry below 72 * 135 * 2^32 < 2^46: 64-bit words hold them.
// a * a is below 2^86: the products are formed in 128 bits (__umul64hi) and summed in two words, the carry of
// the low word counted in the high one.  At most 2^32 entries: a sum stays below 2^118.
//
// Every address is a function of nrows, ncols, h and the strata alone: the words with d > j (the left-edge
// triangle) and the trailing word are never addressed, whatever the bands hold.
//
// LDS: scc_smooth 73 * 137 * 8 = 80 008 bytes, static, whatever h is: two workgroups = 16 waves on a CU's
// 160 KiB; scc_stream 7 * 11 * 64 * 8 = 39 424 bytes.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "modle_pixels.h"
#include "pixels_context.h"
#include "pixels_device.h"

namespace {

using modle_pixels_device::add128;
using modle_pixels_device::sat_scan_pass;
using modle_pixels_device::u64;

constexpr int kStrip = 64;                                      // strata of a workgroup = lanes of a wave
constexpr unsigned kThreads = 512;
constexpr int kWaves = kThreads / 64;                           // 8
constexpr int kUnroll = 4;                                      // loads a wave of scc_stream keeps in flight
constexpr int kTableUnroll = 2;                                 // and of scc_smooth's loader (per band)
constexpr int kWords = MODLE_PIXELS_SCC_ROWS;                   // 11
constexpr int kStreamCols = 64;                                 // columns of a tile of scc_stream
constexpr int kTile = 32;                                       // matrix rows of a tile of scc_smooth
constexpr int kPerLane = kTile / kWaves;                        // rows of a tile per wave: 4
constexpr int kMaxH = MODLE_PIXELS_MAX_SCC_SMOOTH;              // 20
constexpr int kMaxTileRows = kTile + 2 * kMaxH;                 // 72
constexpr int kMaxTileCols = kTile + kStrip - 1 + 2 * kMaxH;    // 135
constexpr int kPitch = kMaxTileCols + 2;                        // 137 64-bit words, odd
constexpr int kSatWords = (kMaxTileRows + 1) * kPitch;          // a zero row and column in front
constexpr int kMaxSeg = 8;                                      // threads per line of a scan pass at most
constexpr int kMeetWords = (kWaves - 1) * kWords * kStrip;      // where the waves' sums meet
constexpr unsigned kMaxGroups = MODLE_SCC_MAX_GROUPS;
static_assert(kPitch % 2 == 1, "an odd pitch keeps both passes free of bank conflicts");
static_assert(kTile % kWaves == 0 && kStreamCols % (kWaves * kUnroll) == 0, "whole trips");
static_assert(kMaxTileCols <= static_cast<int>(kThreads) && kMaxTileRows <= static_cast<int>(kThreads),
              "a thread per line of a scan pass");
static_assert(kMeetWords <= kSatWords, "the waves meet in the table's LDS");

// the eleven words of a stratum, in the order of the output rows
// (Mom / Acc<kWhat> of modle_stripes.hip are not merged with this: either layout is its pinned output rows, 11 and 9
// words, and n is counted differently; only add128 underneath is shared)
struct Acc {
  u64 w[kWords];
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int k = 0; k < kWords; ++k) w[k] = 0;
  }
  // one entry (a, b); an entry that is zero in both adds nothing.  kWide: a and b may pass 2^32
  template <bool kWide>
  __device__ __forceinline__ void add(u64 a, u64 b) {
    w[0] += (a | b) != 0 ? 1u : 0u;
    add128(w[1], w[2], a, 0);
    add128(w[3], w[4], b, 0);
    add128(w[5], w[6], a * a, kWide ? __umul64hi(a, a) : 0);
    add128(w[7], w[8], b * b, kWide ? __umul64hi(b, b) : 0);
    add128(w[9], w[10], a * b, kWide ? __umul64hi(a, b) : 0);
  }
  __device__ __forceinline__ void merge(const Acc& o) {
    w[0] += o.w[0];
#pragma unroll
    for (int k = 1; k < kWords; k += 2) add128(w[k], w[k + 1], o.w[k], o.w[k + 1]);
  }
};

// The end of a walk: the waves' sums meet in `meet` (kMeetWords words nobody else uses any more) and wave 0
// stores the workgroup's eleven words of every stratum of the strip, the lanes beyond the strata included
// (they hold zeros).
__device__ __forceinline__ void leave_partial(Acc& acc, u64* meet, u64* __restrict__ partial) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (wv != 0) {
#pragma unroll
    for (int k = 0; k < kWords; ++k) meet[((wv - 1) * kWords + k) * kStrip + lane] = acc.w[k];
  }
  __syncthreads();
  if (wv == 0) {
#pragma unroll
    for (int x = 0; x < kWaves - 1; ++x) {
      Acc o;
#pragma unroll
      for (int k = 0; k < kWords; ++k) o.w[k] = meet[(x * kWords + k) * kStrip + lane];
      acc.merge(o);
    }
    u64* mine = partial + (static_cast<u64>(blockIdx.x) * gridDim.y + blockIdx.y) * (kWords * kStrip);
#pragma unroll
    for (int k = 0; k < kWords; ++k) mine[k * kStrip + lane] = acc.w[k];
  }
}

// grid (strips, G): the strata lo + 64 * blockIdx.x ..., the tiles blockIdx.y, blockIdx.y + G, ...
__global__ __launch_bounds__(kThreads) void scc_stream(const uint32_t* __restrict__ ref,
                                                       const uint32_t* __restrict__ tgt, int64_t nrows,
                                                       int64_t ncols, int64_t lo, int64_t hi,
                                                       u64* __restrict__ partial) {
  __shared__ u64 meet[kMeetWords];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t d0 = lo + static_cast<int64_t>(blockIdx.x) * kStrip;
  const int64_t d = d0 + lane;
  const bool mine = d <= hi;  // (hi <= nrows - 1)
  // the columns d0 .. ncols - 1 hold the pixels of the strip, kStreamCols of them a tile
  const int64_t ntiles = (ncols - d0 + kStreamCols - 1) / kStreamCols;
  Acc acc;
  acc.zero();
  for (int64_t t = blockIdx.y; t < ntiles; t += gridDim.y) {
    const int64_t jb = d0 + t * kStreamCols;
    for (int jj0 = wv; jj0 < kStreamCols; jj0 += kWaves * kUnroll) {
      uint32_t va[kUnroll], vb[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int64_t j = jb + jj0 + u * kWaves;
        // a pixel of the strata: d <= j (not in the left-edge triangle), j < ncols, d <= hi < nrows
        const bool ok = mine && j < ncols && d <= j;
        const u64 at = static_cast<u64>(j) * static_cast<u64>(nrows) + static_cast<u64>(d);
        va[u] = ok ? ref[at] : 0u;
        vb[u] = ok ? tgt[at] : 0u;
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) acc.add<false>(va[u], vb[u]);
    }
  }
  leave_partial(acc, meet, partial);
}

// The summed-area table of the tile of `band` whose cell (0, 0) is matrix cell (r0, c0): A[r + 1][c + 1] = the
// sum of the cells (<= r, <= c), r < sr, c < sc.  Only the cells on the signed diagonals dlo .. dhi (column
// minus row) are loaded; the others count 0.  Ends with a barrier.
// (The loader of modle_dots.hip is not merged with this: its tile is square, loaded a column per wave with the lanes
// reversed and without the symmetry; only the two scan passes are shared.)
__device__ __forceinline__ void build_table(u64* sat, const uint32_t* __restrict__ band, int64_t nrows,
                                            int64_t ncols, int64_t r0, int64_t c0, int sr, int sc, int64_t dlo,
                                            int64_t dhi) {
  for (int t = threadIdx.x; t <= max(sr, sc); t += kThreads) {
    if (t <= sc) sat[t] = 0;
    if (t <= sr) sat[t * kPitch] = 0;
  }
  // item = (c, r descending): above the main diagonal the words of a column lie at ascending addresses
  const int items = sr * sc;
  for (int it0 = threadIdx.x; it0 < items; it0 += kThreads * kTableUnroll) {
    uint32_t v[kTableUnroll];
#pragma unroll
    for (int u = 0; u < kTableUnroll; ++u) {
      const int it = it0 + u * static_cast<int>(kThreads);
      const int c = it / sr, r = sr - 1 - it % sr;
      const int64_t R = r0 + r, C = c0 + c, ds = C - R;
      const int64_t dd = ds < 0 ? -ds : ds, far = ds < 0 ? R : C;  // the symmetry: M(R, C) == M(C, R)
      const bool ok = it < items && R >= 0 && C >= 0 && R < ncols && C < ncols && ds >= dlo && ds <= dhi && dd < nrows;
      v[u] = ok ? band[static_cast<u64>(far) * static_cast<u64>(nrows) + static_cast<u64>(dd)] : 0u;
    }
#pragma unroll
    for (int u = 0; u < kTableUnroll; ++u) {
      const int it = it0 + u * static_cast<int>(kThreads);
      if (it < items) sat[(sr - it % sr) * kPitch + (it / sr + 1)] = v[u];
    }
  }
  __syncthreads();
  sat_scan_pass<kThreads, kPitch, kMaxSeg>(sat, sc, sr, 1, kPitch);  // along r, a line per c
  sat_scan_pass<kThreads, kPitch, kMaxSeg>(sat, sr, sc, kPitch, 1);  // along c, a line per r
}

// grid (strips, G), h >= 1; two workgroups on a CU are four waves on a SIMD
__global__ __launch_bounds__(kThreads, 4) void scc_smooth(const uint32_t* __restrict__ ref,
                                                       const uint32_t* __restrict__ tgt, int64_t nrows,
                                                       int64_t ncols, int h, int64_t lo, int64_t hi,
                                                       u64* __restrict__ partial) {
  __shared__ u64 sat[kSatWords];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t d0 = lo + static_cast<int64_t>(blockIdx.x) * kStrip;
  const int64_t dtop = min(hi, d0 + kStrip - 1), d = d0 + lane;
  const int sr = kTile + 2 * h, sc = kTile + kStrip - 1 + 2 * h;
  // the rows 0 .. ncols - 1 - d0 hold the entries of the strip, kTile of them a tile
  const int64_t ntiles = (ncols - d0 + kTile - 1) / kTile;
  Acc acc;
  acc.zero();
  for (int64_t t = blockIdx.y; t < ntiles; t += gridDim.y) {  // (the same in every thread of the workgroup)
    const int64_t i0 = t * kTile;
    u64 a[kPerLane];
#pragma unroll
    for (int side = 0; side < 2; ++side) {
      build_table(sat, side == 0 ? ref : tgt, nrows, ncols, i0 - h, i0 + d0 - h, sr, sc, d0 - 2 * h, dtop + 2 * h);
#pragma unroll
      for (int k = 0; k < kPerLane; ++k) {
        // entry (i, i + d): its box is the tile cells [ii, ii + 2h] x [ii + lane, ii + lane + 2h]
        const int ii = wv * kPerLane + k;
        const bool ok = d <= dtop && i0 + ii + d < ncols;
        const int ra = ii, rb = ii + 2 * h + 1, ca = ii + lane, cb = ii + lane + 2 * h + 1;
        u64 x = sat[rb * kPitch + cb] - sat[ra * kPitch + cb] - sat[rb * kPitch + ca] + sat[ra * kPitch + ca];
        x = ok ? x : 0;
        if (side == 0) a[k] = x; else acc.add<true>(a[k], x);
      }
      __syncthreads();  // the table is free for the other band, the next tile or the meeting of the waves
    }
  }
  leave_partial(acc, sat, partial);
}

// Stratum d of every thread: the sum of the `groups` partial sums of its strip, every output word stored once;
// the columns outside lo .. hi hold 0.
__global__ __launch_bounds__(256) void scc_fold(const u64* __restrict__ partial, int64_t nrows, int64_t lo, int64_t hi,
                                                unsigned groups, u64* __restrict__ out) {
  const int64_t d = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (d >= nrows) return;
  Acc acc;
  acc.zero();
  if (d >= lo && d <= hi) {
    const u64 strip = static_cast<u64>(d - lo) / kStrip, l = static_cast<u64>(d - lo) % kStrip;
    for (unsigned g = 0; g < groups; ++g) {
      const u64* p = partial + (strip * groups + g) * (kWords * kStrip) + l;
      Acc o;
#pragma unroll
      for (int k = 0; k < kWords; ++k) o.w[k] = p[k * kStrip];
      acc.merge(o);
    }
  }
#pragma unroll
  for (int k = 0; k < kWords; ++k) out[static_cast<u64>(k) * static_cast<u64>(nrows) + static_cast<u64>(d)] = acc.w[k];
}

using modle_pixels_detail::set_err;

constexpr const char* kRule =
    "(0 < nrows <= ncols, smooth <= 20, min_diag <= max_diag, max_diag + 2 * smooth <= nrows - 1, out_words == "
    "11 * nrows, an 8-byte aligned output)";

// what both entry points refuse of the shape, the smoothing and the strata
bool bad_request(uint64_t nrows, uint64_t ncols, uint64_t smooth, uint64_t min_diag, uint64_t max_diag) {
  return nrows == 0 || modle_pixels_detail::bad_shape(nrows, ncols) || smooth > MODLE_PIXELS_MAX_SCC_SMOOTH ||
         min_diag > max_diag || max_diag > nrows - 1 || max_diag + 2 * smooth > nrows - 1;
}

// enqueues the kernels on checked arguments
int scc_impl(modle_pixels_handle* h, const uint32_t* d_ref, const uint32_t* d_tgt, uint64_t nrows, uint64_t ncols,
             uint64_t smooth, uint64_t min_diag, uint64_t max_diag, uint64_t* d_out, hipStream_t stream, char* err,
             size_t errlen) {
  PIX_TRY(hipSetDevice(h->device));
  const uint64_t strips = (max_diag - min_diag) / kStrip + 1;
  // the tiles of the first strip, the longest one
  const uint64_t per_tile = smooth == 0 ? kStreamCols : kTile;
  const uint64_t tiles = (ncols - min_diag + per_tile - 1) / per_tile;
  const unsigned groups = static_cast<unsigned>(std::min<uint64_t>(tiles, kMaxGroups));
  const int rc = h->scc_partial.ensure(strips * groups * (kWords * kStrip), err, errlen);
  if (rc != MODLE_PIXELS_OK) return rc;
  const dim3 grid(static_cast<unsigned>(strips), groups);
  const int64_t nr = static_cast<int64_t>(nrows), nc = static_cast<int64_t>(ncols);
  const int64_t lo = static_cast<int64_t>(min_diag), hi = static_cast<int64_t>(max_diag);
  u64* partial = reinterpret_cast<u64*>(h->scc_partial.dev);
  if (smooth == 0)
    hipLaunchKernelGGL(scc_stream, grid, dim3(kThreads), 0, stream, d_ref, d_tgt, nr, nc, lo, hi, partial);
  else
    hipLaunchKernelGGL(scc_smooth, grid, dim3(kThreads), 0, stream, d_ref, d_tgt, nr, nc, static_cast<int>(smooth), lo,
                       hi, partial);
  PIX_TRY(hipGetLastError());
  hipLaunchKernelGGL(scc_fold, dim3(static_cast<unsigned>((nrows + 255) / 256)), dim3(256), 0, stream, partial, nr, lo,
                     hi, groups, reinterpret_cast<u64*>(d_out));
  PIX_TRY(hipGetLastError());
  return MODLE_PIXELS_OK;
}

}  // namespace

extern "C" uint64_t modle_pixels_scc_groups(void) { return kMaxGroups; }

extern "C" int modle_pixels_scc(modle_pixels_handle* h, const uint32_t* d_ref, const uint32_t* d_tgt, uint64_t nrows,
                                uint64_t ncols, uint64_t smooth, uint64_t min_diag, uint64_t max_diag,
                                uint64_t* d_out, uint64_t out_words, void* stream, char* err, size_t errlen) {
  if (h == nullptr || d_ref == nullptr || d_tgt == nullptr || d_out == nullptr ||
      bad_request(nrows, ncols, smooth, min_diag, max_diag) || out_words != uint64_t{kWords} * nrows ||
      (reinterpret_cast<uintptr_t>(d_out) & 7) != 0) {
    set_err(err, errlen, std::string("modle_pixels_scc: invalid argument ") + kRule);
    return MODLE_PIXELS_ERR_ARG;
  }
  const uint64_t band = modle_pixels_detail::band_bytes(nrows, ncols);
  if (modle_pixels_detail::any_overlap({{d_out, out_words * 8}}, {{d_ref, band}, {d_tgt, band}})) {
    set_err(err, errlen, "modle_pixels_scc: the output overlaps a band");
    return MODLE_PIXELS_ERR_ARG;
  }
  return scc_impl(h, d_ref, d_tgt, nrows, ncols, smooth, min_diag, max_diag, d_out, static_cast<hipStream_t>(stream),
                  err, errlen);
}

extern "C" int modle_pixels_scc_to_host(modle_pixels_handle* h, const uint32_t* d_ref, const uint32_t* d_tgt,
                                        uint64_t nrows, uint64_t ncols, uint64_t smooth, uint64_t min_diag,
                                        uint64_t max_diag, const uint64_t** rows, void* stream, char* err,
                                        size_t errlen) {
  if (rows != nullptr) *rows = nullptr;
  if (h == nullptr || d_ref == nullptr || d_tgt == nullptr || rows == nullptr ||
      bad_request(nrows, ncols, smooth, min_diag, max_diag)) {
    set_err(err, errlen, std::string("modle_pixels_scc_to_host: invalid argument ") + kRule);
    return MODLE_PIXELS_ERR_ARG;
  }
  const hipStream_t st = static_cast<hipStream_t>(stream);
  return modle_pixels_detail::sums_to_host(h, uint64_t{kWords} * nrows, rows, st, err, errlen, [&](uint64_t* d_out) {
    return scc_impl(h, d_ref, d_tgt, nrows, ncols, smooth, min_diag, max_diag, d_out, st, err, errlen);
  });
}
