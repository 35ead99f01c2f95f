// modle_profiles.hip -- the cross-sections of every bin's stripes, summed on the MI355X
// (include/modle_pixels.h: modle_pixels_stripe_profiles / _stripe_profiles_to_host / _coarse_stripe_profiles_to_host).
//
// For bin c, offset o in [-m, m] and length L_k the library writes
//   V[k][o][c] = sum over d0 <= d < L_k of M(c - d, c + o)   the stripe upstream of c, seen o columns to the side
//   H[k][o][c] = sum over d0 <= d < L_k of M(c + o, c + d)   the stripe downstream of c, seen o rows to the side
// into out[2][K][2 m + 1][ncols], cells outside the chromosome counting 0.  With d0 >= m no cell crosses the main
// diagonal and with L_K + m <= nrows none leaves the band, so
//   V[k][o][c] is a segment of band column q = c + o: the contiguous words [d0 + o, L_k + o) that are pixels (<= q);
//   H[k][o][c] is a segment of matrix row r = c + o: the diagonals [d0 - o, L_k - o), words nrows + 1 apart, whose
//              column r + e is below ncols.
// So the output is the prefix sums of the columns and of the rows, read off at (K + 1)(2 m + 1) <= 85 cut points
// (boundary b of d0, L_1 .. L_K, shifted by o), and the band is read once per direction, not 2 m + 1 times.
// Two kernels, both output-stationary: a segment has one owner, nothing is cleared beforehand, there are no atomics
// and every output word is stored once, with a plain store.
//
//   vertical    a wave owns a column.  It reads the words d0 - m .. min(L_K + m, q + 1) - 1 in whole-wave
//               contiguous loads (four in flight), forms their 64-bit prefix sums with a wave scan carried from
//               chunk to chunk, and every lane picks the prefix at its cut points (two per lane: 85 <= 128) out of
//               the chunk that holds them by a shuffle.  The words d > q (the left-edge triangle, the same cells
//               as c - d < 0) are never addressed.
//   horizontal  a workgroup owns the 64 rows r0 .. r0 + 63 and lane l of every wave stands for row r0 + l.  Of
//               column j = r0 + jj the words e = jj - l, 64 contiguous ones, belong to these rows, one per lane
//               (the access pattern of stripes_horizontal: every pixel is read once, in memory order).  A lane
//               keeps its row's running sum and leaves it in LDS when its diagonal is a cut point: the cut points
//               of boundary b are the 2 m + 1 consecutive diagonals b - m .. b + m.  The four waves split the
//               columns into four consecutive segments; a snapshot is taken by the one wave whose segment holds
//               column r + e and counts from that segment's start, and the totals of the segments before it,
//               which the waves leave in LDS too, are added when the words are stored.
//
// The output words whose column or row c + o lies outside [0, ncols) have no owning column or row: the owner of
// column (row) c stores their zeros, so that every word of the output still has exactly one writer.
//
// LDS of the horizontal kernel: (K + 1)(2 m + 1) snapshots + 4 totals, each 64 lanes of 8 bytes, lane-contiguous
// (a wave's ds_write_b64 / ds_read_b64 touches 64 consecutive 8-byte words: no bank conflict): 45.5 KiB at m = 8,
// K = 4 (three workgroups = 12 waves on a CU's 160 KiB), 3 KiB at m = 0, K = 1.  It is dynamic, so that a small
// request does not pay for the largest one.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "modle_pixels.h"
#include "pixels_context.h"
#include "pixels_device.h"

namespace {

using modle_pixels_device::grid_of;
using modle_pixels_device::group_id;
using modle_pixels_device::u64;
using modle_pixels_device::wave_last;
using modle_pixels_device::wave_scan;

constexpr unsigned kBins = 64;    // rows of a workgroup of the horizontal kernel = lanes of a wave
constexpr unsigned kWaves = 4;    // waves of a workgroup
constexpr unsigned kUnroll = 4;   // loads in flight per lane
constexpr unsigned kMaxOffset = MODLE_PIXELS_MAX_PROFILE_OFFSET;
constexpr unsigned kMaxLengths = MODLE_PIXELS_MAX_PROFILE_LENGTHS;
static_assert((kMaxLengths + 1) * (2 * kMaxOffset + 1) <= 128, "two cut points per lane of the vertical kernel");

// the boundaries of the segments: b[0] = min_diag, b[1 .. K] = the lengths
struct Cuts {
  uint32_t b[kMaxLengths + 1];
};

// cuts.b[i] without an indexed read of the kernel's arguments (which would go through scratch)
__device__ __forceinline__ uint32_t cut_at(const Cuts& cuts, unsigned i) {
  uint32_t v = cuts.b[0];
#pragma unroll
  for (unsigned k = 1; k <= kMaxLengths; ++k) v = i == k ? cuts.b[k] : v;
  return v;
}

// out: direction 0, [K][W][ncols]
__global__ __launch_bounds__(64 * kWaves) void profiles_vertical(const uint32_t* __restrict__ band, u64 nrows,
                                                                 u64 ncols, Cuts cuts, unsigned K, unsigned m,
                                                                 u64* __restrict__ out) {
  const unsigned lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const u64 q = group_id() * kWaves + wv;  // (the same in every lane of the wave; no barrier below)
  if (q >= ncols) return;
  const unsigned W = 2 * m + 1, ncut = (K + 1) * W;
  const u64 npix = min(q + 1, nrows);                                  // the words d <= q are pixels
  const u64 dlo = cuts.b[0] - m;                                       // the lowest cut point
  const u64 dtop = max(min(static_cast<u64>(cut_at(cuts, K)) + m, npix), dlo);  // one past the last word read

  // the cut points of this lane: e = bi * W + oi for e = lane and lane + 64, clamped to [dlo, dtop]
  unsigned bi[2], oi[2];
  u64 t[2], p[2] = {0, 0};
  bool has[2];
#pragma unroll
  for (unsigned s = 0; s < 2; ++s) {
    const unsigned e = lane + 64 * s;
    has[s] = e < ncut;
    bi[s] = has[s] ? e / W : 0;
    oi[s] = has[s] ? e - bi[s] * W : 0;
    t[s] = min(max(static_cast<u64>(cut_at(cuts, bi[s])) + oi[s] - m, dlo), dtop);  // (b + o >= dlo: b >= d0)
  }

  const uint32_t* col = band + q * nrows;
  u64 carry = 0, base = dlo;
  // (modle_insulation.hip has a loop like this one; only the scan inside is shared: there every word of the prefix
  // goes to LDS, here it is picked at the cut points by a shuffle)
  for (u64 s0 = dlo; s0 < dtop; s0 += kUnroll * 64) {  // (the same in every lane)
    uint32_t v[kUnroll];
#pragma unroll
    for (unsigned u = 0; u < kUnroll; ++u) {
      const u64 d = s0 + u * 64 + lane;
      v[u] = d < dtop ? col[d] : 0u;
    }
#pragma unroll
    for (unsigned u = 0; u < kUnroll; ++u) {
      if (s0 + u * 64 >= dtop) break;  // (the same in every lane)
      const u64 x = wave_scan(v[u], lane);
      const u64 excl = carry + x - v[u];  // the sum of the words dlo .. base + lane - 1
#pragma unroll
      for (unsigned s = 0; s < 2; ++s) {
        const u64 at = t[s] - base;  // (wraps below the chunk: not < 64)
        const u64 y = __shfl(excl, static_cast<int>(at & 63));
        if (at < 64) p[s] = y;
      }
      carry += wave_last(x);
      base += 64;
    }
  }
#pragma unroll
  for (unsigned s = 0; s < 2; ++s)
    if (t[s] >= base) p[s] = carry;  // the cut point one past the last chunk (or no chunk at all: 0)

  // the cut points of d0 (bi == 0) are e = oi < 17: in p[0] of lane oi
#pragma unroll
  for (unsigned s = 0; s < 2; ++s) {
    const u64 lo = __shfl(p[0], static_cast<int>(oi[s]));
    if (!has[s] || bi[s] == 0) continue;
    u64* row = out + (static_cast<u64>(bi[s] - 1) * W + oi[s]) * ncols;
    // column q is c + o of the anchor c = q - o
    const u64 c = q + m - oi[s];  // (wraps below 0: not < ncols)
    if (c < ncols) row[c] = p[s] - lo;
    // the anchor c = q itself has no column q + o: its zero
    const u64 side = q + oi[s] - m;  // (wraps below 0)
    if (side >= ncols) row[q] = 0;
  }
}

// out: direction 1, [K][W][ncols]; dynamic LDS: ((K + 1) * W + kWaves) * 64 words of 8 bytes
__global__ __launch_bounds__(kBins * kWaves) void profiles_horizontal(const uint32_t* __restrict__ band, u64 nrows,
                                                                      u64 ncols, Cuts cuts, unsigned K, unsigned m,
                                                                      u64* __restrict__ out) {
  extern __shared__ u64 lds[];
  const unsigned lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const unsigned W = 2 * m + 1, ncut = (K + 1) * W;
  u64* snap = lds;                      // [bi * W + (e - (b - m))][lane]
  u64* total = lds + ncut * kBins;      // [wave][lane]
  const u64 r0 = group_id() * kBins;    // (the same in every thread of the workgroup)
  if (r0 >= ncols) return;
  const unsigned elo = cuts.b[0] - m, etop = cut_at(cuts, K) + m;  // the diagonals elo <= e < etop are summed
  // row r0 + lane meets diagonal e in column r0 + jj, jj = e + lane: jj in [elo, etop + 63], etop a cut point
  const unsigned n = etop - elo + kBins, seg = (n + kWaves - 1) / kWaves;
  const unsigned j0 = elo + wv * seg, j1 = min(j0 + seg, elo + n);  // the columns of this wave

  u64 run = 0;
  for (unsigned jj0 = j0; jj0 < j1; jj0 += kUnroll) {  // (the same in every lane of the wave)
    uint32_t v[kUnroll];
#pragma unroll
    for (unsigned u = 0; u < kUnroll; ++u) {
      const unsigned jj = jj0 + u;
      const u64 j = r0 + jj;
      // elo <= e < etop <= nrows and j < ncols: a pixel (e <= j as jj - lane <= r0 + jj)
      const bool ok = jj < j1 && jj >= lane + elo && jj - lane < etop && j < ncols;
      v[u] = ok ? band[j * nrows + (jj - lane)] : 0u;
    }
#pragma unroll
    for (unsigned u = 0; u < kUnroll; ++u) {
      const unsigned jj = jj0 + u;
      if (jj >= j1) break;  // (the same in every lane)
      const unsigned e = jj - lane;  // (wraps below 0: no cut point)
#pragma unroll
      for (unsigned b = 0; b <= kMaxLengths; ++b) {
        const unsigned at = e - (cuts.b[b] - m);  // (wraps below the boundary's cut points)
        if (b <= K && at < W) snap[(b * W + at) * kBins + lane] = run;
      }
      run += v[u];
    }
  }
  total[wv * kBins + lane] = run;
  __syncthreads();

  // every output word of the rows r0 .. r0 + 63, and the zeros of the anchors r0 .. r0 + 63 without a row
  const u64 r = r0 + lane;
  if (r >= ncols) return;
  u64 before[kWaves];  // the totals of the segments before wave x
  before[0] = 0;
#pragma unroll
  for (unsigned x = 1; x < kWaves; ++x) before[x] = before[x - 1] + total[(x - 1) * kBins + lane];
  for (unsigned item = wv; item < K * W; item += kWaves) {  // (the same in every lane of the wave)
    const unsigned k = item / W, oi = item - k * W;
    u64* row = out + static_cast<u64>(item) * ncols;
    // row r is c + o of the anchor c = r - o; its cut points are b - o = (b - m) + (2 m - oi)
    const unsigned at = 2 * m - oi;
    const u64 c = r + m - oi;  // (wraps below 0: not < ncols)
    if (c < ncols) {
      u64 sum[2];
#pragma unroll
      for (unsigned s = 0; s < 2; ++s) {
        const unsigned b = s == 0 ? 0 : k + 1;
        const unsigned jj = cut_at(cuts, b) - m + at + lane;  // the column of that diagonal: whose segment?
        const unsigned x = (jj - elo) / seg;
        u64 add = before[0];
#pragma unroll
        for (unsigned y = 1; y < kWaves; ++y) add = x == y ? before[y] : add;
        sum[s] = snap[(b * W + at) * kBins + lane] + add;
      }
      row[c] = sum[1] - sum[0];
    }
    const u64 side = r + oi - m;  // (wraps below 0)
    if (side >= ncols) row[r] = 0;
  }
}

using modle_pixels_detail::set_err;

constexpr const char* kRule =
    "(0 < nrows <= ncols, max_offset <= 8, 1..4 lengths, min_diag >= max_offset, min_diag < L_1 < ... < L_K, "
    "L_K + max_offset <= nrows, out_words == 2 * K * (2 * max_offset + 1) * ncols, an 8-byte aligned output)";

// what every entry point refuses of the offset, the lengths and min_diag on a band of `nrows`
bool bad_request(uint64_t nrows, uint64_t m, const uint64_t* lengths, uint64_t n_lengths, uint64_t min_diag) {
  if (lengths == nullptr || n_lengths == 0 || n_lengths > kMaxLengths || m > kMaxOffset || min_diag < m) return true;
  uint64_t last = min_diag;
  for (uint64_t k = 0; k < n_lengths; ++k) {
    if (lengths[k] <= last) return true;
    last = lengths[k];
  }
  return last > nrows || m > nrows - last;  // L_K + m <= nrows, without a sum that wraps
}

uint64_t words_of(uint64_t m, uint64_t n_lengths, uint64_t ncols) { return 2 * n_lengths * (2 * m + 1) * ncols; }

// enqueues the kernels on checked arguments
int profiles_impl(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows, uint64_t ncols, uint64_t m,
                  const uint64_t* lengths, uint64_t n_lengths, uint64_t min_diag, uint64_t* d_out, hipStream_t stream,
                  char* err, size_t errlen) {
  PIX_TRY(hipSetDevice(h->device));
  Cuts cuts{};
  cuts.b[0] = static_cast<uint32_t>(min_diag);  // (below nrows <= 65535 * 256)
  for (uint64_t k = 0; k < n_lengths; ++k) cuts.b[k + 1] = static_cast<uint32_t>(lengths[k]);
  for (uint64_t k = n_lengths + 1; k <= kMaxLengths; ++k) cuts.b[k] = cuts.b[n_lengths];
  const unsigned K = static_cast<unsigned>(n_lengths), mo = static_cast<unsigned>(m), W = 2 * mo + 1;
  u64* out = reinterpret_cast<u64*>(d_out);
  hipLaunchKernelGGL(profiles_vertical, grid_of((ncols + kWaves - 1) / kWaves), dim3(64 * kWaves), 0, stream, d_band,
                     nrows, ncols, cuts, K, mo, out);
  PIX_TRY(hipGetLastError());
  const size_t lds = (size_t{K + 1} * W + kWaves) * kBins * sizeof(u64);
  hipLaunchKernelGGL(profiles_horizontal, grid_of((ncols + kBins - 1) / kBins), dim3(kBins * kWaves), lds, stream,
                     d_band, nrows, ncols, cuts, K, mo, out + static_cast<uint64_t>(K) * W * ncols);
  PIX_TRY(hipGetLastError());
  return MODLE_PIXELS_OK;
}

// modle_pixels_stripe_profiles_to_host (`cs` null) and modle_pixels_coarse_stripe_profiles_to_host under their
// `name`: the band resolved, profiles_impl into the sums of the context, their copy to the pinned mirror, the wait
int profiles_one_call(const char* name, const modle_pixels_detail::CoarseSpec* cs, modle_pixels_handle* h,
                      const uint32_t* d_band, uint64_t nrows, uint64_t ncols, uint64_t m, const uint64_t* lengths,
                      uint64_t n_lengths, uint64_t min_diag, const uint64_t** profiles, void* stream, char* err,
                      size_t errlen) {
  if (profiles != nullptr) *profiles = nullptr;
  modle_pixels_detail::BandView v;
  if (h == nullptr || profiles == nullptr || !modle_pixels_detail::view_shape(d_band, nrows, ncols, cs, &v) ||
      bad_request(v.nrows, m, lengths, n_lengths, min_diag)) {
    set_err(err, errlen, modle_pixels_detail::refusal(name, cs, kRule));
    return MODLE_PIXELS_ERR_ARG;
  }
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const int rc = modle_pixels_detail::resolve_band(h, d_band, nrows, ncols, cs, &v, st, err, errlen);
  if (rc != MODLE_PIXELS_OK) return rc;
  return modle_pixels_detail::sums_to_host(h, words_of(m, n_lengths, v.ncols), profiles, st, err, errlen,
                                           [&](uint64_t* d_out) {
    return profiles_impl(h, v.d, v.nrows, v.ncols, m, lengths, n_lengths, min_diag, d_out, st, err, errlen);
  });
}

}  // namespace

extern "C" int modle_pixels_stripe_profiles(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                                            uint64_t ncols, uint64_t max_offset, const uint64_t* lengths,
                                            uint64_t n_lengths, uint64_t min_diag, uint64_t* d_out,
                                            uint64_t out_words, void* stream, char* err, size_t errlen) {
  if (h == nullptr || d_band == nullptr || d_out == nullptr || nrows == 0 ||
      modle_pixels_detail::bad_shape(nrows, ncols) || bad_request(nrows, max_offset, lengths, n_lengths, min_diag) ||
      out_words != words_of(max_offset, n_lengths, ncols) || (reinterpret_cast<uintptr_t>(d_out) & 7) != 0) {
    set_err(err, errlen, std::string("modle_pixels_stripe_profiles: invalid argument ") + kRule);
    return MODLE_PIXELS_ERR_ARG;
  }
  if (modle_pixels_detail::any_overlap({{d_out, out_words * 8}},
                                       {{d_band, modle_pixels_detail::band_bytes(nrows, ncols)}})) {
    set_err(err, errlen, "modle_pixels_stripe_profiles: the output overlaps the band");
    return MODLE_PIXELS_ERR_ARG;
  }
  return profiles_impl(h, d_band, nrows, ncols, max_offset, lengths, n_lengths, min_diag, d_out,
                       static_cast<hipStream_t>(stream), err, errlen);
}

extern "C" int modle_pixels_stripe_profiles_to_host(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                                                    uint64_t ncols, uint64_t max_offset, const uint64_t* lengths,
                                                    uint64_t n_lengths, uint64_t min_diag, const uint64_t** profiles,
                                                    void* stream, char* err, size_t errlen) {
  return profiles_one_call("modle_pixels_stripe_profiles_to_host", nullptr, h, d_band, nrows, ncols, max_offset,
                           lengths, n_lengths, min_diag, profiles, stream, err, errlen);
}

extern "C" int modle_pixels_coarse_stripe_profiles_to_host(modle_pixels_handle* h, const uint32_t* d_band,
                                                           uint64_t nrows, uint64_t ncols, uint64_t factor,
                                                           uint64_t first_bin, uint64_t max_offset,
                                                           const uint64_t* lengths, uint64_t n_lengths,
                                                           uint64_t min_diag, const uint64_t** profiles, void* stream,
                                                           char* err, size_t errlen) {
  const modle_pixels_detail::CoarseSpec cs{factor, first_bin};
  return profiles_one_call("modle_pixels_coarse_stripe_profiles_to_host", &cs, h, d_band, nrows, ncols, max_offset,
                           lengths, n_lengths, min_diag, profiles, stream, err, errlen);
}
