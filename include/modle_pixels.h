/* modle_pixels.h -- C ABI of the sparse-pixel extraction (modle_amd/libmodle_pixels.so), of the
 * coarsening of a band, of its dense regions, of its marginals, of its insulation sums, of its
 * dot candidates, of its pileups (fixed windows and rescaled ones) and of its random sampling, of the
 * way back from sorted pixels to a band, of the comparison of two bands stripe by stripe and diagonal
 * by diagonal, of the stripe profiles of one band and of its triangle sums (further down).
 *
 * The simulation leaves every interval as a dense band matrix in device memory
 * (modle_hip_interval_outputs).  A cooler file is made of the non-zero pixels only, sorted by
 * (bin1_id, bin2_id), plus the bin1_offset index; the reference converts on its IO thread
 * (src/libmodle_io/contact_matrix_dense_io_impl.hpp:51-71).  This library does the conversion
 * where the matrix lies: a count + scan + stream compaction over the band on the MI355X, so that
 * only the pixels cross to the host.  The result feeds modle_cool_append_pixels
 * (modle_cooler_pixels.h) or any other writer (hictk: INTEGRATION.md).
 *
 * Band layout (modle_cooler.h): pixel (i, j), 0 <= i <= j < ncols, j - i < nrows <= ncols, lies at
 * band[j * nrows + (j - i)].  Words with j - i > j (the left-edge triangle) and the trailing word
 * band[nrows * ncols] are not pixels: they are never read.  `d_band` is a DEVICE pointer
 * (modle_hip_interval_outputs' d_contacts, a torch tensor's data_ptr()).
 *
 * Result: the pixels with a non-zero count in cooler order (ascending bin1 = i, then ascending
 * bin2 = j) as three arrays, int64 bin1, int64 bin2, int32 count, with `bin_offset` (the
 * interval's first bin within the file) added to both ids, and int64 bin1_offset[ncols + 1]: the
 * exclusive scan of the pixels per row, relative to this interval (bin1_offset[ncols] == nnz).
 *
 * `stream` is a hipStream_t (NULL = default stream).  No call throws; errors are negative return
 * codes with a message in `err`.
 */
#ifndef MODLE_PIXELS_H
#define MODLE_PIXELS_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define MODLE_PIXELS_OK 0
#define MODLE_PIXELS_ERR_ARG (-1)    /* null pointer, nrows > ncols, nnz that does not match, ... */
#define MODLE_PIXELS_ERR_DEVICE (-2) /* a HIP call failed */
#define MODLE_PIXELS_ERR_RANGE (-3)  /* a count does not fit the int32 pixel type */

typedef struct modle_pixels_handle modle_pixels_handle;

typedef struct modle_pixels_stats {
  uint64_t nnz;       /* pixels with a non-zero count */
  uint64_t sum;       /* sum of the counts of all pixels */
  uint32_t max_count; /* largest count */
  uint32_t reserved_;
} modle_pixels_stats;

/* A context on HIP device `device`: a few words of device and pinned host memory, and the
 * buffers of the one-call form.  One context serves one call at a time. */
int modle_pixels_create(int device, modle_pixels_handle** out, char* err, size_t errlen);
void modle_pixels_destroy(modle_pixels_handle* h);

/* Step 1 of the two-step form: counts the pixels per row and scans the counts.  Fills the device
 * array d_bin1_offset (int64[ncols + 1]) and *stats, so that the caller can allocate exactly.
 * d_bin1_offset may be NULL when only the statistics are wanted.  Waits for `stream`.  A count
 * above INT32_MAX gives MODLE_PIXELS_ERR_RANGE (like modle_cool_append_matrix); *stats is filled
 * also then. */
int modle_pixels_count(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                       uint64_t ncols, int64_t* d_bin1_offset, modle_pixels_stats* stats,
                       void* stream, char* err, size_t errlen);

/* Step 2: writes the pixels into the caller-owned device arrays d_bin1, d_bin2 (int64[nnz]) and
 * d_count (int32[nnz]).  `d_bin1_offset` and `nnz` are step 1's, of the same unchanged band;
 * nothing is stored at or beyond entry `nnz` whatever the band holds.  The kernel is enqueued on
 * `stream`; the call does not wait for it. */
int modle_pixels_extract(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                         uint64_t ncols, int64_t bin_offset, const int64_t* d_bin1_offset,
                         int64_t* d_bin1, int64_t* d_bin2, int32_t* d_count, uint64_t nnz,
                         void* stream, char* err, size_t errlen);

/* One-call form: both steps and the copy of the result to the host.  *bin1, *bin2, *count
 * (stats->nnz entries) and *bin1_offset (ncols + 1 entries) point to pinned host buffers owned by
 * the context: they stay valid until the next call on it.  On MODLE_PIXELS_ERR_RANGE nothing
 * is extracted and the pointers are NULL. */
int modle_pixels_to_host(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                         uint64_t ncols, int64_t bin_offset, const int64_t** bin1,
                         const int64_t** bin2, const int32_t** count, const int64_t** bin1_offset,
                         modle_pixels_stats* stats, void* stream, char* err, size_t errlen);

/* ---- Coarsening: the same contacts at `factor` times the bin size -------------------------
 *
 * `first_bin` is the chromosome-relative index of the interval's first fine bin (offset_bp /
 * bin_size): coarse bins are anchored at the chromosome's start, not at the interval's.  With
 * p = first_bin % factor, fine column i belongs to coarse column (i + p) / factor, and coarse pixel
 * (I, J) is the sum of the fine pixels (i, j) with (i + p) / factor == I and (j + p) / factor == J
 * (in a diagonal block the upper triangle only, like `cooler coarsen`).  The result is a band in
 * the layout above, of
 *     ncols' = (p + ncols + factor - 1) / factor
 *     nrows' = min(ncols', (nrows - 1 + factor - 1) / factor + 1)
 * and nrows' * ncols' + 1 words, EVERY one of which is written: pixels hold their sums, the words
 * that are no pixels (left-edge triangle, trailing word) hold 0; the caller does not pre-zero.
 * A sum that does not fit 32 bits is stored as 0xFFFFFFFF (saturation), which the range check of
 * modle_pixels_count then reports.  Coarsening by k1 with first_bin and then by k2 with
 * first_bin / k1 equals coarsening by k1 * k2 with first_bin.
 *
 * `factor` < 2 (or above 2^32), nrows == 0 and nrows > ncols are MODLE_PIXELS_ERR_ARG. */

/* The shape of the coarse band.  Host only: no device is needed. */
int modle_pixels_coarse_shape(uint64_t nrows, uint64_t ncols, uint64_t factor, uint64_t first_bin,
                              uint64_t* nrows_out, uint64_t* ncols_out);

/* Enqueues the coarsening of the band at `d_band` into the device array `d_out` of `out_words`
 * words (>= nrows' * ncols' + 1, else MODLE_PIXELS_ERR_ARG and nothing is written) on `stream`;
 * the call does not wait.  The input is read, never written, and must not overlap `d_out`. */
int modle_pixels_coarsen(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                         uint64_t ncols, uint64_t factor, uint64_t first_bin, uint32_t* d_out,
                         uint64_t out_words, void* stream, char* err, size_t errlen);

/* One call: coarsen into a scratch band owned by the context (grown on demand, freed by
 * modle_pixels_destroy), then modle_pixels_to_host on it.  `bin_offset` is the interval's first
 * bin within the COARSE file; *bin1_offset has ncols' + 1 entries. */
int modle_pixels_coarse_to_host(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                                uint64_t ncols, uint64_t factor, uint64_t first_bin,
                                int64_t bin_offset, const int64_t** bin1, const int64_t** bin2,
                                const int32_t** count, const int64_t** bin1_offset,
                                modle_pixels_stats* stats, void* stream, char* err, size_t errlen);

/* ---- Dense regions: the band unpacked into square tiles -------------------------------------
 *
 * A run of `count` tiles: tile t covers the bins lo_t = first + t * step .. lo_t + size - 1 of the
 * band and becomes the symmetric size x size matrix
 *     out[t][r][c] = d < nrows ? band[j * nrows + d] : 0,   a = lo_t + r, b = lo_t + c,
 *                                                             d = |a - b|, j = max(a, b)
 * of uint32[count][size][size], row-major: the same integers in another layout.  EVERY output word is
 * written exactly once, the zeros outside the band included; the caller does not pre-zero.  The
 * words of the band that are no pixels are never read.  A single region is count == 1. */

/* How many tiles of the run lie inside [0, ncols): (ncols - first - size) / step + 1.  Host only.
 * size == 0, step == 0 and first + size > ncols are MODLE_PIXELS_ERR_ARG. */
int modle_pixels_tiles_fit(uint64_t ncols, uint64_t first, uint64_t size, uint64_t step,
                           uint64_t* max_count);

/* Enqueues the unpacking of `count` tiles into the device array `d_out` of `out_words` words on
 * `stream`; the call does not wait.  MODLE_PIXELS_ERR_ARG, with nothing written: a null pointer,
 * nrows == 0, nrows > ncols, count == 0, count > modle_pixels_tiles_fit's max_count, out_words <
 * count * size * size (a product that overflows included), d_out overlapping the band.  The input is
 * read, never written. */
int modle_pixels_dense_tiles(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                             uint64_t ncols, uint64_t first, uint64_t size, uint64_t step,
                             uint64_t count, uint32_t* d_out, uint64_t out_words, void* stream,
                             char* err, size_t errlen);

/* One call for the single region [lo, hi), 0 <= lo < hi <= ncols: unpacks into a scratch buffer
 * of the context and copies it to a pinned host buffer of the context (both grown on demand, freed
 * by modle_pixels_destroy).  *dense (uint32[hi - lo][hi - lo]) stays valid until the next call on
 * the context.  Waits for `stream`. */
int modle_pixels_dense_to_host(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                               uint64_t ncols, uint64_t lo, uint64_t hi, const uint32_t** dense,
                               void* stream, char* err, size_t errlen);

/* ---- Marginals: the sums per diagonal and per bin --------------------------------------------
 *
 *     diag_sum[d] = sum of band[j * nrows + d] over d <= j < ncols,          0 <= d < nrows
 * is the numerator of the distance-decay curve ("expected"); its denominator, the number of pixels
 * of diagonal d, is ncols - d and needs no device.
 *     coverage[i],  0 <= i < ncols,
 * is row i of the symmetric matrix, with the diagonal pixel counted once and the diagonals below
 * `min_diag` left out: the column part, band[i * nrows + d] over max(min_diag, 0) <= d <=
 * min(i, nrows - 1), plus the row part, band[(i + d) * nrows + d] over max(min_diag, 1) <= d <=
 * min(nrows - 1, ncols - 1 - i).  So the sum of diag_sum is modle_pixels_stats.sum, and with
 * min_diag == 0 the sum of coverage is 2 * sum - diag_sum[0].  min_diag >= nrows gives a coverage
 * of zeros.
 *
 * Both are exact 64-bit integer sums, whatever the order of summation, from one pass that reads
 * every pixel word once; the words that are no pixels are never read.  EVERY output word is written
 * by the call: the caller does not pre-zero.  No sum can overflow for ncols < 2^32: diag_sum[d] is a
 * sum of at most ncols words below 2^32, coverage[i] of fewer than 2 * nrows, and nrows is below 2^24
 * (the largest modle_pixels_count accepts).
 *
 * MODLE_PIXELS_ERR_ARG, with nothing written: a null handle or band, nrows == 0, nrows > ncols, no
 * output asked for, an output that overlaps the band. */

/* Enqueues the sums into the device arrays d_diag_sum (uint64[nrows]) and d_coverage
 * (uint64[ncols]) on `stream`; the call does not wait.  Either may be NULL when that result is not
 * wanted.  The sums are formed in words of the context and copied out whole, so the arrays need only
 * be 4-byte aligned (any other alignment is MODLE_PIXELS_ERR_ARG). */
int modle_pixels_marginals(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                           uint64_t ncols, uint64_t min_diag, uint64_t* d_diag_sum,
                           uint64_t* d_coverage, void* stream, char* err, size_t errlen);

/* The same into pinned host buffers of the context (grown on demand, freed by
 * modle_pixels_destroy): *diag_sum (nrows entries) and *coverage (ncols entries) stay valid until
 * the next call on the context.  Either of `diag_sum` and `coverage` may be NULL.  Waits for
 * `stream`. */
int modle_pixels_marginals_to_host(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                                   uint64_t ncols, uint64_t min_diag, const uint64_t** diag_sum,
                                   const uint64_t** coverage, void* stream, char* err,
                                   size_t errlen);

/* One call at `factor` times the bin size: coarsens into the scratch band of the context (like
 * modle_pixels_coarse_to_host), then modle_pixels_marginals_to_host on it.  *diag_sum has nrows'
 * and *coverage ncols' entries (modle_pixels_coarse_shape); `min_diag` counts coarse diagonals.  A
 * coarse pixel that saturated enters the sums as 0xFFFFFFFF: modle_pixels_coarse_to_host reports
 * such a band as MODLE_PIXELS_ERR_RANGE. */
int modle_pixels_coarse_marginals_to_host(modle_pixels_handle* h, const uint32_t* d_band,
                                          uint64_t nrows, uint64_t ncols, uint64_t factor,
                                          uint64_t first_bin, uint64_t min_diag,
                                          const uint64_t** diag_sum, const uint64_t** coverage,
                                          void* stream, char* err, size_t errlen);

/* ---- Insulation: the sums over a sliding diamond window --------------------------------------
 *
 * For a window of `w` bins the diamond of bin b is the set of pixels (a, c) with
 *     b - w + 1 <= a <= b <= c <= b + w - 1,   a >= 0,   c < ncols,   c - a >= min_diag
 * (cooltools' insul_diamond convention: bin b lies on both sides of its own diamond), and
 *     ins_sum[k][b] = sum of band[c * nrows + (c - a)] over the diamond of b for windows[k]
 *     n_valid[b]    = the number of pixels of that diamond
 *                   = na * nc - #{(p, q): p < na, q < nc, p + q < min_diag},
 *                     na = min(w, b + 1), nc = min(w, ncols - b).
 * Their quotient is the mean the insulation score is the log-ratio of; its minima are the domain
 * boundaries.  The sums are exact 64-bit integers (at most w^2 <= 2^20 words below 2^32: no sum can
 * overflow); the words of the band that are no pixels are never read.  EVERY output word is written
 * exactly once, with a plain store: the caller does not pre-zero.  min_diag >= 2 * w - 1 gives zeros
 * for that window.
 *
 * A window is accepted only when its whole diamond lies in the band: 1 <= w <= MODLE_PIXELS_MAX_WINDOW
 * and 2 * w - 1 <= nrows; a call takes 1 .. MODLE_PIXELS_MAX_WINDOWS windows, in any order, from the
 * HOST array `windows`.  MODLE_PIXELS_ERR_ARG, with nothing written: a window or a number of windows
 * that is not accepted, a null pointer, nrows == 0, nrows > ncols, out_words < n_windows * ncols, a
 * d_out that is not 8-byte aligned or overlaps the band. */
#define MODLE_PIXELS_MAX_WINDOW 1024
#define MODLE_PIXELS_MAX_WINDOWS 8

/* n_valid[b] for every bin b < ncols.  Host only: no device is needed.  window == 0 or above
 * MODLE_PIXELS_MAX_WINDOW and a null pointer are MODLE_PIXELS_ERR_ARG. */
int modle_pixels_insulation_n_valid(uint64_t ncols, uint64_t window, uint64_t min_diag,
                                    uint64_t* n_valid /* [ncols] */);

/* Enqueues the sums into the device array d_out (uint64[n_windows][ncols], of `out_words` >=
 * n_windows * ncols words) on `stream`; the call does not wait. */
int modle_pixels_insulation(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                            uint64_t ncols, const uint64_t* windows, uint64_t n_windows,
                            uint64_t min_diag, uint64_t* d_out, uint64_t out_words, void* stream,
                            char* err, size_t errlen);

/* The same into a pinned host buffer of the context (grown on demand, freed by modle_pixels_destroy):
 * *ins_sum (uint64[n_windows][ncols]) stays valid until the next call on the context.  Waits for
 * `stream`. */
int modle_pixels_insulation_to_host(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                                    uint64_t ncols, const uint64_t* windows, uint64_t n_windows,
                                    uint64_t min_diag, const uint64_t** ins_sum, void* stream,
                                    char* err, size_t errlen);

/* One call at `factor` times the bin size: coarsens into the scratch band of the context (like
 * modle_pixels_coarse_marginals_to_host), then modle_pixels_insulation_to_host on it.  *ins_sum is
 * uint64[n_windows][ncols'] (modle_pixels_coarse_shape); the windows and `min_diag` count coarse bins
 * and the rule for the windows holds against nrows'. */
int modle_pixels_coarse_insulation_to_host(modle_pixels_handle* h, const uint32_t* d_band,
                                           uint64_t nrows, uint64_t ncols, uint64_t factor,
                                           uint64_t first_bin, const uint64_t* windows,
                                           uint64_t n_windows, uint64_t min_diag,
                                           const uint64_t** ins_sum, void* stream, char* err,
                                           size_t errlen);

/* ---- Dots: HiCCUPS neighbourhood sums and the candidate pixels ---------------------------------
 *
 * A dot is a focal enrichment of a pixel over its surroundings.  For pixel (i, j), i <= j, d = j - i,
 * obs = band[j * nrows + d], a window half-width `w` and a peak half-width `p`, 0 <= p < w <=
 * MODLE_PIXELS_MAX_DOT_WINDOW, the four neighbourhoods of Rao et al. 2014 (and of cooltools), in (row,
 * column) of the symmetric matrix, are
 *   k = 0  donut       [i-w, i+w] x [j-w, j+w] without [i-p, i+p] x [j-p, j+p] and without the rest of
 *                      row i and of column j                    area (2w+1)^2 - (2p+1)^2 - 4 (w-p)
 *   k = 1  lower-left  [i+1, i+w] x [j-w, j-1] without [i+1, i+p] x [j-p, j-1]       area w^2 - p^2
 *   k = 2  horizontal  rows i-1 .. i+1, columns [j-w, j-p-1] and [j+p+1, j+w]        area 6 (w-p)
 *   k = 3  vertical    rows [i-w, i-p-1] and [i+p+1, i+w], columns j-1 .. j+1        area 6 (w-p)
 * and O_k(i, j) is the exact integer sum of the band over neighbourhood k: at most 1681 words below
 * 2^32, so below 2^43 -- it cannot overflow 64 bits and is exact as a double.
 *
 * A pixel is VALID when its whole (2w+1)^2 square lies inside the matrix, inside the band and on or
 * above diagonal `min_diag`: i >= w, j + w < ncols, 2w + min_diag <= d <= nrows - 1 - 2w.  A call is
 * accepted only when 4w + 1 + min_diag <= nrows; then no word that is no pixel (left-edge triangle,
 * trailing word, d >= nrows) is ever read.  A band without a valid pixel is legal and gives zeros.
 *
 * The decision uses the HOST table scale[4][nrows] of doubles, every entry >= 0 and no NaN (+inf is
 * allowed); only the entries at valid d are read.  A valid pixel is a CANDIDATE when obs >= min_count
 * (min_count >= 1) and, for every k, (double)obs >= (double)O_k * scale[k][d]: one IEEE-754 double
 * multiplication and one comparison, which is false against NaN (0 * inf).  Nothing else on the device
 * uses floating point.
 *
 * Outputs (at least one; the call defines EVERY word of both, the caller does not pre-zero):
 *   d_cand  uint32[nrows * ncols + 1] in the band's layout: obs at a candidate, 0 everywhere else
 *           (triangle and trailing word included) -- a band modle_pixels_count / _extract accept as is;
 *   d_sums  uint64[4][nrows * ncols], 8-byte aligned: d_sums[k][j * nrows + d] = O_k at a valid pixel,
 *           0 elsewhere.  Without d_cand the table is not used and may be NULL.
 *
 * MODLE_PIXELS_ERR_ARG, with nothing written: a null handle or band, no output, nrows == 0, nrows >
 * ncols, p >= w, w == 0, w > 20, 4w + 1 + min_diag > nrows, min_count == 0, a NaN or negative table
 * entry at a valid d, a misaligned d_sums, an output that overlaps the band or the other output. */
#define MODLE_PIXELS_MAX_DOT_WINDOW 20

/* Enqueues the work on `stream`; the call does not wait. */
int modle_pixels_dots(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows, uint64_t ncols,
                      uint64_t w, uint64_t p, uint64_t min_diag, uint64_t min_count,
                      const double* scale, uint32_t* d_cand, uint64_t* d_sums, void* stream, char* err,
                      size_t errlen);

/* The candidates as sorted pixels: the kernel fills a scratch band of the context, then the count /
 * scan / extract of modle_pixels_to_host run on it.  Results and `bin_offset` as for
 * modle_pixels_to_host (pinned buffers of the context, valid until the next call on it). */
int modle_pixels_dots_to_host(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                              uint64_t ncols, uint64_t w, uint64_t p, uint64_t min_diag,
                              uint64_t min_count, const double* scale, int64_t bin_offset,
                              const int64_t** bin1, const int64_t** bin2, const int32_t** count,
                              const int64_t** bin1_offset, modle_pixels_stats* stats, void* stream,
                              char* err, size_t errlen);

/* The same at `factor` times the bin size: coarsens into the scratch band of the context (like
 * modle_pixels_coarse_to_host), the candidates go to a second scratch band.  `w`, `p`, `min_diag`
 * count coarse bins, the table has nrows' columns and the acceptance rule holds against nrows'
 * (modle_pixels_coarse_shape); `bin_offset` is the interval's first bin within the COARSE file. */
int modle_pixels_coarse_dots_to_host(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                                     uint64_t ncols, uint64_t factor, uint64_t first_bin, uint64_t w,
                                     uint64_t p, uint64_t min_diag, uint64_t min_count,
                                     const double* scale, int64_t bin_offset, const int64_t** bin1,
                                     const int64_t** bin2, const int32_t** count,
                                     const int64_t** bin1_offset, modle_pixels_stats* stats,
                                     void* stream, char* err, size_t errlen);

/* ---- Dots, the statistical test: lambda-chunk histograms and count thresholds -------------------
 *
 * The other half of HiCCUPS (Rao et al. 2014; `cooltools dots`): every pixel is binned by its locally
 * adjusted expected value into logarithmic "lambda chunks", the observed counts of every chunk are
 * histogrammed over the whole genome, the host turns every chunk's histogram into a count threshold (a
 * Poisson tail under a Benjamini-Hochberg rule: pixels.dot_thresholds) and a pixel is called when it
 * clears the threshold of its chunk for all four neighbourhoods.  Shape, `w`, `p`, `min_diag`, the VALID
 * pixels, O_k and the acceptance rule 4w + 1 + min_diag <= nrows are those of modle_pixels_dots.
 *
 *   lam[4][nrows]   HOST doubles; at the valid d every entry >= 0 and no NaN (+inf is allowed), only those
 *                   are read.  In the front end e[d] / X_k[d], pixels.dot_scales with folds of 1.  The
 *                   lambda of a valid pixel is lambda_k = (double)O_k * lam[k][d]: one IEEE-754 double
 *                   product, never contracted.
 *   edges[n_edges]  HOST doubles, 1 <= n_edges <= MODLE_PIXELS_MAX_DOT_EDGES, finite, > 0, strictly
 *                   increasing; n_chunks = n_edges + 1.
 *   chunk(lambda)   the number of edges strictly below lambda: chunk c is (edges[c-1], edges[c]], the
 *                   pd.cut convention of cooltools.  A NaN lambda (0 * inf) goes to the top chunk n_edges;
 *                   +inf goes there by the rule itself.  The top chunk has no finite upper edge.
 *
 * HISTOGRAM: uint64 hist[4][n_chunks][n_obs], 2 <= n_obs <= MODLE_PIXELS_MAX_DOT_OBS.  For every VALID
 * pixel (a zero is a pixel too) and every k, modle_pixels_dot_hist ADDS one to
 *     hist[k][chunk(lambda_k)][min(obs, n_obs - 1)]:
 * the caller zeroes the table, and the intervals of a genome accumulate into one.  Nothing else is
 * written.  d_hist is 8-byte aligned and does not overlap the band.  The adds are integer atomics, so
 * the table does not depend on their order.
 *
 * DECISION: thr[4][n_chunks] is a HOST table of uint32, 0 = "never".  A valid pixel is a CANDIDATE when
 * obs >= min_count (>= 1), for every k  t = thr[k][chunk(lambda_k)] != 0 and obs >= t, and, when `scale`
 * is not NULL, also the fold test of modle_pixels_dots, (double)obs >= (double)O_k * scale[k][d] (the
 * table as there).  d_cand is that of modle_pixels_dots: the call defines every word, the trailing one
 * included.
 *
 * MODLE_PIXELS_ERR_ARG, with nothing written: what modle_pixels_dots refuses of handle, band, shape, w, p,
 * min_diag (and of min_count, scale and d_cand in the decision), a null lam, edges, thr or output, a NaN or
 * negative lam entry at a valid d, n_edges or n_obs out of range, edges that are not finite, positive and
 * strictly increasing, a misaligned d_hist, an output that overlaps the band. */
#define MODLE_PIXELS_MAX_DOT_EDGES 63
#define MODLE_PIXELS_MAX_DOT_OBS 16384

/* Enqueues the work on `stream`; the call does not wait. */
int modle_pixels_dot_hist(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows, uint64_t ncols,
                          uint64_t w, uint64_t p, uint64_t min_diag, const double* lam,
                          const double* edges, uint64_t n_edges, uint64_t n_obs, uint64_t* d_hist,
                          void* stream, char* err, size_t errlen);

/* One call: zeroes a scratch table of the context, runs the kernel, copies the table to pinned memory of
 * the context (*hist: uint64[4][n_chunks][n_obs], valid until the next call on it) and waits. */
int modle_pixels_dot_hist_to_host(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                                  uint64_t ncols, uint64_t w, uint64_t p, uint64_t min_diag,
                                  const double* lam, const double* edges, uint64_t n_edges,
                                  uint64_t n_obs, const uint64_t** hist, void* stream, char* err,
                                  size_t errlen);

/* The same at `factor` times the bin size, as modle_pixels_coarse_dots_to_host: `w`, `p`, `min_diag` count
 * coarse bins and lam has nrows' columns. */
int modle_pixels_coarse_dot_hist_to_host(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                                         uint64_t ncols, uint64_t factor, uint64_t first_bin, uint64_t w,
                                         uint64_t p, uint64_t min_diag, const double* lam,
                                         const double* edges, uint64_t n_edges, uint64_t n_obs,
                                         const uint64_t** hist, void* stream, char* err, size_t errlen);

/* The decision into d_cand; enqueues the work on `stream`, the call does not wait. */
int modle_pixels_dots_fdr(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows, uint64_t ncols,
                          uint64_t w, uint64_t p, uint64_t min_diag, uint64_t min_count,
                          const double* lam, const double* edges, uint64_t n_edges, const uint32_t* thr,
                          const double* scale, uint32_t* d_cand, void* stream, char* err, size_t errlen);

/* The candidates as sorted pixels, as modle_pixels_dots_to_host. */
int modle_pixels_dots_fdr_to_host(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                                  uint64_t ncols, uint64_t w, uint64_t p, uint64_t min_diag,
                                  uint64_t min_count, const double* lam, const double* edges,
                                  uint64_t n_edges, const uint32_t* thr, const double* scale,
                                  int64_t bin_offset, const int64_t** bin1, const int64_t** bin2,
                                  const int32_t** count, const int64_t** bin1_offset,
                                  modle_pixels_stats* stats, void* stream, char* err, size_t errlen);

/* The same at `factor` times the bin size, as modle_pixels_coarse_dots_to_host. */
int modle_pixels_coarse_dots_fdr_to_host(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                                         uint64_t ncols, uint64_t factor, uint64_t first_bin, uint64_t w,
                                         uint64_t p, uint64_t min_diag, uint64_t min_count,
                                         const double* lam, const double* edges, uint64_t n_edges,
                                         const uint32_t* thr, const double* scale, int64_t bin_offset,
                                         const int64_t** bin1, const int64_t** bin2,
                                         const int32_t** count, const int64_t** bin1_offset,
                                         modle_pixels_stats* stats, void* stream, char* err,
                                         size_t errlen);

/* ---- Pileups: windows around anchor pairs, summed ------------------------------------------------
 *
 * M(x, y) is the symmetric matrix of the band: M(x, y) = band[j * nrows + (j - i)], i = min(x, y),
 * j = max(x, y).  For a flank `f`, S = 2 f + 1, 0 <= f <= MODLE_PIXELS_MAX_PILEUP_FLANK, and `n` anchors
 * (a_t, b_t) = (bin1[t] - bin_offset, bin2[t] - bin_offset) from int64 arrays (modle_pixels_extract's or
 * a dot caller's output feeds in as it is), anchor t is ACCEPTED when
 *     a_t <= b_t,   a_t >= f,   b_t + f <= ncols - 1,   (b_t - a_t) + 2 f <= nrows - 1:
 * every cell of its window lies in the matrix and in the band, so no word that is no pixel (left-edge
 * triangle, trailing word) is ever read.  The rule is evaluated without signed overflow for any int64
 * value and a `bin_offset` of either sign.  a == b is a legitimate anchor, an on-diagonal pileup: its
 * window crosses the diagonal and is read through the symmetry.  The outputs are
 *     pile[r][c] = sum over the accepted t of M(a_t - f + r, b_t - f + c)     uint64[S][S], row-major
 *     n_used     = the number of accepted anchors                             uint64[1]
 * (APA, `cooltools pileup`: the average loop; with a == b the average barrier).  Duplicates count as often
 * as they are listed, the order of the anchors is free, and n == 0 or no accepted anchor gives zeros.
 * EVERY output word is written exactly once, with a plain store: the caller does not pre-zero.  The sums
 * are exact 64-bit integers, whatever the order of summation: n < 2^31 words below 2^32 cannot overflow.
 * The anchors are spread over at most MODLE_PIXELS_PILEUP_GROUPS workgroups, whose partial sums meet in
 * scratch of the context (grown on demand).
 *
 * MODLE_PIXELS_ERR_ARG, with nothing written: a null handle or band, null anchors with n > 0, f > 32,
 * 2 f + 1 > nrows, nrows == 0, nrows > ncols, n >= 2^31, an output that is not 8-byte aligned or overlaps
 * the band, the anchors or the other output. */
#define MODLE_PIXELS_MAX_PILEUP_FLANK 32
#define MODLE_PIXELS_PILEUP_GROUPS 256

/* accept[t] = 1 when anchor t is accepted, else 0: the rule above on HOST arrays.  Host only: no device
 * is needed.  The shapes and flanks modle_pixels_pileup refuses, and a null pointer with n > 0, are
 * MODLE_PIXELS_ERR_ARG. */
int modle_pixels_pileup_accepts(uint64_t nrows, uint64_t ncols, uint64_t flank, int64_t bin_offset,
                                const int64_t* bin1, const int64_t* bin2, uint64_t n, uint8_t* accept);

/* Enqueues the sums of the DEVICE anchors d_bin1, d_bin2 (int64[n]) into the device arrays d_pile
 * (uint64[S * S]) and d_n_used (uint64[1]; may be NULL) on `stream`; the call does not wait. */
int modle_pixels_pileup(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows, uint64_t ncols,
                        uint64_t flank, int64_t bin_offset, const int64_t* d_bin1, const int64_t* d_bin2,
                        uint64_t n, uint64_t* d_pile, uint64_t* d_n_used, void* stream, char* err,
                        size_t errlen);

/* The same for HOST anchors, which are copied up, into pinned host buffers of the context (grown on
 * demand, freed by modle_pixels_destroy): *pile (S * S entries) and *n_used (one) stay valid until the
 * next call on the context.  Waits for `stream`. */
int modle_pixels_pileup_to_host(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                                uint64_t ncols, uint64_t flank, int64_t bin_offset, const int64_t* bin1,
                                const int64_t* bin2, uint64_t n, const uint64_t** pile,
                                const uint64_t** n_used, void* stream, char* err, size_t errlen);

/* One call at `factor` times the bin size: coarsens into the scratch band of the context (like
 * modle_pixels_coarse_dots_to_host), then modle_pixels_pileup_to_host on it.  `flank` and the anchors
 * count coarse bins, and the acceptance rule holds against nrows' / ncols' (modle_pixels_coarse_shape). */
int modle_pixels_coarse_pileup_to_host(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                                       uint64_t ncols, uint64_t factor, uint64_t first_bin, uint64_t flank,
                                       int64_t bin_offset, const int64_t* bin1, const int64_t* bin2,
                                       uint64_t n, const uint64_t** pile, const uint64_t** n_used,
                                       void* stream, char* err, size_t errlen);

/* ---- Rescaled pileups: windows of different sizes on the diagonal, rescaled to one grid and summed ---
 *
 * The average domain (coolpup.py's --rescale; Flyamer et al. 2017).  M is the symmetric matrix of the band
 * as above.  For a grid side R = `size`, 1 <= R <= MODLE_PIXELS_MAX_RESCALE, and `n` windows
 * [s_t, e_t) = [start[t] - bin_offset, end[t] - bin_offset) from int64 arrays, window t of width W = e - s
 * is ACCEPTED when
 *     0 <= s < e <= ncols,   R <= W,   W <= nrows:
 * every cell of the W x W square on the diagonal lies in the matrix and in the band, so no word that is no
 * pixel (left-edge triangle, trailing word) is ever read, and no output cell is empty of source pixels.  The
 * rule is evaluated without signed overflow for any int64 value and a `bin_offset` of either sign.  With
 * u(x) = floor(x * R / W) for 0 <= x < W the outputs are
 *     pile[u][v] = sum over the accepted t, over 0 <= x, y < W with u(x) == u, u(y) == v,
 *                  of M(s_t + x, s_t + y)                                       uint64[R][R], row-major
 *     area[u][v] = sum over the accepted t of #{x : u(x) == u} * #{y : u(y) == v}      uint64[R][R]
 *     n_used     = the number of accepted windows                               uint64[1]
 * A diagonal pixel counts once and an off-diagonal one in both places, as in the on-diagonal pileup above.
 * pile / area is the POOLED mean of a cell: every source pixel weighs the same, so large windows weigh more.
 * It is not coolpup.py's mean of per-snippet interpolations.  Duplicates count as often as they are listed,
 * the order of the windows is free, and n == 0 or no accepted window gives zeros.  EVERY output word is
 * written exactly once, with a plain store: the caller does not pre-zero.  The sums are exact 64-bit
 * integers whatever the order of summation and the launch geometry: the windows are spread over at most
 * modle_pixels_rescale_groups() workgroups, whose partial sums meet in scratch of the context (grown on
 * demand).
 *
 * MODLE_PIXELS_ERR_ARG, with nothing written, judged from the arguments alone: a null handle or band, null
 * windows with n > 0, size == 0, size > 128, nrows == 0, nrows > ncols, n >= 2^31,
 * n * ceil(min(nrows, ncols) / size)^2 >= 2^32 (a cell of a window has at most that many source pixels, each a
 * word below 2^32: with this bound no sum can wrap), an output that is not 8-byte aligned or overlaps the
 * band, the windows or another output. */
#define MODLE_PIXELS_MAX_RESCALE 128

/* The workgroups at most that this build of the library was compiled with (256; a test build lowers it).
 * No result depends on it.  Host only: no device is needed. */
uint64_t modle_pixels_rescale_groups(void);

/* accept[t] = 1 when window t is accepted, else 0: the rule above on HOST arrays.  Host only: no device is
 * needed.  The shapes, sizes and counts modle_pixels_rescale refuses, and a null pointer with n > 0, are
 * MODLE_PIXELS_ERR_ARG. */
int modle_pixels_rescale_accepts(uint64_t nrows, uint64_t ncols, uint64_t size, int64_t bin_offset,
                                 const int64_t* start, const int64_t* end, uint64_t n, uint8_t* accept);

/* Enqueues the sums of the DEVICE windows d_start, d_end (int64[n]) into the device arrays d_pile
 * (uint64[R * R]), d_area (uint64[R * R]; may be NULL) and d_n_used (uint64[1]; may be NULL) on `stream`;
 * the call does not wait. */
int modle_pixels_rescale(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows, uint64_t ncols,
                         uint64_t size, int64_t bin_offset, const int64_t* d_start, const int64_t* d_end,
                         uint64_t n, uint64_t* d_pile, uint64_t* d_area, uint64_t* d_n_used, void* stream,
                         char* err, size_t errlen);

/* The same for HOST windows, which are copied up, into pinned host buffers of the context (grown on demand,
 * freed by modle_pixels_destroy): *pile and *area (R * R entries each) and *n_used (one) stay valid until
 * the next call on the context.  Waits for `stream`. */
int modle_pixels_rescale_to_host(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                                 uint64_t ncols, uint64_t size, int64_t bin_offset, const int64_t* start,
                                 const int64_t* end, uint64_t n, const uint64_t** pile, const uint64_t** area,
                                 const uint64_t** n_used, void* stream, char* err, size_t errlen);

/* One call at `factor` times the bin size: coarsens into the scratch band of the context (like
 * modle_pixels_coarse_pileup_to_host), then modle_pixels_rescale_to_host on it.  The windows count coarse
 * bins, and `size` and the acceptance rule hold against nrows' / ncols' (modle_pixels_coarse_shape). */
int modle_pixels_coarse_rescale_to_host(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                                        uint64_t ncols, uint64_t factor, uint64_t first_bin, uint64_t size,
                                        int64_t bin_offset, const int64_t* start, const int64_t* end,
                                        uint64_t n, const uint64_t** pile, const uint64_t** area,
                                        const uint64_t** n_used, void* stream, char* err, size_t errlen);

/* ---- Random sampling: binomial thinning of the band -----------------------------------------------
 *
 * Every contact of the band is kept with one probability, independently of the others (the default mode
 * of `cooltools random-sample`): the same matrix at a lower depth, or two disjoint pseudo-replicates.
 * Which contacts are kept is defined by a counter-based generator keyed by the pixel's coordinates.  A
 * pixel is (i, j) with the count n = band[j * nrows + (j - i)]; its absolute ids are I = i + bin_offset
 * and J = j + bin_offset, both in [0, 2^32).  For trial t in [0, n):
 *     word(t) = philox4x32_10(counter = (I, J, t >> 2, salt), key = (seed & 0xFFFFFFFF, seed >> 32))[t & 3]
 *     kept    = #{ t < n : word(t) < threshold },   rest = n - kept
 * (Philox4x32-10 of Salmon et al., SC'11: Random123's and rocRAND's function.)  `threshold` is a uint64
 * in [0, 2^32]: the probability is threshold / 2^32, 2^32 keeps every contact and 0 keeps none; `seed` is
 * a uint64 and `salt` a uint32 (another salt: another, independent draw of the same seed).  No float
 * crosses this interface.  What follows from the definition:
 *   - kept depends on nothing but (I, J, n, threshold, seed, salt): not on nrows, not on how the genome
 *     was cut into intervals (give `bin_offset` the interval's first bin in the file), not on the stream
 *     or the launch;
 *   - kept at threshold a <= kept at threshold b for a <= b, pixel by pixel: a series of depths is nested;
 *   - kept + rest == n word for word: the two outputs are disjoint pseudo-replicates;
 *   - every trial is an independent Bernoulli draw, so kept is Binomial(n, threshold / 2^32) and the total
 *     is random around its target, not equal to it.  There is no exact-total mode.
 * The work is one Philox call per four contacts: the cost of a call is proportional to the sum of the
 * band, and a band of more than MODLE_PIXELS_MAX_SAMPLE_TRIALS contacts is refused: about two seconds of
 * one MI355X at the 520 G trials/s measured on a band with a distance decay
 * (profiles/sample/sample_vs_torch.txt) -- a mistaken call must not hold a shared GPU for minutes.  A lane
 * of the kernel draws the first MODLE_PIXELS_SAMPLE_TIER1_TRIALS trials of its own pixel; what a pixel has
 * beyond them is drawn by its whole wave, and by that wave alone (1.45 G trials/s: a pixel of 2^32 - 1
 * contacts takes three seconds whatever the sum).
 *
 * The outputs d_kept and d_rest are uint32[nrows * ncols + 1] in the band's layout; either may be NULL,
 * not both.  EVERY word of an output that is given is written exactly once, with a plain store: pixels
 * hold their counts, the words that are no pixels (left-edge triangle, trailing word) hold 0; the caller
 * does not pre-zero.  The words of the band that are no pixels are never read.
 *
 * There is no coarse form: a sampled band is a band in device memory, which modle_pixels_coarsen and every
 * other call of this header take as it is.  Sample at the base bin size and coarsen the result -- then the
 * levels of a sampled .mcool agree with each other, which sampling every level on its own would not give.
 *
 * MODLE_PIXELS_ERR_ARG, with nothing written: a null handle, band or stats, both outputs null, threshold >
 * 2^32, nrows == 0, nrows > ncols, an output that overlaps the band or the other output.
 * MODLE_PIXELS_ERR_RANGE, with nothing written: bin_offset < 0 or bin_offset + ncols > 2^32; a sum above
 * MODLE_PIXELS_MAX_SAMPLE_TRIALS. */
#define MODLE_PIXELS_SAMPLE_TIER1_TRIALS 64
#define MODLE_PIXELS_MAX_SAMPLE_TRIALS (1ull << 40)
#define MODLE_PIXELS_SAMPLE_KEPT 0
#define MODLE_PIXELS_SAMPLE_REST 1

/* kept[t] of the `n` pixels (bin1[t] + bin_offset, bin2[t] + bin_offset) with count[t] trials: the
 * definition above on HOST arrays, compiled from the same Philox function as the kernel.  Host only: no
 * device is needed.  threshold > 2^32 and a null pointer with n > 0 are MODLE_PIXELS_ERR_ARG, an id outside
 * [0, 2^32) is MODLE_PIXELS_ERR_RANGE; nothing is written then. */
int modle_pixels_sample_pixels(uint64_t seed, uint32_t salt, uint64_t threshold, int64_t bin_offset,
                               const int64_t* bin1, const int64_t* bin2, const uint32_t* count, uint64_t n,
                               uint32_t* kept);

/* Enqueues the sampling of the band into the device arrays d_kept and / or d_rest on `stream`; the call
 * does not wait.  `stats` is the HOST modle_pixels_stats of the same band from modle_pixels_count: its sum
 * is held against MODLE_PIXELS_MAX_SAMPLE_TRIALS and decides nothing else -- a caller who passes a smaller
 * sum than the band has gets the correct result later, not a wrong one. */
int modle_pixels_sample(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows, uint64_t ncols,
                        int64_t bin_offset, uint64_t threshold, uint64_t seed, uint32_t salt,
                        const modle_pixels_stats* stats, uint32_t* d_kept, uint32_t* d_rest, void* stream,
                        char* err, size_t errlen);

/* One call: modle_pixels_count on the band (whose sum is held against the cap), the sampling into a
 * scratch band of the context (grown on demand, freed by modle_pixels_destroy; one for the kept and one
 * for the rest band), then modle_pixels_to_host on the kept (`which` == MODLE_PIXELS_SAMPLE_KEPT) or the
 * rest (MODLE_PIXELS_SAMPLE_REST) band: its sorted non-zero pixels with `bin_offset` added to the ids and
 * its statistics in *stats_out (pinned buffers of the context, valid until the next call on it).  Any
 * other `which` is MODLE_PIXELS_ERR_ARG.  Waits for `stream`. */
int modle_pixels_sample_to_host(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows, uint64_t ncols,
                                int64_t bin_offset, uint64_t threshold, uint64_t seed, uint32_t salt, int which,
                                const int64_t** bin1, const int64_t** bin2, const int32_t** count,
                                const int64_t** bin1_offset, modle_pixels_stats* stats_out, void* stream,
                                char* err, size_t errlen);

/* ---- Pixels to band: the inverse of modle_pixels_extract --------------------------------------------
 *
 * A pixel list is three DEVICE arrays d_bin1, d_bin2 (int64[n], 8-byte aligned) and d_count (int32[n]),
 * n < 2^31: what modle_pixels_extract writes and what a cooler holds.  With i = bin1 - bin_offset and
 * j = bin2 - bin_offset a pixel is
 *     IN       0 <= i <= j < ncols and j - i <  nrows: a word of the band;
 *     BEYOND   0 <= i <= j < ncols and j - i >= nrows: a contact the band is too narrow for;
 *     OUTSIDE  everything else: the bins of another chromosome (the trans pixels that end every row of a
 *              cooler), i > j, a negative id.
 * The rule is evaluated without signed overflow for any int64 value and a `bin_offset` of either sign, as
 * modle_pixels_pileup's is.  Only IN pixels reach the band; the others are counted.
 *
 * The WHOLE list, whatever the classes, must be strictly increasing in (bin1, bin2) -- cooler's own
 * invariant, which rules duplicates out --, else MODLE_PIXELS_ERR_ORDER; a negative count is
 * MODLE_PIXELS_ERR_RANGE.  stats->first_bad is then the smallest index t whose pixel is not after pixel
 * t - 1, or whose count is negative, and the code is that of the smaller index (ORDER where both name one).
 * A count of 0 is legal and is stored as 0.
 *
 * Laws: for any band B, band_fill(extract(B)) equals B at every pixel word and is 0 at every word that is
 * no pixel; modle_pixels_count of the result reports nnz == nnz_in, sum == sum_in and max_count ==
 * max_count; the result does not depend on the launch.  No floating point is used, and the fill uses no
 * atomics: a workgroup owns a tile of MODLE_PIXELS_BAND_TILE_COLS columns times
 * MODLE_PIXELS_BAND_TILE_DIAGS diagonals of the band, gathers the tile's pixels in LDS and stores it whole.
 *
 * MODLE_PIXELS_ERR_ARG, with nothing written: a null handle, stats or output, null pixel arrays with n > 0,
 * n >= 2^31, the shapes modle_pixels_count refuses, out_words < nrows * ncols + 1, an int64 array that is
 * not 8-byte aligned, an output that overlaps an input.  d_out needs 4-byte alignment only.  n == 0 is legal
 * and gives a band of zeros. */
#define MODLE_PIXELS_ERR_ORDER (-4) /* a pixel list that is not strictly increasing in (bin1, bin2) */
#define MODLE_PIXELS_BAND_IN 0
#define MODLE_PIXELS_BAND_BEYOND 1
#define MODLE_PIXELS_BAND_OUTSIDE 2
#define MODLE_PIXELS_BAND_TILE_COLS 64
#define MODLE_PIXELS_BAND_TILE_DIAGS 128

typedef struct modle_pixels_band_stats {
  uint64_t n_in, sum_in;           /* IN pixels and the sum of their counts */
  uint64_t nnz_in;                 /* IN pixels with a count above 0: modle_pixels_count's nnz of the result */
  uint64_t n_beyond, sum_beyond;   /* exact integer sums: n < 2^31 counts below 2^31 cannot overflow */
  uint64_t n_outside, sum_outside;
  int64_t first_bad;               /* -1 when the list is in order and no count is negative */
  uint32_t max_count;              /* largest count of an IN pixel */
  uint32_t reserved_;
} modle_pixels_band_stats;

/* cls[t] = MODLE_PIXELS_BAND_IN / _BEYOND / _OUTSIDE of pixel t: the rule above on HOST arrays.  Host only:
 * no device is needed.  The shapes modle_pixels_count refuses, n >= 2^31 and a null pointer with n > 0 are
 * MODLE_PIXELS_ERR_ARG. */
int modle_pixels_band_classify(uint64_t nrows, uint64_t ncols, int64_t bin_offset, const int64_t* bin1,
                               const int64_t* bin2, uint64_t n, uint8_t* cls);

/* Step 1: one pass over the list -- class, order, sign and the reductions -- into *stats, which is filled
 * on MODLE_PIXELS_ERR_ORDER and _RANGE as well (a negative count enters no sum).  Fills the device array
 * d_row_start (int64[ncols + 1]; may be NULL when only the statistics are wanted): row_start[i] is the
 * index of the first pixel with bin1 >= i + bin_offset, 0 <= i <= ncols.  Waits for `stream`. */
int modle_pixels_band_check(modle_pixels_handle* h, const int64_t* d_bin1, const int64_t* d_bin2,
                            const int32_t* d_count, uint64_t n, uint64_t nrows, uint64_t ncols,
                            int64_t bin_offset, int64_t* d_row_start, modle_pixels_band_stats* stats,
                            void* stream, char* err, size_t errlen);

/* Step 2: enqueues the fill of d_out (uint32[nrows * ncols + 1], the band's layout, `out_words` words) on
 * `stream`; the call does not wait.  EVERY word is defined by the call, the caller does not pre-zero: an IN
 * pixel holds its count, every other pixel word, the left-edge triangle and the trailing word hold 0.  The
 * result is the band of the list only when step 1 returned MODLE_PIXELS_OK on the same unchanged arrays.
 * WHATEVER the arrays hold -- a stale d_row_start, a list changed in between --, nothing is stored outside
 * d_out[0, nrows * ncols + 1) and nothing is read outside the n entries and the ncols + 1 row starts: the
 * kernel clamps what it reads of d_row_start to [0, n] and derives (i, j) of every entry anew before it
 * stores.  (bin1 is not needed: the row of an entry is the one whose range of d_row_start holds it.) */
int modle_pixels_band_fill(modle_pixels_handle* h, const int64_t* d_bin2, const int32_t* d_count, uint64_t n,
                           uint64_t nrows, uint64_t ncols, int64_t bin_offset, const int64_t* d_row_start,
                           uint32_t* d_out, uint64_t out_words, void* stream, char* err, size_t errlen);

/* One call for HOST pixel arrays: copies them into scratch of the context (grown on demand, freed by
 * modle_pixels_destroy), then check and fill into the caller's device array d_out.  Fills *stats and waits
 * for `stream`.  On MODLE_PIXELS_ERR_ORDER and _RANGE nothing is written to d_out. */
int modle_pixels_band_from_host(modle_pixels_handle* h, const int64_t* bin1, const int64_t* bin2,
                                const int32_t* count, uint64_t n, uint64_t nrows, uint64_t ncols,
                                int64_t bin_offset, uint32_t* d_out, uint64_t out_words,
                                modle_pixels_band_stats* stats, void* stream, char* err, size_t errlen);

/* ---- Stripes: two bands compared stripe by stripe -----------------------------------------------------
 *
 * Two bands A (the reference, d_ref) and B (the target, d_tgt) of one shape, each in the layout above; they
 * may be the same pointer.  With M(i, j) = band[j * nrows + (j - i)] the stripes of bin c, 0 <= c < ncols,
 * have nrows entries each (evaluate.stripes; the method of `modle_tools evaluate`):
 *     vertical    v[i] = M(c - i, c) for i <= c,          0 for the i above c
 *     horizontal  h[i] = M(c, c + i) for c + i < ncols,   0 beyond
 * and the zero padding counts as entries.  Per direction and bin the call writes the integer sums that
 * Pearson's and Spearman's correlation, the RMSE and the Euclidean distance of the two stripes are made of;
 * the scores themselves are one host statement (modle_amd/pixels.py: stripe_scores).  `what` is a mask that
 * selects three blocks of rows, each row ncols uint64 words, one per bin:
 *     MODLE_PIXELS_STRIPES_MOMENTS  9 rows  n, Sa, Sb, Saa_lo, Saa_hi, Sbb_lo, Sbb_hi, Sab_lo, Sab_hi
 *         n == nrows, Sa = sum a, Saa = sum a * a, Sab = sum a * b over the nrows entries; the second
 *         moments are 128-bit sums in two words, so every shape and every uint32 count is exact: there is
 *         no range refusal.
 *     MODLE_PIXELS_STRIPES_MASKED   9 rows  the same sums over the entries with a != 0 and b != 0 (the
 *         weight-0/1 form of --exclude-zero-pixels); n is their number.
 *     MODLE_PIXELS_STRIPES_RANKS    3 rows  Raa, Rbb, Rab: the sums of R2(a) * R2(a), R2(b) * R2(b) and
 *         R2(a) * R2(b) over the nrows entries, R2(x) = 2 * #{y < x} + #{y == x} + 1 counted within x's own
 *         stripe, padding included: twice the average rank (ties share the mean of their positions).  The
 *         sum of R2 over a stripe is nrows * (nrows + 1) whatever it holds and is not stored.  Accepted for
 *         nrows <= MODLE_PIXELS_MAX_STRIPE.
 * The output is uint64[2][rows][ncols]: direction 0 vertical, 1 horizontal; the blocks in bit order; rows =
 * modle_pixels_stripes_rows(what).  EVERY output word is written exactly once, with a plain store: the caller
 * does not pre-zero.  The words of either band that are no pixels are never read, and every address is a
 * function of nrows and ncols alone.  Nothing here uses floating point.
 *
 * There is no coarse form: coarsen either band with modle_pixels_coarsen and pass the result.
 *
 * MODLE_PIXELS_ERR_ARG, with nothing written: a null pointer, nrows == 0, nrows > ncols, what == 0 or with
 * a bit that is not defined, RANKS with nrows > MODLE_PIXELS_MAX_STRIPE, out_words != 2 * rows * ncols, a
 * d_out that is not 8-byte aligned or overlaps either band. */
#define MODLE_PIXELS_STRIPES_MOMENTS 1
#define MODLE_PIXELS_STRIPES_MASKED 2
#define MODLE_PIXELS_STRIPES_RANKS 4
#define MODLE_PIXELS_MAX_STRIPE 4096

/* The rows per direction of the mask `what`: 9, 9 and 3 for the three blocks.  Host only: no device is
 * needed.  what == 0 and a bit that is not defined are MODLE_PIXELS_ERR_ARG. */
int modle_pixels_stripes_rows(uint64_t what);

/* Enqueues the sums into the device array d_out (uint64[2][rows][ncols], `out_words` == 2 * rows * ncols
 * words) on `stream`; the call does not wait. */
int modle_pixels_stripes(modle_pixels_handle* h, const uint32_t* d_ref, const uint32_t* d_tgt, uint64_t nrows,
                         uint64_t ncols, uint64_t what, uint64_t* d_out, uint64_t out_words, void* stream,
                         char* err, size_t errlen);

/* The same into a pinned host buffer of the context (grown on demand, freed by modle_pixels_destroy): *rows
 * (uint64[2][rows][ncols]) stays valid until the next call on the context.  Waits for `stream`. */
int modle_pixels_stripes_to_host(modle_pixels_handle* h, const uint32_t* d_ref, const uint32_t* d_tgt,
                                 uint64_t nrows, uint64_t ncols, uint64_t what, const uint64_t** rows,
                                 void* stream, char* err, size_t errlen);

/* ---- SCC: two bands compared diagonal by diagonal -----------------------------------------------------
 *
 * The sums the stratum-adjusted correlation coefficient of HiCRep (Yang et al., Genome Research 2017) is made
 * of.  Two bands A (the reference, d_ref) and B (the target, d_tgt) of one shape, each in the layout above;
 * they may be the same pointer.  M(x, y) is the symmetric matrix of a band: M(x, y) = band[max(x, y) * nrows +
 * |x - y|] for 0 <= x, y < ncols, and 0 outside the matrix.  For the smoothing half-width `smooth` = h, 0 <= h
 * <= MODLE_PIXELS_MAX_SCC_SMOOTH, the smoothed value of a pixel is the box SUM
 *     X(i, j) = sum over |di| <= h, |dj| <= h of M(i + di, j + dj):
 * the box crosses the main diagonal through the symmetry and the cells outside the chromosome count 0 (HiCRep's
 * zero-padded mean filter; Pearson's correlation does not see the division by (2h + 1)^2 a mean would add, so
 * nothing on the device is a float).  The strata are the diagonals d, min_diag <= d <= max_diag; the call
 * requires max_diag + 2 h <= nrows - 1, so no box of a stratum reaches a diagonal the band does not hold and the
 * result is that of the full matrix.  Stratum d has the ncols - d entries a_i = X_A(i, i + d) and b_i =
 * X_B(i, i + d), 0 <= i < ncols - d, and per stratum the call writes MODLE_PIXELS_SCC_ROWS words:
 *     n, Sa_lo, Sa_hi, Sb_lo, Sb_hi, Saa_lo, Saa_hi, Sbb_lo, Sbb_hi, Sab_lo, Sab_hi
 *   n = #{ i : a_i != 0 or b_i != 0 }; an entry that is zero in both adds nothing to any other sum, so the
 *       caller has both of HiCRep's sample conventions from one output: n, or ncols - d;
 *   Sa = sum a, Saa = sum a * a, Sab = sum a * b: 128-bit sums in two words each.  a < 1681 * 2^32 < 2^43, so Sa
 *       can pass 2^64 and Saa stays below 2^118: every shape and every uint32 count is exact and there is no
 *       range refusal.
 * The scores are one host statement (modle_amd/pixels.py: scc_scores).  The output is uint64[11][nrows],
 * row-major, column d; the columns outside [min_diag, max_diag] hold 0.  EVERY output word is written exactly
 * once, with a plain store: the caller does not pre-zero.  The words of either band that are no pixels are never
 * read, every address is a function of nrows, ncols, h and the strata alone, and no result depends on the launch
 * geometry: a strip of 64 strata is walked by at most modle_pixels_scc_groups() workgroups, whose partial sums
 * meet in scratch of the context (grown on demand).
 *
 * There is no coarse form: coarsen either band with modle_pixels_coarsen and pass the result.
 *
 * MODLE_PIXELS_ERR_ARG, with nothing written: a null pointer, nrows == 0, nrows > ncols, smooth > 20, min_diag >
 * max_diag, max_diag + 2 * smooth > nrows - 1, out_words != 11 * nrows, a d_out that is not 8-byte aligned or
 * overlaps either band. */
#define MODLE_PIXELS_SCC_ROWS 11
#define MODLE_PIXELS_MAX_SCC_SMOOTH 20

/* The workgroups per strip of 64 strata at most that this build of the library was compiled with (128; a test
 * build lowers it).  No result depends on it.  Host only: no device is needed. */
uint64_t modle_pixels_scc_groups(void);

/* Enqueues the sums into the device array d_out (uint64[11][nrows], `out_words` == 11 * nrows words) on
 * `stream`; the call does not wait. */
int modle_pixels_scc(modle_pixels_handle* h, const uint32_t* d_ref, const uint32_t* d_tgt, uint64_t nrows,
                     uint64_t ncols, uint64_t smooth, uint64_t min_diag, uint64_t max_diag, uint64_t* d_out,
                     uint64_t out_words, void* stream, char* err, size_t errlen);

/* The same into a pinned host buffer of the context (grown on demand, freed by modle_pixels_destroy): *rows
 * (uint64[11][nrows]) stays valid until the next call on the context.  Waits for `stream`. */
int modle_pixels_scc_to_host(modle_pixels_handle* h, const uint32_t* d_ref, const uint32_t* d_tgt, uint64_t nrows,
                             uint64_t ncols, uint64_t smooth, uint64_t min_diag, uint64_t max_diag,
                             const uint64_t** rows, void* stream, char* err, size_t errlen);

/* ---- stripe profiles: the cross-sections of every bin's stripes ----------------------------------------
 *
 * Where one band has a stripe, how long it is and how sharply it stands out of its neighbourhood (the comparison
 * above takes two bands and says none of that).  M(x, y) is the symmetric matrix of the band, 0 outside the
 * chromosome.  For the largest offset `max_offset` = m <= MODLE_PIXELS_MAX_PROFILE_OFFSET, the lengths L_1 < ... <
 * L_K in bins (1 <= K <= MODLE_PIXELS_MAX_PROFILE_LENGTHS, a HOST array) and `min_diag` = d0, for every bin c <
 * ncols, offset o in [-m, m] and k:
 *     V[k][o][c] = sum over d0 <= d < L_k of M(c - d, c + o)   the stripe upstream of c, seen o columns to the side
 *     H[k][o][c] = sum over d0 <= d < L_k of M(c + o, c + d)   the stripe downstream of c, seen o rows to the side
 * The output is uint64[2][K][2 m + 1][ncols]: direction 0 is V, 1 is H, offset index o + m; the words whose column
 * or row c + o lies outside [0, ncols) hold 0.  A sum has fewer than nrows terms below 2^32: 64 bits cannot
 * overflow and there is no range refusal.  The cross-section over o is what makes a stripe a stripe, a peak at o =
 * 0 over flat shoulders; the decision is one host statement (modle_amd/pixels.py: stripe_calls).
 *
 * The accepted call:
 *     nrows >= 1,  nrows <= ncols,  m <= 8,  1 <= K <= 4,  d0 >= m,  d0 < L_1 < ... < L_K,  L_K + m <= nrows
 * d0 >= m keeps every cell on its own side of the main diagonal (V reads band[(c + o) * nrows + (d + o)], H reads
 * band[(c + d) * nrows + (d - o)]: nothing goes through the symmetry), and L_K + m <= nrows keeps every cell inside
 * the band, so the result is that of the full matrix.  EVERY output word is written exactly once, with a plain
 * store: the caller does not pre-zero.  Every band word is read at most once per direction; the words that are no
 * pixels are never read, and every address is a function of the arguments alone.  Nothing here uses floating point.
 *
 * MODLE_PIXELS_ERR_ARG, with nothing written: everything outside the accepted call, a null pointer, out_words !=
 * 2 * K * (2 m + 1) * ncols, a d_out that is not 8-byte aligned or overlaps the band. */
#define MODLE_PIXELS_MAX_PROFILE_OFFSET 8
#define MODLE_PIXELS_MAX_PROFILE_LENGTHS 4

/* Enqueues the sums into the device array d_out (uint64[2][K][2 m + 1][ncols]) on `stream`; the call does not
 * wait (`lengths` is read before it returns). */
int modle_pixels_stripe_profiles(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows, uint64_t ncols,
                                 uint64_t max_offset, const uint64_t* lengths, uint64_t n_lengths,
                                 uint64_t min_diag, uint64_t* d_out, uint64_t out_words, void* stream, char* err,
                                 size_t errlen);

/* The same into a pinned host buffer of the context (grown on demand, freed by modle_pixels_destroy): *profiles
 * (uint64[2][K][2 m + 1][ncols]) stays valid until the next call on the context.  Waits for `stream`. */
int modle_pixels_stripe_profiles_to_host(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                                         uint64_t ncols, uint64_t max_offset, const uint64_t* lengths,
                                         uint64_t n_lengths, uint64_t min_diag, const uint64_t** profiles,
                                         void* stream, char* err, size_t errlen);

/* The band coarsened by `factor` into scratch of the context (as modle_pixels_coarse_marginals_to_host), then
 * modle_pixels_stripe_profiles_to_host on it.  *profiles is uint64[2][K][2 m + 1][ncols'];  the lengths, the offset
 * and min_diag count coarse bins, and the accepted call holds against nrows'. */
int modle_pixels_coarse_stripe_profiles_to_host(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                                                uint64_t ncols, uint64_t factor, uint64_t first_bin,
                                                uint64_t max_offset, const uint64_t* lengths, uint64_t n_lengths,
                                                uint64_t min_diag, const uint64_t** profiles, void* stream,
                                                char* err, size_t errlen);

/* ---- triangle sums: the contacts inside every window on the diagonal --------------------------------------
 *
 * What every dynamic-programming domain caller scores (Armatus, Filippova et al. 2014; the modularity form of
 * MrTADFinder, Yan et al. 2017).  M(a, c) is the matrix of the band, band[c * nrows + (c - a)].  For `max_width` =
 * W, `min_diag` = d0, every start s < ncols and every k < W:
 *     T[k][s] = sum of M(a, c) over  s <= a <= c < min(s + k + 1, ncols),  c - a >= d0
 * the upper triangle of the window of k + 1 bins that starts at bin s, diagonal included, clipped at the
 * chromosome's end.  The output is uint64[W][ncols].  1 <= W <= nrows keeps every cell inside the band, so the
 * result is that of the full matrix; d0 >= W gives zeros.  A sum has at most W (W + 1) / 2 terms below 2^32, which
 * stays below 2^64 for W <= MODLE_PIXELS_MAX_TRIANGLE_WIDTH: wider tables are refused from the arguments alone.
 * With one table any score f(sum, width) costs O(1) per window, and a diamond of the insulation is a difference
 * of three triangles.  The decision is one host statement (modle_amd/pixels.py: domain_calls).
 *
 * EVERY output word is written, and its final value stored last, with plain stores: the caller does not pre-zero.
 * The table is formed in the output itself (the column prefixes first, then their prefix along k in place): no
 * scratch memory of the context is used, there are no atomics and no result depends on the launch.  The words of
 * the band that are no pixels (d > c, and the one word beyond the band) are never read.  Nothing here uses floating
 * point.
 *
 * MODLE_PIXELS_ERR_ARG, with nothing written: a null pointer, nrows == 0, nrows > ncols, max_width == 0, max_width
 * > nrows, max_width > MODLE_PIXELS_MAX_TRIANGLE_WIDTH, out_words < max_width * ncols, a d_out that is not 8-byte
 * aligned or overlaps the band. */
#define MODLE_PIXELS_MAX_TRIANGLE_WIDTH 65535

/* Enqueues the table into the device array d_out (uint64[W][ncols]) on `stream`; the call does not wait. */
int modle_pixels_triangles(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows, uint64_t ncols,
                           uint64_t max_width, uint64_t min_diag, uint64_t* d_out, uint64_t out_words, void* stream,
                           char* err, size_t errlen);

/* The same into a pinned host buffer of the context (grown on demand, freed by modle_pixels_destroy): *table
 * (uint64[W][ncols]) stays valid until the next call on the context.  Waits for `stream`. */
int modle_pixels_triangles_to_host(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows, uint64_t ncols,
                                   uint64_t max_width, uint64_t min_diag, const uint64_t** table, void* stream,
                                   char* err, size_t errlen);

/* The band coarsened by `factor` into scratch of the context (as modle_pixels_coarse_insulation_to_host), then
 * modle_pixels_triangles_to_host on it.  *table is uint64[W][ncols']; the widths and min_diag count coarse bins,
 * and the rule holds against nrows'. */
int modle_pixels_coarse_triangles_to_host(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows,
                                          uint64_t ncols, uint64_t factor, uint64_t first_bin, uint64_t max_width,
                                          uint64_t min_diag, const uint64_t** table, void* stream, char* err,
                                          size_t errlen);

/* Host only, no device is needed: the number of pixels behind every word of the table, cells[k * ncols + s] =
 * (w' - d0)(w' - d0 + 1) / 2 with w' = min(k + 1, ncols - s), or 0 when w' <= d0.  MODLE_PIXELS_ERR_ARG for a null
 * pointer, max_width == 0 or a width above the cap. */
int modle_pixels_triangle_cells(uint64_t ncols, uint64_t max_width, uint64_t min_diag, uint64_t* cells);

/* The launch caps this build of the library was compiled with, for the tests that lower them: caps[0] the
 * workgroups of a stripes launch at most (2^20), caps[1] the grid's y of the band fill at most (65535),
 * caps[2] the workgroups of the band check at most (1024), caps[3] the threads of the bin1_offset scan
 * (1024).  No result depends on any of them.  Host only: no device is needed. */
void modle_pixels_build_caps(uint64_t caps[4]);

#ifdef __cplusplus
}
#endif
#endif
