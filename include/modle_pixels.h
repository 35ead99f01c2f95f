/* modle_pixels.h -- C ABI of the sparse-pixel extraction (modle_amd/libmodle_pixels.so).
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

#ifdef __cplusplus
}
#endif
#endif
