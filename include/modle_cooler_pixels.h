/* modle_cooler_pixels.h -- the cooler writer of modle_cooler.h fed with sorted pixels instead of a
 * dense band matrix (same library, modle_amd/libmodle_cooler.so; host side only).
 *
 * The pixels are what modle_pixels.h extracts on the device: the non-zero cells of one interval
 * in cooler order with file-wide bin ids.  A file written through this entry point is identical,
 * dataset for dataset and attribute for attribute, to the one modle_cool_append_matrix writes from
 * the band the pixels came from.
 */
#ifndef MODLE_COOLER_PIXELS_H
#define MODLE_COOLER_PIXELS_H
#include "modle_cooler.h"
#ifdef __cplusplus
extern "C" {
#endif

/* First bin id, within the file, of the interval of chromosome `chrom_id` that starts at
 * `offset_bp`: the `bin_offset` to extract its pixels with. */
int modle_cool_bin_offset(const modle_cool_file* f, size_t chrom_id, uint64_t offset_bp,
                          int64_t* bin_offset, char* err, size_t errlen);

/* Appends the `n` pixels (bin1[k], bin2[k], count[k]) of one interval of `ncols` bins that starts
 * at `offset_bp` of chromosome `chrom_id`.  The ordering rules are modle_cool_append_matrix's:
 * intervals in genome order, not overlapping.  The pixels must be sorted by (bin1, bin2) without
 * duplicates, with bin_offset <= bin1 <= bin2 < bin_offset + ncols and count > 0; `bin1_offset`
 * (ncols + 1 entries, relative to this interval: pixels [bin1_offset[i], bin1_offset[i + 1]) have
 * bin1 == bin_offset + i) is checked against them, or derived from them when NULL.  n == 0 appends
 * an interval without contacts.  Everything is validated before anything is written: after
 * MODLE_COOL_ERR_ARG (order, duplicates, bin2 < bin1, count == 0, index mismatch) or
 * MODLE_COOL_ERR_RANGE (bin id outside the interval or the chromosome, negative count) the file
 * is as it was before the call. */
int modle_cool_append_pixels(modle_cool_file* f, size_t chrom_id, uint64_t offset_bp, uint64_t ncols,
                             const int64_t* bin1, const int64_t* bin2, const int32_t* count,
                             uint64_t n, const int64_t* bin1_offset, char* err, size_t errlen);

#ifdef __cplusplus
}
#endif
#endif
