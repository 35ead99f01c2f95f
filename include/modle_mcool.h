/* modle_mcool.h -- multi-resolution cooler (.mcool) writer of modle_amd/libmodle_cooler.so.
 *
 * One HDF5 file that holds a complete cooler (modle_cooler.h: chroms, bins, pixels, indexes and
 * attributes) per bin size, under /resolutions/<bin size>, which is what HiGlass and
 * `cooler` / `hictk` open as `file.mcool::/resolutions/<bin size>`.  The root carries the
 * attributes hictk's multi-resolution writer sets: format = "HDF5::MCOOL" (string),
 * format-version = 2 (int64) and bin-type = "fixed" (string).
 *
 * Every resolution is written like a file of its own, through the handle
 * modle_mcool_resolution returns: modle_cool_bin_offset and modle_cool_append_pixels
 * (modle_cooler_pixels.h) or modle_cool_append_matrix work on it unchanged, with that
 * resolution's bin size, in genome order per resolution.  The pixels of a coarse resolution come
 * from modle_pixels_coarse_to_host (modle_pixels.h).  No call throws; the codes are modle_cooler.h's.
 */
#ifndef MODLE_MCOOL_H
#define MODLE_MCOOL_H
#include <stddef.h>
#include <stdint.h>

#include "modle_cooler.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct modle_mcool_file modle_mcool_file;

/* Creates the file with the root attributes and one empty cooler per entry of `bin_sizes`
 * (n_res >= 1), each with all chromosomes and its own bins.  `bin_sizes` must be ascending and
 * distinct, and each a multiple of bin_sizes[0]: anything else is MODLE_COOL_ERR_ARG, and no file
 * is created.  The other arguments are modle_cool_create's. */
int modle_mcool_create(const char* path, int force_overwrite, const char* const* chrom_names,
                       const uint32_t* chrom_sizes, size_t n_chroms, const uint32_t* bin_sizes,
                       size_t n_res, const char* assembly, const char* generated_by,
                       const char* metadata_json, modle_mcool_file** out, char* err, size_t errlen);

/* The cooler of bin_sizes[index]: a BORROWED handle, valid until modle_mcool_close (never pass
 * it to modle_cool_close, which refuses it); NULL if `index` is out of range. */
modle_cool_file* modle_mcool_resolution(modle_mcool_file* f, size_t index);

/* Writes the indexes and attributes of every resolution and closes the file.  The handle and the
 * borrowed ones are freed on an error as well. */
int modle_mcool_close(modle_mcool_file* f, char* err, size_t errlen);

#ifdef __cplusplus
}
#endif
#endif
