/* modle_cooler_read.h -- a cooler (v3) reader that hands over pixels (modle_amd/libmodle_cooler.so,
 * modle_amd/csrc/cooler_reader.cpp).
 *
 * The counterpart of modle_cooler_pixels.h: where modle_cool_read_band (modle_cooler.h) scatters a
 * chromosome into a dense band on the host, this reader hands over the slice of pixels/{bin1_id, bin2_id,
 * count} that belongs to a chromosome as it lies in the file, so that the sparse form crosses to the device
 * and modle_pixels_band_from_host (modle_pixels.h) builds the band there.
 *
 * A file is named by a URI: `path` is the cooler at the root of the file, `path::/resolutions/10000` the
 * cooler in that group of a multi-resolution file.  Only fixed-width bins and integer counts are read.
 * Balancing weights (bins/weight) are ignored: raw counts are what every kernel of this project works on.
 *
 * No call throws; errors are the negative codes of modle_cooler.h with a message in `err`.
 */
#ifndef MODLE_COOLER_READ_H
#define MODLE_COOLER_READ_H
#include <stddef.h>
#include <stdint.h>

#include "modle_cooler.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct modle_cool_reader modle_cool_reader;

/* Opens `uri` for reading and loads its chromosomes and indexes.  MODLE_COOL_ERR_IO: a file that cannot be
 * opened or read.  MODLE_COOL_ERR_ARG: a null pointer; a group that is not in the file (the message lists
 * the resolutions the file has); a `bin-type` other than "fixed"; a pixels/count that is no integer type;
 * an indexes/chrom_offset or indexes/bin1_offset of the wrong length. */
int modle_cool_reader_open(const char* uri, modle_cool_reader** out, char* err, size_t errlen);

/* The bin size in bp and the number of chromosomes. */
int modle_cool_reader_info(const modle_cool_reader* r, uint32_t* bin_size, size_t* n_chroms);

/* Chromosome `chrom_id`: its name (owned by the reader), its size in bp, the id of its first bin within the
 * file (indexes/chrom_offset) and its number of bins.  Any output may be NULL. */
int modle_cool_reader_chrom(const modle_cool_reader* r, size_t chrom_id, const char** name, uint64_t* size,
                            int64_t* first_bin, uint64_t* n_bins);

/* The pixels whose bin1 lies in chromosome `chrom_id`: the slice [bin1_offset[b0], bin1_offset[b1]) of
 * pixels/bin1_id, bin2_id (int64) and count (int32), b0 = *first_bin and b1 the first bin of the next
 * chromosome.  The bin ids are the file's; the trans pixels that end every row are handed over as they are
 * (modle_pixels_band_classify classes them as outside).  *bin1, *bin2, *count (*n entries) point to buffers
 * owned by the reader: they stay valid until the next call on it. */
int modle_cool_reader_pixels(modle_cool_reader* r, size_t chrom_id, const int64_t** bin1, const int64_t** bin2,
                             const int32_t** count, uint64_t* n, int64_t* first_bin, char* err, size_t errlen);

/* The file's own indexes, owned by the reader: chrom_offset (n_chroms + 1 entries) and bin1_offset
 * (*n_bins + 1 entries).  Any output may be NULL. */
int modle_cool_reader_indexes(const modle_cool_reader* r, const int64_t** chrom_offset,
                              const int64_t** bin1_offset, uint64_t* n_bins);

void modle_cool_reader_close(modle_cool_reader* r);

#ifdef __cplusplus
}
#endif
#endif
