// pixels_context.h -- what the sources of libmodle_pixels.so share: the context behind
// modle_pixels_handle and the one-call extraction (private; the C ABI is include/modle_pixels.h).
#ifndef MODLE_PIXELS_CONTEXT_H
#define MODLE_PIXELS_CONTEXT_H
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "modle_pixels.h"

struct DeviceStats {
  unsigned long long nnz;
  unsigned long long sum;
  unsigned int max_count;
  unsigned int pad_;
};

struct modle_pixels_handle {
  int device = 0;
  DeviceStats* d_stats = nullptr;
  DeviceStats* h_stats = nullptr;  // pinned
  // one-call form: device arrays and their pinned host mirrors, grown on demand
  void *d_bin1 = nullptr, *d_bin2 = nullptr, *d_count = nullptr, *d_offsets = nullptr;
  void *h_bin1 = nullptr, *h_bin2 = nullptr, *h_count = nullptr, *h_offsets = nullptr;
  uint64_t cap_pixels = 0, cap_offsets = 0;
  // modle_pixels_coarse_to_host: the coarse band (modle_coarsen.hip), grown on demand
  uint32_t* d_coarse = nullptr;
  uint64_t cap_coarse = 0;  // words
  // modle_pixels_dense_to_host: the region (modle_dense.hip) and its pinned host mirror, grown on demand
  uint32_t *d_dense = nullptr, *h_dense = nullptr;
  uint64_t cap_dense = 0;  // words
};

namespace modle_pixels_detail {

void set_err(char* err, size_t errlen, const std::string& msg);

// the shapes modle_pixels_count accepts
bool bad_shape(uint64_t nrows, uint64_t ncols);

// count + extract + copy to the pinned host buffers of `h` (modle_pixels_to_host after its
// argument checks); waits for `stream`
int to_host(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows, uint64_t ncols,
            int64_t bin_offset, const int64_t** bin1, const int64_t** bin2, const int32_t** count,
            const int64_t** bin1_offset, modle_pixels_stats* stats, hipStream_t stream, char* err,
            size_t errlen);

}  // namespace modle_pixels_detail

#define PIX_TRY(call)                                                                           \
  do {                                                                                          \
    const hipError_t e_ = (call);                                                               \
    if (e_ != hipSuccess) {                                                                     \
      modle_pixels_detail::set_err(err, errlen, std::string(#call) + ": " + hipGetErrorString(e_)); \
      return MODLE_PIXELS_ERR_DEVICE;                                                           \
    }                                                                                           \
  } while (0)

#endif
