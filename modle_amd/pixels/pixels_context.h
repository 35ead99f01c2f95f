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

// A device array grown on demand, with (kMirror) a pinned host array of the same size.
template <class T, bool kMirror = false>
struct GrowBuf {
  T* dev = nullptr;
  T* host = nullptr;  // pinned; null without a mirror
  uint64_t cap = 0;   // elements
  ~GrowBuf() { release(); }
  void release() {
    (void)hipFree(dev), dev = nullptr;
    (void)hipHostFree(host), host = nullptr;
    cap = 0;
  }
  // Room for `n` elements: only when n exceeds the capacity, the arrays are freed and allocated
  // anew, `room` adding an eighth (the next interval is rarely the same size).  A failure leaves
  // the capacity at 0, so that the next call allocates again.
  int ensure(uint64_t n, char* err, size_t errlen, bool room = true) {
    if (n <= cap) return MODLE_PIXELS_OK;
    release();
    if (room) n += n / 8;
    PIX_TRY(hipMalloc(reinterpret_cast<void**>(&dev), n * sizeof(T)));
    if (kMirror) PIX_TRY(hipHostMalloc(reinterpret_cast<void**>(&host), n * sizeof(T), hipHostMallocDefault));
    cap = n;
    return MODLE_PIXELS_OK;
  }
};

struct modle_pixels_handle {
  int device = 0;
  DeviceStats* d_stats = nullptr;
  DeviceStats* h_stats = nullptr;  // pinned
  // one-call form: the pixels (sized by nnz) and the bin1_offset index (ncols + 1 entries, exactly)
  GrowBuf<int64_t, true> bin1, bin2, offsets;
  GrowBuf<int32_t, true> count;
  GrowBuf<uint32_t> coarse;       // modle_pixels_coarse_to_host: the coarse band (modle_coarsen.hip)
  GrowBuf<uint32_t, true> dense;  // modle_pixels_dense_to_host: the region (modle_dense.hip)
  // modle_pixels_marginals*: diag_sum (nrows words), then coverage (ncols words) (modle_marginals.hip)
  GrowBuf<uint64_t, true> marginals;
  // modle_pixels_insulation_to_host: n_windows rows of ncols words (modle_insulation.hip)
  GrowBuf<uint64_t, true> insulation;
  // modle_pixels_dots*: the candidate band of the to-host forms, and the scale table (4 rows of nrows
  // doubles) with the event that marks its pinned copy as read (modle_dots.hip)
  GrowBuf<uint32_t> dot_cand;
  GrowBuf<double, true> dot_scale;
  hipEvent_t dot_scale_copied = nullptr;
  // modle_pixels_pileup*: the workgroups' partial sums (S * S words each, then their counts), and of the
  // to-host forms the anchors (bin1, then bin2) and the pile with n_used behind it (modle_pileup.hip)
  GrowBuf<uint64_t> pile_partial;
  GrowBuf<int64_t> pile_anchors;
  GrowBuf<uint64_t, true> pile_out;
  // modle_pixels_sample_to_host: the kept band and the rest band (modle_sample.hip)
  GrowBuf<uint32_t> sample_kept, sample_rest;
};

#endif
