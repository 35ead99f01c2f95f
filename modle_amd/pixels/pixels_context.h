// pixels_context.h -- what the sources of libmodle_pixels.so share: the context behind
// modle_pixels_handle and the one-call extraction (private; the C ABI is include/modle_pixels.h).
#ifndef MODLE_PIXELS_CONTEXT_H
#define MODLE_PIXELS_CONTEXT_H
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "modle_pixels.h"

// The launch geometry whose caps a test build lowers (`make smallgrid`), so that the loops behind them take
// a second trip on small shapes; modle_pixels_build_caps reports the compiled values in this order.
#ifndef MODLE_STRIPES_MAX_GRID  // workgroups of a launch of modle_stripes.hip at most
#define MODLE_STRIPES_MAX_GRID (1u << 20)
#endif
#ifndef MODLE_BAND_FILL_MAX_Y  // gridDim.y of band_fill at most (modle_band.hip)
#define MODLE_BAND_FILL_MAX_Y 65535u
#endif
#ifndef MODLE_BAND_CHECK_GROUPS  // workgroups of band_check at most (modle_band.hip)
#define MODLE_BAND_CHECK_GROUPS 1024u
#endif
#ifndef MODLE_PIXELS_SCAN_THREADS  // threads of the one workgroup of pixels_scan (modle_pixels.hip)
#define MODLE_PIXELS_SCAN_THREADS 1024u
#endif
#ifndef MODLE_SCC_MAX_GROUPS  // workgroups per strip of 64 strata at most (modle_scc.hip); modle_pixels_scc_groups
#define MODLE_SCC_MAX_GROUPS 128u
#endif
#ifndef MODLE_RESCALE_MAX_GROUPS  // workgroups of pixels_rescale at most (modle_rescale.hip): _rescale_groups
#define MODLE_RESCALE_MAX_GROUPS 256u
#endif
static_assert(MODLE_RESCALE_MAX_GROUPS >= 1 && MODLE_RESCALE_MAX_GROUPS <= 65535u, "a grid's x; partials in scratch");
static_assert(MODLE_SCC_MAX_GROUPS >= 1 && MODLE_SCC_MAX_GROUPS <= 65535u, "a grid's y");
static_assert(MODLE_STRIPES_MAX_GRID >= 1 && MODLE_STRIPES_MAX_GRID <= (1u << 20), "a grid's x");
static_assert(MODLE_BAND_FILL_MAX_Y >= 1 && MODLE_BAND_FILL_MAX_Y <= 65535u, "a grid's y");
static_assert(MODLE_BAND_CHECK_GROUPS >= 1 && MODLE_BAND_CHECK_GROUPS <= 1024u, "workgroups of band_check");
static_assert(MODLE_PIXELS_SCAN_THREADS % 64 == 0 && MODLE_PIXELS_SCAN_THREADS >= 64 &&
                  MODLE_PIXELS_SCAN_THREADS <= 1024u, "whole waves of one workgroup");

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

// The first step of every modle_pixels_coarse_*_to_host, on arguments modle_pixels_coarse_shape accepted with
// the shape (nr, nc): sets the device, makes room in h->coarse and enqueues the coarsening into h->coarse.dev
// (modle_coarsen.hip).  The fine form of the analysis on (h->coarse.dev, nr, nc) follows.  (Hidden: the
// library's dynamic symbols stay as they are.)
__attribute__((visibility("hidden")))
int coarsen_to_scratch(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows, uint64_t ncols,
                       uint64_t factor, uint64_t first_bin, uint64_t nr, uint64_t nc, hipStream_t stream,
                       char* err, size_t errlen);

// the bytes of a band: its nrows * ncols words and the trailing word
inline uint64_t band_bytes(uint64_t nrows, uint64_t ncols) { return (nrows * ncols + 1) * 4; }

// Whether two byte ranges share a byte; a range that ends where the other begins does not, and an empty range
// overlaps nothing (only modle_pixels_pileup passes an empty one: every other size is non-zero where this is called).
inline bool overlap(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a_bytes != 0 && b_bytes != 0 && a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

// what the forms that return pixels refuse of their five outputs and of the id of the first bin
inline bool bad_pixel_outputs(const int64_t** bin1, const int64_t** bin2, const int32_t** count,
                              const int64_t** bin1_offset, const modle_pixels_stats* stats, int64_t bin_offset) {
  return bin1 == nullptr || bin2 == nullptr || count == nullptr || bin1_offset == nullptr || stats == nullptr ||
         bin_offset < 0;
}

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
  // modle_pixels_dot_hist* / _dots_fdr*: the lambda table (4 rows of nrows doubles), then 64 doubles of
  // edges, then 4 x 64 words of thresholds, with the event that marks the pinned copy as read; and of
  // modle_pixels_dot_hist_to_host the table 4 x n_chunks x n_obs (modle_dots.hip)
  GrowBuf<double, true> dot_lam;
  hipEvent_t dot_lam_copied = nullptr;
  GrowBuf<uint64_t, true> dot_hist;
  // modle_pixels_pileup*: the workgroups' partial sums (S * S words each, then their counts), and of the
  // to-host forms the anchors (bin1, then bin2) and the pile with n_used behind it (modle_pileup.hip)
  GrowBuf<uint64_t> pile_partial;
  GrowBuf<int64_t> pile_anchors;
  GrowBuf<uint64_t, true> pile_out;
  // modle_pixels_sample_to_host: the kept band and the rest band (modle_sample.hip)
  GrowBuf<uint32_t> sample_kept, sample_rest;
  // modle_pixels_band_*: the words band_check reduces into, and of modle_pixels_band_from_host the pixels
  // and their row starts (modle_band.hip)
  GrowBuf<uint64_t, true> band_words;
  GrowBuf<int64_t> band_bin1, band_bin2, band_rows;
  GrowBuf<int32_t> band_count;
  // modle_pixels_stripes_to_host: two directions of rows(what) rows of ncols words (modle_stripes.hip)
  GrowBuf<uint64_t, true> stripes;
  // modle_pixels_scc*: the workgroups' partial sums (per strip and group 11 rows of 64 words), and of the
  // to-host form the 11 rows of nrows words (modle_scc.hip)
  GrowBuf<uint64_t> scc_partial;
  GrowBuf<uint64_t, true> scc;
  // modle_pixels_rescale*: the workgroups' partial sums (per workgroup R (R + 1) / 2 words of pile, as many of
  // area, then their counts), and of the to-host forms the windows (start, then end) and pile, area and n_used
  // (modle_rescale.hip)
  GrowBuf<uint64_t> rescale_partial;
  GrowBuf<int64_t> rescale_windows;
  GrowBuf<uint64_t, true> rescale_out;
};

#endif
