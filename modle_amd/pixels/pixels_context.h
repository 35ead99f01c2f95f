// pixels_context.h -- what the sources of libmodle_pixels.so share (private; the C ABI is include/modle_pixels.h):
// the context behind modle_pixels_handle, the band a one-call form works on (the caller's, or the scratch band
// it is coarsened into), the tail of the forms that wait for their 64-bit sums, and the overlap rule.
#ifndef MODLE_PIXELS_CONTEXT_H
#define MODLE_PIXELS_CONTEXT_H
#include <hip/hip_runtime.h>

#include <cstdint>
#include <initializer_list>
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

// The band a one-call form works on.  Every modle_pixels_*_to_host has a twin modle_pixels_coarse_*_to_host
// that coarsens into the scratch band of the context first; one body serves both, told apart by a CoarseSpec
// (a null pointer: the band itself).
struct CoarseSpec { uint64_t factor, first_bin; };
struct BandView { const uint32_t* d; uint64_t nrows, ncols; };

// Host only: the shape the analysis will see, into `v` -- the shape as given, or what modle_pixels_coarse_shape
// gives.  False for a null band, for a shape the fine form refuses (nrows == 0, bad_shape; `empty_ok`: the empty
// band with or without a pointer is a shape, as modle_pixels_count has it), and for a refused factor.
// (Hidden, like every function marked so below: the library's dynamic symbols stay as they are.)
__attribute__((visibility("hidden")))
bool view_shape(const uint32_t* d_band, uint64_t nrows, uint64_t ncols, const CoarseSpec* cs, BandView* v,
                bool empty_ok = false);

// Makes the view of view_shape real on `stream`.  The band itself: v->d is d_band, and no HIP call is made.
// Coarse: sets the device, makes room in h->coarse, enqueues the coarsening (modle_coarsen.hip); v->d is h->coarse.dev.
__attribute__((visibility("hidden")))
int resolve_band(modle_pixels_handle* h, const uint32_t* d_band, uint64_t nrows, uint64_t ncols, const CoarseSpec* cs,
                 BandView* v, hipStream_t stream, char* err, size_t errlen);

// "<name>: invalid argument <rule>", of the coarse twin "<name>: invalid argument (factor >= 2; of the coarse band:) <rule>"
__attribute__((visibility("hidden")))
std::string refusal(const char* name, const CoarseSpec* cs, const char* rule);

// modle_pixels_to_host (`cs` null) and modle_pixels_coarse_to_host under their `name`: the checks, the band
// resolved, to_host (modle_pixels.hip)
__attribute__((visibility("hidden")))
int pixels_one_call(const char* name, const CoarseSpec* cs, modle_pixels_handle* h, const uint32_t* d_band,
                    uint64_t nrows, uint64_t ncols, int64_t bin_offset, const int64_t** bin1, const int64_t** bin2,
                    const int32_t** count, const int64_t** bin1_offset, modle_pixels_stats* stats, void* stream,
                    char* err, size_t errlen);

// the bytes of a band: its nrows * ncols words and the trailing word
inline uint64_t band_bytes(uint64_t nrows, uint64_t ncols) { return (nrows * ncols + 1) * 4; }

// Whether two byte ranges share a byte; a range that ends where the other begins does not, and an empty range
// (no bytes, or a null pointer: an output that is not asked for) overlaps nothing.
inline bool overlap(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 != 0 && b0 != 0 && a_bytes != 0 && b_bytes != 0 && a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

// The overlap rule of the forms that enqueue: whether any output shares a byte with an input or with another output.
struct Bytes { const void* p; uint64_t n; };
__attribute__((visibility("hidden")))
inline bool any_overlap(std::initializer_list<Bytes> outs, std::initializer_list<Bytes> ins) {
  for (const Bytes* o = outs.begin(); o != outs.end(); ++o) {
    for (const Bytes& i : ins)
      if (overlap(o->p, o->n, i.p, i.n)) return true;
    for (const Bytes* q = outs.begin(); q != o; ++q)
      if (overlap(o->p, o->n, q->p, q->n)) return true;
  }
  return false;
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

// One context serves one call at a time, and a form that waits for its stream has read its buffers when it
// returns.  So the forms that wait share what they can: `sums` and `lists`.  What stays apart, and why:
//  * marginals, pile_partial, scc_partial, rescale_partial serve forms that enqueue and return: two analyses
//    enqueued on two streams must not share scratch, or they race;
//  * dense holds uint32; the pinned copies of dot_scale and dot_lam are guarded by events, one each;
//  * dot_cand, coarse and sample_* are alive across the to_host nested in their form, the band_* across check and fill.
struct modle_pixels_handle {
  int device = 0;
  DeviceStats* d_stats = nullptr;
  DeviceStats* h_stats = nullptr;  // pinned
  // one-call form: the pixels (sized by nnz) and the bin1_offset index (ncols + 1 entries, exactly)
  GrowBuf<int64_t, true> bin1, bin2, offsets;
  GrowBuf<int32_t, true> count;
  GrowBuf<uint32_t> coarse;       // modle_pixels_coarse_*_to_host: the coarse band (resolve_band)
  GrowBuf<uint32_t, true> dense;  // modle_pixels_dense_to_host: the region (modle_dense.hip)
  // modle_pixels_marginals*: diag_sum (nrows words), then coverage (ncols words) (modle_marginals.hip)
  GrowBuf<uint64_t, true> marginals;
  // The result of the form that waits, whichever ran last (sums_to_host): of _insulation_to_host n_windows rows of
  // ncols words; of _dot_hist_to_host the table 4 x n_chunks x n_obs; of _pileup_to_host the pile with n_used
  // behind it; of _rescale_to_host pile, area and n_used; of _stripes_to_host two directions of rows(what) rows
  // of ncols words; of _scc_to_host 11 rows of nrows words; of _stripe_profiles_to_host 2 x K x (2 m + 1) rows of ncols words;
  // of _triangles_to_host max_width rows of ncols words.
  GrowBuf<uint64_t, true> sums;
  // the two host lists of _pileup_to_host (bin1, then bin2) and of _rescale_to_host (start, then end) (upload_lists)
  GrowBuf<int64_t> lists;
  // modle_pixels_dots*: the candidate band of the to-host forms, and the scale table (4 rows of nrows
  // doubles) with the event that marks its pinned copy as read (modle_dots.hip)
  GrowBuf<uint32_t> dot_cand;
  GrowBuf<double, true> dot_scale;
  hipEvent_t dot_scale_copied = nullptr;
  // modle_pixels_dot_hist* / _dots_fdr*: the lambda table (4 rows of nrows doubles), then 64 doubles of
  // edges, then 4 x 64 words of thresholds, with the event that marks the pinned copy as read (modle_dots.hip)
  GrowBuf<double, true> dot_lam;
  hipEvent_t dot_lam_copied = nullptr;
  // the workgroups' partial sums: of modle_pixels_pileup* S * S words each, then their counts (modle_pileup.hip);
  // of _scc* per strip and group 11 rows of 64 words (modle_scc.hip); of _rescale* per workgroup R (R + 1) / 2
  // words of pile, as many of area, then their counts (modle_rescale.hip)
  GrowBuf<uint64_t> pile_partial, scc_partial, rescale_partial;
  // modle_pixels_sample_to_host: the kept band and the rest band (modle_sample.hip)
  GrowBuf<uint32_t> sample_kept, sample_rest;
  // modle_pixels_band_*: the words band_check reduces into, and of modle_pixels_band_from_host the pixels
  // and their row starts (modle_band.hip)
  GrowBuf<uint64_t, true> band_words;
  GrowBuf<int64_t> band_bin1, band_bin2, band_rows;
  GrowBuf<int32_t> band_count;
};

namespace modle_pixels_detail {

// The tail of the forms that wait for 64-bit sums: sets the device, makes room for `words` in h->sums, has
// `enqueue(h->sums.dev)` put the work on `stream`, copies the words to the pinned mirror, waits, and hands the
// mirror out in *out (valid until the next call on the context).
template <class Enqueue>
__attribute__((visibility("hidden")))
int sums_to_host(modle_pixels_handle* h, uint64_t words, const uint64_t** out, hipStream_t stream, char* err,
                 size_t errlen, Enqueue&& enqueue) {
  PIX_TRY(hipSetDevice(h->device));
  int rc = h->sums.ensure(words, err, errlen);
  if (rc == MODLE_PIXELS_OK) rc = enqueue(h->sums.dev);
  if (rc != MODLE_PIXELS_OK) return rc;
  PIX_TRY(hipMemcpyAsync(h->sums.host, h->sums.dev, words * 8, hipMemcpyDeviceToHost, stream));
  PIX_TRY(hipStreamSynchronize(stream));
  *out = h->sums.host;
  return MODLE_PIXELS_OK;
}

// Two host lists of `n` entries into h->lists on `stream`, `a` first: their device addresses in d[0] and d[1].
// No copy is issued for n == 0.  (The caller waits for the stream before it returns: the lists are host memory.)
__attribute__((visibility("hidden")))
inline int upload_lists(modle_pixels_handle* h, const int64_t* a, const int64_t* b, uint64_t n, const int64_t* d[2],
                        hipStream_t stream, char* err, size_t errlen) {
  const int rc = h->lists.ensure(2 * n, err, errlen);
  if (rc != MODLE_PIXELS_OK) return rc;
  d[0] = h->lists.dev;
  d[1] = h->lists.dev + n;
  if (n != 0) {
    PIX_TRY(hipMemcpyAsync(h->lists.dev, a, n * 8, hipMemcpyHostToDevice, stream));
    PIX_TRY(hipMemcpyAsync(h->lists.dev + n, b, n * 8, hipMemcpyHostToDevice, stream));
  }
  return MODLE_PIXELS_OK;
}

}  // namespace modle_pixels_detail

#endif
