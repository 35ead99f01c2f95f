"""ctypes view of the sparse-pixel extraction, include/modle_pixels.h (modle_amd/libmodle_pixels.so,
built by `make -C modle_amd/pixels`): the non-zero pixels of a band matrix that lies in device
memory, in cooler order, found on the GPU; the band at a multiple of its bin size; square regions
of it as dense matrices; its marginals, the sums per diagonal and per bin; its insulation sums
over sliding diamond windows; its dots, the pixels enriched over their HiCCUPS neighbourhoods, by fold and by
the statistical test (the lambda-chunk histogram counted on the GPU, dot_thresholds, the threshold decision);
its pileups, the windows around anchor pairs summed into one, and its rescaled pileups, windows of different
sizes on the diagonal cut into one grid of blocks and summed; and its random sampling, every contact
kept with one probability by a generator keyed by the pixel's coordinates; the way back, sorted pixels
checked and scattered into a band on the GPU; and two bands compared stripe by stripe, the integer sums of
every bin's vertical and horizontal stripe formed on the GPU and turned into scores by stripe_scores, and
diagonal by diagonal, the sums of every stratum of the two smoothed matrices formed on the GPU and turned into
HiCRep's stratum-adjusted correlation coefficient by scc_scores; and the stripe profiles of one band, the sums
of every bin's upstream and downstream stripe at up to four lengths with their cross-section, formed on the GPU
and turned into stripe calls by stripe_calls; and its triangle sums, the contacts inside every window on the
diagonal up to a largest width, formed on the GPU and turned into domain calls by domain_calls.
There is no host fallback: without the library or
without a device the calls fail."""
import ctypes as C
import math
import os
from collections import namedtuple
from fractions import Fraction

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# (MODLE_PIXELS_LIB: another build of the library, e.g. libmodle_pixels_smallgrid.so of `make smallgrid`)
SO_PATH = os.path.join(_HERE, os.environ.get("MODLE_PIXELS_LIB", "libmodle_pixels.so"))
ERR_ARG, ERR_DEVICE, ERR_RANGE, ERR_ORDER = -1, -2, -3, -4
MAX_WINDOW, MAX_WINDOWS = 1024, 8  # MODLE_PIXELS_MAX_WINDOW, MODLE_PIXELS_MAX_WINDOWS
MAX_DOT_WINDOW = 20  # MODLE_PIXELS_MAX_DOT_WINDOW
MAX_PILEUP_FLANK, PILEUP_GROUPS = 32, 256  # MODLE_PIXELS_MAX_PILEUP_FLANK, MODLE_PIXELS_PILEUP_GROUPS
MAX_RESCALE = 128  # MODLE_PIXELS_MAX_RESCALE: the largest grid side of a rescaled pileup
SAMPLE_TIER1_TRIALS = 64  # MODLE_PIXELS_SAMPLE_TIER1_TRIALS: what a lane draws of its own pixel
MAX_SAMPLE_TRIALS = 1 << 40  # MODLE_PIXELS_MAX_SAMPLE_TRIALS
SAMPLE_KEPT, SAMPLE_REST = 0, 1  # MODLE_PIXELS_SAMPLE_KEPT, MODLE_PIXELS_SAMPLE_REST
BAND_IN, BAND_BEYOND, BAND_OUTSIDE = 0, 1, 2  # MODLE_PIXELS_BAND_IN, _BEYOND, _OUTSIDE
BAND_TILE_COLS, BAND_TILE_DIAGS = 64, 128  # MODLE_PIXELS_BAND_TILE_COLS, _DIAGS: the tile of a workgroup of the fill
STRIPES_MOMENTS, STRIPES_MASKED, STRIPES_RANKS = 1, 2, 4  # MODLE_PIXELS_STRIPES_MOMENTS, _MASKED, _RANKS
MAX_STRIPE = 4096  # MODLE_PIXELS_MAX_STRIPE: the deepest band the rank sums are formed of
STRIPE_METRICS = ("pearson", "spearman", "rmse", "eucl_dist")  # what stripe_scores forms (evaluate.METRICS)
SCC_ROWS = 11  # MODLE_PIXELS_SCC_ROWS: n and the five 128-bit sums of a stratum
MAX_SCC_SMOOTH = 20  # MODLE_PIXELS_MAX_SCC_SMOOTH: the largest half-width of the smoothing box
MAX_PROFILE_OFFSET, MAX_PROFILE_LENGTHS = 8, 4  # MODLE_PIXELS_MAX_PROFILE_OFFSET, MODLE_PIXELS_MAX_PROFILE_LENGTHS
# The defaults of stripe_calls: product choices, not measured claims.  A centre 1.5 times either shoulder is the
# enrichment HiCCUPS asks of a dot against its horizontal and vertical neighbourhoods (DOT_FOLDS); one contact
# keeps empty stripes out; no thinning unless asked for.
STRIPE_FOLD, STRIPE_MIN_COUNT, STRIPE_RADIUS = 1.5, 1, 0
MAX_TRIANGLE_WIDTH = 65535  # MODLE_PIXELS_MAX_TRIANGLE_WIDTH: W (W + 1) / 2 pixels below 2^32 stay below 2^64
# The defaults of domain_calls: product choices, not measured claims.  gamma 1 scores a window against the mean
# window of its width; three bins is the smallest window that has a pixel beyond the two diagonals `simulate`
# ignores by default.
DOMAIN_GAMMA, DOMAIN_MIN_WIDTH = 1.0, 3
DOT_FOLDS = (1.75, 1.75, 1.5, 1.5)  # HiCCUPS' thresholds: donut, lower-left, horizontal, vertical
MAX_DOT_EDGES, MAX_DOT_OBS = 63, 16384  # MODLE_PIXELS_MAX_DOT_EDGES, MODLE_PIXELS_MAX_DOT_OBS
DOT_LAMBDA_CHUNKS = 40  # HiCCUPS' number of lambda-chunk edges (dot_lambda_edges)
EXPORTS = ["modle_pixels_create", "modle_pixels_destroy", "modle_pixels_count", "modle_pixels_extract",
           "modle_pixels_to_host", "modle_pixels_coarse_shape", "modle_pixels_coarsen",
           "modle_pixels_coarse_to_host", "modle_pixels_tiles_fit", "modle_pixels_dense_tiles",
           "modle_pixels_dense_to_host", "modle_pixels_marginals", "modle_pixels_marginals_to_host",
           "modle_pixels_coarse_marginals_to_host", "modle_pixels_insulation_n_valid", "modle_pixels_insulation",
           "modle_pixels_insulation_to_host", "modle_pixels_coarse_insulation_to_host", "modle_pixels_dots",
           "modle_pixels_dots_to_host", "modle_pixels_coarse_dots_to_host", "modle_pixels_dot_hist",
           "modle_pixels_dot_hist_to_host", "modle_pixels_coarse_dot_hist_to_host", "modle_pixels_dots_fdr",
           "modle_pixels_dots_fdr_to_host", "modle_pixels_coarse_dots_fdr_to_host", "modle_pixels_pileup_accepts",
           "modle_pixels_pileup", "modle_pixels_pileup_to_host",
           "modle_pixels_coarse_pileup_to_host", "modle_pixels_rescale_groups", "modle_pixels_rescale_accepts",
           "modle_pixels_rescale", "modle_pixels_rescale_to_host", "modle_pixels_coarse_rescale_to_host",
           "modle_pixels_sample_pixels", "modle_pixels_sample",
           "modle_pixels_sample_to_host", "modle_pixels_band_classify", "modle_pixels_band_check",
           "modle_pixels_band_fill", "modle_pixels_band_from_host", "modle_pixels_stripes_rows",
           "modle_pixels_stripes", "modle_pixels_stripes_to_host", "modle_pixels_scc_groups", "modle_pixels_scc",
           "modle_pixels_scc_to_host", "modle_pixels_stripe_profiles", "modle_pixels_stripe_profiles_to_host",
           "modle_pixels_coarse_stripe_profiles_to_host", "modle_pixels_triangles", "modle_pixels_triangles_to_host",
           "modle_pixels_coarse_triangles_to_host", "modle_pixels_triangle_cells",
           "modle_pixels_build_caps"]  # every symbol include/modle_pixels.h declares
# what modle_pixels_build_caps reports of the default build: the workgroups of a stripes launch, the grid's y of
# the band fill, the workgroups of the band check, the threads of the bin1_offset scan
BuildCaps = namedtuple("BuildCaps", "stripes_grid fill_grid_y check_groups scan_threads")
DEFAULT_BUILD_CAPS = BuildCaps(1 << 20, 65535, 1024, 1024)

_LIB = None
_EXTRACTORS = {}

Stats = namedtuple("Stats", "nnz sum max_count")
Pixels = namedtuple("Pixels", "bin1 bin2 count bin1_offset stats")  # what extract / coarse_extract return
# what band_check / band_from_host return (modle_pixels_band_stats)
BandStats = namedtuple("BandStats", "n_in sum_in nnz_in n_beyond sum_beyond n_outside sum_outside max_count first_bad")


class _CStats(C.Structure):  # modle_pixels_stats
    _fields_ = [("nnz", C.c_uint64), ("sum", C.c_uint64), ("max_count", C.c_uint32),
                ("reserved_", C.c_uint32)]


class _CBandStats(C.Structure):  # modle_pixels_band_stats
    _fields_ = [(name, C.c_uint64) for name in ("n_in", "sum_in", "nnz_in", "n_beyond", "sum_beyond", "n_outside",
                                                "sum_outside")] + \
               [("first_bad", C.c_int64), ("max_count", C.c_uint32), ("reserved_", C.c_uint32)]

    def tuple(self):
        return BandStats(self.n_in, self.sum_in, self.nnz_in, self.n_beyond, self.sum_beyond, self.n_outside,
                         self.sum_outside, self.max_count, self.first_bad)


class PixelsError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"modle_pixels error {code}: {message}")
        self.code = code


class BandListError(PixelsError):
    """ERR_ORDER / ERR_RANGE of band_check and band_from_host: `stats` is the BandStats the library filled,
    stats.first_bad the smallest offending index"""

    def __init__(self, code, message, stats):
        super().__init__(code, message)
        self.stats = stats


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(SO_PATH):
            raise ImportError(f"{SO_PATH} is missing: run `make -C modle_amd/pixels` "
                              "(python -c 'import __graft_entry__ as g; g.build()')")
        from ._lib import _share_the_hip_runtime_with_torch

        _share_the_hip_runtime_with_torch()  # one HIP runtime per process (see _lib.py)
        lb = C.CDLL(SO_PATH)
        err = [C.c_char_p, C.c_size_t]
        shape = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64]  # handle, d_band, nrows, ncols
        lb.modle_pixels_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)] + err
        lb.modle_pixels_destroy.argtypes = [C.c_void_p]
        lb.modle_pixels_destroy.restype = None
        lb.modle_pixels_count.argtypes = shape + [C.c_void_p, C.POINTER(_CStats), C.c_void_p] + err
        lb.modle_pixels_extract.argtypes = shape + [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_uint64, C.c_void_p] + err
        # bin_offset, bin1, bin2, count, bin1_offset, stats, stream: the tail of every form that returns pixels
        pix = [C.c_int64] + [C.POINTER(C.c_void_p)] * 4 + [C.POINTER(_CStats), C.c_void_p] + err
        lb.modle_pixels_to_host.argtypes = shape + pix
        u64p = C.POINTER(C.c_uint64)
        lb.modle_pixels_coarse_shape.argtypes = [C.c_uint64] * 4 + [u64p, u64p]
        lb.modle_pixels_coarsen.argtypes = shape + [C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64,
                                                    C.c_void_p] + err
        lb.modle_pixels_coarse_to_host.argtypes = shape + [C.c_uint64] * 2 + pix
        lb.modle_pixels_tiles_fit.argtypes = [C.c_uint64] * 4 + [u64p]
        lb.modle_pixels_dense_tiles.argtypes = shape + [C.c_uint64] * 4 + [C.c_void_p, C.c_uint64, C.c_void_p] + err
        lb.modle_pixels_dense_to_host.argtypes = shape + [C.c_uint64, C.c_uint64, C.POINTER(C.c_void_p),
                                                          C.c_void_p] + err
        sums = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_void_p] + err  # diag_sum, coverage, stream
        lb.modle_pixels_marginals.argtypes = shape + [C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p] + err
        lb.modle_pixels_marginals_to_host.argtypes = shape + [C.c_uint64] + sums
        lb.modle_pixels_coarse_marginals_to_host.argtypes = shape + [C.c_uint64] * 3 + sums
        wins = [u64p, C.c_uint64, C.c_uint64]  # windows (a host array), n_windows, min_diag
        lb.modle_pixels_insulation_n_valid.argtypes = [C.c_uint64] * 3 + [u64p]
        lb.modle_pixels_insulation.argtypes = shape + wins + [C.c_void_p, C.c_uint64, C.c_void_p] + err
        lb.modle_pixels_insulation_to_host.argtypes = shape + wins + [C.POINTER(C.c_void_p), C.c_void_p] + err
        lb.modle_pixels_coarse_insulation_to_host.argtypes = shape + [C.c_uint64] * 2 + wins + \
            [C.POINTER(C.c_void_p), C.c_void_p] + err
        dots = [C.c_uint64] * 4 + [C.POINTER(C.c_double)]  # w, p, min_diag, min_count, scale (a host table)
        lb.modle_pixels_dots.argtypes = shape + dots + [C.c_void_p, C.c_void_p, C.c_void_p] + err
        lb.modle_pixels_dots_to_host.argtypes = shape + dots + pix
        lb.modle_pixels_coarse_dots_to_host.argtypes = shape + [C.c_uint64] * 2 + dots + pix
        f64p = C.POINTER(C.c_double)
        chunks = [f64p, f64p, C.c_uint64]  # lam, edges (host tables), n_edges
        hist = [C.c_uint64] * 3 + chunks + [C.c_uint64]  # w, p, min_diag, the tables, n_obs
        fdr = [C.c_uint64] * 4 + chunks + [C.POINTER(C.c_uint32), f64p]  # w .. min_count, the tables, thr, scale
        lb.modle_pixels_dot_hist.argtypes = shape + hist + [C.c_void_p, C.c_void_p] + err
        lb.modle_pixels_dot_hist_to_host.argtypes = shape + hist + [C.POINTER(C.c_void_p), C.c_void_p] + err
        lb.modle_pixels_coarse_dot_hist_to_host.argtypes = shape + [C.c_uint64] * 2 + hist + \
            [C.POINTER(C.c_void_p), C.c_void_p] + err
        lb.modle_pixels_dots_fdr.argtypes = shape + fdr + [C.c_void_p, C.c_void_p] + err
        lb.modle_pixels_dots_fdr_to_host.argtypes = shape + fdr + pix
        lb.modle_pixels_coarse_dots_fdr_to_host.argtypes = shape + [C.c_uint64] * 2 + fdr + pix
        i64p = C.POINTER(C.c_int64)
        piled = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_void_p] + err  # pile, n_used, stream
        lb.modle_pixels_pileup_accepts.argtypes = [C.c_uint64] * 3 + [C.c_int64, i64p, i64p, C.c_uint64,
                                                                      C.POINTER(C.c_uint8)]
        lb.modle_pixels_pileup.argtypes = shape + [C.c_uint64, C.c_int64, C.c_void_p, C.c_void_p, C.c_uint64,
                                                   C.c_void_p, C.c_void_p, C.c_void_p] + err
        lb.modle_pixels_pileup_to_host.argtypes = shape + [C.c_uint64, C.c_int64, i64p, i64p, C.c_uint64] + piled
        lb.modle_pixels_coarse_pileup_to_host.argtypes = shape + [C.c_uint64] * 3 + [C.c_int64, i64p, i64p,
                                                                                     C.c_uint64] + piled
        scaled = [C.POINTER(C.c_void_p)] * 3 + [C.c_void_p] + err  # pile, area, n_used, stream
        lb.modle_pixels_rescale_groups.argtypes = []
        lb.modle_pixels_rescale_groups.restype = C.c_uint64
        lb.modle_pixels_rescale_accepts.argtypes = [C.c_uint64] * 3 + [C.c_int64, i64p, i64p, C.c_uint64,
                                                                       C.POINTER(C.c_uint8)]
        lb.modle_pixels_rescale.argtypes = shape + [C.c_uint64, C.c_int64, C.c_void_p, C.c_void_p, C.c_uint64,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p] + err
        lb.modle_pixels_rescale_to_host.argtypes = shape + [C.c_uint64, C.c_int64, i64p, i64p, C.c_uint64] + scaled
        lb.modle_pixels_coarse_rescale_to_host.argtypes = shape + [C.c_uint64] * 3 + [C.c_int64, i64p, i64p,
                                                                                      C.c_uint64] + scaled
        u32p = C.POINTER(C.c_uint32)
        draw = [C.c_int64, C.c_uint64, C.c_uint64, C.c_uint32]  # bin_offset, threshold, seed, salt
        lb.modle_pixels_sample_pixels.argtypes = [C.c_uint64, C.c_uint32, C.c_uint64, C.c_int64, i64p, i64p, u32p,
                                                  C.c_uint64, u32p]
        lb.modle_pixels_sample.argtypes = shape + draw + [C.POINTER(_CStats), C.c_void_p, C.c_void_p, C.c_void_p] + err
        lb.modle_pixels_sample_to_host.argtypes = shape + draw + [C.c_int] + pix[1:]
        lb.modle_pixels_band_classify.argtypes = [C.c_uint64, C.c_uint64, C.c_int64, i64p, i64p, C.c_uint64,
                                                  C.POINTER(C.c_uint8)]
        # handle, (d_bin1,) d_bin2, d_count, n, nrows, ncols, bin_offset
        lb.modle_pixels_band_check.argtypes = [C.c_void_p] * 4 + [C.c_uint64] * 3 + [C.c_int64, C.c_void_p,
                                                                                     C.POINTER(_CBandStats), C.c_void_p] + err
        lb.modle_pixels_band_fill.argtypes = [C.c_void_p] * 3 + [C.c_uint64] * 3 + [C.c_int64, C.c_void_p, C.c_void_p,
                                                                                    C.c_uint64, C.c_void_p] + err
        lb.modle_pixels_band_from_host.argtypes = [C.c_void_p] * 4 + [C.c_uint64] * 3 + \
            [C.c_int64, C.c_void_p, C.c_uint64, C.POINTER(_CBandStats), C.c_void_p] + err
        pair = [C.c_void_p] * 3 + [C.c_uint64] * 3  # handle, d_ref, d_tgt, nrows, ncols, what
        lb.modle_pixels_stripes_rows.argtypes = [C.c_uint64]
        lb.modle_pixels_stripes.argtypes = pair + [C.c_void_p, C.c_uint64, C.c_void_p] + err
        lb.modle_pixels_stripes_to_host.argtypes = pair + [C.POINTER(C.c_void_p), C.c_void_p] + err
        strata = [C.c_void_p] * 3 + [C.c_uint64] * 5  # handle, d_ref, d_tgt, nrows, ncols, smooth, min_diag, max_diag
        lb.modle_pixels_scc_groups.argtypes = []
        lb.modle_pixels_scc_groups.restype = C.c_uint64
        lb.modle_pixels_scc.argtypes = strata + [C.c_void_p, C.c_uint64, C.c_void_p] + err
        lb.modle_pixels_scc_to_host.argtypes = strata + [C.POINTER(C.c_void_p), C.c_void_p] + err
        prof = [C.c_uint64, u64p, C.c_uint64, C.c_uint64]  # max_offset, lengths (a host array), n_lengths, min_diag
        lb.modle_pixels_stripe_profiles.argtypes = shape + prof + [C.c_void_p, C.c_uint64, C.c_void_p] + err
        lb.modle_pixels_stripe_profiles_to_host.argtypes = shape + prof + [C.POINTER(C.c_void_p), C.c_void_p] + err
        lb.modle_pixels_coarse_stripe_profiles_to_host.argtypes = shape + [C.c_uint64] * 2 + prof + \
            [C.POINTER(C.c_void_p), C.c_void_p] + err
        tri = [C.c_uint64, C.c_uint64]  # max_width, min_diag
        lb.modle_pixels_triangles.argtypes = shape + tri + [C.c_void_p, C.c_uint64, C.c_void_p] + err
        lb.modle_pixels_triangles_to_host.argtypes = shape + tri + [C.POINTER(C.c_void_p), C.c_void_p] + err
        lb.modle_pixels_coarse_triangles_to_host.argtypes = shape + [C.c_uint64] * 2 + tri + \
            [C.POINTER(C.c_void_p), C.c_void_p] + err
        lb.modle_pixels_triangle_cells.argtypes = [C.c_uint64] * 3 + [u64p]
        lb.modle_pixels_build_caps.argtypes = [u64p]
        lb.modle_pixels_build_caps.restype = None
        for name in EXPORTS:
            getattr(lb, name)  # raises AttributeError if a declared symbol is not exported
        _LIB = lb
    return _LIB


def _stream_ptr(stream):
    """None, a raw hipStream_t value, or a torch.cuda.Stream"""
    if stream is None:
        return None
    return int(getattr(stream, "cuda_stream", stream)) or None


def _host_array(ptr, n, dtype):
    if n == 0 or not ptr:
        return np.zeros(0, dtype=dtype)
    ctype = {np.int64: C.c_int64, np.int32: C.c_int32, np.uint64: C.c_uint64}[dtype]
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=(n,)).copy()


def _call(fn, *args):
    """`fn(*args, err, errlen)`: every entry point of the library that can fail"""
    err = C.create_string_buffer(512)
    rc = fn(*args, err, len(err))
    if rc != 0:
        raise PixelsError(rc, err.value.decode(errors="replace"))


def build_caps():
    """the launch caps the loaded library was compiled with, BuildCaps (modle_pixels_build_caps; no device is
    needed): DEFAULT_BUILD_CAPS unless MODLE_PIXELS_LIB names a test build"""
    caps = (C.c_uint64 * 4)()
    lib().modle_pixels_build_caps(caps)
    return BuildCaps(*(int(c) for c in caps))


def coarse_shape(nrows, ncols, factor, first_bin=0):
    """(nrows', ncols') of the band coarsened by `factor` (modle_pixels_coarse_shape; no device is
    needed).  `first_bin`: chromosome-relative index of the interval's first fine bin."""
    nr, nc = C.c_uint64(), C.c_uint64()
    rc = lib().modle_pixels_coarse_shape(int(nrows), int(ncols), int(factor), int(first_bin),
                                         C.byref(nr), C.byref(nc))
    if rc != 0:
        raise PixelsError(rc, "coarse_shape: invalid argument (factor >= 2, 0 < nrows <= ncols)")
    return nr.value, nc.value


def band_shape(nrows, ncols, factor=1, first_bin=0):
    """(nrows, ncols) of the band at `factor` times its bin size: its own at factor 1, else coarse_shape"""
    return (int(nrows), int(ncols)) if int(factor) == 1 else coarse_shape(nrows, ncols, factor, first_bin)


def tiles_fit(ncols, first, size, step):
    """how many tiles of `size` bins, `step` apart from bin `first`, lie inside [0, ncols)
    (modle_pixels_tiles_fit; no device is needed)"""
    if min(int(ncols), int(first), int(size), int(step)) < 0:
        raise PixelsError(ERR_ARG, "tiles_fit: negative argument")
    n = C.c_uint64()
    rc = lib().modle_pixels_tiles_fit(int(ncols), int(first), int(size), int(step), C.byref(n))
    if rc != 0:
        raise PixelsError(rc, "tiles_fit: invalid argument (size > 0, step > 0, first + size <= ncols)")
    return n.value


def _windows(windows):
    """(a ctypes uint64 array or None, its length) of a sequence of window sizes in bins; a negative
    size is refused here, everything else by the library"""
    ws = [int(w) for w in windows]
    if any(w < 0 for w in ws):
        raise PixelsError(ERR_ARG, "insulation: negative window")
    return ((C.c_uint64 * len(ws))(*ws) if ws else None), len(ws)


def insulation_n_valid(ncols, window, min_diag=2):
    """the number of pixels of every bin's diamond of `window` bins without the diagonals below
    `min_diag`, numpy uint64[ncols] (modle_pixels_insulation_n_valid; no device is needed)"""
    if min(int(ncols), int(window), int(min_diag)) < 0:
        raise PixelsError(ERR_ARG, "insulation_n_valid: negative argument")
    out = np.zeros(int(ncols), dtype=np.uint64)
    rc = lib().modle_pixels_insulation_n_valid(int(ncols), int(window), int(min_diag),
                                               out.ctypes.data_as(C.POINTER(C.c_uint64)))
    if rc != 0:
        raise PixelsError(rc, "insulation_n_valid: invalid argument (1 <= window <= 1024)")
    return out


def dot_offsets(w, p):
    """the four HiCCUPS neighbourhoods of a pixel for the window half-width `w` and the peak half-width
    `p` (0 <= p < w), each a list of (row, column) offsets from the pixel in the symmetric matrix: donut,
    lower-left, horizontal, vertical (include/modle_pixels.h)"""
    w, p = int(w), int(p)
    if not 0 <= p < w:
        raise ValueError(f"dots: the peak half-width {p} is not in [0, window half-width {w})")
    span = range(-w, w + 1)
    donut = [(a, b) for a in span for b in span if max(abs(a), abs(b)) > p and a != 0 and b != 0]
    lower_left = [(a, b) for a in range(1, w + 1) for b in range(-w, 0) if a > p or -b > p]
    horizontal = [(a, b) for a in (-1, 0, 1) for b in span if abs(b) > p]
    vertical = [(a, b) for a in span if abs(a) > p for b in (-1, 0, 1)]
    return [donut, lower_left, horizontal, vertical]


def dot_areas(w, p):
    """the number of pixels of the four neighbourhoods: ((2w+1)^2 - (2p+1)^2 - 4(w-p), w^2 - p^2,
    6(w-p), 6(w-p))"""
    w, p = int(w), int(p)
    if not 0 <= p < w:
        raise ValueError(f"dots: the peak half-width {p} is not in [0, window half-width {w})")
    return ((2 * w + 1) ** 2 - (2 * p + 1) ** 2 - 4 * (w - p), w * w - p * p, 6 * (w - p), 6 * (w - p))


def dot_valid_diags(nrows, w, min_diag=2):
    """(first, last) diagonal of the valid pixels, 2w + min_diag and nrows - 1 - 2w.  ValueError when
    the band has none: 4w + 1 + min_diag > nrows."""
    nrows, w, min_diag = int(nrows), int(w), int(min_diag)
    if w < 1 or min_diag < 0 or 4 * w + 1 + min_diag > nrows:
        raise ValueError(f"dots: a window half-width of {w} bins with the first {min_diag} diagonals left out "
                         f"needs {4 * w + 1 + min_diag} diagonals, the band has {nrows}")
    return 2 * w + min_diag, nrows - 1 - 2 * w


def dot_scales(diag_sum, ncols, w, p, folds=DOT_FOLDS, min_diag=2):
    """The table modle_pixels_dots decides with, numpy float64 [4, nrows], from the diagonal sums of the
    band (marginals): with the expected e[d] = diag_sum[d] / (ncols - d) and X_k[d] = the sum of
    e[d + b - a] over the offsets (a, b) of neighbourhood k,
        scale[k][d] = folds[k] * e[d] / X_k[d]    (+inf where X_k[d] == 0, 0 at an invalid d),
    so that obs >= O_k * scale[k][d] says obs >= folds[k] * (O_k / X_k[d]) * e[d]: the pixel stands
    folds[k] above the expected, rescaled by what its neighbourhood holds (Rao et al. 2014)."""
    diag = np.asarray(diag_sum, dtype=np.uint64)
    nrows = len(diag)
    lo, hi = dot_valid_diags(nrows, w, min_diag)
    if len(folds) != 4 or any(not float(f) >= 0 for f in folds):
        raise ValueError(f"dots: {folds!r} is not four non-negative thresholds")
    if int(ncols) < nrows:
        raise ValueError(f"dots: ncols {ncols} is below nrows {nrows}")
    e = diag.astype(np.float64) / (np.float64(int(ncols)) - np.arange(nrows, dtype=np.float64))
    out = np.zeros((4, nrows), dtype=np.float64)
    d = np.arange(lo, hi + 1)
    for k, offs in enumerate(dot_offsets(w, p)):
        x = np.zeros(len(d), dtype=np.float64)
        for a, b in offs:
            x += e[d + (b - a)]
        with np.errstate(divide="ignore", invalid="ignore"):
            out[k, d] = np.where(x == 0, np.inf, np.float64(float(folds[k])) * e[d] / x)
    return out


def _scale_table(scale, nrows):
    """(the float64 [4, nrows] array to keep alive, its ctypes pointer) of a table of dot_scales' shape;
    None stays None.  The shape is checked against the band's `nrows` once the library has accepted
    the rest (a coarse band: by the caller)."""
    if scale is None:
        return None, None
    t = np.ascontiguousarray(scale, dtype=np.float64)
    if t.ndim != 2 or t.shape[0] != 4 or (nrows is not None and t.shape[1] != int(nrows)):
        raise PixelsError(ERR_ARG, f"dots: the scale table has shape {t.shape}, not (4, nrows)")
    return t, t.ctypes.data_as(C.POINTER(C.c_double))


def dot_lambda_edges(n=DOT_LAMBDA_CHUNKS):
    """HiCCUPS' lambda-chunk edges, numpy float64[n]: 2 ** (i / 3), i = 0 .. n - 1 (n = 40: up to 8192).  Chunk c
    is (edges[c - 1], edges[c]]; the chunk above the last edge never calls."""
    n = int(n)
    if not 1 <= n <= MAX_DOT_EDGES:
        raise ValueError(f"dots: {n} lambda chunks are not in [1, {MAX_DOT_EDGES}]")
    return np.float64(2.0) ** (np.arange(n, dtype=np.float64) / np.float64(3.0))


def _edge_table(edges):
    """(the float64 array to keep alive, its ctypes pointer, n_edges) of the lambda-chunk edges; None: HiCCUPS'"""
    e = dot_lambda_edges() if edges is None else np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
    return e, e.ctypes.data_as(C.POINTER(C.c_double)), len(e)


def _thr_table(thresholds, n_edges):
    """(the uint32 [4, n_edges + 1] array to keep alive, its ctypes pointer) of a table of dot_thresholds' shape"""
    raw = np.asarray(thresholds)
    if raw.shape != (4, n_edges + 1) or raw.dtype.kind not in "iu" or (raw < 0).any() or (raw > 0xFFFFFFFF).any():
        raise PixelsError(ERR_ARG, f"dots: the threshold table has shape {raw.shape} and type {raw.dtype}, not "
                                   f"(4, {n_edges + 1}) of uint32 values")
    t = np.ascontiguousarray(raw, dtype=np.uint32)
    return t, t.ctypes.data_as(C.POINTER(C.c_uint32))


def poisson_tail(mean, n):
    """P(Poisson(mean) >= t) for t = 0 .. n - 1, numpy float64[n], for a finite mean > 0.  The probabilities are
    formed relative to the one at the mode, by the recurrence p(k + 1) = p(k) * mean / (k + 1) upwards and downwards
    from it, summed from the far tail towards it, the small terms first, and divided by their total: nothing
    depends on exp(-mean), which underflows beyond 745, and only a term below 1e-308 of the mode's is lost."""
    mean, n = float(mean), int(n)
    if not (mean > 0 and math.isfinite(mean)) or n < 1:
        raise ValueError(f"dots: the Poisson tail needs a finite mean > 0 and n >= 1, not {mean!r}, {n}")
    mode = int(mean)
    top = max(n, mode + int(40.0 * math.sqrt(mean) + 64.0))  # beyond it the terms add nothing to a double
    rel = np.ones(top + 1, dtype=np.float64)
    with np.errstate(under="ignore"):
        rel[mode + 1:] = np.cumprod(mean / np.arange(mode + 1, top + 1, dtype=np.float64))
        rel[:mode] = np.cumprod(np.arange(mode, 0, -1, dtype=np.float64) / mean)[::-1]
    tail = np.cumsum(rel[::-1])[::-1]
    return tail[:n] / tail[0]


def dot_thresholds(hist, edges, fdr):
    """The count thresholds of the lambda chunks, numpy uint32 [4, n_chunks], from the histograms of
    modle_pixels_dot_hist (uint64 [4, n_chunks, n_obs]): for neighbourhood k and chunk c below the top one, with
    L = edges[c], N the chunk's pixels and tail[t] those with a count >= t, the smallest t in 1 .. n_obs - 1 with
    tail[t] > 0 and N * P(Poisson(L) >= t) <= fdr * tail[t] -- the Benjamini-Hochberg rule against the Poisson
    law of the chunk's upper edge (Rao et al. 2014) -- and 0, "never", where there is none and for the top chunk.
    The last bin holds every count >= n_obs - 1, so tail[n_obs - 1] and with it every threshold is exact."""
    h = np.asarray(hist)
    e = np.asarray(edges, dtype=np.float64).reshape(-1)
    fdr = float(fdr)
    if h.ndim != 3 or h.shape[0] != 4 or h.shape[1] != len(e) + 1 or h.shape[2] < 2 or h.dtype.kind not in "iu":
        raise ValueError(f"dots: a histogram of shape {h.shape} is not (4, {len(e) + 1}, n_obs >= 2) of integers")
    if not 0.0 < fdr < 1.0:
        raise ValueError(f"dots: the false discovery rate {fdr!r} is not in (0, 1)")
    if len(e) < 1 or not np.isfinite(e).all() or not (e > 0).all() or not (np.diff(e) > 0).all():
        raise ValueError("dots: the lambda-chunk edges are not finite, positive and strictly increasing")
    n_obs = h.shape[2]
    out = np.zeros((4, len(e) + 1), dtype=np.uint32)
    for c in range(len(e)):
        if not h[:, c].any():
            continue
        q = poisson_tail(e[c], n_obs)
        for k in range(4):
            above = np.cumsum(h[k, c][::-1].astype(np.uint64))[::-1]  # above[t]: the pixels with a count >= t
            n = float(int(above[0]))
            met = (above > 0) & (n * q <= fdr * above.astype(np.float64))
            met[0] = False
            if met.any():
                out[k, c] = int(np.argmax(met))
    return out


def _anchors(bin1, bin2):
    """(the two contiguous int64 arrays to keep alive, their ctypes pointers or None, n) of host anchors"""
    b1 = np.ascontiguousarray(bin1, dtype=np.int64).reshape(-1)
    b2 = np.ascontiguousarray(bin2, dtype=np.int64).reshape(-1)
    if len(b1) != len(b2):
        raise PixelsError(ERR_ARG, f"pileup: {len(b1)} first and {len(b2)} second anchors")
    if len(b1) == 0:
        return (b1, b2), None, None, 0
    i64p = C.POINTER(C.c_int64)
    return (b1, b2), b1.ctypes.data_as(i64p), b2.ctypes.data_as(i64p), len(b1)


def _flank(flank):
    if int(flank) < 0:
        raise PixelsError(ERR_ARG, "pileup: negative flank")
    return int(flank)


def pileup_accepts(nrows, ncols, flank, bin1, bin2, bin_offset=0):
    """which anchors (bin1[t] - bin_offset, bin2[t] - bin_offset) = (a, b) a pileup of `flank` bins uses,
    a numpy bool array: a <= b, a >= flank, b + flank <= ncols - 1, (b - a) + 2 * flank <= nrows - 1, for
    any int64 values (modle_pixels_pileup_accepts; no device is needed)"""
    if min(int(nrows), int(ncols)) < 0:
        raise PixelsError(ERR_ARG, "pileup_accepts: negative shape")
    keep, p1, p2, n = _anchors(bin1, bin2)
    out = np.zeros(n, dtype=np.uint8)
    rc = lib().modle_pixels_pileup_accepts(int(nrows), int(ncols), _flank(flank), int(bin_offset), p1, p2, n,
                                           out.ctypes.data_as(C.POINTER(C.c_uint8)))
    del keep
    if rc != 0:
        raise PixelsError(rc, "pileup_accepts: invalid argument (0 < nrows <= ncols, flank <= 32, "
                              "2 * flank + 1 <= nrows, n < 2^31)")
    return out.astype(bool)


def rescale_groups():
    """the workgroups of a rescaled pileup at most that the loaded library was compiled with
    (modle_pixels_rescale_groups; no device is needed): 256 unless MODLE_PIXELS_LIB names a test build"""
    return int(lib().modle_pixels_rescale_groups())


def _size(size):
    if int(size) < 0:
        raise PixelsError(ERR_ARG, "rescale: negative size")
    return int(size)


def rescale_accepts(nrows, ncols, size, start, end, bin_offset=0):
    """which windows [start[t] - bin_offset, end[t] - bin_offset) = [s, e) a rescaled pileup on a grid of
    `size` uses, a numpy bool array: 0 <= s < e <= ncols, size <= e - s <= nrows, for any int64 values
    (modle_pixels_rescale_accepts; no device is needed)"""
    if min(int(nrows), int(ncols)) < 0:
        raise PixelsError(ERR_ARG, "rescale_accepts: negative shape")
    keep, p1, p2, n = _anchors(start, end)
    out = np.zeros(n, dtype=np.uint8)
    rc = lib().modle_pixels_rescale_accepts(int(nrows), int(ncols), _size(size), int(bin_offset), p1, p2, n,
                                            out.ctypes.data_as(C.POINTER(C.c_uint8)))
    del keep
    if rc != 0:
        raise PixelsError(rc, "rescale_accepts: invalid argument (0 < nrows <= ncols, 1 <= size <= 128, n < 2^31, "
                              "n * ceil(nrows / size)^2 < 2^32)")
    return out.astype(bool)


def band_classify(nrows, ncols, bin1, bin2, bin_offset=0):
    """the class of every pixel (bin1[t] - bin_offset, bin2[t] - bin_offset) = (i, j) against a band of `nrows`
    diagonals and `ncols` columns, a numpy uint8 array: BAND_IN for 0 <= i <= j < ncols and j - i < nrows,
    BAND_BEYOND for 0 <= i <= j < ncols and j - i >= nrows, BAND_OUTSIDE for everything else, for any int64
    values (modle_pixels_band_classify; no device is needed)"""
    if min(int(nrows), int(ncols)) < 0:
        raise PixelsError(ERR_ARG, "band_classify: negative shape")
    keep, p1, p2, n = _anchors(bin1, bin2)
    out = np.zeros(n, dtype=np.uint8)
    rc = lib().modle_pixels_band_classify(int(nrows), int(ncols), int(bin_offset), p1, p2, n,
                                          out.ctypes.data_as(C.POINTER(C.c_uint8)))
    del keep
    if rc != 0:
        raise PixelsError(rc, "band_classify: invalid argument (0 < nrows <= ncols, or both 0; n < 2^31)")
    return out


def _band_call(fn, st, *args):
    """a call of the library that fills the modle_pixels_band_stats `st`: BandStats, or BandListError when the
    list is out of order or holds a negative count"""
    err = C.create_string_buffer(512)
    rc = fn(*args, err, len(err))
    if rc in (ERR_ORDER, ERR_RANGE):
        raise BandListError(rc, err.value.decode(errors="replace"), st.tuple())
    if rc != 0:
        raise PixelsError(rc, err.value.decode(errors="replace"))
    return st.tuple()


def sample_threshold(frac):
    """the threshold of the fraction `frac` of the contacts, floor(frac * 2^32), an int in [0, 2^32]: exact
    in double (a multiplication by a power of two).  ValueError outside [0, 1] and for NaN.  No float goes
    further than this."""
    f = float(frac)
    if not 0.0 <= f <= 1.0:  # (false for NaN)
        raise ValueError(f"sample: the fraction {frac!r} is not in [0, 1]")
    return int(f * 4294967296.0)


def _draw(threshold, seed, salt):
    """the integers of a draw, refused outside their C types (ctypes would wrap them silently)"""
    threshold, seed, salt = int(threshold), int(seed), int(salt)
    if not 0 <= threshold <= 1 << 32:
        raise PixelsError(ERR_ARG, f"sample: the threshold {threshold} is not in [0, 2^32]")
    if not 0 <= seed < 1 << 64 or not 0 <= salt < 1 << 32:
        raise PixelsError(ERR_ARG, f"sample: seed {seed} / salt {salt} is no uint64 / uint32")
    return threshold, seed, salt


def sample_pixels(bin1, bin2, count, threshold, seed, salt=0, bin_offset=0):
    """kept[t] of the host pixels (bin1[t] + bin_offset, bin2[t] + bin_offset) with count[t] contacts, a
    numpy uint32 array: trial t of a pixel is kept when word t & 3 of philox4x32_10((I, J, t >> 2, salt),
    seed) is below `threshold` (sample_threshold) -- the host statement of what the kernel draws, compiled
    from the same function (modle_pixels_sample_pixels; no device is needed)"""
    threshold, seed, salt = _draw(threshold, seed, salt)
    keep, p1, p2, n = _anchors(bin1, bin2)
    cnt = np.asarray(count).reshape(-1)
    if len(cnt) != n:
        raise PixelsError(ERR_ARG, f"sample_pixels: {n} pixels and {len(cnt)} counts")
    if n and (int(cnt.min()) < 0 or int(cnt.max()) >= 1 << 32):
        raise PixelsError(ERR_RANGE, "sample_pixels: a count is no uint32")
    cnt = np.ascontiguousarray(cnt, dtype=np.uint32)
    out = np.zeros(n, dtype=np.uint32)
    u32p = C.POINTER(C.c_uint32)
    rc = lib().modle_pixels_sample_pixels(seed, salt, threshold, int(bin_offset), p1, p2,
                                          cnt.ctypes.data_as(u32p) if n else None, n,
                                          out.ctypes.data_as(u32p) if n else None)
    del keep
    if rc != 0:
        raise PixelsError(rc, "sample_pixels: invalid argument (threshold <= 2^32, ids in [0, 2^32))")
    return out


def _what(what):
    """the mask of a stripes call, refused outside uint64 (ctypes would wrap it silently)"""
    what = int(what)
    if not 0 <= what < 1 << 64:
        raise PixelsError(ERR_ARG, f"stripes: the mask {what} is no uint64")
    return what


def stripes_rows(what):
    """the rows per direction of the mask `what` of STRIPES_MOMENTS (9), STRIPES_MASKED (9) and STRIPES_RANKS (3)
    (modle_pixels_stripes_rows; no device is needed)"""
    rc = lib().modle_pixels_stripes_rows(_what(what))
    if rc < 0:
        raise PixelsError(rc, "stripes_rows: invalid argument (a non-empty mask of MOMENTS 1, MASKED 2, RANKS 4)")
    return rc


def _pearson(n, sa, sb, saa, sbb, sab):
    """(n Sab - Sa Sb) / sqrt((n Saa - Sa^2)(n Sbb - Sb^2)) of Python ints, clipped to [-1, 1]; NaN when the
    product under the root is 0.  Exact up to one division and one root."""
    num = n * sab - sa * sb
    den = (n * saa - sa * sa) * (n * sbb - sb * sb)
    if den == 0:
        return math.nan
    # as the root of num^2 / den, the quotient of two ints, which Python rounds correctly: a stripe against
    # itself (num^2 == den) scores 1.0 exactly, whatever the size of the sums
    return max(-1.0, min(1.0, math.copysign(math.sqrt(num * num / den), num)))


def stripe_scores(rows, metric, masked=False):
    """The scores of the stripes from the integer sums `rows` of one direction, uint64 [rows(what), ncols]
    with the blocks of `what` in bit order (Extractor.stripes(...)[direction], or the sums restated on the
    host): a numpy float64 [ncols].  The one statement of what a score is; every metric is formed in Python
    integers, exactly, up to one final float / math.sqrt / division:
        pearson    (n Sab - Sa Sb) / sqrt((n Saa - Sa^2)(n Sbb - Sb^2)), clipped to [-1, 1]; NaN when the
                   product under the root is 0
        rmse       sqrt((Saa - 2 Sab + Sbb) / n); NaN when n is 0
        eucl_dist  sqrt(Saa - 2 Sab + Sbb)
        spearman   the Pearson formula on (nrows, nrows (nrows + 1), nrows (nrows + 1), Raa, Rbb, Rab), the
                   sums of the doubled average ranks; 1.0 where Sa == 0 or Sb == 0 (a stripe of zeros), as
                   evaluate.compare has it
    `masked`: from the block over the entries where both stripes are non-zero (--exclude-zero-pixels); there
    is no masked spearman (its weighted ranks are not integers: evaluate.compare has it).  Which blocks
    `rows` holds follows from its number of rows: 3 RANKS, 18 MOMENTS | MASKED, 21 all three, and of the two
    masks that 9 and 12 rows leave open the one with MASKED when `masked` is asked for, else the one with
    MOMENTS.  ValueError when the block a metric needs is missing: pearson and the distances need MOMENTS
    (`masked`: MASKED), spearman MOMENTS and RANKS.  No sum can leave the doubles: the largest, the product
    under Pearson's root, is below 2^224."""
    if metric not in STRIPE_METRICS:
        raise ValueError(f"stripe_scores: the metric must be one of {STRIPE_METRICS}")
    rows = np.asarray(rows)
    if rows.ndim != 2 or rows.dtype != np.uint64 or rows.shape[0] not in (3, 9, 12, 18, 21):
        raise ValueError(f"stripe_scores: rows of shape {rows.shape} and type {rows.dtype} are no uint64 "
                         "[rows(what), ncols]")
    if metric == "spearman" and masked:
        raise ValueError("stripe_scores: there is no masked spearman (evaluate.compare forms it on the host)")
    nr = rows.shape[0]
    side = STRIPES_MASKED if masked else STRIPES_MOMENTS
    what = {3: STRIPES_RANKS, 9: side, 12: side | STRIPES_RANKS, 18: 3, 21: 7}[nr]
    need = side | (STRIPES_RANKS if metric == "spearman" else 0)
    if what & need != need:
        raise ValueError(f"stripe_scores: {metric}{' (masked)' if masked else ''} needs the blocks {need} of the "
                         f"mask, the {nr} rows hold {what}")
    at = 9 if masked and what & STRIPES_MOMENTS else 0
    mom = [[int(x) for x in rows[at + k]] for k in range(9)]
    ranks = [[int(x) for x in rows[nr - 3 + k]] for k in range(3)] if metric == "spearman" else None
    out = np.empty(rows.shape[1], dtype=np.float64)
    for c in range(rows.shape[1]):
        n, sa, sb = mom[0][c], mom[1][c], mom[2][c]
        saa, sbb, sab = (mom[k][c] | (mom[k + 1][c] << 64) for k in (3, 5, 7))
        if metric == "pearson":
            out[c] = _pearson(n, sa, sb, saa, sbb, sab)
        elif metric == "spearman":
            # (unmasked moments: n is the depth of the band, and the sum of the doubled ranks n (n + 1))
            out[c] = 1.0 if sa == 0 or sb == 0 else \
                _pearson(n, n * (n + 1), n * (n + 1), ranks[0][c], ranks[1][c], ranks[2][c])
        else:
            ss = saa - 2 * sab + sbb  # the sum of (a - b)^2: never negative
            if metric == "eucl_dist":
                out[c] = math.sqrt(ss)
            else:
                out[c] = math.sqrt(ss / n) if n else math.nan  # (the quotient of two ints is correctly rounded)
    return out


def scc_groups():
    """the workgroups per strip of 64 strata at most that the loaded library was compiled with
    (modle_pixels_scc_groups; no device is needed): 128 unless MODLE_PIXELS_LIB names a test build"""
    return int(lib().modle_pixels_scc_groups())


def _strata(smooth, min_diag, max_diag):
    """the three numbers of an scc call, refused outside uint64 (ctypes would wrap them silently)"""
    got = tuple(int(x) for x in (smooth, min_diag, max_diag))
    if not all(0 <= x < 1 << 64 for x in got):
        raise PixelsError(ERR_ARG, f"scc: smooth, min_diag, max_diag = {got} are no uint64")
    return got


def scc_scores(rows, ncols, min_diag, max_diag, include_zeros=False):
    """(scc, rho, weight): the stratum-adjusted correlation coefficient of HiCRep (Yang et al., Genome Research
    2017) from the integer sums `rows`, uint64 [SCC_ROWS, nrows] (Extractor.scc, or the sums restated on the
    host), of the strata min_diag .. max_diag of two bands of `ncols` bins.  The one statement of what the score
    is, formed in Python integers, exactly, up to a final division and root.  Per stratum d:
        n       rows[0][d], the entries that are non-zero in either matrix; with `include_zeros` all ncols - d
                entries (an entry that is zero in both adds nothing to any sum, so n alone changes)
        rho_d   (n Sab - Sa Sb) / sqrt((n Saa - Sa^2)(n Sbb - Sb^2)), clipped to [-1, 1]; NaN when a variance
                is 0 or n < 2
        w_d     n (1 + 1 / n) (1 - 1 / n) / 12 = (n^2 - 1) / (12 n) for n >= 2, else 0: n times the variance of
                the ranks of n distinct values scaled to (0, 1], HiCRep's variance-stabilised weight
        scc     sum of w_d rho'_d / sum of w_d, rho'_d = rho_d with 0 where it is not finite (such a stratum
                keeps its weight); NaN when the weights add up to 0
    `rho` and `weight` are float64 arrays of max_diag - min_diag + 1 entries; `rho` keeps its NaNs.  The rule is
    modelled on the Python package `hicrep`; where the two differ, what is written here holds."""
    rows = np.asarray(rows)
    ncols, lo, hi = int(ncols), int(min_diag), int(max_diag)
    if rows.ndim != 2 or rows.dtype != np.uint64 or rows.shape[0] != SCC_ROWS:
        raise ValueError(f"scc_scores: rows of shape {rows.shape} and type {rows.dtype} are no uint64 [{SCC_ROWS}, nrows]")
    if not 0 <= lo <= hi < rows.shape[1] or hi >= ncols:
        raise ValueError(f"scc_scores: the strata {lo} .. {hi} are not strata of a band of {rows.shape[1]} diagonals "
                         f"and {ncols} bins")
    rho = np.empty(hi - lo + 1, dtype=np.float64)
    weight = np.empty(hi - lo + 1, dtype=np.float64)
    top, bottom = 0.0, 0.0
    for d in range(lo, hi + 1):
        w = [int(rows[k][d]) for k in range(SCC_ROWS)]
        n = ncols - d if include_zeros else w[0]
        sa, sb, saa, sbb, sab = (w[k] | (w[k + 1] << 64) for k in (1, 3, 5, 7, 9))
        r = _pearson(n, sa, sb, saa, sbb, sab) if n >= 2 else math.nan
        wd = (n * n - 1) / (12 * n) if n >= 2 else 0.0  # (the quotient of two ints is correctly rounded)
        rho[d - lo], weight[d - lo] = r, wd
        top += wd * (r if math.isfinite(r) else 0.0)
        bottom += wd
    return (top / bottom if bottom > 0 else math.nan), rho, weight


PROFILE_RULE = "nrows >= 1, nrows <= ncols, m <= 8, 1 <= K <= 4, d0 >= m, d0 < L_1 < ... < L_K, L_K + m <= nrows"


def stripe_profile_misfit(nrows, ncols, max_offset, lengths, min_diag):
    """None when a stripe-profile call is the accepted one, PROFILE_RULE (include/modle_pixels.h states it for
    the library, this is the one statement on the host; no device and no library is needed), else which part
    of the rule it breaks.  d0 >= m keeps every cell on its own side of the main diagonal, L_K + m <= nrows
    inside the band."""
    nrows, ncols, m, d0 = int(nrows), int(ncols), int(max_offset), int(min_diag)
    ls = [int(x) for x in lengths]
    if not 1 <= nrows <= ncols:
        return f"a band of {nrows} diagonals and {ncols} bins (1 <= nrows <= ncols)"
    if not 0 <= m <= MAX_PROFILE_OFFSET:
        return f"the offset {m} is not in [0, {MAX_PROFILE_OFFSET}]"
    if not 1 <= len(ls) <= MAX_PROFILE_LENGTHS:
        return f"{len(ls)} lengths (1 to {MAX_PROFILE_LENGTHS})"
    if d0 < m:
        return f"min_diag {d0} is below the offset {m}: a cell would cross the main diagonal"
    if any(b <= a for a, b in zip([d0] + ls, ls)):
        return f"min_diag and the lengths {[d0] + ls} do not increase strictly"
    if ls[-1] + m > nrows:
        return f"the length {ls[-1]} with the offset {m} leaves the {nrows} diagonals of the band"
    return None


def _profile_args(max_offset, lengths, min_diag):
    """(m, a ctypes uint64 array or None, K, d0) of a stripe-profile call; what is no uint64 is refused here
    (ctypes would wrap it silently), everything else by the library"""
    m, d0, ls = int(max_offset), int(min_diag), [int(x) for x in lengths]
    if not all(0 <= x < 1 << 64 for x in [m, d0] + ls):
        raise PixelsError(ERR_ARG, f"stripe_profiles: max_offset, min_diag, lengths = {m}, {d0}, {ls} are no uint64")
    return m, ((C.c_uint64 * len(ls))(*ls) if ls else None), len(ls), d0


def stripe_profile_n_valid(ncols, max_offset, lengths, min_diag):
    """the number of cells inside the chromosome behind every word of a stripe profile, numpy uint64
    [2, K, 2 m + 1, ncols] (host only, a closed form): V max(0, min(L_k - 1, c) - d0 + 1), H max(0, min(L_k - 1,
    ncols - 1 - c) - d0 + 1), and 0 where the column or row c + o lies outside [0, ncols)"""
    ncols, m, d0 = int(ncols), int(max_offset), int(min_diag)
    ls = [int(x) for x in lengths]
    if ncols < 0 or m < 0 or d0 < 0 or not ls or any(x < 0 for x in ls):
        raise PixelsError(ERR_ARG, "stripe_profile_n_valid: a negative argument or no length")
    c = np.arange(ncols, dtype=np.int64)
    out = np.zeros((2, len(ls), 2 * m + 1, ncols), dtype=np.uint64)
    for k, length in enumerate(ls):
        up = np.maximum(0, np.minimum(length - 1, c) - d0 + 1)
        down = np.maximum(0, np.minimum(length - 1, ncols - 1 - c) - d0 + 1)
        for o in range(-m, m + 1):
            inside = (c + o >= 0) & (c + o < ncols)
            out[0, k, o + m] = np.where(inside, up, 0)
            out[1, k, o + m] = np.where(inside, down, 0)
    return out


StripeCall = namedtuple("StripeCall", "direction bin k centre n_centre left n_left right n_right")


def stripe_calls(profiles, n_valid, max_offset, lengths, min_diag, half_width=0, fold=STRIPE_FOLD,
                 min_count=STRIPE_MIN_COUNT, radius=STRIPE_RADIUS):
    """The stripes of a band from its profiles (Extractor.stripe_profiles, uint64 [2, K, 2 m + 1, ncols]) and
    stripe_profile_n_valid of the same call: a list of StripeCall, sorted by (direction, bin).  The one statement
    of what a stripe is, in Python integers and Fractions.  For direction (0: the stripe runs upstream of the
    anchor, 1: downstream), length class k and anchor c, with h = `half_width` < m:
        centre   C = the sum over |o| <= h of T[k][o][c], nC its valid cells
        left     Bl = the sum over o < -h, nBl its valid cells; right Br, nBr over o > h
    (direction, k, c) passes when every centre and shoulder cell is valid (every one of the 2 m + 1 words has its
    L_k - d0 cells: no anchor nearer than m to an end, no stripe that runs off the chromosome at that length),
    C >= min_count, and C / nC >= fold * max(Bl / nBl, Br / nBr), compared as cross-multiplied integers.  An
    anchor's call is the largest passing k.  The calls of one direction are thinned to local maxima: a call stays
    unless another call of its direction within `radius` bins has a larger C / nC, or the same and a smaller bin
    (api.cluster_dots' rule in one dimension).  `fold`, `min_count` and `radius` default to STRIPE_FOLD,
    STRIPE_MIN_COUNT, STRIPE_RADIUS: product choices, not measured claims.  A float `fold` means the decimal
    number it prints as."""
    m, h, d0 = int(max_offset), int(half_width), int(min_diag)
    ls = [int(x) for x in lengths]
    prof, nv = np.asarray(profiles), np.asarray(n_valid)
    if prof.ndim != 4 or prof.dtype != np.uint64 or prof.shape[:3] != (2, len(ls), 2 * m + 1) or nv.shape != prof.shape:
        raise ValueError(f"stripe_calls: profiles of shape {prof.shape} and type {prof.dtype} with valid cells of "
                         f"shape {nv.shape} are no uint64 [2, {len(ls)}, {2 * m + 1}, ncols]")
    if not 0 <= h < m:
        raise ValueError(f"stripe_calls: the half width {h} must be below the offset {m}: no shoulder is left")
    fold = Fraction(str(fold)) if isinstance(fold, float) else Fraction(fold)
    min_count, radius = int(min_count), int(radius)
    if fold < 0 or radius < 0:
        raise ValueError(f"stripe_calls: fold {fold} or radius {radius} is negative")
    ncols = prof.shape[3]
    fn, fd = fold.numerator, fold.denominator
    calls = []
    for direction in range(2):
        found = {}  # anchor -> StripeCall of the largest passing k
        for k, length in enumerate(ls):
            t = [[int(x) for x in prof[direction, k, o]] for o in range(2 * m + 1)]
            n = [[int(x) for x in nv[direction, k, o]] for o in range(2 * m + 1)]
            for c in range(ncols):
                if any(n[o][c] != length - d0 for o in range(2 * m + 1)):
                    continue
                centre = sum(t[o][c] for o in range(m - h, m + h + 1))
                left, right = sum(t[o][c] for o in range(m - h)), sum(t[o][c] for o in range(m + h + 1, 2 * m + 1))
                n_centre, n_side = (2 * h + 1) * (length - d0), (m - h) * (length - d0)
                # C / nC >= (fn / fd) * B / nB  <=>  C * nB * fd >= fn * B * nC
                if centre >= min_count and all(centre * n_side * fd >= fn * b * n_centre for b in (left, right)):
                    found[c] = StripeCall(direction, c, k, centre, n_centre, left, n_side, right, n_side)
        kept = sorted(found.values(), key=lambda s: s.bin)
        means = [Fraction(s.centre, s.n_centre) for s in kept]
        for i, s in enumerate(kept):
            beaten = False
            for step in (-1, 1):
                j = i + step
                while 0 <= j < len(kept) and abs(kept[j].bin - s.bin) <= radius and not beaten:
                    beaten = means[j] > means[i] or (means[j] == means[i] and kept[j].bin < s.bin)
                    j += step
            if not beaten:
                calls.append(s)
    return calls


TRIANGLE_RULE = ("no null pointer, 0 < nrows <= ncols, 1 <= max_width <= nrows, max_width <= 65535, "
                 "out_words >= max_width * ncols, an 8-byte aligned output that does not overlap the band")


def _triangle_args(max_width, min_diag):
    """(W, d0) of a triangle call; what is no uint64 is refused here (ctypes would wrap it silently), everything
    else by the library"""
    w, d0 = int(max_width), int(min_diag)
    if not all(0 <= x < 1 << 64 for x in (w, d0)):
        raise PixelsError(ERR_ARG, f"triangles: max_width, min_diag = {w}, {d0} are no uint64")
    return w, d0


def triangle_cells(ncols, max_width, min_diag=0):
    """the number of pixels behind every word of the triangle table, numpy uint64 [max_width, ncols]
    (modle_pixels_triangle_cells; no device is needed): (w' - d0)(w' - d0 + 1) / 2 with w' = min(k + 1, ncols - s),
    0 when w' <= d0"""
    ncols = int(ncols)
    w, d0 = _triangle_args(max_width, min_diag)
    if not 0 <= ncols < 1 << 63:
        raise PixelsError(ERR_ARG, f"triangle_cells: ncols = {ncols} is no column count")
    if not 1 <= w <= MAX_TRIANGLE_WIDTH:  # (before the array is made)
        raise PixelsError(ERR_ARG, f"triangle_cells: invalid argument (1 <= max_width <= {MAX_TRIANGLE_WIDTH})")
    out = np.zeros((w, ncols), dtype=np.uint64)
    rc = lib().modle_pixels_triangle_cells(ncols, w, d0, out.ctypes.data_as(C.POINTER(C.c_uint64)))
    if rc != 0:
        raise PixelsError(rc, f"triangle_cells: invalid argument (1 <= max_width <= {MAX_TRIANGLE_WIDTH})")
    return out


def triangle_sums_host(band, nrows, ncols, max_width, min_diag=0):
    """The triangle table of a band on the host, numpy uint64 [max_width, ncols]: what the tests hold the kernels
    against, and a way to try a score without a device.  It shares no code with the library.  T[k][s] is the sum of
    the pixels (a, c), s <= a <= c < min(s + k + 1, ncols), c - a >= min_diag, of the band `band[c * nrows + (c -
    a)]` (numpy uint32, nrows * ncols words or more).  Formed in uint64, in which the sums are exact (max_width <=
    MAX_TRIANGLE_WIDTH): per column the running sums down the diagonals, the words that are no pixels (d > c)
    masked before they are used; those sums read along the matrix rows; their running sums over the widths.
    ValueError outside 1 <= max_width <= nrows <= ncols."""
    nrows, ncols, w, d0 = int(nrows), int(ncols), int(max_width), int(min_diag)
    if not (1 <= w <= nrows <= ncols and w <= MAX_TRIANGLE_WIDTH and d0 >= 0):
        raise ValueError(f"triangle_sums_host: max_width {w}, min_diag {d0} on a band of {nrows} x {ncols} "
                         f"(1 <= max_width <= nrows <= ncols, max_width <= {MAX_TRIANGLE_WIDTH})")
    words = np.asarray(band).reshape(-1)[:nrows * ncols].reshape(ncols, nrows)[:, :w]
    d, c = np.arange(w, dtype=np.int64)[None, :], np.arange(ncols, dtype=np.int64)[:, None]
    column = np.cumsum(np.where((d >= d0) & (d <= c), words, 0).astype(np.uint64), axis=1, dtype=np.uint64)
    added = np.zeros((w, ncols), dtype=np.uint64)  # what width k + 1 adds to width k at start s: column s + k
    for k in range(w):
        added[k, :ncols - k] = column[k:, k]
    return np.cumsum(added, axis=0, dtype=np.uint64)


DomainCall = namedtuple("DomainCall", "start end width sum cells score strength")


def domain_calls(table, cells, *, gamma=DOMAIN_GAMMA, min_width=DOMAIN_MIN_WIDTH, max_width=None):
    """The domains of a band from its triangle table (Extractor.triangles_to_host, uint64 [W, ncols]) and
    triangle_cells of the same call: a list of DomainCall sorted by start, bins [start, end).  The one statement
    of what a domain is; the project's own rule: modularity against the chromosome's own windows, neither
    Armatus' gamma exponent nor a p-value.  For a width w = k + 1 (min_width <= w <= max_width; None: W) let n_w =
    ncols - w + 1 be the number of windows that lie wholly in the chromosome and, where n_w >= 1,
        mu_w = (the sum of T[k][s] over s < n_w, in Python integers) / n_w      one division, rounded once
        Q(s, w) = float64(T[k][s]) - gamma * mu_w                               the product rounded, then the difference
        strength(s, w) = float64(T[k][s]) / mu_w                                NaN where mu_w == 0
    The called domains are the disjoint windows wholly in the chromosome that maximise the sum of Q; a bin may
    stay outside every domain at a score of 0.  opt[0] = 0, and for e = 1 .. ncols
        opt[e] = max(opt[e - 1], max over w <= e of opt[e - w] + Q(e - w, w)),
    every sum one float64 addition.  Ties: leaving bin e - 1 out wins over any window that only equals it, and of
    equal windows the shorter wins (a candidate replaces the best so far only when it is strictly larger, the
    widths taken upwards); the domains are read back from e = ncols.  Everything is IEEE float64 arithmetic in a
    fixed order, without a fused multiply-add, on integers that a float64 holds exactly: the same table gives the
    same calls on any machine.  ValueError: a table entry at or above 2^53 (refused, not rounded), shapes that do
    not agree, min_width < 1, a gamma that is not finite.  `gamma` and `min_width` default to DOMAIN_GAMMA and
    DOMAIN_MIN_WIDTH: product choices, not measured claims."""
    tab, cel = np.asarray(table), np.asarray(cells)
    if tab.ndim != 2 or tab.dtype != np.uint64 or cel.shape != tab.shape:
        raise ValueError(f"domain_calls: a table of shape {tab.shape} and type {tab.dtype} with cells of shape "
                         f"{cel.shape} are no uint64 [W, ncols]")
    width, ncols = tab.shape
    gamma = float(gamma)
    lo = int(min_width)
    hi = min(width if max_width is None else int(max_width), width, ncols)
    if lo < 1 or not math.isfinite(gamma):
        raise ValueError(f"domain_calls: min_width {lo} is below 1 or gamma {gamma} is not finite")
    if tab.size and int(tab.max()) >= 1 << 53:
        raise ValueError(f"domain_calls: a table entry of {int(tab.max())} is at or above 2^53: a float64 would round it")
    if hi < lo or ncols == 0:
        return []
    ks = np.arange(lo - 1, hi, dtype=np.int64)  # the rows of the table that are asked for, widths upwards
    # (the exact sum of a row: its words are below 2^53, so numpy's uint64 sum of fewer than 2^11 of them cannot wrap)
    totals = [sum(int(tab[k, i:min(i + 2047, ncols - k)].sum(dtype=np.uint64)) for i in range(0, ncols - k, 2047))
              for k in ks]
    mu = np.array([t / (ncols - k) for t, k in zip(totals, ks)], dtype=np.float64)
    gmu = gamma * mu
    opt = np.zeros(ncols + 1, dtype=np.float64)
    choice = np.zeros(ncols + 1, dtype=np.int64)  # the width of the window that ends at e, 0: bin e - 1 is left out
    for e in range(1, ncols + 1):
        fit = ks[:max(0, min(len(ks), e - lo + 1))]  # w = k + 1 <= e
        best, taken = opt[e - 1], 0
        if len(fit):
            cand = opt[e - 1 - fit] + (tab[fit, e - 1 - fit].astype(np.float64) - gmu[:len(fit)])
            i = int(np.argmax(cand))  # (the first of equal ones: the shortest)
            if cand[i] > best:
                best, taken = cand[i], int(fit[i]) + 1
        opt[e], choice[e] = best, taken
    calls, e = [], ncols
    while e > 0:
        w = int(choice[e])
        if w == 0:
            e -= 1
            continue
        s, k = e - w, w - 1
        t, m = int(tab[k, s]), float(mu[k - (lo - 1)])
        calls.append(DomainCall(s, e, w, t, int(cel[k, s]), float(np.float64(t) - gmu[k - (lo - 1)]),
                                float(t) / m if m != 0.0 else math.nan))
        e -= w
    return calls[::-1]


class Extractor:
    """One context of the library on one device (modle_pixels_create)."""

    def __init__(self, device=0):
        self._L = lib()
        self._h = C.c_void_p()
        try:
            _call(self._L.modle_pixels_create, int(device), C.byref(self._h))
        except PixelsError:
            self._h = None
            raise
        self.device = int(device)

    def close(self):
        if self._h:
            h, self._h = self._h, None
            self._L.modle_pixels_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def count(self, d_band, nrows, ncols, d_bin1_offset=None, stream=None):
        """step 1: fills the device array `d_bin1_offset` (int64[ncols + 1], a device pointer; None
        when only the statistics are wanted) and returns Stats; waits for the stream"""
        st = _CStats()
        _call(self._L.modle_pixels_count, self._h, d_band, int(nrows), int(ncols), d_bin1_offset,
              C.byref(st), _stream_ptr(stream))
        return Stats(st.nnz, st.sum, st.max_count)

    def extract_into(self, d_band, nrows, ncols, bin_offset, d_bin1_offset, d_bin1, d_bin2, d_count,
                     nnz, stream=None):
        """step 2: enqueues the extraction into caller-owned device arrays of `nnz` entries"""
        _call(self._L.modle_pixels_extract, self._h, d_band, int(nrows), int(ncols), int(bin_offset),
              d_bin1_offset, d_bin1, d_bin2, d_count, int(nnz), _stream_ptr(stream))

    def _form(self, stem, d_band, nrows, ncols, factor, first_bin, coarse):
        """The one place that chooses between the one-call form modle_pixels_<stem>to_host on the band and
        modle_pixels_coarse_<stem>to_host at `factor` times its bin size: (the C function, its arguments
        from d_band to the analysis' own, shape), where shape() is (nrows, ncols) of the band the analysis
        sees.  `coarse` None: the coarse form unless factor is 1; True, what the coarse_* methods pass:
        always, so that the library refuses a factor of 1."""
        if coarse or (coarse is None and int(factor) != 1):
            return getattr(self._L, f"modle_pixels_coarse_{stem}to_host"), \
                (d_band, int(nrows), int(ncols), int(factor), int(first_bin)), \
                lambda: coarse_shape(nrows, ncols, factor, first_bin)
        return getattr(self._L, f"modle_pixels_{stem}to_host"), (d_band, int(nrows), int(ncols)), \
            lambda: (int(nrows), int(ncols))

    def _to_host(self, fn, shape, *args, stream=None):
        """a one-call form `fn(handle, *args, four array pointers, stats, stream, err)`: the
        context's pinned arrays, copied into numpy arrays the caller owns.  `shape()` is asked
        for the shape of the extracted band once the library has accepted the arguments."""
        p1, p2, pc, po = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        st = _CStats()
        _call(fn, self._h, *args, C.byref(p1), C.byref(p2), C.byref(pc), C.byref(po), C.byref(st),
              _stream_ptr(stream))
        n = int(st.nnz)
        return Pixels(_host_array(p1.value, n, np.int64), _host_array(p2.value, n, np.int64),
                      _host_array(pc.value, n, np.int32), _host_array(po.value, shape()[1] + 1, np.int64),
                      Stats(st.nnz, st.sum, st.max_count))

    def extract(self, d_band, nrows, ncols, bin_offset=0, stream=None, factor=1, first_bin=0, coarse=None):
        """one-call form: Pixels of numpy bin1, bin2 (int64), count (int32), bin1_offset
        (int64[ncols + 1]) and Stats(nnz, sum, max_count).  A count above INT32_MAX raises
        PixelsError(ERR_RANGE).  `factor`, `first_bin`, here and in the four analyses below: of the band
        at `factor` times its bin size, see the coarse_* method."""
        fn, band, shape = self._form("", d_band, nrows, ncols, factor, first_bin, coarse)
        return self._to_host(fn, shape, *band, int(bin_offset), stream=stream)

    def coarsen_into(self, d_band, nrows, ncols, factor, first_bin, d_out, out_words, stream=None):
        """enqueues the coarsening of the band by `factor` into the caller-owned device array
        `d_out` of `out_words` >= nrows' * ncols' + 1 words, all of which are written
        (modle_pixels_coarsen); returns (nrows', ncols')"""
        _call(self._L.modle_pixels_coarsen, self._h, d_band, int(nrows), int(ncols), int(factor),
              int(first_bin), d_out, int(out_words), _stream_ptr(stream))
        return coarse_shape(nrows, ncols, factor, first_bin)

    def coarse_extract(self, d_band, nrows, ncols, factor, first_bin, bin_offset=0, stream=None):
        """one-call form at `factor` times the bin size (modle_pixels_coarse_to_host): what
        extract returns, for the coarse band; bin1_offset has ncols' + 1 entries and `bin_offset`
        counts coarse bins.  A sum above INT32_MAX raises PixelsError(ERR_RANGE)."""
        return self.extract(d_band, nrows, ncols, bin_offset, stream, factor, first_bin, True)

    def dense_tiles_into(self, d_band, nrows, ncols, first, size, step, count, d_out, out_words, stream=None):
        """enqueues the unpacking of `count` square tiles (tile t: the bins first + t * step ..
        + size - 1) into the caller-owned device array `d_out` of `out_words` >= count * size * size
        words, uint32[count][size][size], all of which are written (modle_pixels_dense_tiles)"""
        _call(self._L.modle_pixels_dense_tiles, self._h, d_band, int(nrows), int(ncols), int(first), int(size),
              int(step), int(count), d_out, int(out_words), _stream_ptr(stream))

    def dense(self, d_band, nrows, ncols, lo, hi, stream=None):
        """the symmetric matrix of the bins [lo, hi) as a numpy uint32[hi - lo, hi - lo] the caller
        owns, unpacked on the device (modle_pixels_dense_to_host)"""
        ptr = C.c_void_p()
        _call(self._L.modle_pixels_dense_to_host, self._h, d_band, int(nrows), int(ncols), int(lo), int(hi),
              C.byref(ptr), _stream_ptr(stream))
        n = int(hi) - int(lo)
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint32)), shape=(n, n)).copy()

    def marginals_into(self, d_band, nrows, ncols, min_diag, d_diag_sum, d_coverage, stream=None):
        """enqueues the sums per diagonal into the caller-owned device array `d_diag_sum`
        (uint64[nrows]) and the coverage per bin, without the diagonals below `min_diag`, into
        `d_coverage` (uint64[ncols]); either may be None; every word is written, at any 4-byte
        aligned address (modle_pixels_marginals)"""
        _call(self._L.modle_pixels_marginals, self._h, d_band, int(nrows), int(ncols), int(min_diag), d_diag_sum,
              d_coverage, _stream_ptr(stream))

    def marginals(self, d_band, nrows, ncols, min_diag=0, stream=None, factor=1, first_bin=0, coarse=None):
        """(diag_sum, coverage) as numpy uint64[nrows] and uint64[ncols] the caller owns, summed on
        the device in one pass over the band (modle_pixels_marginals_to_host): diag_sum[d] is the sum
        of diagonal d, coverage[i] the sum of row i of the symmetric matrix without the diagonals
        below `min_diag`"""
        fn, band, shape = self._form("marginals_", d_band, nrows, ncols, factor, first_bin, coarse)
        pd, pc = C.c_void_p(), C.c_void_p()
        _call(fn, self._h, *band, int(min_diag), C.byref(pd), C.byref(pc), _stream_ptr(stream))
        nr, nc = shape()
        return _host_array(pd.value, nr, np.uint64), _host_array(pc.value, nc, np.uint64)

    def coarse_marginals(self, d_band, nrows, ncols, factor, first_bin, min_diag=0, stream=None):
        """`marginals` of the band at `factor` times its bin size, coarsened on the device
        (modle_pixels_coarse_marginals_to_host): uint64[nrows'] and uint64[ncols'] of coarse_shape;
        `min_diag` counts coarse diagonals"""
        return self.marginals(d_band, nrows, ncols, min_diag, stream, factor, first_bin, True)

    def insulation_into(self, d_band, nrows, ncols, windows, min_diag, d_out, out_words, stream=None):
        """enqueues the insulation sums of the `windows` (1 to 8 sizes in bins, 2 * w - 1 <= nrows,
        w <= 1024), without the diagonals below `min_diag`, into the caller-owned device array `d_out`
        (uint64[len(windows)][ncols], 8-byte aligned, `out_words` >= len(windows) * ncols); every word is
        written (modle_pixels_insulation)"""
        ws, n = _windows(windows)
        _call(self._L.modle_pixels_insulation, self._h, d_band, int(nrows), int(ncols), ws, n, int(min_diag), d_out,
              int(out_words), _stream_ptr(stream))

    def insulation(self, d_band, nrows, ncols, windows, min_diag=2, stream=None, factor=1, first_bin=0,
                   coarse=None):
        """the insulation sums as a numpy uint64[len(windows), ncols] the caller owns: for every window
        w and bin b the sum of the pixels (a, c), b - w < a <= b <= c < b + w, c - a >= min_diag, formed
        on the device (modle_pixels_insulation_to_host)"""
        fn, band, shape = self._form("insulation_", d_band, nrows, ncols, factor, first_bin, coarse)
        ws, n = _windows(windows)
        ptr = C.c_void_p()
        _call(fn, self._h, *band, ws, n, int(min_diag), C.byref(ptr), _stream_ptr(stream))
        return _host_array(ptr.value, n * shape()[1], np.uint64).reshape(n, -1)

    def coarse_insulation(self, d_band, nrows, ncols, factor, first_bin, windows, min_diag=2, stream=None):
        """`insulation` of the band at `factor` times its bin size, coarsened on the device
        (modle_pixels_coarse_insulation_to_host): uint64[len(windows), ncols'] of coarse_shape; the
        windows and `min_diag` count coarse bins"""
        return self.insulation(d_band, nrows, ncols, windows, min_diag, stream, factor, first_bin, True)

    def dots_into(self, d_band, nrows, ncols, w, p, min_diag, min_count, scale, d_cand, d_sums, stream=None):
        """enqueues the dot kernel (modle_pixels_dots): into the caller-owned device array `d_cand`
        (uint32[nrows * ncols + 1], the band's layout: the count at a candidate, 0 elsewhere) and / or
        `d_sums` (uint64[4][nrows * ncols], 8-byte aligned: the four neighbourhood sums at a valid pixel,
        0 elsewhere); either may be None, every word of both is written.  `scale`: float64 [4, nrows]
        (dot_scales), None without `d_cand`."""
        keep, ptr = _scale_table(scale, nrows)
        _call(self._L.modle_pixels_dots, self._h, d_band, int(nrows), int(ncols), int(w), int(p), int(min_diag),
              int(min_count), ptr, d_cand, d_sums, _stream_ptr(stream))
        del keep

    def dots(self, d_band, nrows, ncols, w, p, min_diag, min_count, scale, bin_offset=0, stream=None, factor=1,
             first_bin=0, coarse=None):
        """the candidates as Pixels, what extract returns of the candidate band
        (modle_pixels_dots_to_host)"""
        fn, band, shape = self._form("dots_", d_band, nrows, ncols, factor, first_bin, coarse)
        keep, ptr = _scale_table(scale, shape()[0])
        return self._to_host(fn, shape, *band, int(w), int(p), int(min_diag), int(min_count), ptr, int(bin_offset),
                             stream=stream)

    def coarse_dots(self, d_band, nrows, ncols, factor, first_bin, w, p, min_diag, min_count, scale, bin_offset=0,
                    stream=None):
        """`dots` of the band at `factor` times its bin size, coarsened on the device
        (modle_pixels_coarse_dots_to_host): `w`, `p`, `min_diag` count coarse bins, `scale` is
        float64 [4, nrows'] of coarse_shape and `bin_offset` counts coarse bins"""
        return self.dots(d_band, nrows, ncols, w, p, min_diag, min_count, scale, bin_offset, stream, factor,
                         first_bin, True)

    def dot_hist_into(self, d_band, nrows, ncols, w, p, min_diag, lam, edges, n_obs, d_hist, stream=None):
        """enqueues the lambda-chunk histogram (modle_pixels_dot_hist): ADDS, for every valid pixel and every
        neighbourhood k, one to the caller-owned device array `d_hist` (uint64[4][len(edges) + 1][n_obs], 8-byte
        aligned, zeroed by the caller before the first band) at [k][chunk of O_k * lam[k][d]][min(count,
        n_obs - 1)].  `lam`: float64 [4, nrows] (dot_scales with folds of 1); `edges`: None for HiCCUPS'."""
        keep, ptr = _scale_table(lam, nrows)
        e, eptr, n_edges = _edge_table(edges)
        _call(self._L.modle_pixels_dot_hist, self._h, d_band, int(nrows), int(ncols), int(w), int(p), int(min_diag),
              ptr, eptr, n_edges, int(n_obs), d_hist, _stream_ptr(stream))
        del keep, e

    def dot_hist(self, d_band, nrows, ncols, w, p, min_diag, lam, edges, n_obs, stream=None, factor=1, first_bin=0,
                 coarse=None):
        """the lambda-chunk histogram of the band alone as a numpy uint64 [4, len(edges) + 1, n_obs] the caller
        owns (modle_pixels_dot_hist_to_host)"""
        fn, band, shape = self._form("dot_hist_", d_band, nrows, ncols, factor, first_bin, coarse)
        keep, ptr = _scale_table(lam, shape()[0])
        e, eptr, n_edges = _edge_table(edges)
        out = C.c_void_p()
        _call(fn, self._h, *band, int(w), int(p), int(min_diag), ptr, eptr, n_edges, int(n_obs), C.byref(out),
              _stream_ptr(stream))
        del keep, e
        return _host_array(out.value, 4 * (n_edges + 1) * int(n_obs), np.uint64).reshape(4, n_edges + 1, int(n_obs))

    def coarse_dot_hist(self, d_band, nrows, ncols, factor, first_bin, w, p, min_diag, lam, edges, n_obs,
                        stream=None):
        """`dot_hist` of the band at `factor` times its bin size, coarsened on the device
        (modle_pixels_coarse_dot_hist_to_host): `w`, `p`, `min_diag` count coarse bins, `lam` is float64
        [4, nrows'] of coarse_shape"""
        return self.dot_hist(d_band, nrows, ncols, w, p, min_diag, lam, edges, n_obs, stream, factor, first_bin, True)

    def dots_fdr_into(self, d_band, nrows, ncols, w, p, min_diag, min_count, lam, edges, thresholds, scale, d_cand,
                      stream=None):
        """enqueues the threshold decision (modle_pixels_dots_fdr) into the caller-owned device array `d_cand`
        (uint32[nrows * ncols + 1], every word written): the count where a valid pixel has count >= min_count,
        clears the non-zero threshold `thresholds[k][chunk of O_k * lam[k][d]]` (uint32 [4, len(edges) + 1],
        dot_thresholds) for every k and, with a `scale` table (dot_scales; or None), passes the fold test too."""
        keep, ptr = _scale_table(lam, nrows)
        e, eptr, n_edges = _edge_table(edges)
        t, tptr = _thr_table(thresholds, n_edges)
        keep_s, sptr = _scale_table(scale, nrows)
        _call(self._L.modle_pixels_dots_fdr, self._h, d_band, int(nrows), int(ncols), int(w), int(p), int(min_diag),
              int(min_count), ptr, eptr, n_edges, tptr, sptr, d_cand, _stream_ptr(stream))
        del keep, e, t, keep_s

    def dots_fdr(self, d_band, nrows, ncols, w, p, min_diag, min_count, lam, edges, thresholds, scale=None,
                 bin_offset=0, stream=None, factor=1, first_bin=0, coarse=None):
        """the candidates of the threshold decision as Pixels (modle_pixels_dots_fdr_to_host)"""
        fn, band, shape = self._form("dots_fdr_", d_band, nrows, ncols, factor, first_bin, coarse)
        keep, ptr = _scale_table(lam, shape()[0])
        e, eptr, n_edges = _edge_table(edges)
        t, tptr = _thr_table(thresholds, n_edges)
        keep_s, sptr = _scale_table(scale, shape()[0])
        return self._to_host(fn, shape, *band, int(w), int(p), int(min_diag), int(min_count), ptr, eptr, n_edges, tptr,
                             sptr, int(bin_offset), stream=stream)

    def coarse_dots_fdr(self, d_band, nrows, ncols, factor, first_bin, w, p, min_diag, min_count, lam, edges,
                        thresholds, scale=None, bin_offset=0, stream=None):
        """`dots_fdr` of the band at `factor` times its bin size, coarsened on the device
        (modle_pixels_coarse_dots_fdr_to_host)"""
        return self.dots_fdr(d_band, nrows, ncols, w, p, min_diag, min_count, lam, edges, thresholds, scale,
                             bin_offset, stream, factor, first_bin, True)

    def pileup_into(self, d_band, nrows, ncols, flank, d_bin1, d_bin2, n, d_pile, d_n_used=None, bin_offset=0,
                    stream=None):
        """enqueues the pileup of the `n` anchors in the device arrays `d_bin1`, `d_bin2` (int64) into the
        caller-owned device arrays `d_pile` (uint64[2 * flank + 1][2 * flank + 1]) and `d_n_used`
        (uint64[1], or None), both 8-byte aligned; every word is written (modle_pixels_pileup)"""
        _call(self._L.modle_pixels_pileup, self._h, d_band, int(nrows), int(ncols), _flank(flank), int(bin_offset),
              d_bin1, d_bin2, int(n), d_pile, d_n_used, _stream_ptr(stream))

    def pileup(self, d_band, nrows, ncols, flank, bin1, bin2, bin_offset=0, stream=None, factor=1, first_bin=0,
               coarse=None):
        """(pile, n_used): the sum of the (2 * flank + 1)^2 windows of the symmetric matrix around the
        accepted ones of the host anchors (bin1[t] - bin_offset, bin2[t] - bin_offset), numpy
        uint64[S, S], and how many were accepted (pileup_accepts), summed on the device
        (modle_pixels_pileup_to_host)"""
        fn, band, _ = self._form("pileup_", d_band, nrows, ncols, factor, first_bin, coarse)
        keep, p1, p2, n = _anchors(bin1, bin2)
        pp, pn = C.c_void_p(), C.c_void_p()
        _call(fn, self._h, *band, _flank(flank), int(bin_offset), p1, p2, n, C.byref(pp), C.byref(pn),
              _stream_ptr(stream))
        del keep
        s = 2 * int(flank) + 1
        return _host_array(pp.value, s * s, np.uint64).reshape(s, s), int(_host_array(pn.value, 1, np.uint64)[0])

    def coarse_pileup(self, d_band, nrows, ncols, factor, first_bin, flank, bin1, bin2, bin_offset=0, stream=None):
        """`pileup` of the band at `factor` times its bin size, coarsened on the device
        (modle_pixels_coarse_pileup_to_host): `flank` and the anchors count coarse bins"""
        return self.pileup(d_band, nrows, ncols, flank, bin1, bin2, bin_offset, stream, factor, first_bin, True)

    def rescale_into(self, d_band, nrows, ncols, size, d_start, d_end, n, d_pile, d_area=None, d_n_used=None,
                     bin_offset=0, stream=None):
        """enqueues the rescaled pileup of the `n` windows in the device arrays `d_start`, `d_end` (int64) into
        the caller-owned device arrays `d_pile` (uint64[size][size]), `d_area` (the same, or None) and
        `d_n_used` (uint64[1], or None), all 8-byte aligned; every word is written (modle_pixels_rescale)"""
        _call(self._L.modle_pixels_rescale, self._h, d_band, int(nrows), int(ncols), _size(size), int(bin_offset),
              d_start, d_end, int(n), d_pile, d_area, d_n_used, _stream_ptr(stream))

    def rescale(self, d_band, nrows, ncols, size, start, end, bin_offset=0, stream=None, factor=1, first_bin=0,
                coarse=None):
        """(pile, area, n_used): the accepted ones (rescale_accepts) of the host windows
        [start[t] - bin_offset, end[t] - bin_offset) of the symmetric matrix, each cut into size x size blocks
        and the blocks summed, numpy uint64[size, size]; how many source pixels every cell took; and how many
        windows were accepted, summed on the device (modle_pixels_rescale_to_host).  pile / area is the pooled
        mean of a cell: large windows weigh more."""
        fn, band, _ = self._form("rescale_", d_band, nrows, ncols, factor, first_bin, coarse)
        keep, p1, p2, n = _anchors(start, end)
        pp, pa, pn = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _call(fn, self._h, *band, _size(size), int(bin_offset), p1, p2, n, C.byref(pp), C.byref(pa), C.byref(pn),
              _stream_ptr(stream))
        del keep
        r = int(size)
        return _host_array(pp.value, r * r, np.uint64).reshape(r, r), \
            _host_array(pa.value, r * r, np.uint64).reshape(r, r), int(_host_array(pn.value, 1, np.uint64)[0])

    def coarse_rescale(self, d_band, nrows, ncols, factor, first_bin, size, start, end, bin_offset=0, stream=None):
        """`rescale` of the band at `factor` times its bin size, coarsened on the device
        (modle_pixels_coarse_rescale_to_host): the windows count coarse bins"""
        return self.rescale(d_band, nrows, ncols, size, start, end, bin_offset, stream, factor, first_bin, True)

    def sample_into(self, d_band, nrows, ncols, threshold, seed, stats, d_kept, d_rest=None, salt=0, bin_offset=0,
                    stream=None):
        """enqueues the sampling of the band (modle_pixels_sample): of the n contacts of pixel (i, j) those
        trials t are kept whose Philox word, keyed by (i + bin_offset, j + bin_offset, t, salt) and `seed`,
        is below `threshold` (sample_threshold).  The kept counts go to the caller-owned device array
        `d_kept`, the others to `d_rest` (uint32[nrows * ncols + 1] each, the band's layout; either may be
        None); every word is written.  `stats`: the Stats of the same band from count(); a sum above
        MAX_SAMPLE_TRIALS raises PixelsError(ERR_RANGE)."""
        threshold, seed, salt = _draw(threshold, seed, salt)
        st = None if stats is None else _CStats(int(stats.nnz), int(stats.sum), int(stats.max_count), 0)
        _call(self._L.modle_pixels_sample, self._h, d_band, int(nrows), int(ncols), int(bin_offset), threshold, seed,
              salt, None if st is None else C.byref(st), d_kept, d_rest, _stream_ptr(stream))

    def sample(self, d_band, nrows, ncols, threshold, seed, salt=0, bin_offset=0, rest=False, stream=None):
        """the kept contacts of the band (`rest`: the others) as Pixels, what extract returns of the sampled
        band: counted, sampled into a scratch band of the context and extracted on the device
        (modle_pixels_sample_to_host).  The total is binomial around threshold / 2^32 of the band's sum."""
        threshold, seed, salt = _draw(threshold, seed, salt)
        return self._to_host(self._L.modle_pixels_sample_to_host, lambda: (int(nrows), int(ncols)), d_band, int(nrows), int(ncols),
                             int(bin_offset), threshold, seed, salt, SAMPLE_REST if rest else SAMPLE_KEPT,
                             stream=stream)


    def band_check(self, d_bin1, d_bin2, d_count, n, nrows, ncols, bin_offset=0, d_row_start=None, stream=None):
        """step 1 of pixels to band: one pass over the `n` pixels in the device arrays `d_bin1`, `d_bin2` (int64)
        and `d_count` (int32) -- class, order, sign and the sums -- and the fill of the device array
        `d_row_start` (int64[ncols + 1]; None when only the statistics are wanted).  Returns BandStats; a list
        that is not strictly increasing in (bin1, bin2) or holds a negative count raises BandListError (ERR_ORDER,
        ERR_RANGE) with the statistics.  Waits for the stream (modle_pixels_band_check)."""
        st = _CBandStats()
        return _band_call(self._L.modle_pixels_band_check, st, self._h, d_bin1, d_bin2, d_count, int(n), int(nrows),
                          int(ncols), int(bin_offset), d_row_start, C.byref(st), _stream_ptr(stream))

    def band_fill_into(self, d_bin2, d_count, n, nrows, ncols, bin_offset, d_row_start, d_out, out_words, stream=None):
        """step 2: enqueues the fill of the caller-owned device array `d_out` (uint32[nrows * ncols + 1], the
        band's layout) from the pixels band_check accepted and the row starts it wrote; every word is written,
        none outside (modle_pixels_band_fill)"""
        _call(self._L.modle_pixels_band_fill, self._h, d_bin2, d_count, int(n), int(nrows), int(ncols),
              int(bin_offset), d_row_start, d_out, int(out_words), _stream_ptr(stream))

    def band_from_host(self, bin1, bin2, count, nrows, ncols, bin_offset, d_out, out_words, stream=None):
        """host pixels (int64 ids, int32 counts) up, checked and scattered into the device array `d_out`
        (uint32[nrows * ncols + 1]); returns BandStats, raises BandListError with nothing written.  Waits
        (modle_pixels_band_from_host)."""
        keep, p1, p2, n = _anchors(bin1, bin2)
        cnt = np.ascontiguousarray(count, dtype=np.int32).reshape(-1)
        if len(cnt) != n:
            raise PixelsError(ERR_ARG, f"band_from_host: {n} pixels and {len(cnt)} counts")
        st = _CBandStats()
        i64 = lambda a: a.ctypes.data if n else None
        out = _band_call(self._L.modle_pixels_band_from_host, st, self._h, i64(keep[0]), i64(keep[1]), i64(cnt), n,
                         int(nrows), int(ncols), int(bin_offset), d_out, int(out_words), C.byref(st),
                         _stream_ptr(stream))
        del keep
        return out

    def stripes_into(self, d_ref, d_tgt, nrows, ncols, what, d_out, out_words, stream=None):
        """enqueues the comparison of the bands at `d_ref` and `d_tgt` (one shape; they may be the same) stripe
        by stripe into the caller-owned device array `d_out` (uint64[2][stripes_rows(what)][ncols], 8-byte
        aligned, `out_words` == 2 * rows * ncols): per direction (vertical, horizontal) and bin the moments
        (STRIPES_MOMENTS), the moments over the entries where both are non-zero (STRIPES_MASKED) and the
        rank sums (STRIPES_RANKS; nrows <= MAX_STRIPE); every word is written (modle_pixels_stripes)"""
        _call(self._L.modle_pixels_stripes, self._h, d_ref, d_tgt, int(nrows), int(ncols), _what(what), d_out,
              int(out_words), _stream_ptr(stream))

    def stripes(self, d_ref, d_tgt, nrows, ncols, what=STRIPES_MOMENTS, stream=None):
        """the sums of stripes_into as a numpy uint64[2, stripes_rows(what), ncols] the caller owns, formed on
        the device (modle_pixels_stripes_to_host); stripe_scores turns a direction of it into scores"""
        ptr = C.c_void_p()
        _call(self._L.modle_pixels_stripes_to_host, self._h, d_ref, d_tgt, int(nrows), int(ncols), _what(what),
              C.byref(ptr), _stream_ptr(stream))
        rows = stripes_rows(what)
        return _host_array(ptr.value, 2 * rows * int(ncols), np.uint64).reshape(2, rows, int(ncols))

    def scc_into(self, d_ref, d_tgt, nrows, ncols, smooth, min_diag, max_diag, d_out, out_words, stream=None):
        """enqueues the comparison of the bands at `d_ref` and `d_tgt` (one shape; they may be the same)
        diagonal by diagonal into the caller-owned device array `d_out` (uint64[SCC_ROWS][nrows], 8-byte aligned,
        `out_words` == SCC_ROWS * nrows): per stratum min_diag <= d <= max_diag of the matrices smoothed by a box
        of half-width `smooth` <= MAX_SCC_SMOOTH (max_diag + 2 * smooth <= nrows - 1) n and the 128-bit sums of
        a, b, a * a, b * b and a * b; the other columns hold 0; every word is written (modle_pixels_scc)"""
        _call(self._L.modle_pixels_scc, self._h, d_ref, d_tgt, int(nrows), int(ncols),
              *_strata(smooth, min_diag, max_diag), d_out, int(out_words), _stream_ptr(stream))

    def scc(self, d_ref, d_tgt, nrows, ncols, smooth=0, min_diag=1, max_diag=None, stream=None):
        """the sums of scc_into as a numpy uint64[SCC_ROWS, nrows] the caller owns, formed on the device
        (modle_pixels_scc_to_host); `max_diag` None: the widest the band allows, nrows - 1 - 2 * smooth;
        scc_scores turns it into the score"""
        if max_diag is None:
            max_diag = int(nrows) - 1 - 2 * int(smooth)
        ptr = C.c_void_p()
        _call(self._L.modle_pixels_scc_to_host, self._h, d_ref, d_tgt, int(nrows), int(ncols),
              *_strata(smooth, min_diag, max_diag), C.byref(ptr), _stream_ptr(stream))
        return _host_array(ptr.value, SCC_ROWS * int(nrows), np.uint64).reshape(SCC_ROWS, int(nrows))

    def stripe_profiles_into(self, d_band, nrows, ncols, max_offset, lengths, min_diag, d_out, out_words, stream=None):
        """enqueues the stripe profiles of the band into the caller-owned device array `d_out` (uint64[2][K][2 m +
        1][ncols], 8-byte aligned, `out_words` == 2 * K * (2 m + 1) * ncols): per direction (0 V, the stripe
        upstream of the anchor; 1 H, downstream), length L_k and offset o in [-m, m] the sum of the stripe's cells
        at the distances min_diag <= d < L_k, seen o bins to the side; PROFILE_RULE is the accepted call; every
        word is written (modle_pixels_stripe_profiles)"""
        m, ls, n, d0 = _profile_args(max_offset, lengths, min_diag)
        _call(self._L.modle_pixels_stripe_profiles, self._h, d_band, int(nrows), int(ncols), m, ls, n, d0, d_out,
              int(out_words), _stream_ptr(stream))

    def stripe_profiles(self, d_band, nrows, ncols, max_offset, lengths, min_diag, stream=None, factor=1, first_bin=0,
                        coarse=None):
        """the sums of stripe_profiles_into as a numpy uint64[2, K, 2 m + 1, ncols] the caller owns, formed on the
        device (modle_pixels_stripe_profiles_to_host); stripe_calls turns them into calls"""
        fn, band, shape = self._form("stripe_profiles_", d_band, nrows, ncols, factor, first_bin, coarse)
        m, ls, n, d0 = _profile_args(max_offset, lengths, min_diag)
        ptr = C.c_void_p()
        _call(fn, self._h, *band, m, ls, n, d0, C.byref(ptr), _stream_ptr(stream))
        nc = shape()[1]
        return _host_array(ptr.value, 2 * n * (2 * m + 1) * nc, np.uint64).reshape(2, n, 2 * m + 1, nc)

    def coarse_stripe_profiles(self, d_band, nrows, ncols, factor, first_bin, max_offset, lengths, min_diag,
                               stream=None):
        """`stripe_profiles` of the band at `factor` times its bin size, coarsened on the device
        (modle_pixels_coarse_stripe_profiles_to_host): uint64[2, K, 2 m + 1, ncols'] of coarse_shape; the lengths,
        the offset and `min_diag` count coarse bins, and PROFILE_RULE holds against nrows'"""
        return self.stripe_profiles(d_band, nrows, ncols, max_offset, lengths, min_diag, stream, factor, first_bin, True)

    def triangles_into(self, d_band, nrows, ncols, max_width, min_diag, d_out, out_words, stream=None):
        """enqueues the triangle table of the band into the caller-owned device array `d_out` (uint64[max_width]
        [ncols], 8-byte aligned, `out_words` >= max_width * ncols): T[k][s] the sum of the pixels inside the window of
        k + 1 bins that starts at bin s, without the diagonals below `min_diag`; TRIANGLE_RULE is the accepted call;
        every word is written (modle_pixels_triangles)"""
        w, d0 = _triangle_args(max_width, min_diag)
        _call(self._L.modle_pixels_triangles, self._h, d_band, int(nrows), int(ncols), w, d0, d_out, int(out_words),
              _stream_ptr(stream))

    def triangles_to_host(self, d_band, nrows, ncols, max_width, min_diag=0, stream=None, factor=1, first_bin=0,
                          coarse=None):
        """the table of triangles_into as a numpy uint64[max_width, ncols] the caller owns, formed on the device
        (modle_pixels_triangles_to_host); domain_calls turns it into calls"""
        fn, band, shape = self._form("triangles_", d_band, nrows, ncols, factor, first_bin, coarse)
        w, d0 = _triangle_args(max_width, min_diag)
        ptr = C.c_void_p()
        _call(fn, self._h, *band, w, d0, C.byref(ptr), _stream_ptr(stream))
        nc = shape()[1]
        return _host_array(ptr.value, w * nc, np.uint64).reshape(w, nc)

    def coarse_triangles_to_host(self, d_band, nrows, ncols, factor, first_bin, max_width, min_diag=0, stream=None):
        """`triangles_to_host` of the band at `factor` times its bin size, coarsened on the device
        (modle_pixels_coarse_triangles_to_host): uint64[max_width, ncols'] of coarse_shape; the widths and
        `min_diag` count coarse bins, and TRIANGLE_RULE holds against nrows'"""
        return self.triangles_to_host(d_band, nrows, ncols, max_width, min_diag, stream, factor, first_bin, True)


def extractor(device=0):
    """the process-wide context of `device`"""
    ex = _EXTRACTORS.get(int(device))
    if ex is None or not ex._h:
        ex = _EXTRACTORS[int(device)] = Extractor(device)
    return ex


def extract(d_band, nrows, ncols, bin_offset=0, stream=None, device=0):
    """Pixels of the band at device pointer `d_band` (uint32, layout of modle_hip_interval_outputs;
    e.g. a torch tensor's data_ptr()): returns bin1, bin2, count, bin1_offset, stats."""
    return extractor(device).extract(d_band, nrows, ncols, bin_offset, stream)


def coarse_extract(d_band, nrows, ncols, factor, first_bin, bin_offset=0, stream=None, device=0):
    """Pixels of the band at device pointer `d_band` at `factor` times its bin size, coarsened and
    extracted on the device: returns bin1, bin2, count, bin1_offset, stats."""
    return extractor(device).coarse_extract(d_band, nrows, ncols, factor, first_bin, bin_offset, stream)


def dense_tiles_into(d_band, nrows, ncols, first, size, step, count, d_out, out_words, stream=None, device=0):
    """`count` square tiles of the band at device pointer `d_band`, unpacked into the device array
    `d_out` (uint32[count][size][size]); enqueued on `stream`, nothing crosses to the host."""
    extractor(device).dense_tiles_into(d_band, nrows, ncols, first, size, step, count, d_out, out_words, stream)


def dense(d_band, nrows, ncols, lo, hi, stream=None, device=0):
    """The symmetric matrix of the bins [lo, hi) of the band at device pointer `d_band`: numpy
    uint32[hi - lo, hi - lo], unpacked on the device."""
    return extractor(device).dense(d_band, nrows, ncols, lo, hi, stream)


def marginals_into(d_band, nrows, ncols, min_diag, d_diag_sum, d_coverage, stream=None, device=0):
    """The sums per diagonal and the coverage per bin of the band at device pointer `d_band`, into
    the device arrays `d_diag_sum` (uint64[nrows]) and `d_coverage` (uint64[ncols]; either may be
    None); enqueued on `stream`, nothing crosses to the host."""
    extractor(device).marginals_into(d_band, nrows, ncols, min_diag, d_diag_sum, d_coverage, stream)


def marginals(d_band, nrows, ncols, min_diag=0, stream=None, device=0):
    """(diag_sum, coverage) of the band at device pointer `d_band`: numpy uint64[nrows] and
    uint64[ncols], summed on the device."""
    return extractor(device).marginals(d_band, nrows, ncols, min_diag, stream)


def coarse_marginals(d_band, nrows, ncols, factor, first_bin, min_diag=0, stream=None, device=0):
    """(diag_sum, coverage) of the band at device pointer `d_band` at `factor` times its bin size,
    coarsened and summed on the device."""
    return extractor(device).coarse_marginals(d_band, nrows, ncols, factor, first_bin, min_diag, stream)


def insulation_into(d_band, nrows, ncols, windows, min_diag, d_out, out_words, stream=None, device=0):
    """The insulation sums of the band at device pointer `d_band` for the `windows` (bins), into the
    device array `d_out` (uint64[len(windows)][ncols]); enqueued on `stream`, nothing crosses to the
    host."""
    extractor(device).insulation_into(d_band, nrows, ncols, windows, min_diag, d_out, out_words, stream)


def insulation(d_band, nrows, ncols, windows, min_diag=2, stream=None, device=0):
    """The insulation sums of the band at device pointer `d_band`: numpy uint64[len(windows), ncols],
    formed on the device."""
    return extractor(device).insulation(d_band, nrows, ncols, windows, min_diag, stream)


def coarse_insulation(d_band, nrows, ncols, factor, first_bin, windows, min_diag=2, stream=None, device=0):
    """The insulation sums of the band at device pointer `d_band` at `factor` times its bin size,
    coarsened and summed on the device."""
    return extractor(device).coarse_insulation(d_band, nrows, ncols, factor, first_bin, windows, min_diag, stream)


def dots_into(d_band, nrows, ncols, w, p, min_diag, min_count, scale, d_cand, d_sums, stream=None, device=0):
    """The dot kernel on the band at device pointer `d_band`, into the device arrays `d_cand` and / or
    `d_sums`; enqueued on `stream`, nothing crosses to the host but the scale table."""
    extractor(device).dots_into(d_band, nrows, ncols, w, p, min_diag, min_count, scale, d_cand, d_sums, stream)


def dots(d_band, nrows, ncols, w, p, min_diag, min_count, scale, bin_offset=0, stream=None, device=0):
    """The dot candidates of the band at device pointer `d_band` as Pixels, found on the device."""
    return extractor(device).dots(d_band, nrows, ncols, w, p, min_diag, min_count, scale, bin_offset, stream)


def coarse_dots(d_band, nrows, ncols, factor, first_bin, w, p, min_diag, min_count, scale, bin_offset=0,
                stream=None, device=0):
    """The dot candidates of the band at device pointer `d_band` at `factor` times its bin size,
    coarsened and found on the device."""
    return extractor(device).coarse_dots(d_band, nrows, ncols, factor, first_bin, w, p, min_diag, min_count, scale,
                                         bin_offset, stream)


def pileup_into(d_band, nrows, ncols, flank, d_bin1, d_bin2, n, d_pile, d_n_used=None, bin_offset=0, stream=None,
                device=0):
    """The pileup of the band at device pointer `d_band` around `n` anchors in device arrays, into the
    device arrays `d_pile` and `d_n_used`; enqueued on `stream`, nothing crosses to the host."""
    extractor(device).pileup_into(d_band, nrows, ncols, flank, d_bin1, d_bin2, n, d_pile, d_n_used, bin_offset, stream)


def pileup(d_band, nrows, ncols, flank, bin1, bin2, bin_offset=0, stream=None, device=0):
    """(pile, n_used) of the band at device pointer `d_band` around host anchors: numpy uint64[S, S] and
    an int, summed on the device."""
    return extractor(device).pileup(d_band, nrows, ncols, flank, bin1, bin2, bin_offset, stream)


def coarse_pileup(d_band, nrows, ncols, factor, first_bin, flank, bin1, bin2, bin_offset=0, stream=None, device=0):
    """(pile, n_used) of the band at device pointer `d_band` at `factor` times its bin size, coarsened
    and summed on the device."""
    return extractor(device).coarse_pileup(d_band, nrows, ncols, factor, first_bin, flank, bin1, bin2, bin_offset,
                                           stream)


def rescale_into(d_band, nrows, ncols, size, d_start, d_end, n, d_pile, d_area=None, d_n_used=None, bin_offset=0,
                 stream=None, device=0):
    """The rescaled pileup of the band at device pointer `d_band` over `n` windows in device arrays, into the
    device arrays `d_pile`, `d_area` and `d_n_used`: see Extractor.rescale_into."""
    extractor(device).rescale_into(d_band, nrows, ncols, size, d_start, d_end, n, d_pile, d_area, d_n_used, bin_offset,
                                   stream)


def rescale(d_band, nrows, ncols, size, start, end, bin_offset=0, stream=None, device=0):
    """(pile, area, n_used) of the rescaled pileup of the band at device pointer `d_band` over host windows:
    see Extractor.rescale."""
    return extractor(device).rescale(d_band, nrows, ncols, size, start, end, bin_offset, stream)


def coarse_rescale(d_band, nrows, ncols, factor, first_bin, size, start, end, bin_offset=0, stream=None, device=0):
    """(pile, area, n_used) of the band at `factor` times its bin size: see Extractor.coarse_rescale."""
    return extractor(device).coarse_rescale(d_band, nrows, ncols, factor, first_bin, size, start, end, bin_offset,
                                            stream)


def sample_into(d_band, nrows, ncols, threshold, seed, stats, d_kept, d_rest=None, salt=0, bin_offset=0, stream=None,
                device=0):
    """The band at device pointer `d_band` thinned into the device arrays `d_kept` and / or `d_rest`;
    enqueued on `stream`, nothing crosses to the host."""
    extractor(device).sample_into(d_band, nrows, ncols, threshold, seed, stats, d_kept, d_rest, salt, bin_offset,
                                  stream)


def sample(d_band, nrows, ncols, threshold, seed, salt=0, bin_offset=0, rest=False, stream=None, device=0):
    """The kept contacts (`rest`: the others) of the band at device pointer `d_band` as Pixels, sampled and
    extracted on the device."""
    return extractor(device).sample(d_band, nrows, ncols, threshold, seed, salt, bin_offset, rest, stream)


def band_check(d_bin1, d_bin2, d_count, n, nrows, ncols, bin_offset=0, d_row_start=None, stream=None, device=0):
    """BandStats of the `n` pixels in device arrays against a band of the given shape, and their row starts into
    the device array `d_row_start`; waits."""
    return extractor(device).band_check(d_bin1, d_bin2, d_count, n, nrows, ncols, bin_offset, d_row_start, stream)


def band_fill_into(d_bin2, d_count, n, nrows, ncols, bin_offset, d_row_start, d_out, out_words, stream=None, device=0):
    """The band of the checked pixels, scattered into the device array `d_out`; enqueued on `stream`, nothing
    crosses to the host."""
    extractor(device).band_fill_into(d_bin2, d_count, n, nrows, ncols, bin_offset, d_row_start, d_out, out_words,
                                     stream)


def band_from_host(bin1, bin2, count, nrows, ncols, bin_offset, d_out, out_words, stream=None, device=0):
    """The band of host pixels in the device array `d_out`: copied up, checked and scattered on the device;
    returns BandStats."""
    return extractor(device).band_from_host(bin1, bin2, count, nrows, ncols, bin_offset, d_out, out_words, stream)


def stripes_into(d_ref, d_tgt, nrows, ncols, what, d_out, out_words, stream=None, device=0):
    """The sums of the stripes of the bands at device pointers `d_ref` and `d_tgt`, into the device array `d_out`
    (uint64[2][stripes_rows(what)][ncols]); enqueued on `stream`, nothing crosses to the host."""
    extractor(device).stripes_into(d_ref, d_tgt, nrows, ncols, what, d_out, out_words, stream)


def stripes(d_ref, d_tgt, nrows, ncols, what=STRIPES_MOMENTS, stream=None, device=0):
    """The sums of the stripes of the bands at device pointers `d_ref` and `d_tgt`: numpy uint64[2,
    stripes_rows(what), ncols], formed on the device."""
    return extractor(device).stripes(d_ref, d_tgt, nrows, ncols, what, stream)


def scc_into(d_ref, d_tgt, nrows, ncols, smooth, min_diag, max_diag, d_out, out_words, stream=None, device=0):
    """The sums of the strata of the bands at device pointers `d_ref` and `d_tgt`, into the device array `d_out`
    (uint64[SCC_ROWS][nrows]); enqueued on `stream`, nothing crosses to the host."""
    extractor(device).scc_into(d_ref, d_tgt, nrows, ncols, smooth, min_diag, max_diag, d_out, out_words, stream)


def scc(d_ref, d_tgt, nrows, ncols, smooth=0, min_diag=1, max_diag=None, stream=None, device=0):
    """The sums of the strata of the bands at device pointers `d_ref` and `d_tgt`: numpy uint64[SCC_ROWS, nrows],
    formed on the device."""
    return extractor(device).scc(d_ref, d_tgt, nrows, ncols, smooth, min_diag, max_diag, stream)


def stripe_profiles_into(d_band, nrows, ncols, max_offset, lengths, min_diag, d_out, out_words, stream=None, device=0):
    """The stripe profiles of the band at device pointer `d_band`, into the device array `d_out`
    (uint64[2][K][2 m + 1][ncols]); enqueued on `stream`, nothing crosses to the host."""
    extractor(device).stripe_profiles_into(d_band, nrows, ncols, max_offset, lengths, min_diag, d_out, out_words, stream)


def stripe_profiles(d_band, nrows, ncols, max_offset, lengths, min_diag, stream=None, device=0):
    """The stripe profiles of the band at device pointer `d_band`: numpy uint64[2, K, 2 m + 1, ncols], formed
    on the device."""
    return extractor(device).stripe_profiles(d_band, nrows, ncols, max_offset, lengths, min_diag, stream)


def coarse_stripe_profiles(d_band, nrows, ncols, factor, first_bin, max_offset, lengths, min_diag, stream=None,
                           device=0):
    """The stripe profiles of the band at `factor` times its bin size: numpy uint64[2, K, 2 m + 1, ncols'],
    coarsened and formed on the device."""
    return extractor(device).coarse_stripe_profiles(d_band, nrows, ncols, factor, first_bin, max_offset, lengths,
                                                    min_diag, stream)


def triangles_into(d_band, nrows, ncols, max_width, min_diag, d_out, out_words, stream=None, device=0):
    """The triangle table of the band at device pointer `d_band`, into the device array `d_out`
    (uint64[max_width][ncols]); enqueued on `stream`, nothing crosses to the host."""
    extractor(device).triangles_into(d_band, nrows, ncols, max_width, min_diag, d_out, out_words, stream)


def triangles_to_host(d_band, nrows, ncols, max_width, min_diag=0, stream=None, device=0):
    """The triangle table of the band at device pointer `d_band`: numpy uint64[max_width, ncols], formed on the
    device."""
    return extractor(device).triangles_to_host(d_band, nrows, ncols, max_width, min_diag, stream)


def coarse_triangles_to_host(d_band, nrows, ncols, factor, first_bin, max_width, min_diag=0, stream=None, device=0):
    """The triangle table of the band at `factor` times its bin size: numpy uint64[max_width, ncols'], coarsened
    and formed on the device."""
    return extractor(device).coarse_triangles_to_host(d_band, nrows, ncols, factor, first_bin, max_width, min_diag,
                                                      stream)
