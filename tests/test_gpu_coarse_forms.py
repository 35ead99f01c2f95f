"""The composites of libmodle_pixels.so on the MI355X (include/modle_pixels.h: modle_pixels_coarse_to_host,
_coarse_marginals_to_host, _coarse_insulation_to_host, _coarse_dots_to_host, _coarse_pileup_to_host,
_coarse_dot_hist_to_host, _coarse_dots_fdr_to_host, _coarse_rescale_to_host) are the fine one-call form on the
coarsened band, word for word: the reference of every case is coarsen_into a caller-owned buffer and then extract,
marginals, insulation, dots, pileup, dot_hist, dots_fdr and rescale on that buffer.  On ONE
pixels.Extractor the composites then run on two bands of one shape and different content, alternating
between the bands from one analysis to the next, so a composite that skipped its coarsening, sized the
scratch band by the fine shape or mixed up `factor` and `first_bin` would hand back the other band's, or
another band's, numbers.  Everything is an integer: nothing here has a tolerance."""
import numpy as np
import pytest

from test_gpu_coarsen import POISON, Guarded, output_buffer
from test_gpu_pixels_context import mixed_band

pytestmark = pytest.mark.gpu

NROWS, NCOLS = 23, 70
# (factor, first_bin) -> the coarse shape; first_bin % factor is 1 at both factors
CASES = {(2, 0): (12, 35), (2, 5): (12, 36), (3, 4): (9, 24)}
W, P, MIN_COUNT = 1, 0, 1  # dots with min_diag 0: 5 diagonals
FOLDS = (0.5, 0.5, 0.5, 0.5)  # half of what the neighbourhoods expect: a band without structure still has dots
WINDOWS, FLANK = [1, 2], 1
N_OBS, FDR, SIZE = 33, 0.1, 2  # the histogram's counts, the rate of its thresholds, the grid of the rescaled pileup
NAMES = ("extract", "marginals", "insulation", "dots", "pileup", "dot_hist", "dots_fdr", "rescale", "dots_fdr_scaled")
OFFSET = 7  # bin_offset of the pixels and the dots


def anchors(nr, nc):
    """a dozen anchors of the coarse band, some of them rejected: a < flank, the window beyond the band,
    beyond the last column, a > b"""
    a = np.array([1, 2, 3, 5, 7, 0, 4, nc - 2, nc - 1, 6, 3, 8], dtype=np.int64)
    d = np.array([0, 1, 2, 3, 6, 0, nr, 0, 0, -1, 4, 5], dtype=np.int64)
    return a, a + d


def windows(nr):
    """windows [start, end) of the coarse band of widths 1, 2, 3, 5, nr and nr + 1 and one that starts before the
    band: some are accepted, some refused (rescale_accepts)"""
    start = np.array([1, 2, 3, 4, 0, 0, -1], dtype=np.int64)
    return start, start + np.array([1, 2, 3, 5, nr, nr + 1, 3], dtype=np.int64)


def same(got, want):
    """arrays, ints, Stats and tuples of them, compared exactly"""
    if isinstance(want, np.ndarray):
        return isinstance(got, np.ndarray) and got.dtype == want.dtype and np.array_equal(got, want)
    if isinstance(want, tuple):
        return len(got) == len(want) and all(same(g, w) for g, w in zip(got, want))
    return got == want


def fine_forms(ex, d_band, factor, first_bin):
    """the eight analyses of the band at `factor` times its bin size, by the fine forms on a coarsened copy"""
    from modle_amd import pixels

    nr, nc = CASES[(factor, first_bin)]
    scratch = output_buffer(nr * nc + 1)
    assert ex.coarsen_into(d_band.data_ptr(), NROWS, NCOLS, factor, first_bin, scratch.data_ptr(), nr * nc + 1) == (nr, nc)
    ptr = scratch.data_ptr()
    a, b = anchors(nr, nc)
    ok = pixels.pileup_accepts(nr, nc, FLANK, a, b)
    assert 0 < ok.sum() < len(a)
    diag_sum, _ = ex.marginals(ptr, nr, nc, 0)
    want = {"extract": ex.extract(ptr, nr, nc, OFFSET),
            "marginals": ex.marginals(ptr, nr, nc, 1),
            "insulation": ex.insulation(ptr, nr, nc, WINDOWS, 1),
            "scale": pixels.dot_scales(diag_sum, nc, W, P, FOLDS, 0),
            "pileup": ex.pileup(ptr, nr, nc, FLANK, a, b)}
    want["dots"] = ex.dots(ptr, nr, nc, W, P, 0, MIN_COUNT, want["scale"], OFFSET)
    want["lam"] = pixels.dot_scales(diag_sum, nc, W, P, (1.0, 1.0, 1.0, 1.0), 0)
    want["dot_hist"] = ex.dot_hist(ptr, nr, nc, W, P, 0, want["lam"], None, N_OBS)
    want["thr"] = pixels.dot_thresholds(want["dot_hist"], pixels.dot_lambda_edges(), FDR)
    want["dots_fdr"] = ex.dots_fdr(ptr, nr, nc, W, P, 0, MIN_COUNT, want["lam"], None, want["thr"], None, OFFSET)
    want["dots_fdr_scaled"] = ex.dots_fdr(ptr, nr, nc, W, P, 0, MIN_COUNT, want["lam"], None, want["thr"], want["scale"],
                                          OFFSET)
    s, e = windows(nr)
    taken = pixels.rescale_accepts(nr, nc, SIZE, s, e)
    assert 0 < taken.sum() < len(s)
    want["rescale"] = ex.rescale(ptr, nr, nc, SIZE, s, e)
    assert want["rescale"][2] == taken.sum() and want["rescale"][0].any() and want["dot_hist"].any()
    assert want["dot_hist"].shape == (4, len(pixels.dot_lambda_edges()) + 1, N_OBS)
    assert scratch.guards_intact()
    assert want["extract"].stats.nnz > 0 and want["dots"].stats.nnz > 0 and want["pileup"][1] == ok.sum() and want["pileup"][0].any()
    assert want["extract"].bin1_offset.shape == (nc + 1,) and want["insulation"].shape == (2, nc)
    return want


def test_a_composite_is_the_fine_form_on_the_coarsened_band():
    from modle_amd import pixels

    bands = [mixed_band(NROWS, NCOLS, 0.5, seed) for seed in (11, 12)]
    assert (bands[0] != bands[1]).any() and all((b == POISON).any() for b in bands)
    d_bands = [Guarded(b) for b in bands]
    with pixels.Extractor(0) as ex:
        for (factor, first_bin), (nr, nc) in CASES.items():
            assert pixels.coarse_shape(NROWS, NCOLS, factor, first_bin) == (nr, nc)
            want = [fine_forms(ex, d, factor, first_bin) for d in d_bands]
            assert not same(want[0]["extract"], want[1]["extract"])  # the bands tell each other apart
            a, b = anchors(nr, nc)
            s, e = windows(nr)
            shape = (NROWS, NCOLS, factor, first_bin)
            at = dict(factor=factor, first_bin=first_bin)
            for keywords in (False, True):
                for x, y in ((0, 1), (1, 0)):  # A, B, A, B, ... across the analyses, then exchanged
                    px, py, wx, wy = d_bands[x].data_ptr(), d_bands[y].data_ptr(), want[x], want[y]
                    fdr = (W, P, 0, MIN_COUNT, wx["lam"], None, wx["thr"])
                    if keywords:
                        got = [ex.extract(px, NROWS, NCOLS, OFFSET, **at),
                               ex.marginals(py, NROWS, NCOLS, 1, **at),
                               ex.insulation(px, NROWS, NCOLS, WINDOWS, 1, **at),
                               ex.dots(py, NROWS, NCOLS, W, P, 0, MIN_COUNT, wy["scale"], OFFSET, **at),
                               ex.pileup(px, NROWS, NCOLS, FLANK, a, b, **at),
                               ex.dot_hist(py, NROWS, NCOLS, W, P, 0, wy["lam"], None, N_OBS, **at),
                               ex.dots_fdr(px, NROWS, NCOLS, *fdr, None, OFFSET, **at),
                               ex.rescale(py, NROWS, NCOLS, SIZE, s, e, **at),
                               ex.dots_fdr(px, NROWS, NCOLS, *fdr, wx["scale"], OFFSET, **at)]
                    else:
                        got = [ex.coarse_extract(px, *shape, OFFSET),
                               ex.coarse_marginals(py, *shape, 1),
                               ex.coarse_insulation(px, *shape, WINDOWS, 1),
                               ex.coarse_dots(py, *shape, W, P, 0, MIN_COUNT, wy["scale"], OFFSET),
                               ex.coarse_pileup(px, *shape, FLANK, a, b),
                               ex.coarse_dot_hist(py, *shape, W, P, 0, wy["lam"], None, N_OBS),
                               ex.coarse_dots_fdr(px, *shape, *fdr, None, OFFSET),
                               ex.coarse_rescale(py, *shape, SIZE, s, e),
                               ex.coarse_dots_fdr(px, *shape, *fdr, wx["scale"], OFFSET)]
                    for n, (name, g) in enumerate(zip(NAMES, got)):
                        assert same(g, (wx, wy)[n % 2][name]), (factor, first_bin, keywords, x, name)
    assert d_bands[0].unchanged() and d_bands[1].unchanged()
