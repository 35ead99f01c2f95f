"""The buffers of one libmodle_pixels.so context (modle_amd/pixels/pixels_context.h) on the MI355X: a
fixed sequence of one-call forms on ONE pixels.Extractor makes every buffer -- the bin1_offset index,
the pixel arrays, the coarse band, the dense region -- grow, be reused at a smaller size, and grow
again, and every result equals, exactly, the numpy restatements of test_gpu_coarsen and
test_gpu_dense.  The bands are seeded mixes of zeros and non-zeros of different densities, so that nnz
differs from call to call, and the words that are no pixels hold 0xFFFFFFFF."""
import numpy as np
import pytest

from test_gpu_coarsen import Guarded, assert_pixels, make_band, reference_coarsen, reference_pixels
from test_gpu_dense import reference_dense

pytestmark = pytest.mark.gpu


def mixed_band(nrows, ncols, density, seed):
    """make_band's layout and poison, with about `density` of the pixels non-zero"""
    band = make_band(nrows, ncols, "empty", 2)
    rng = np.random.default_rng([seed, nrows, ncols])
    for j in range(ncols):  # the pixels of column j: d <= min(j, nrows - 1)
        n = min(j, nrows - 1) + 1
        keep = rng.random(n) < density
        band[j * nrows:j * nrows + n][keep] = rng.integers(1, 2**20, size=int(keep.sum()))
    return band


def test_every_buffer_grows_is_reused_and_grows_again():
    from modle_amd import pixels

    small, mid, large = mixed_band(3, 70, 0.5, 1), mixed_band(40, 300, 0.3, 2), mixed_band(64, 900, 0.6, 3)
    d_small, d_mid, d_large = Guarded(small), Guarded(mid), Guarded(large)
    want_small, want_mid = reference_pixels(small, 3, 70), reference_pixels(mid, 40, 300)
    coarse_mid, coarse_large = reference_coarsen(mid, 40, 300, 2, 0), reference_coarsen(large, 64, 900, 2, 0)
    want_coarse_mid, want_coarse_large = reference_pixels(*coarse_mid), reference_pixels(*coarse_large)
    # nnz differs between the calls, and the fifth call needs more of every array than any before it
    sizes = [want_small["nnz"], want_mid["nnz"], want_coarse_mid["nnz"], want_coarse_large["nnz"]]
    assert 0 < sizes[0] < sizes[2] < sizes[1] < sizes[3]
    assert coarse_mid[1] * coarse_mid[2] < coarse_large[1] * coarse_large[2] and coarse_large[2] + 1 > 301
    with pixels.Extractor(0) as ex:
        first = ex.extract(d_small.data_ptr(), 3, 70)                       # 1: index and pixels are made
        assert_pixels(first, want_small)
        second = ex.extract(d_mid.data_ptr(), 40, 300, bin_offset=7)        # 2: both grow
        assert_pixels(second, want_mid, 7)
        assert_pixels(ex.extract(d_small.data_ptr(), 3, 70), want_small)    # 3: both are reused
        got = ex.coarse_extract(d_mid.data_ptr(), 40, 300, 2, 0)            # 4: the coarse band is made
        assert_pixels(got, want_coarse_mid)
        got = ex.coarse_extract(d_large.data_ptr(), 64, 900, 2, 0, bin_offset=11)  # 5: all of them grow
        assert_pixels(got, want_coarse_large, 11)
        for lo, hi, band, d_band, nrows, ncols in [(5, 15, small, d_small, 3, 70),        # 6: below one block
                                                   (100, 230, mid, d_mid, 40, 300),       # 7: grows, three blocks
                                                   (690, 700, large, d_large, 64, 900)]:  # 8: reused
            dense = ex.dense(d_band.data_ptr(), nrows, ncols, lo, hi)
            assert dense.dtype == np.uint32 and dense.flags.owndata
            assert np.array_equal(dense, reference_dense(band, nrows, lo, hi - lo, 1, 1)[0]), (lo, hi)
        # the arrays handed out earlier are the caller's: no later growth changed them
        assert_pixels(first, want_small)
        assert_pixels(second, want_mid, 7)
    assert d_small.unchanged() and d_mid.unchanged() and d_large.unchanged()
