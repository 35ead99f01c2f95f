"""The buffers of one libmodle_pixels.so context (modle_amd/pixels/pixels_context.h) on the MI355X: a
fixed sequence of one-call forms on ONE pixels.Extractor makes every buffer -- the bin1_offset index,
the pixel arrays, the coarse band, the dense region -- grow, be reused at a smaller size, and grow
again, and every result equals, exactly, the numpy restatements of test_gpu_coarsen and
test_gpu_dense.  The bands are seeded mixes of zeros and non-zeros of different densities, so that nnz
differs from call to call, and the words that are no pixels hold 0xFFFFFFFF.  The forms that wait for 64-bit
sums share one result buffer, and the two that upload host lists one more: a second sequence makes those grow, be
reused smaller and grow again, and holds every result against the same call on a fresh context."""
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


def test_the_shared_sums_and_lists_grow_are_reused_and_grow_again():
    from modle_amd import pixels
    from test_gpu_coarse_forms import same

    small, mid, large = mixed_band(3, 70, 0.5, 1), mixed_band(40, 300, 0.3, 2), mixed_band(64, 900, 0.6, 3)
    d_small, d_mid, d_large = Guarded(small), Guarded(mid), Guarded(large)
    a = np.arange(2, 14, dtype=np.int64)  # 12 anchors, on the diagonal (accepted) and beside it (too near the band's edge)
    b = a + np.tile(np.array([0, 1], dtype=np.int64), 6)
    start, end = np.array([10, 50, 100], dtype=np.int64), np.array([20, 75, 139], dtype=np.int64)
    n_piled = int(pixels.pileup_accepts(3, 70, 1, a, b).sum())
    assert 0 < n_piled < len(a) and pixels.rescale_accepts(40, 300, 2, start, end).all()
    with pixels.Extractor(0) as fresh:
        diag_sum, _ = fresh.marginals(d_mid.data_ptr(), 40, 300, 0)
    lam = pixels.dot_scales(diag_sum, 300, 1, 0, (1.0, 1.0, 1.0, 1.0), 0)
    calls = [lambda ex: ex.insulation(d_small.data_ptr(), 3, 70, [1, 2], 1),       # 1: the sums are made
             lambda ex: ex.pileup(d_small.data_ptr(), 3, 70, 1, a, b),             # 2: reused smaller; the lists are made
             lambda ex: ex.scc(d_mid.data_ptr(), d_mid.data_ptr(), 40, 300),       # 3: the sums grow
             lambda ex: ex.stripes(d_large.data_ptr(), d_large.data_ptr(), 64, 900),  # 4: and grow again
             lambda ex: ex.rescale(d_mid.data_ptr(), 40, 300, 2, start, end),      # 5: both reused smaller
             lambda ex: ex.dot_hist(d_mid.data_ptr(), 40, 300, 1, 0, 0, lam, None, 33),  # 6: reused
             lambda ex: ex.insulation(d_small.data_ptr(), 3, 70, [1, 2], 1)]       # 7: reused
    # the words of the shared result per call, and the entries of the shared lists; a buffer grows by an eighth more
    words = [2 * 70, 3 * 3 + 1, pixels.SCC_ROWS * 40, 2 * pixels.stripes_rows(pixels.STRIPES_MOMENTS) * 900, 2 * 2 * 2 + 1,
             4 * (len(pixels.dot_lambda_edges()) + 1) * 33, 2 * 70]
    assert words[1] < words[0] and words[0] + words[0] // 8 < words[2] and words[2] + words[2] // 8 < words[3]
    assert words[4] < words[5] < words[3] and words[6] < words[3]
    assert 2 * len(start) < 2 * len(a)
    want = []
    for call in calls:
        with pixels.Extractor(0) as fresh:
            want.append(call(fresh))
    assert want[0].any() and want[1][1] == n_piled and want[2].any() and want[3].any() and want[4][2] == 3 and want[5].any()
    with pixels.Extractor(0) as ex:
        got = []
        for n, call in enumerate(calls):
            got.append(call(ex))
            assert same(got[n], want[n]), n
        # the arrays handed out earlier are the caller's: no later growth or reuse changed them
        for n in range(len(calls)):
            assert same(got[n], want[n]), n
    assert d_small.unchanged() and d_mid.unchanged() and d_large.unchanged()
