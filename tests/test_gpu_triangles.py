"""The triangle sums of a band formed on the MI355X (include/modle_pixels.h: modle_pixels_triangles,
_triangles_to_host, _coarse_triangles_to_host; modle_amd/pixels.py; api.BandAnalyses.triangle_sums,
triangle_sums_tensor and call_domains): every word equals, word for word, the numpy restatement
pixels.triangle_sums_host, which tests/test_triangles_outputs.py holds against the definition.  The band lies
between poisoned guard words at an address that is 4-byte aligned only and its words that are no pixels (the
left-edge triangle, the trailing word) hold 0xFFFFFFFF: a word that must never be read shows in the sum.  The
output lies at an 8-byte aligned address between guard words and is filled with 0xA5 bytes before every call: a
word that is not stored shows.  Nothing here has a tolerance."""
import numpy as np
import pytest

from test_gpu_marginals import POISON, Guarded, make_band, reference_coarsen, reference_marginals
from test_gpu_stripe_profiles import FilledOut

pytestmark = pytest.mark.gpu

# the smallest band and the square whole matrix; the edges of the 64 x 64 tiles on both axes, one off each
SHAPES = [(1, 1), (5, 5), (7, 63), (64, 64), (65, 129), (130, 257)]


def widths(nrows):
    """1, the whole band, and one below and one above every multiple of 64 that fits"""
    return sorted({1, nrows} | {w for m in range(64, nrows + 2, 64) for w in (m - 1, m + 1) if 1 <= w <= nrows})


def min_diags(width):
    return sorted({0, min(2, width), width - 1, width})  # the last: all zeros


@pytest.fixture(scope="module")
def ex():
    from modle_amd import pixels

    with pixels.Extractor(0) as e:
        yield e


def zeroed(band, nrows, ncols):
    """the band with its words that are no pixels at 0"""
    out = band.copy()
    for j in range(min(nrows, ncols)):
        out[j * nrows + j + 1:(j + 1) * nrows] = 0
    out[nrows * ncols] = 0
    return out


@pytest.mark.parametrize("nrows,ncols", SHAPES)
def test_the_table_equals_the_restatement(ex, nrows, ncols):
    from modle_amd import pixels

    band = make_band(nrows, ncols, "full")
    assert band[nrows * ncols] == POISON and (nrows == 1 or band[1] == POISON)
    src, clean = Guarded(band), Guarded(zeroed(band, nrows, ncols))
    for width in widths(nrows):
        for d0 in min_diags(width):
            want = pixels.triangle_sums_host(band, nrows, ncols, width, d0)
            if d0 == width:
                assert not want.any()
            # the windows that the chromosome's end clips: the starts s + W > ncols, W - 1 of them
            assert sum(1 for s in range(ncols) if s + width > ncols) == min(width - 1, ncols)
            d_out = FilledOut(width * ncols)  # stale 0xA5 bytes: every word is stored
            ex.triangles_into(src.data_ptr(), nrows, ncols, width, d0, d_out.data_ptr(), width * ncols)
            got = d_out.sums((width, ncols))
            assert np.array_equal(got, want), (width, d0, np.argwhere(got != want)[:8])
            assert d_out.guards_intact()
            # the same call on the band whose non-pixels are zero: the same table, so none of them was read
            d_out = FilledOut(width * ncols)
            ex.triangles_into(clean.data_ptr(), nrows, ncols, width, d0, d_out.data_ptr(), width * ncols)
            assert np.array_equal(d_out.sums((width, ncols)), want), (width, d0)
            # the host form, twice: the same again
            for _ in range(2):
                got = ex.triangles_to_host(src.data_ptr(), nrows, ncols, width, d0)
                assert got.dtype == np.uint64 and got.shape == (width, ncols) and np.array_equal(got, want)
    assert src.unchanged() and clean.unchanged()


def test_more_words_than_needed_leave_the_rest_alone(ex):
    from modle_amd import pixels

    nrows, ncols, width = 65, 129, 65
    band = make_band(nrows, ncols, "tenth")
    src = Guarded(band)
    d_out = FilledOut(width * ncols + 5)
    ex.triangles_into(src.data_ptr(), nrows, ncols, width, 1, d_out.data_ptr(), width * ncols + 5)
    got = d_out.sums((width * ncols + 5,))
    assert np.array_equal(got[:width * ncols].reshape(width, ncols), pixels.triangle_sums_host(band, nrows, ncols, width, 1))
    assert (got[width * ncols:] == 0xA5A5A5A5A5A5A5A5).all() and d_out.guards_intact()


@pytest.mark.parametrize("nrows,ncols,over", [(300, 320, 1 << 32), (2100, 2200, 1 << 53)])
def test_the_carries_of_a_band_of_the_largest_counts(ex, nrows, ncols, over):
    """every pixel 0xFFFFFFFF, and every word that is no pixel as well: the table is the number of pixels of every
    window times 0xFFFFFFFF, past 2^32 wherever a window has more than one pixel and, on the larger band, past 2^53"""
    import torch

    from modle_amd import api, pixels

    width = nrows
    band = np.full(nrows * ncols + 1, POISON, dtype=np.uint32)
    want = pixels.triangle_cells(ncols, width, 0) * np.uint64(0xFFFFFFFF)
    assert int(want.max()) == width * (width + 1) // 2 * 0xFFFFFFFF >= over
    assert (want[1:, :-1] > 1 << 32).all()  # (the last start holds one bin)
    assert np.array_equal(want, pixels.triangle_sums_host(band, nrows, ncols, width, 0))
    src = Guarded(band)
    d_out = FilledOut(width * ncols)
    ex.triangles_into(src.data_ptr(), nrows, ncols, width, 0, d_out.data_ptr(), width * ncols)
    got = d_out.sums((width, ncols))
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert d_out.guards_intact() and src.unchanged()
    if over == 1 << 53:  # exact on the device, and the decision refuses to round it
        with api.LoadedBands(0) as lb:
            bid = lb.add_band(torch.from_numpy(band.view(np.int32)).to("cuda:0"), nrows, ncols)
            with pytest.raises(ValueError) as e:
                lb.call_domains(bid, width)
            assert "2^53" in str(e.value)


@pytest.mark.parametrize("factor,first_bin", [(2, 0), (2, 3), (5, 0), (5, 3)])
def test_the_coarse_table_is_that_of_the_coarse_band(ex, factor, first_bin):
    from modle_amd import pixels

    nrows, ncols = 65, 129
    band = make_band(nrows, ncols, "full")
    band[band != POISON] >>= 12  # no coarse sum saturates
    coarse, nr, nc = reference_coarsen(band, nrows, ncols, factor, first_bin)
    assert pixels.coarse_shape(nrows, ncols, factor, first_bin) == (nr, nc)
    src = Guarded(band)
    for width, d0 in ((nr, 0), (nr, 2), (1, 0), (nr - 1, nr - 2)):
        want = pixels.triangle_sums_host(coarse, nr, nc, width, d0)
        for got in (ex.coarse_triangles_to_host(src.data_ptr(), nrows, ncols, factor, first_bin, width, d0),
                    pixels.coarse_triangles_to_host(src.data_ptr(), nrows, ncols, factor, first_bin, width, d0),
                    ex.triangles_to_host(src.data_ptr(), nrows, ncols, width, d0, factor=factor, first_bin=first_bin)):
            assert got.dtype == np.uint64 and got.shape == (width, nc)
            assert np.array_equal(got, want), (width, d0)
    # the fine path still serves, and the module-level form (the process-wide context of the device)
    fine = pixels.triangle_sums_host(band, nrows, ncols, nrows, 1)
    for got in (ex.triangles_to_host(src.data_ptr(), nrows, ncols, nrows, 1),
                pixels.triangles_to_host(src.data_ptr(), nrows, ncols, nrows, 1)):
        assert np.array_equal(got, fine)
    # a width that fits the fine band only is refused against the coarse shape
    with pytest.raises(pixels.PixelsError) as e:
        ex.coarse_triangles_to_host(src.data_ptr(), nrows, ncols, factor, first_bin, nr + 1, 0)
    assert e.value.code == pixels.ERR_ARG and "of the coarse band" in str(e.value)
    with pytest.raises(pixels.PixelsError) as e:
        ex.coarse_triangles_to_host(src.data_ptr(), nrows, ncols, 1, first_bin, 1, 0)
    assert e.value.code == pixels.ERR_ARG
    assert src.unchanged()


def test_the_tensor_form_never_leaves_the_device_and_the_other_callers_of_the_table():
    import torch

    from modle_amd import api, driver, pixels

    nrows, ncols, d0 = 40, 200, 2
    band = make_band(nrows, ncols, "tenth", seed=2)
    band[band != POISON] >>= 20
    for a, b in ((10, 40), (40, 75), (120, 150)):  # three domains on a sparse background
        for c in range(a, b):
            band[c * nrows:c * nrows + min(c - a, nrows - 1) + 1] += 5000
    want = pixels.triangle_sums_host(band, nrows, ncols, nrows, d0)
    with api.LoadedBands(0) as lb:
        bid = lb.add_band(torch.from_numpy(band.view(np.int32)).to("cuda:0"), nrows, ncols)
        out = lb.triangle_sums_tensor(bid, nrows, d0)
        assert out.is_cuda and out.dtype == torch.int64 and tuple(out.shape) == want.shape
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint64), want)
        table = lb.triangle_sums(bid, nrows, d0)
        assert table.dtype == np.uint64 and np.array_equal(table, want)
        assert np.array_equal(lb.triangle_sums(bid, 7), pixels.triangle_sums_host(band, nrows, ncols, 7, 0))  # min_diag 0
        # three triangles are a diamond: the insulation kernel's own sums of the same band
        windows = [1, 3, 10, 20]
        ins_sum, _ = lb.insulation(bid, windows, d0)
        assert np.array_equal(api.insulation_from_triangles(table, windows), ins_sum)
        # the identity that ties the table to the diagonal sums, and what it says of one word changed by 1
        diag_sum, _ = lb.marginals(bid, 0)
        assert np.array_equal(diag_sum, reference_marginals(band, nrows, ncols, 0)[0])
        driver.check_triangles("chrA:0-200", table, d0, diag_sum, windows, ins_sum)
        for k, s in ((0, 0), (17, 101), (nrows - 1, ncols - 1)):
            wrong = table.copy()
            wrong[k, s] += np.uint64(1)
            with pytest.raises(RuntimeError):
                driver.check_triangles("chrA:0-200", wrong, d0, diag_sum)
        # the calls are those of the decision on the host table
        calls = lb.call_domains(bid, nrows, d0)
        assert calls == pixels.domain_calls(want, pixels.triangle_cells(ncols, nrows, d0))
        assert [(c.start, c.end) for c in calls if c.strength > 2] == [(10, 40), (40, 75), (120, 150)]
        # at twice the bin size: the table of the coarse band
        coarse, nr, nc = reference_coarsen(band, nrows, ncols, 2, 1)
        assert np.array_equal(lb.triangle_sums(bid, nr, 1, factor=2, first_bin=1), pixels.triangle_sums_host(coarse, nr, nc, nr, 1))


def test_what_is_refused_with_a_device(ex):
    from modle_amd import pixels

    nrows, ncols, width = 20, 65, 9
    n = width * ncols
    src = Guarded(make_band(nrows, ncols, "tenth"))
    d_out = FilledOut(n)
    band_bytes = (nrows * ncols + 1) * 4
    refused = [
        (width, d_out.data_ptr(), n - 1),  # out_words
        (width, d_out.data_ptr() + 4, n),  # alignment
        (width, src.data_ptr() + 4, n), (width, src.data_ptr() + band_bytes - 4, n), (width, src.data_ptr() + 4 - 8 * n + 8, n),  # overlap
        (0, d_out.data_ptr(), n), (nrows + 1, d_out.data_ptr(), (nrows + 1) * ncols),
    ]
    for w, out, out_words in refused:
        with pytest.raises(pixels.PixelsError) as e:
            ex.triangles_into(src.data_ptr(), nrows, ncols, w, 0, out, out_words)
        assert e.value.code == pixels.ERR_ARG
    for w in (0, nrows + 1):
        with pytest.raises(pixels.PixelsError):
            ex.triangles_to_host(src.data_ptr(), nrows, ncols, w, 0)
    assert d_out.unchanged() and src.unchanged()  # nothing was written
