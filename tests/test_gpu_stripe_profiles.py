"""The stripe profiles of a band formed on the MI355X (include/modle_pixels.h: modle_pixels_stripe_profiles,
_stripe_profiles_to_host, _coarse_stripe_profiles_to_host; modle_amd/pixels.py; api.BandAnalyses.stripe_profiles,
stripe_profiles_tensor and call_stripes): every word equals, word for word, the numpy restatement of
tests/test_stripe_calls_outputs.py.  The band lies between poisoned guard words at an address that is 4-byte
aligned only and its words that are no pixels (the left-edge triangle, the trailing word) hold 0xFFFFFFFF: a word
that must never be read shows in the sum.  The output lies at an 8-byte aligned address between guard words and
is filled with 0xA5 bytes before every call: a word that is not stored shows.  Nothing here has a tolerance."""
import numpy as np
import pytest

from test_gpu_marginals import BACK, POISON, Guarded, reference_coarsen
from test_stripe_calls_outputs import diag_sums, make_band, restate

pytestmark = pytest.mark.gpu

# (nrows, ncols, m, d0, lengths): the smallest band; the smallest band for m = 8, both bounds at equality and every
# anchor within m of an end; the edges of the workgroups of both kernels (4 columns, 64 rows); a column past one
# chunk of 256 words; m = 0 and the whole band; many workgroups
SHAPES = [(1, 1, 0, 0, [1]), (17, 17, 8, 8, [9]), (20, 63, 3, 3, [5, 9, 17]), (20, 64, 3, 3, [5, 9, 17]),
          (20, 65, 3, 3, [5, 9, 17]), (20, 129, 3, 3, [5, 9, 17]), (257, 321, 8, 8, [16, 64, 128, 249]),
          (600, 700, 0, 1, [600]), (70, 8200, 4, 4, [8, 66])]
FILLS = ["sparse", "max", "corners", "ones"]
COARSE = [(130, 260, 2, 3, 2, 2, [5, 20, 60]), (600, 700, 7, 25, 8, 8, [9, 40, 78])]  # nrows, ncols, factor, first_bin, m, d0, lengths
FRONT8 = 66  # guard words in front of an output: the words behind them are 8-byte aligned
FILLER = 0xA5A5A5A5


class FilledOut:
    """`n_sums` 64-bit words of 0xA5 bytes in device memory, 8-byte aligned, between guard words that hold
    POISON: the caller does not pre-zero, and a write beyond either end shows up"""

    def __init__(self, n_sums):
        import torch

        self.n = 2 * n_sums
        self.host = np.full(FRONT8 + self.n + BACK, POISON, dtype=np.uint32)
        self.host[FRONT8:FRONT8 + self.n] = FILLER
        self.tensor = torch.from_numpy(self.host.view(np.int32)).to("cuda:0")
        torch.cuda.synchronize()
        assert self.data_ptr() % 8 == 0

    def data_ptr(self):
        return self.tensor.data_ptr() + 4 * FRONT8

    def read(self):
        import torch

        torch.cuda.synchronize()
        return self.tensor.cpu().numpy().view(np.uint32)

    def unchanged(self):
        return np.array_equal(self.read(), self.host)

    def guards_intact(self):
        got = self.read()
        return (got[:FRONT8] == POISON).all() and (got[FRONT8 + self.n:] == POISON).all()

    def sums(self, shape):
        return self.read()[FRONT8:FRONT8 + self.n].copy().view(np.uint64).reshape(shape)


@pytest.fixture(scope="module")
def ex():
    from modle_amd import pixels

    with pixels.Extractor(0) as e:
        yield e


def words(m, lengths, ncols):
    return 2 * len(lengths) * (2 * m + 1) * ncols


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("nrows,ncols,m,d0,lengths", SHAPES)
def test_the_profiles_equal_the_definition(ex, nrows, ncols, m, d0, lengths, fill):
    from modle_amd import pixels

    band = make_band(nrows, ncols, fill)
    want = restate(band, nrows, ncols, m, lengths, d0)
    shape = (2, len(lengths), 2 * m + 1, ncols)
    if fill == "ones":
        assert np.array_equal(want, pixels.stripe_profile_n_valid(ncols, m, lengths, d0))
    if fill == "max" and lengths[-1] - d0 > 1 and ncols > 2 * m + lengths[-1]:
        assert int(want.max()) == (lengths[-1] - d0) * 0xFFFFFFFF > 2**32  # the carries into the high half are live
    src = Guarded(band)
    # the device form, into an array of 0xA5 bytes
    d_out = FilledOut(words(m, lengths, ncols))
    ex.stripe_profiles_into(src.data_ptr(), nrows, ncols, m, lengths, d0, d_out.data_ptr(), words(m, lengths, ncols))
    got = d_out.sums(shape)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert d_out.guards_intact()
    # the host form, twice: the same again
    for _ in range(2):
        got = ex.stripe_profiles(src.data_ptr(), nrows, ncols, m, lengths, d0)
        assert got.dtype == np.uint64 and got.shape == shape
        assert np.array_equal(got, want)
    assert src.unchanged()


@pytest.mark.parametrize("nrows,ncols,m,d0,lengths", [s for s in SHAPES if len(s[4]) > 1])
def test_a_length_alone_is_its_rows_of_the_call_with_all(ex, nrows, ncols, m, d0, lengths):
    src = Guarded(make_band(nrows, ncols, "sparse", seed=1))
    together = ex.stripe_profiles(src.data_ptr(), nrows, ncols, m, lengths, d0)
    for k, length in enumerate(lengths):
        assert np.array_equal(ex.stripe_profiles(src.data_ptr(), nrows, ncols, m, [length], d0)[:, 0], together[:, k]), length
    if m >= 1:  # a narrower cross-section is the middle of the wider one
        narrow = ex.stripe_profiles(src.data_ptr(), nrows, ncols, m - 1, lengths, d0)
        assert np.array_equal(narrow, together[:, :, 1:-1])
    assert src.unchanged()


@pytest.mark.parametrize("nrows,ncols,factor,first_bin,m,d0,lengths", COARSE)
def test_the_coarse_profiles_are_those_of_the_coarse_band(ex, nrows, ncols, factor, first_bin, m, d0, lengths):
    from modle_amd import pixels

    band = make_band(nrows, ncols, "sparse")
    band[band != POISON] >>= 12  # no coarse sum saturates
    coarse, nr, nc = reference_coarsen(band, nrows, ncols, factor, first_bin)
    assert pixels.coarse_shape(nrows, ncols, factor, first_bin) == (nr, nc) and lengths[-1] + m <= nr
    want = restate(coarse, nr, nc, m, lengths, d0)
    src = Guarded(band)
    for got in (ex.coarse_stripe_profiles(src.data_ptr(), nrows, ncols, factor, first_bin, m, lengths, d0),
                pixels.coarse_stripe_profiles(src.data_ptr(), nrows, ncols, factor, first_bin, m, lengths, d0)):
        assert got.dtype == np.uint64 and got.shape == (2, len(lengths), 2 * m + 1, nc)
        assert np.array_equal(got, want)
    # the fine path still serves, and the module-level form (the process-wide context of the device)
    fine = restate(band, nrows, ncols, m, lengths, d0)
    for got in (ex.stripe_profiles(src.data_ptr(), nrows, ncols, m, lengths, d0),
                pixels.stripe_profiles(src.data_ptr(), nrows, ncols, m, lengths, d0)):
        assert np.array_equal(got, fine)
    # a length that fits the fine band only is refused against the coarse shape
    with pytest.raises(pixels.PixelsError) as e:
        ex.coarse_stripe_profiles(src.data_ptr(), nrows, ncols, factor, first_bin, m, [nr - m + 1], d0)
    assert e.value.code == pixels.ERR_ARG and "of the coarse band" in str(e.value)
    with pytest.raises(pixels.PixelsError) as e:
        ex.coarse_stripe_profiles(src.data_ptr(), nrows, ncols, 1, first_bin, m, lengths, d0)
    assert e.value.code == pixels.ERR_ARG
    assert src.unchanged()


def test_the_tensor_form_never_leaves_the_device_and_the_calls_follow():
    import torch

    from modle_amd import api, pixels

    nrows, ncols, m, d0, lengths = 40, 200, 3, 3, [8, 16, 32]
    band = make_band(nrows, ncols, "sparse", seed=2)
    band[band != POISON] >>= 20
    band[100 * nrows + 1:100 * nrows + 16] = 1 << 14  # a stripe upstream of bin 100: M(100 - d, 100), d < 16
    want = restate(band, nrows, ncols, m, lengths, d0)
    with api.LoadedBands(0) as lb:
        tensor = torch.from_numpy(band.view(np.int32)).to("cuda:0")
        bid = lb.add_band(tensor, nrows, ncols)
        out = lb.stripe_profiles_tensor(bid, m, lengths, d0)
        assert out.is_cuda and out.dtype == torch.int64 and tuple(out.shape) == want.shape
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint64), want)
        prof, n_valid = lb.stripe_profiles(bid, m, lengths, d0)
        assert np.array_equal(prof, want) and np.array_equal(n_valid, pixels.stripe_profile_n_valid(ncols, m, lengths, d0))
        rows = lb.call_stripes(bid, m, lengths, d0, fold=4, min_count=13 << 14)
        assert rows == api.stripe_rows(want, diag_sums(band, nrows, ncols), m, lengths, d0, fold=4, min_count=13 << 14)
        assert [(r.direction, r.bin, r.length) for r in rows] == [(0, 100, 32)]
        # at twice the bin size: the profiles of the coarse band
        coarse, nr, nc = reference_coarsen(band, nrows, ncols, 2, 1)
        prof2, n_valid2 = lb.stripe_profiles(bid, 2, [5, 10], 2, factor=2, first_bin=1)
        assert np.array_equal(prof2, restate(coarse, nr, nc, 2, [5, 10], 2)) and n_valid2.shape == prof2.shape


def test_what_is_refused_with_a_device(ex):
    from modle_amd import pixels

    nrows, ncols, m, d0, lengths = 20, 65, 3, 3, [5, 9, 17]
    n = words(m, lengths, ncols)
    src = Guarded(make_band(nrows, ncols, "sparse"))
    d_out = FilledOut(n)
    band_bytes = (nrows * ncols + 1) * 4
    refused = [
        (src.data_ptr(), d_out.data_ptr(), n - 1), (src.data_ptr(), d_out.data_ptr(), n + 1),  # out_words
        (src.data_ptr(), d_out.data_ptr() + 4, n),  # alignment
        (src.data_ptr(), src.data_ptr() + 4, n), (src.data_ptr(), src.data_ptr() + band_bytes - 4, n),  # overlap
        (src.data_ptr(), src.data_ptr() + 4 - 8 * n + 8, n),
    ]
    for d_band, out, out_words in refused:
        with pytest.raises(pixels.PixelsError) as e:
            ex.stripe_profiles_into(d_band, nrows, ncols, m, lengths, d0, out, out_words)
        assert e.value.code == pixels.ERR_ARG
    for bad in ((m, lengths, d0 - 1), (m, [5, 9, 18], d0), (9, [10], 9), (m, [], d0), (m, [5, 5], d0)):
        with pytest.raises(pixels.PixelsError) as e:
            ex.stripe_profiles_into(src.data_ptr(), nrows, ncols, bad[0], bad[1], bad[2], d_out.data_ptr(),
                                    words(bad[0], bad[1], ncols))
        assert e.value.code == pixels.ERR_ARG
        with pytest.raises(pixels.PixelsError):
            ex.stripe_profiles(src.data_ptr(), nrows, ncols, *bad)
    assert d_out.unchanged() and src.unchanged()  # nothing was written
