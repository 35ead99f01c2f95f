"""Two bands compared diagonal by diagonal on the MI355X (include/modle_pixels.h: modle_pixels_scc, _scc_to_host;
modle_amd/pixels.py; api.BandAnalyses.scc_moments, scc, scc_moments_tensor): the eleven words of every stratum
equal, word for word, the numpy / Python-int restatement of tests/test_scc_outputs.py, for bands built on the
host with a seeded generator.  The inputs lie between poisoned guard words at an address that is 4-byte aligned
only, the output at an 8-byte aligned address between guard words, poisoned before the call (the library, not
the caller, defines every word), and in every input band the words that are no pixels hold 0xFFFFFFFF: they
must not be read as counts.  Nothing the kernels write has a tolerance."""
import numpy as np
import pytest

from test_gpu_insulation import GuardedOut
from test_gpu_marginals import POISON, Guarded, reference_coarsen
from test_scc_outputs import restate, wide

pytestmark = pytest.mark.gpu

# (nrows, ncols, h): one word, with min_diag = 0; all triangle; a box that crosses the diagonal at both corners of
# the matrix; nrows - 1 - 2h == 0, the single stratum 0 under the widest halo, every box clipped on all sides; one
# below, exactly and one past a strip of 64 strata / a tile; several strips and tiles with ragged ends; the
# streaming kernel past 256 threads; many strips
SHAPES = [(1, 1, 0), (5, 5, 0), (5, 9, 1), (41, 41, 20), (63, 65, 3), (64, 64, 3), (65, 130, 3), (129, 200, 5),
          (257, 321, 0), (600, 700, 20)]
FILLS = ["empty", "tenth", "full", "ties"]


def make_pair(nrows, ncols, fill, seed=0):
    """the reference and the target band: `empty` zeros; `tenth` a tenth of the pixels with counts up to
    0xFFFFFFFE, each band its own; `full` every pixel 0xFFFFFFFF in both; `ties` counts of 0, 1 and 2, so
    that n depends on the or of the two.  The words that are no pixels hold 0xFFFFFFFF."""
    rng = np.random.default_rng([seed, nrows, ncols])
    n = nrows * ncols
    bands = []
    for _ in range(2):
        band = np.zeros(n + 1, dtype=np.uint32)
        if fill == "tenth":
            mask = rng.random(n) < 0.1
            band[:-1][mask] = rng.integers(1, 0xFFFFFFFF, size=int(mask.sum()), dtype=np.int64)
        elif fill == "full":
            band[:] = 0xFFFFFFFF
        elif fill == "ties":
            band[:-1] = rng.integers(0, 3, size=n, dtype=np.int64)
        for j in range(min(nrows, ncols)):
            band[j * nrows + j + 1:(j + 1) * nrows] = POISON
        band[n] = POISON
        bands.append(band)
    return bands


def default_strata(nrows, h):
    """the widest range: from the main diagonal where it is the only one, else from the first"""
    hi = nrows - 1 - 2 * h
    return min(1, hi), hi


@pytest.fixture(scope="module")
def ex():
    from modle_amd import pixels

    with pixels.Extractor(0) as e:
        yield e


def scc_into(ex, ref, tgt, nrows, ncols, h, lo, hi):
    """the [11, nrows] words modle_pixels_scc stores into a poisoned, guarded output"""
    d_out = GuardedOut(11 * nrows)
    ex.scc_into(ref.data_ptr(), tgt.data_ptr(), nrows, ncols, h, lo, hi, d_out.data_ptr(), 11 * nrows)
    got = d_out.sums(11)
    assert d_out.guards_intact()
    return got


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("nrows,ncols,h", SHAPES)
def test_the_strata_equal_the_restatement(ex, nrows, ncols, h, fill):
    a, b = make_pair(nrows, ncols, fill)
    lo, hi = default_strata(nrows, h)
    want = restate(a, b, nrows, ncols, h, lo, hi)
    if fill == "full" and h == 20:
        # Saa_hi: beyond 2^64.  (Sa passes 2^64 only from 2^32 / 1681 entries on: test_a_stratum_whose_sum_passes_64_bits)
        assert want[6].any() and want[8].any() and want[10].any() and not want[2].any()
    if fill == "empty":
        assert not want.any()
    if fill == "ties" and nrows > 5 and h == 0:
        n = want[0, lo:hi + 1].astype(np.int64)
        assert (n < ncols - np.arange(lo, hi + 1)).any() and n.any()  # some entries are zero in both, not all
    ref, tgt = Guarded(a), Guarded(b)
    assert ref.data_ptr() % 8 == 4
    assert np.array_equal(scc_into(ex, ref, tgt, nrows, ncols, h, lo, hi), want)
    for _ in range(2):  # the host form, twice: the same again
        got = ex.scc(ref.data_ptr(), tgt.data_ptr(), nrows, ncols, h, lo, hi)
        assert got.dtype == np.uint64 and got.shape == (11, nrows)
        assert np.array_equal(got, want)
    assert ref.unchanged() and tgt.unchanged()


@pytest.mark.parametrize("nrows,ncols,h,lo,hi", [(5, 9, 1, 0, 2), (65, 130, 3, 0, 58), (129, 200, 5, 0, 118),
                                                 (257, 321, 0, 0, 256),               # from the main diagonal
                                                 (5, 9, 0, 3, 3), (129, 200, 5, 64, 64), (257, 321, 0, 256, 256),
                                                 (600, 700, 20, 559, 559),            # one stratum
                                                 (65, 130, 3, 7, 40), (129, 200, 5, 60, 70), (257, 321, 0, 100, 200),
                                                 (600, 700, 20, 130, 300)])           # in the middle
def test_strata_other_than_the_default(ex, nrows, ncols, h, lo, hi):
    a, b = make_pair(nrows, ncols, "tenth", seed=1)
    want = restate(a, b, nrows, ncols, h, lo, hi)
    assert not want[:, :lo].any() and not want[:, hi + 1:].any() and want[:, lo:hi + 1].any()
    ref, tgt = Guarded(a), Guarded(b)
    assert np.array_equal(scc_into(ex, ref, tgt, nrows, ncols, h, lo, hi), want)  # zeros outside, over the poison
    assert ref.unchanged() and tgt.unchanged()


@pytest.mark.parametrize("nrows,ncols,h,fill", [(5, 9, 1, "ties"), (65, 130, 3, "tenth"), (257, 321, 0, "tenth"),
                                                (129, 200, 5, "full")])
def test_a_band_against_itself_through_one_pointer(ex, nrows, ncols, h, fill):
    from modle_amd import pixels

    a, _ = make_pair(nrows, ncols, fill, seed=1)
    lo, hi = default_strata(nrows, h)
    src = Guarded(a)
    got = ex.scc(src.data_ptr(), src.data_ptr(), nrows, ncols, h, lo, hi)
    assert np.array_equal(got, restate(a, a, nrows, ncols, h, lo, hi))
    for d in range(lo, hi + 1):
        _, sa, sb, saa, sbb, sab = wide(got, d)
        assert sa == sb and saa == sbb == sab
    _, rho, _ = pixels.scc_scores(got, ncols, lo, hi)
    assert ((rho == 1.0) | np.isnan(rho)).all()
    assert np.array_equal(pixels.scc(src.data_ptr(), src.data_ptr(), nrows, ncols, h, lo, hi), got)  # the module-level form
    if hi >= 1:
        assert np.array_equal(pixels.scc(src.data_ptr(), src.data_ptr(), nrows, ncols, h), got)  # its default strata
    assert src.unchanged()


def test_a_stratum_whose_sum_passes_64_bits(ex):
    """Sa = sum a leaves its low word only when a stratum has more than 2^32 / 1681 = 2.56 million entries of
    full boxes of full counts: a band of 41 diagonals and 2.6 million bins that holds 0xFFFFFFFF everywhere, the
    one stratum 0 under the widest box, one pointer as both bands.  The box of (i, i) has c_i = min(i, 20) +
    min(ncols - 1 - i, 20) + 1 rows and as many columns inside the matrix, so a_i = V c_i^2 and the sums have a
    closed form in Python integers."""
    import torch

    nrows, ncols, h, v = 41, 2_600_000, 20, 0xFFFFFFFF
    i = np.arange(ncols, dtype=np.int64)
    c = np.minimum(i, h) + np.minimum(ncols - 1 - i, h) + 1
    sa, saa = v * int((c ** 2).sum()), v * v * int((c ** 4).sum())
    assert sa >> 64 == 1 and saa >> 64
    band = torch.full((nrows * ncols + 1,), -1, dtype=torch.int32, device="cuda:0")
    got = ex.scc(band.data_ptr(), band.data_ptr(), nrows, ncols, h, 0, 0)
    assert wide(got, 0) == (ncols, sa, sa, saa, saa, saa)
    assert not got[:, 1:].any()


def test_a_stream_of_the_caller_and_buffers_that_grow():
    import torch

    from modle_amd import pixels

    stream = torch.cuda.Stream(device="cuda:0")
    assert stream.cuda_stream != 0
    small, large = make_pair(5, 9, "ties", seed=2), make_pair(70, 193, "tenth", seed=2)
    want_small, want_large = restate(*small, 5, 9, 1, 0, 2), restate(*large, 70, 193, 2, 1, 65)
    s, l = [Guarded(x) for x in small], [Guarded(x) for x in large]
    with pixels.Extractor(0) as e:
        first = e.scc(s[0].data_ptr(), s[1].data_ptr(), 5, 9, 1, 0, 2, stream=stream)
        again = e.scc(l[0].data_ptr(), l[1].data_ptr(), 70, 193, 2, 1, 65, stream=stream)  # grows
        assert np.array_equal(again, want_large)
        d_out = GuardedOut(11 * 5)
        e.scc_into(s[0].data_ptr(), s[1].data_ptr(), 5, 9, 1, 0, 2, d_out.data_ptr(), 11 * 5, stream=stream)
        shrunk = e.scc(s[0].data_ptr(), s[1].data_ptr(), 5, 9, 0, 1, 4, stream=stream)  # reused
        stream.synchronize()
        assert np.array_equal(d_out.sums(11), want_small) and d_out.guards_intact()
        assert np.array_equal(shrunk, restate(*small, 5, 9, 0, 1, 4))
        assert np.array_equal(first, want_small)  # the caller's
    assert all(g.unchanged() for g in s + l)


def test_invalid_calls_are_argument_errors_and_write_nothing(ex):
    from modle_amd import pixels

    nrows, ncols = 50, 90
    a, b = make_pair(nrows, ncols, "ties", seed=3)
    ref, tgt = Guarded(a), Guarded(b)
    words = 11 * nrows
    d_out = GuardedOut(11 * (ncols + 1))
    out, r, t = d_out.data_ptr(), ref.data_ptr(), tgt.data_ptr()
    inside = r + 4 * (nrows * ncols)  # the band's trailing word: the last that is the band's
    inside -= inside % 8
    for name, args in [("no reference", (None, t, nrows, ncols, 0, 1, 49, out, words)),
                       ("no target", (r, None, nrows, ncols, 0, 1, 49, out, words)),
                       ("no output", (r, t, nrows, ncols, 0, 1, 49, None, words)),
                       ("nrows 0", (r, t, 0, ncols, 0, 0, 0, out, 0)),
                       ("nrows > ncols", (r, t, ncols + 1, ncols, 0, 1, 49, out, 11 * (ncols + 1))),
                       ("a smoothing above 20", (r, t, nrows, ncols, 21, 1, 7, out, words)),
                       ("min_diag > max_diag", (r, t, nrows, ncols, 0, 5, 4, out, words)),
                       ("max_diag beyond the band", (r, t, nrows, ncols, 0, 1, 50, out, words)),
                       ("a box beyond the band", (r, t, nrows, ncols, 3, 1, 44, out, words)),
                       ("the widest box beyond the band", (r, t, nrows, ncols, 20, 1, 10, out, words)),
                       ("out_words too small", (r, t, nrows, ncols, 0, 1, 49, out, words - 1)),
                       ("out_words too large", (r, t, nrows, ncols, 0, 1, 49, out, words + 1)),
                       ("a misaligned output", (r, t, nrows, ncols, 0, 1, 49, out + 4, words)),
                       ("the output overlaps the reference", (r, t, nrows, ncols, 0, 1, 49, inside, words)),
                       ("the output ends inside the target", (r, t, nrows, ncols, 0, 1, 49, t - t % 8 - 8 * words + 8, words))]:
        with pytest.raises(pixels.PixelsError) as e:
            ex.scc_into(*args)
        assert e.value.code == pixels.ERR_ARG, name
    for args in [(None, t, nrows, ncols, 0, 1, 49), (r, None, nrows, ncols, 0, 1, 49), (r, t, 0, ncols, 0, 0, 0),
                 (r, t, ncols + 1, ncols, 0, 1, 49), (r, t, nrows, ncols, 21, 1, 7), (r, t, nrows, ncols, 0, 5, 4),
                 (r, t, nrows, ncols, 0, 1, 50), (r, t, nrows, ncols, 3, 1, 44), (r, t, nrows, ncols, 25)]:
        with pytest.raises(pixels.PixelsError) as e:
            ex.scc(*args)
        assert e.value.code == pixels.ERR_ARG, args
    assert d_out.unchanged() and ref.unchanged() and tgt.unchanged()  # (still poison)
    # the limits themselves are accepted: the widest box that fits, and the last diagonal
    assert np.array_equal(ex.scc(r, t, nrows, ncols, 20, 9, 9), restate(a, b, nrows, ncols, 20, 9, 9))
    assert np.array_equal(ex.scc(r, t, nrows, ncols, 0, 49, 49), restate(a, b, nrows, ncols, 0, 49, 49))


def test_the_api_forms_agree():
    """two bands that lie on the device as api.LoadedBands holds them: the target is coarsened by 3 from fine
    bin 2 on the device and compared with a reference of the coarse shape -- the restatement on
    reference_coarsen's band --, the torch form holds the same words, and the scores are pixels.scc_scores of the
    sums"""
    import torch

    from modle_amd import api, pixels

    nrows, ncols, k, first_bin = 130, 260, 3, 2
    rng = np.random.default_rng(5)
    fine = np.zeros(nrows * ncols + 1, dtype=np.uint32)
    mask = rng.random(nrows * ncols) < 0.3
    fine[:-1][mask] = rng.integers(1, 2**20, size=int(mask.sum()), dtype=np.int64)
    coarse, nr, nc = reference_coarsen(fine, nrows, ncols, k, first_bin)
    assert pixels.coarse_shape(nrows, ncols, k, first_bin) == (nr, nc) and nr < nc
    ref = make_pair(nr, nc, "tenth", seed=5)[0]
    dev = torch.device("cuda", 0)
    with api.LoadedBands(0) as bands, api.LoadedBands(0) as others:
        tid = bands.add_band(torch.from_numpy(fine.view(np.int32)).to(dev), nrows, ncols)
        rid = others.add_band(torch.from_numpy(ref.view(np.int32)).to(dev), nr, nc)
        h, hi = 2, nr - 1 - 4
        want = restate(ref, coarse, nr, nc, h, 1, hi)
        got = bands.scc_moments(tid, others, rid, h, factor=k, first_bin=first_bin)  # the default strata
        assert got.dtype == np.uint64 and got.shape == (11, nr) and np.array_equal(got, want)
        assert np.array_equal(bands.scc_moments(tid, others, rid, h, 3, 9, factor=k, first_bin=first_bin),
                              restate(ref, coarse, nr, nc, h, 3, 9))
        # the other way round: the coarsened band is the reference
        assert np.array_equal(others.scc_moments(rid, bands, tid, h, other_factor=k, other_first_bin=first_bin),
                              restate(coarse, ref, nr, nc, h, 1, hi))
        # a band against itself, at the bin size, without smoothing
        same = restate(fine, fine, nrows, ncols, 0, 1, nrows - 1)
        assert np.array_equal(bands.scc_moments(tid, bands, tid), same)
        t = bands.scc_moments_tensor(tid, others, rid, h, factor=k, first_bin=first_bin)
        assert t.dtype == torch.int64 and t.device == dev and tuple(t.shape) == (11, nr)
        torch.cuda.synchronize()
        assert np.array_equal(t.cpu().numpy().view(np.uint64), got)  # bit for bit the host form
        t = bands.scc_moments_tensor(tid, bands, tid)  # no scratch band: not waited for
        torch.cuda.synchronize()
        assert np.array_equal(t.cpu().numpy().view(np.uint64), same)
        for include_zeros in (False, True):
            scc, rho, weight = bands.scc(tid, others, rid, h, include_zeros=include_zeros, factor=k, first_bin=first_bin)
            mine = pixels.scc_scores(want, nc, 1, hi, include_zeros)
            assert scc == mine[0] and -1.0 <= scc <= 1.0
            assert np.array_equal(rho, mine[1], equal_nan=True) and np.array_equal(weight, mine[2])
        assert bands.scc(tid, bands, tid)[0] == 1.0
        # shapes that differ, and a reference on another device
        with pytest.raises(ValueError):
            bands.scc_moments(tid, others, rid)
        with pytest.raises(ValueError):
            bands.scc_moments_tensor(tid, others, rid, factor=2)
        elsewhere = api.LoadedBands(1)
        with pytest.raises(ValueError):
            bands.scc(tid, elsewhere, 0)
        assert np.array_equal(bands.band(tid).cpu().numpy().view(np.uint32), fine)
