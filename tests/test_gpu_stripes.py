"""Two bands compared stripe by stripe on the MI355X (include/modle_pixels.h: modle_pixels_stripes,
_stripes_to_host; modle_amd/pixels.py; api.BandAnalyses.stripe_moments, stripe_scores, stripe_moments_tensor):
for every non-empty mask the sums of every bin's vertical and horizontal stripe equal, word for word, the
numpy / Python-int restatement of tests/test_stripes_outputs.py, for bands built on the host with a seeded
generator.  The inputs lie between poisoned guard words at an address that is 4-byte aligned only, the output
at an 8-byte aligned address between guard words, poisoned before the call (the library, not the caller,
defines every word), and in every input band the words that are no pixels hold 0xFFFFFFFF: they must not be
read as counts.  Nothing the kernels write has a tolerance; the scores of the api are held against
evaluate.compare with the tolerance of tests/test_stripes_outputs.py."""
import numpy as np
import pytest

from test_gpu_insulation import GuardedOut
from test_gpu_marginals import FRONT, POISON, Guarded, reference_coarsen
from test_stripes_outputs import MASKED, MOMENTS, RANKS, ROWS, TOLERANCE, restate

pytestmark = pytest.mark.gpu

# (nrows, ncols) around the wave of 64 entries and the four loads in flight of the vertical kernel (256), the 64
# stripes a workgroup of the horizontal kernel owns, the powers of two the rank kernel pads to and the 256
# threads of its workgroup: a band one word wide; all triangle; one below and one past a wave, a power of two
# exactly; one past 256 and past 1024; the reference's default band depth; the cap (2 x 67 MB; `tenth` only)
SHAPES = [(1, 1), (1, 7), (5, 5), (5, 9), (63, 65), (64, 64), (65, 130), (255, 300), (256, 256), (257, 321),
          (600, 700), (1024, 1030), (1025, 1100), (4096, 4100)]
FILLS = ["empty", "tenth", "full", "ties", "distinct"]
CASES = [(nr, nc, fill) for nr, nc in SHAPES for fill in FILLS if fill == "tenth" or nr < 4096]
BLOCK = {MOMENTS: slice(0, 9), MASKED: slice(9, 18), RANKS: slice(18, 21)}  # the rows of the mask 7


def make_pair(nrows, ncols, fill, seed=0):
    """the reference and the target band: `empty` zeros; `tenth` a tenth of the pixels with counts up to
    0xFFFFFFFE, each band its own; `full` every pixel 0xFFFFFFFF in both; `ties` counts of 0, 1 and 2;
    `distinct` each band a permutation of 1 .. nrows * ncols, so that no two entries of a stripe tie but
    its padding.  The words that are no pixels hold 0xFFFFFFFF."""
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
        elif fill == "distinct":
            band[:-1] = rng.permutation(n) + 1
        for j in range(min(nrows, ncols)):
            band[j * nrows + j + 1:(j + 1) * nrows] = POISON
        band[n] = POISON
        bands.append(band)
    return bands


def rows_of(all_rows, what):
    """the rows of the mask `what` out of those of the mask 7: the blocks in bit order"""
    return np.concatenate([all_rows[:, BLOCK[b]] for b in (MOMENTS, MASKED, RANKS) if what & b], axis=1)


@pytest.fixture(scope="module")
def ex():
    from modle_amd import pixels

    with pixels.Extractor(0) as e:
        yield e


@pytest.mark.parametrize("nrows,ncols,fill", CASES)
def test_stripes_equal_the_restatement(ex, nrows, ncols, fill):
    a, b = make_pair(nrows, ncols, fill)
    want = restate(a, b, nrows, ncols, 7)
    if fill == "full" and nrows >= 2:
        assert want[:, [4, 6, 8]].any(axis=(0, 2)).all() and want[:, [13, 15, 17]].any(axis=(0, 2)).all()  # beyond 2^64
    if fill == "empty":
        assert not want[:, 1:18].any() and (want[:, 0] == nrows).all()
    ref, tgt = Guarded(a), Guarded(b)
    assert ref.data_ptr() % 8 == 4
    for what in ROWS:
        words = 2 * ROWS[what] * ncols
        d_out = GuardedOut(words)
        ex.stripes_into(ref.data_ptr(), tgt.data_ptr(), nrows, ncols, what, d_out.data_ptr(), words)
        assert np.array_equal(d_out.sums(2 * ROWS[what]).reshape(2, ROWS[what], ncols), rows_of(want, what)), what
        assert d_out.guards_intact()
    for _ in range(2):  # the host form, twice: the same again
        got = ex.stripes(ref.data_ptr(), tgt.data_ptr(), nrows, ncols, 7)
        assert got.dtype == np.uint64 and got.shape == (2, 21, ncols)
        assert np.array_equal(got, want)
    assert ref.unchanged() and tgt.unchanged()


@pytest.mark.parametrize("nrows,ncols,fill", [(5, 9, "ties"), (65, 130, "tenth"), (600, 700, "distinct")])
def test_a_band_against_itself_through_one_pointer(ex, nrows, ncols, fill):
    from modle_amd import pixels

    a, _ = make_pair(nrows, ncols, fill, seed=1)
    src = Guarded(a)
    got = ex.stripes(src.data_ptr(), src.data_ptr(), nrows, ncols, 7)
    assert np.array_equal(got, restate(a, a, nrows, ncols, 7))
    for d in (0, 1):
        assert not pixels.stripe_scores(got[d], "rmse").any()
        p = pixels.stripe_scores(got[d], "pearson")
        assert ((p == 1.0) | np.isnan(p)).all()
    assert np.array_equal(pixels.stripes(src.data_ptr(), src.data_ptr(), nrows, ncols, MOMENTS | RANKS),
                          rows_of(got, MOMENTS | RANKS))  # the module-level form
    assert src.unchanged()


def test_a_stream_of_the_caller_and_buffers_that_grow():
    import torch

    from modle_amd import pixels

    stream = torch.cuda.Stream(device="cuda:0")
    assert stream.cuda_stream != 0
    small, large = make_pair(5, 9, "ties", seed=2), make_pair(70, 193, "tenth", seed=2)
    want_small, want_large = restate(*small, 5, 9, 7), restate(*large, 70, 193, 7)
    s, l = [Guarded(x) for x in small], [Guarded(x) for x in large]
    with pixels.Extractor(0) as e:
        first = e.stripes(s[0].data_ptr(), s[1].data_ptr(), 5, 9, 7, stream=stream)
        again = e.stripes(l[0].data_ptr(), l[1].data_ptr(), 70, 193, 7, stream=stream)  # grows
        assert np.array_equal(again, want_large)
        d_out = GuardedOut(2 * 21 * 9)
        e.stripes_into(s[0].data_ptr(), s[1].data_ptr(), 5, 9, 7, d_out.data_ptr(), 2 * 21 * 9, stream=stream)
        shrunk = e.stripes(s[0].data_ptr(), s[1].data_ptr(), 5, 9, MASKED, stream=stream)  # reused
        stream.synchronize()
        assert np.array_equal(d_out.sums(42).reshape(2, 21, 9), want_small) and d_out.guards_intact()
        assert np.array_equal(shrunk, rows_of(want_small, MASKED))
        assert np.array_equal(first, want_small)  # the caller's
    assert all(g.unchanged() for g in s + l)


def test_invalid_calls_are_argument_errors_and_write_nothing(ex):
    from modle_amd import pixels

    nrows, ncols = 5, 9
    a, b = make_pair(nrows, ncols, "ties", seed=3)
    ref, tgt = Guarded(a), Guarded(b)
    words = 2 * 9 * ncols
    d_out = GuardedOut(2 * 21 * ncols)
    out, r, t = d_out.data_ptr(), ref.data_ptr(), tgt.data_ptr()
    inside = r + 4 * (nrows * ncols)  # the band's trailing word: the last that is the band's
    inside -= inside % 8
    for name, args in [("what == 0", (r, t, nrows, ncols, 0, out, words)),
                       ("an unknown bit", (r, t, nrows, ncols, 9, out, words)),
                       ("only an unknown bit", (r, t, nrows, ncols, 8, out, words)),
                       ("ranks above the cap", (r, t, 4097, 5000, 4, out, 2 * 3 * 5000)),
                       ("no reference", (None, t, nrows, ncols, 1, out, words)),
                       ("no target", (r, None, nrows, ncols, 1, out, words)),
                       ("no output", (r, t, nrows, ncols, 1, None, words)),
                       ("out_words too small", (r, t, nrows, ncols, 1, out, words - 1)),
                       ("out_words too large", (r, t, nrows, ncols, 1, out, words + 1)),
                       ("out_words of another mask", (r, t, nrows, ncols, 7, out, words)),
                       ("a misaligned output", (r, t, nrows, ncols, 1, out + 4, words)),
                       ("the output overlaps the reference", (r, t, nrows, ncols, 1, inside, words)),
                       ("the output ends inside the target", (r, t, nrows, ncols, 1, t - t % 8 - 8 * words + 8, words)),
                       ("nrows > ncols", (r, t, ncols + 1, ncols, 1, out, 2 * 9 * ncols)),
                       ("nrows 0", (r, t, 0, ncols, 1, out, words))]:
        with pytest.raises(pixels.PixelsError) as e:
            ex.stripes_into(*args)
        assert e.value.code == pixels.ERR_ARG, name
    for args in [(r, t, nrows, ncols, 0), (r, t, nrows, ncols, 8), (r, t, 4097, 5000, 5), (None, t, nrows, ncols, 1),
                 (r, None, nrows, ncols, 1), (r, t, ncols + 1, ncols, 1), (r, t, 0, ncols, 1)]:
        with pytest.raises(pixels.PixelsError) as e:
            ex.stripes(*args)
        assert e.value.code == pixels.ERR_ARG, args
    assert d_out.unchanged() and ref.unchanged() and tgt.unchanged()  # (still poison)
    # the cap itself is accepted by the check (the shape of the last case of the table above runs it)
    assert pixels.MAX_STRIPE == 4096 and SHAPES[-1][0] == 4096


def test_the_api_forms_agree():
    """two bands that lie on the device as api.LoadedBands holds them: the target is coarsened by 3 from fine
    bin 2 on the device and compared with a reference of the coarse shape -- the restatement on
    reference_coarsen's band --, the torch form holds the same words, and the scores are pixels.stripe_scores
    of the sums and evaluate.compare's within the tolerance"""
    import torch

    from modle_amd import api, evaluate, pixels

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
        want = restate(ref, coarse, nr, nc, 7)
        got = bands.stripe_moments(tid, others, rid, 7, factor=k, first_bin=first_bin)
        assert got.dtype == np.uint64 and got.shape == (2, 21, nc) and np.array_equal(got, want)
        assert np.array_equal(bands.stripe_moments(tid, others, rid, factor=k, first_bin=first_bin), want[:, :9])
        # the other way round: the coarsened band is the reference
        assert np.array_equal(others.stripe_moments(rid, bands, tid, 7, other_factor=k, other_first_bin=first_bin),
                              restate(coarse, ref, nr, nc, 7))
        # a band against itself, at the bin size
        assert np.array_equal(bands.stripe_moments(tid, bands, tid, MOMENTS), restate(fine, fine, nrows, ncols, MOMENTS))
        for what in (7, MASKED | RANKS):
            t = bands.stripe_moments_tensor(tid, others, rid, what, factor=k, first_bin=first_bin)
            assert t.dtype == torch.int64 and t.device == dev and tuple(t.shape) == (2, ROWS[what], nc)
            torch.cuda.synchronize()
            assert np.array_equal(t.cpu().numpy().view(np.uint64), rows_of(want, what))
        t = bands.stripe_moments_tensor(tid, bands, tid, MOMENTS)  # no scratch band: not waited for
        torch.cuda.synchronize()
        assert np.array_equal(t.cpu().numpy().view(np.uint64), restate(fine, fine, nrows, ncols, MOMENTS))
        for metric in pixels.STRIPE_METRICS:
            for masked in (False, True):
                if metric == "spearman" and masked:
                    with pytest.raises(ValueError):
                        bands.stripe_scores(tid, others, rid, metric, True, factor=k, first_bin=first_bin)
                    continue
                v, h = bands.stripe_scores(tid, others, rid, metric, masked, factor=k, first_bin=first_bin)
                for d, (scores, direction) in enumerate(((v, "vertical"), (h, "horizontal"))):
                    assert np.array_equal(scores, pixels.stripe_scores(want[d], metric, masked), equal_nan=True)
                    host = evaluate.compare(ref, coarse, nr, nc, metric, direction, masked)[0]
                    assert np.array_equal(np.isnan(scores), np.isnan(host))
                    ok = ~np.isnan(host)
                    scale = np.maximum(host[ok], 1.0) if metric in ("rmse", "eucl_dist") else 1.0
                    assert (np.abs(scores[ok] - host[ok]) / scale <= TOLERANCE[metric]).all(), (metric, direction)
        # shapes that differ, and a reference on another device
        with pytest.raises(ValueError):
            bands.stripe_moments(tid, others, rid)
        with pytest.raises(ValueError):
            bands.stripe_moments(tid, others, rid, factor=2)
        elsewhere = api.LoadedBands(1)
        with pytest.raises(ValueError):
            bands.stripe_moments(tid, elsewhere, 0)
        assert np.array_equal(bands.band(tid).cpu().numpy().view(np.uint32), fine)
