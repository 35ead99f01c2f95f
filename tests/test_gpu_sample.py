"""The random sampling of a band on the MI355X (include/modle_pixels.h: modle_pixels_sample, _sample_to_host;
modle_amd/pixels.py; api.Simulator.sample and sample_tensors): the kept and the rest band equal, word for
word, the numpy restatement of tests/test_sample_outputs.py, which shares no code with the kernel.  The
bands are built on the host with a seeded generator and lie between poisoned guard words; the outputs are
poisoned before the call (the library, not the caller, defines every word), and in every input band the
words that are no pixels hold 0xFFFFFFFF: a kernel that interpreted one would draw 2^32 - 1 trials for it.
Nothing here has a tolerance."""
import functools

import numpy as np
import pytest

from test_dots_outputs import candidate_pixels
from test_gpu_marginals import FRONT, POISON, Guarded, make_band, reference_marginals
from test_sample_outputs import SALTS, SEEDS, T1, THRESHOLDS, reference_sample

pytestmark = pytest.mark.gpu

# (nrows, ncols) around the wave of 64 words and the workgroup of 2048: the smallest band; one diagonal;
# all triangle; a column shorter than a wave; one below / exactly / one past a wave; more than one
# workgroup; nine workgroups and a column longer than a workgroup's stride of 256 words
SHAPES = [(1, 1), (1, 7), (3, 3), (7, 30), (63, 65), (64, 64), (65, 130), (70, 300), (257, 321)]
FILLS = ["empty", "tenth", "full", "decay", "giants"]
GIANT = 2**20 + 3


def pixel_words(nrows, ncols):
    """(w, i, j) of the words of the band that are pixels"""
    w = np.arange(nrows * ncols, dtype=np.int64)
    j, d = w // nrows, w % nrows
    ok = d <= j
    return w[ok], (j - d)[ok], j[ok]


@functools.lru_cache(maxsize=None)
def band_of(nrows, ncols, fill):
    """the input band, poisoned where it holds no pixel (computed once per case and left unchanged)"""
    if fill in ("empty", "tenth", "full"):
        band = make_band(nrows, ncols, fill, limit=40, seed=3)
    else:
        band = make_band(nrows, ncols, "empty")
        w, i, j = pixel_words(nrows, ncols)
        rng = np.random.default_rng([5, nrows, ncols])
        if fill == "decay":
            band[w] = rng.poisson(600.0 / (j - i + 1.0))
        else:
            band[w[rng.random(len(w)) < 0.05]] = 3
            band[0] = GIANT                      # the diagonal of column 0
            band[nrows * ncols - 1] = GIANT      # the last word of the last column
            col = min(ncols - 1, 40)             # the tier boundary in adjacent words of one column
            for d, n in enumerate((T1 - 1, T1, T1 + 1, 4 * 64 + T1, 4 * 64 + T1 + 1)):
                if d <= min(col, nrows - 1) and col * nrows + d not in (0, nrows * ncols - 1):
                    band[col * nrows + d] = n
    band.setflags(write=False)
    return band


def reference_bands(band, nrows, ncols, threshold, seed, salt=0, bin_offset=0):
    """(kept, rest) in the band's layout, zeros in the words that are no pixels"""
    w, i, j = pixel_words(nrows, ncols)
    kept, rest = np.zeros(nrows * ncols + 1, dtype=np.uint32), np.zeros(nrows * ncols + 1, dtype=np.uint32)
    kept[w] = reference_sample(i + bin_offset, j + bin_offset, band[w], threshold, seed, salt)
    rest[w] = band[w] - kept[w]
    return kept, rest


def out_buffer(nrows, ncols):
    return Guarded(np.full(nrows * ncols + 1, POISON, dtype=np.uint32))  # the caller does not pre-zero


def words(buf):
    return buf.read()[FRONT:FRONT + buf.n]


def stats_of(band, nrows, ncols):
    from modle_amd import pixels

    v = band[pixel_words(nrows, ncols)[0]]
    return pixels.Stats(int((v != 0).sum()), int(v.sum(dtype=np.uint64)), int(v.max(initial=0)))


@pytest.fixture(scope="module")
def ex():
    from modle_amd import pixels

    with pixels.Extractor(0) as e:
        yield e


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("nrows,ncols", SHAPES)
def test_kept_and_rest_equal_the_definition(ex, nrows, ncols, fill):
    band = band_of(nrows, ncols, fill)
    src, stats = Guarded(band), stats_of(band, nrows, ncols)
    assert ex.count(src.data_ptr(), nrows, ncols) == stats
    for k, threshold in enumerate(THRESHOLDS):
        seed, salt = SEEDS[k % 2], SALTS[(k // 2) % 2]
        want_kept, want_rest = reference_bands(band, nrows, ncols, threshold, seed, salt)
        d_kept, d_rest = out_buffer(nrows, ncols), out_buffer(nrows, ncols)
        ex.sample_into(src.data_ptr(), nrows, ncols, threshold, seed, stats, d_kept.data_ptr(), d_rest.data_ptr(), salt)
        assert np.array_equal(words(d_kept), want_kept), (threshold, seed, salt)
        assert np.array_equal(words(d_rest), want_rest), (threshold, seed, salt)
        assert d_kept.guards_intact() and d_rest.guards_intact()
    assert src.unchanged()


@pytest.mark.parametrize("nrows,ncols,fill", [(1, 1, "full"), (65, 130, "decay"), (257, 321, "tenth")])
def test_each_output_alone(ex, nrows, ncols, fill):
    band = band_of(nrows, ncols, fill)
    src, stats = Guarded(band), stats_of(band, nrows, ncols)
    want_kept, want_rest = reference_bands(band, nrows, ncols, 2**31, 9)
    d_kept, d_rest = out_buffer(nrows, ncols), out_buffer(nrows, ncols)
    ex.sample_into(src.data_ptr(), nrows, ncols, 2**31, 9, stats, d_kept.data_ptr(), None)
    assert np.array_equal(words(d_kept), want_kept) and d_kept.guards_intact() and d_rest.unchanged()
    d_kept = out_buffer(nrows, ncols)
    ex.sample_into(src.data_ptr(), nrows, ncols, 2**31, 9, stats, None, d_rest.data_ptr())
    assert np.array_equal(words(d_rest), want_rest) and d_rest.guards_intact() and d_kept.unchanged()
    assert src.unchanged()


@pytest.mark.parametrize("nrows,ncols,fill,more", [(7, 30, "full", 1), (63, 65, "decay", 2), (70, 300, "giants", 187)])
def test_the_same_pixels_in_a_deeper_band_give_the_same_words(ex, nrows, ncols, fill, more):
    band = band_of(nrows, ncols, fill)
    deep = make_band(nrows + more, ncols, "empty")
    w, i, j = pixel_words(nrows, ncols)
    deep[j * (nrows + more) + (j - i)] = band[w]
    src, stats = Guarded(deep), stats_of(band, nrows, ncols)
    d_kept = out_buffer(nrows + more, ncols)
    ex.sample_into(src.data_ptr(), nrows + more, ncols, THRESHOLDS[-1], 5, stats, d_kept.data_ptr(), None)
    want = reference_bands(band, nrows, ncols, THRESHOLDS[-1], 5)[0]
    got = words(d_kept)
    assert np.array_equal(got[j * (nrows + more) + (j - i)], want[w]) and int(got.sum()) == int(want.sum())
    assert want.any() and src.unchanged()


@pytest.mark.parametrize("nrows,ncols,fill", [(7, 30, "full"), (65, 130, "giants")])
def test_the_offset_shifts_the_ids(ex, nrows, ncols, fill):
    band = band_of(nrows, ncols, fill)
    src, stats = Guarded(band), stats_of(band, nrows, ncols)
    plain = reference_bands(band, nrows, ncols, 2**31, 4, 1)[0]
    for off in (12345, 2**32 - ncols):  # the second: the last bin is 2^32 - 1
        want_kept, want_rest = reference_bands(band, nrows, ncols, 2**31, 4, 1, off)
        assert not np.array_equal(want_kept, plain)
        d_kept, d_rest = out_buffer(nrows, ncols), out_buffer(nrows, ncols)
        ex.sample_into(src.data_ptr(), nrows, ncols, 2**31, 4, stats, d_kept.data_ptr(), d_rest.data_ptr(), 1, off)
        assert np.array_equal(words(d_kept), want_kept) and np.array_equal(words(d_rest), want_rest)


def test_two_streams_give_the_same_words(ex):
    import torch

    nrows, ncols = 70, 300
    band = band_of(nrows, ncols, "decay")
    src, stats = Guarded(band), stats_of(band, nrows, ncols)
    outs = []
    for _ in range(2):
        stream = torch.cuda.Stream(device="cuda:0")
        assert stream.cuda_stream != 0
        out = out_buffer(nrows, ncols)
        ex.sample_into(src.data_ptr(), nrows, ncols, THRESHOLDS[-1], 77, stats, out.data_ptr(), None, stream=stream)
        stream.synchronize()
        outs.append(words(out))
    assert np.array_equal(outs[0], outs[1])
    assert np.array_equal(outs[0], reference_bands(band, nrows, ncols, THRESHOLDS[-1], 77)[0])


@pytest.mark.parametrize("nrows,ncols,fill", [(1, 7, "full"), (64, 64, "decay"), (257, 321, "tenth"), (3, 3, "empty")])
def test_the_host_form_is_the_extraction_of_the_sampled_band(ex, nrows, ncols, fill):
    from modle_amd import pixels

    band = band_of(nrows, ncols, fill)
    src = Guarded(band)
    for off in (0, 4000):
        for which, want in enumerate(reference_bands(band, nrows, ncols, 2**31, 6, 0, off)):
            b1, b2, cnt = candidate_pixels(want, nrows, ncols)
            got = ex.sample(src.data_ptr(), nrows, ncols, 2**31, 6, bin_offset=off, rest=bool(which))
            assert np.array_equal(got.bin1, b1 + off) and np.array_equal(got.bin2, b2 + off)
            assert np.array_equal(got.count, cnt) and got.count.dtype == np.int32
            assert got.stats == pixels.Stats(len(cnt), int(cnt.sum()), int(cnt.max(initial=0)))
            assert len(got.bin1_offset) == ncols + 1 and got.bin1_offset[-1] == len(cnt)
    again = pixels.sample(src.data_ptr(), nrows, ncols, 2**31, 6, bin_offset=4000, rest=True)
    assert np.array_equal(again.count, cnt)
    assert src.unchanged()


def test_invalid_calls_are_refused_and_write_nothing(ex):
    from modle_amd import pixels

    nrows, ncols = 9, 12
    band = make_band(nrows, ncols, "full", limit=40, seed=8)
    src, stats = Guarded(band), stats_of(band, nrows, ncols)
    d_kept, d_rest = out_buffer(nrows, ncols), out_buffer(nrows, ncols)
    b, k, r = src.data_ptr(), d_kept.data_ptr(), d_rest.data_ptr()
    nb = 4 * (nrows * ncols + 1)
    forged = pixels.Stats(1, pixels.MAX_SAMPLE_TRIALS + 1, 1)  # no such band is built
    half = 2**31
    for what, code, args, kw in [
            ("no band", pixels.ERR_ARG, (None, nrows, ncols, half, 1, stats, k, r), {}),
            ("no stats", pixels.ERR_ARG, (b, nrows, ncols, half, 1, None, k, r), {}),
            ("no output", pixels.ERR_ARG, (b, nrows, ncols, half, 1, stats, None, None), {}),
            ("threshold above 2^32", pixels.ERR_ARG, (b, nrows, ncols, 2**32 + 1, 1, stats, k, r), {}),
            ("nrows 0", pixels.ERR_ARG, (b, 0, ncols, half, 1, stats, k, r), {}),
            ("an empty band", pixels.ERR_ARG, (b, 0, 0, half, 1, stats, k, r), {}),
            ("nrows > ncols", pixels.ERR_ARG, (b, ncols + 1, ncols, half, 1, stats, k, r), {}),
            ("kept is the band", pixels.ERR_ARG, (b, nrows, ncols, half, 1, stats, b, r), {}),
            ("kept begins in the band's trailing word", pixels.ERR_ARG, (b, nrows, ncols, half, 1, stats, b + nb - 4, r), {}),
            ("rest ends in the band's first word", pixels.ERR_ARG, (b, nrows, ncols, half, 1, stats, k, b - nb + 4), {}),
            ("the outputs overlap", pixels.ERR_ARG, (b, nrows, ncols, half, 1, stats, k, k + nb - 4), {}),
            ("the outputs are one", pixels.ERR_ARG, (b, nrows, ncols, half, 1, stats, k, k), {}),
            ("a negative offset", pixels.ERR_RANGE, (b, nrows, ncols, half, 1, stats, k, r), {"bin_offset": -1}),
            ("the last bin is 2^32", pixels.ERR_RANGE, (b, nrows, ncols, half, 1, stats, k, r), {"bin_offset": 2**32 - ncols + 1}),
            ("an offset of 2^63 - 1", pixels.ERR_RANGE, (b, nrows, ncols, half, 1, stats, k, r), {"bin_offset": 2**63 - 1}),
            ("a sum above the cap", pixels.ERR_RANGE, (b, nrows, ncols, half, 1, forged, k, r), {}),
            ("a sum above the cap, all kept", pixels.ERR_RANGE, (b, nrows, ncols, 2**32, 1, forged, k, r), {})]:
        with pytest.raises(pixels.PixelsError) as e:
            ex.sample_into(*args, **kw)
        assert e.value.code == code, what
    for kw, code in [({"threshold": 2**32 + 1}, pixels.ERR_ARG), ({"bin_offset": -1}, pixels.ERR_RANGE),
                     ({"bin_offset": 2**32 - ncols + 1}, pixels.ERR_RANGE), ({"salt": 2**32}, pixels.ERR_ARG),
                     ({"seed": -1}, pixels.ERR_ARG)]:
        call = dict(threshold=half, seed=1)
        call.update(kw)
        with pytest.raises(pixels.PixelsError) as e:
            ex.sample(b, nrows, ncols, **call)
        assert e.value.code == code, kw
    with pytest.raises(pixels.PixelsError) as e:
        ex.sample(None, nrows, ncols, half, 1)
    assert e.value.code == pixels.ERR_ARG
    assert d_kept.unchanged() and d_rest.unchanged() and src.unchanged()  # (still poison)
    # the cap itself is accepted, and a sum that is too small changes nothing
    want = reference_bands(band, nrows, ncols, half, 1)
    for st in (pixels.Stats(1, pixels.MAX_SAMPLE_TRIALS, 1), pixels.Stats(0, 0, 0)):
        d_kept, d_rest = out_buffer(nrows, ncols), out_buffer(nrows, ncols)
        ex.sample_into(b, nrows, ncols, half, 1, st, d_kept.data_ptr(), d_rest.data_ptr())
        assert np.array_equal(words(d_kept), want[0]) and np.array_equal(words(d_rest), want[1])


def test_simulator_tensors_feed_the_other_calls():
    """the interval of tests/test_gpu_marginals.py's test of the same kind (80 x 200, 4 cells):
    sample_tensors -> pixels.marginals on the tensor gives the marginals of the restatement, and sample()
    its pixels"""
    import torch

    from modle_amd import api, driver, genome, pixels

    rng = np.random.default_rng(4)
    barriers = "".join(f"chrA\t{p}\t{p + 19}\t.\t{rng.uniform(0.6, 1.0):.3f}\t{'+' if rng.random() < 0.5 else '-'}\n"
                       for p in sorted(rng.choice(1_200_000 - 100, size=16, replace=False)))
    cfg = api.make_config(bin_size=5000, diagonal_width=400_000, num_cells=4, target_contact_density=0.5, seed=5)
    _, ivs, _ = genome.import_genome_text(cfg, "chrA\t1200000\n", barriers, "chrA\t25000\t1025000\n")
    plan = driver.plan_genome(cfg, ivs)
    nrows, ncols = plan[0]["nrows"], plan[0]["ncols"]
    sim = api.Simulator(cfg, 0)
    try:
        iid = driver.enqueue_plan(sim, cfg, plan)[0]
        sim.launch()
        sim.wait()
        band, _, _ = sim.copy_outputs(iid)
        assert band[:-1].any()
        frac, seed, salt, off = 0.3, 2**40 + 3, 9, 1000
        want_kept, want_rest = reference_bands(band, nrows, ncols, pixels.sample_threshold(frac), seed, salt, off)
        assert want_kept.any() and want_rest.any()
        kept, rest = sim.sample_tensors(iid, frac, seed, salt, off, rest=True)
        only = sim.sample_tensors(iid, frac, seed, salt, off)
        for t in (kept, rest, only):
            assert t.dtype == torch.int32 and t.device == torch.device("cuda", 0) and t.numel() == nrows * ncols + 1
        for t, want in ((kept, want_kept), (rest, want_rest), (only, want_kept)):
            diag_sum, coverage = pixels.marginals(t.data_ptr(), nrows, ncols, 2)
            want_diag, want_cov = reference_marginals(want, nrows, ncols, 2)
            assert np.array_equal(diag_sum, want_diag) and np.array_equal(coverage, want_cov)
            assert np.array_equal(t.cpu().numpy().view(np.uint32), want)
        for got, want in zip(sim.sample(iid, frac, seed, salt, off, rest=True) + (sim.sample(iid, frac, seed, salt, off),),
                             (want_kept, want_rest, want_kept)):
            b1, b2, cnt = candidate_pixels(want, nrows, ncols)
            assert np.array_equal(got.bin1, b1 + off) and np.array_equal(got.bin2, b2 + off)
            assert np.array_equal(got.count, cnt)
        assert np.array_equal(sim.copy_outputs(iid)[0], band)
    finally:
        sim.close()
