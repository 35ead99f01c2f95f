"""The analysis kernels of libmodle_pixels.so on bands as long as a real chromosome's (include/modle_pixels.h;
modle_amd/pixels.py).  The other GPU modules stop at 700 columns (4100 for the stripes): there pixels_scan takes
one trip of its 1024 threads and never carries a total into the next, band_check never strides to a second
pixel, and nothing lies beyond column 1024.  Here the bands have 1023 to 8200 columns and the pixel list of
the band loader 347 585 entries, and every result is held, word for word, against the restatements the
other modules already use (imported from where they live; none is restated here).  Bands lie between
poisoned guard words with 0xFFFFFFFF in every word that is no pixel, outputs are poisoned before the call,
the sources must come back unchanged.  Nothing here has a tolerance.

The last test holds stripes_ranks at its real grid cap of 2^20 workgroups, on a band of 2^20 + 70 columns,
against the closed form of tests/test_stripes_shallow.py.  The loops no band of a test can reach on the
default build (the fill's grid y, the other stripes kernels) are run by tests/test_gpu_pixels_smallgrid.py."""
import functools

import numpy as np
import pytest

from test_band_outputs import ERR_ORDER, ERR_RANGE, reference_band, reference_order
from test_dots_outputs import candidate_pixels, reference_candidates, sat_dot_sums, valid_mask
from test_gpu_band import Dev64, band_pixels, check_list, counts_dev, host_band, poisoned_band
from test_gpu_coarsen import assert_pixels, reference_coarsen, reference_pixels
from test_gpu_dense import reference_dense
from test_gpu_dots import cand_buffer, cand_words, tables
from test_gpu_insulation import FRONT8, GuardedOut
from test_gpu_marginals import POISON, Guarded, make_band, output_buffer, reference_marginals
from test_gpu_pileup import run as run_pileup
from test_gpu_sample import out_buffer, pixel_words, reference_bands, stats_of, words
from test_gpu_stripes import make_pair, rows_of
from test_insulation_outputs import prefix_insulation
from test_pileup_outputs import reference_accepts, reference_pileup
from test_sample_outputs import T1
from test_stripes_outputs import ROWS, restate
from test_stripes_shallow import restate_shallow

pytestmark = pytest.mark.gpu

SCAN = 1024  # kScanThreads (modle_pixels.hip): the columns of one trip of pixels_scan
# one below, exactly and one past one trip; the same for two; three trips and a ragged fourth -- each one word
# and three words deep -- and the depths of a real band at a real length (nine trips)
SMALL = [(nr, nc) for nc in (1023, 1024, 1025, 2048, 2049, 3077) for nr in (1, 3)]
LARGE = [(70, 8200), (600, 8200)]
EXTRACT = [(nr, nc, fill) for nr, nc in SMALL for fill in ("empty", "tenth", "full")] + \
          [(nr, nc, fill) for nr, nc in LARGE for fill in ("tenth", "full")]
# (nrows, ncols, factor, first_bin): every factor leaves more than 1024 coarse columns (asserted)
COARSE = [(1, 2048, 2, 1), (3, 2048, 2, 1), (1, 2049, 2, 0), (3, 2049, 2, 0), (1, 3077, 3, 2), (3, 3077, 2, 1),
          (70, 8200, 8, 5), (600, 8200, 2, 1), (600, 8200, 7, 3)]
ANALYSED = [(3, 3077), (70, 8200)]  # where the other analyses run
CHECK = 262144  # kCheckGroups * kCheckThreads (modle_band.hip): the pixels of one trip of band_check


@pytest.fixture(scope="module")
def ex():
    from modle_amd import pixels

    assert pixels.build_caps() == pixels.DEFAULT_BUILD_CAPS  # (the shapes below are chosen for these)
    assert (pixels.DEFAULT_BUILD_CAPS.scan_threads, pixels.DEFAULT_BUILD_CAPS.check_groups * 256) == (SCAN, CHECK)
    with pixels.Extractor(0) as e:
        yield e


def beyond(ncols, *marks):
    """the marks 1024, 2048, 4096 that the band has columns beyond"""
    return [m for m in (marks or (1024, 2048, 4096)) if m + 1 < ncols]


# ---- extraction: the carry of pixels_scan ----------------------------------------------------------------------

@pytest.mark.parametrize("nrows,ncols,fill", EXTRACT)
def test_extraction_across_the_trips_of_the_scan(ex, nrows, ncols, fill):
    band = make_band(nrows, ncols, fill, limit=2**31)
    ref = reference_pixels(band, nrows, ncols)
    if fill == "empty":
        assert ref["nnz"] == 0
    else:  # the first trip hands a total on (a band of 1023 columns has one trip only)
        assert ref["bin1_offset"][min(SCAN, ncols)] > 0
    if fill == "full":
        assert ref["nnz"] == nrows * ncols - nrows * (nrows - 1) // 2
    src = Guarded(band)
    assert_pixels(ex.extract(src.data_ptr(), nrows, ncols), ref)
    if nrows <= 70:  # ids beyond 32 bits; the same buffers again
        offset = 3_000_000_000
        assert_pixels(ex.extract(src.data_ptr(), nrows, ncols, bin_offset=offset), ref, offset)
    assert src.unchanged()


def carry_bands(nrows, ncols):
    """name -> band: pixels in the last column only (they belong to the last `nrows` rows: the carry is 0 until
    one of the last two trips); pixels in row 0 only (the whole total is carried from the first trip to the end); exactly one
    pixel in every row, on a diagonal that changes from row to row (bin1_offset is 0, 1, 2, ...)"""
    def blank():
        return make_band(nrows, ncols, "empty")

    last, row0, one = blank(), blank(), blank()
    d = np.arange(nrows, dtype=np.int64)
    last[(ncols - 1) * nrows + d] = 1 + d
    row0[d * nrows + d] = 7 + d
    i = np.arange(ncols, dtype=np.int64)
    di = (5 * i) % np.minimum(nrows, ncols - i)
    one[(i + di) * nrows + di] = 1 + (i % 1000)
    return {"last column": last, "row 0": row0, "one per row": one}


@pytest.mark.parametrize("nrows,ncols", [(1, 2049), (3, 3077), (70, 8200)])
def test_the_carry_of_the_scan_on_bands_built_for_it(ex, nrows, ncols):
    bands = carry_bands(nrows, ncols)
    for name, band in bands.items():
        assert not (band[:-1][band[:-1] != POISON] >= 2**31).any()
        ref = reference_pixels(band, nrows, ncols)
        off = ref["bin1_offset"]
        if name == "last column":
            assert ref["nnz"] == nrows and not off[:ncols - nrows + 1].any()
            assert (ncols - nrows) // SCAN >= (ncols - 1) // SCAN - 1 >= 1
        elif name == "row 0":
            assert ref["nnz"] == nrows and (off[1:] == nrows).all()
        else:
            assert np.array_equal(off, np.arange(ncols + 1))
        src = Guarded(band)
        assert_pixels(ex.extract(src.data_ptr(), nrows, ncols), ref)
        assert src.unchanged(), name


@pytest.mark.parametrize("nrows,ncols,k,first_bin", COARSE)
def test_coarse_bands_of_more_columns_than_a_trip(ex, nrows, ncols, k, first_bin):
    from modle_amd import pixels

    band = make_band(nrows, ncols, "tenth" if nrows > 3 else "full", limit=2**20, seed=1)
    ref, nr, nc = reference_coarsen(band, nrows, ncols, k, first_bin)
    assert nc > SCAN and int(ref.max()) < 2**31  # the scan of the coarse band carries; no sum saturates
    assert pixels.coarse_shape(nrows, ncols, k, first_bin) == (nr, nc)
    src, dst = Guarded(band), Guarded(np.full(nr * nc + 1, POISON, dtype=np.uint32))
    assert ex.coarsen_into(src.data_ptr(), nrows, ncols, k, first_bin, dst.data_ptr(), nr * nc + 1) == (nr, nc)
    assert np.array_equal(words(dst), ref)  # the whole buffer: sums, and zeros in the triangle and the last word
    assert dst.guards_intact()
    want = reference_pixels(ref, nr, nc)
    assert want["bin1_offset"][SCAN] > 0 and want["nnz"] > want["bin1_offset"][SCAN]
    assert_pixels(ex.coarse_extract(src.data_ptr(), nrows, ncols, k, first_bin), want)
    assert_pixels(ex.coarse_extract(src.data_ptr(), nrows, ncols, k, first_bin, bin_offset=3_000_000_000), want,
                  3_000_000_000)
    assert src.unchanged()


# ---- band loading: the stride of band_check ----------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def long_list():
    """the pixels of a full band of 70 x 5000: 347 585 of them, a second trip of 85 441 for band_check"""
    nrows, ncols = 70, 5000
    band = host_band(nrows, ncols, "full")
    b1, b2, cn = band_pixels(band, nrows, ncols)
    assert len(b1) == 347585 and CHECK < len(b1) < 2 * CHECK
    for a in (b1, b2, cn):
        a.setflags(write=False)
    return nrows, ncols, band, b1, b2, cn


@pytest.mark.parametrize("n", [None, CHECK, CHECK + 1])
def test_a_list_longer_than_the_grid_of_the_check(ex, n):
    """the whole list; exactly one trip; one trip and a single pixel in the second"""
    nrows, ncols, band, b1, b2, cn = long_list()
    b1, b2, cn = b1[:n], b2[:n], cn[:n]
    got = check_list(ex, nrows, ncols, b1, b2, cn, 0)  # check, fill and from-host against reference_band
    if n is None:
        assert np.array_equal(got, np.where(band == POISON, 0, band))
    # ... and the extraction of the band that was filled is the list
    src = Guarded(got)
    px = ex.extract(src.data_ptr(), nrows, ncols)
    assert np.array_equal(px.bin1, b1) and np.array_equal(px.bin2, b2) and np.array_equal(px.count, cn)
    assert px.stats.nnz == len(b1) and src.unchanged()


def spoilt_long_lists():
    """name -> (bin1, bin2, count, code, first_bad): the violations that only the second trip of band_check sees"""
    _, _, _, b1, b2, cn = long_list()

    def swapped(*at):  # the entries k - 1 and k change places: entry k is not after its predecessor
        s1, s2 = b1.copy(), b2.copy()
        for k in at:
            s1[[k - 1, k]], s2[[k - 1, k]] = s1[[k, k - 1]], s2[[k, k - 1]]
        return s1, s2

    def negative(*at):
        c = cn.copy()
        c[list(at)] = [-1 - 4 * n for n in range(len(at))]
        return c

    return {
        "order twice in the second trip": (*swapped(CHECK + 1, CHECK + 50001), cn, ERR_ORDER, CHECK + 1),
        "sign twice in the second trip": (b1, b2, negative(CHECK + 1, CHECK + 70000), ERR_RANGE, CHECK + 1),
        "order at the first pixel of the second trip, a sign behind it":
            (*swapped(CHECK), negative(CHECK + 3), ERR_ORDER, CHECK),
        "order in each trip": (*swapped(1001, CHECK + 1001), cn, ERR_ORDER, 1001),
        "sign in the first trip, order in the second": (*swapped(CHECK + 1001), negative(500), ERR_RANGE, 500),
        "order in the first trip, an earlier sign in the second: by index, not by lane":
            (*swapped(CHECK - 5), negative(CHECK + 2), ERR_ORDER, CHECK - 5),
    }


@pytest.mark.parametrize("case", range(6))
def test_the_smallest_bad_index_of_a_long_list(ex, case):
    from modle_amd import pixels

    nrows, ncols = long_list()[:2]
    what, (b1, b2, cn, code, first_bad) = list(spoilt_long_lists().items())[case]
    assert reference_order(b1, b2, cn) == (code, first_bad), what
    _, st = reference_band(nrows, ncols, b1, b2, cn, 0)
    assert st["first_bad"] == first_bad
    d1, d2, dc = Dev64(b1), Dev64(b2), counts_dev(cn)
    with pytest.raises(pixels.BandListError) as e:
        ex.band_check(d1.data_ptr(), d2.data_ptr(), dc.data_ptr(), len(b1), nrows, ncols, 0)
    assert e.value.code == code and e.value.stats._asdict() == st and str(first_bad) in str(e.value), what
    out = poisoned_band(nrows, ncols)
    with pytest.raises(pixels.BandListError) as e:
        ex.band_from_host(b1, b2, cn, nrows, ncols, 0, out.data_ptr(), out.n)
    assert e.value.code == code and e.value.stats.first_bad == first_bad
    assert out.unchanged() and d1.unchanged() and d2.unchanged() and dc.unchanged()


# ---- the analyses beyond column 1024 -------------------------------------------------------------------------

@pytest.mark.parametrize("fill", ["tenth", "full"])
@pytest.mark.parametrize("nrows,ncols", ANALYSED)
def test_marginals_of_a_long_band(ex, nrows, ncols, fill):
    band = make_band(nrows, ncols, fill)
    src = Guarded(band)
    for m in (0, 1, 2, nrows):
        want_diag, want_cov = reference_marginals(band, nrows, ncols, m)
        assert (m >= nrows) != bool(want_cov[1024:].any())  # (the bins beyond column 1024 hold something)
        d_diag, d_cov = output_buffer(nrows), output_buffer(ncols)
        ex.marginals_into(src.data_ptr(), nrows, ncols, m, d_diag.data_ptr(), d_cov.data_ptr())
        assert np.array_equal(d_diag.sums(), want_diag) and np.array_equal(d_cov.sums(), want_cov), m
        assert d_diag.guards_intact() and d_cov.guards_intact()
        diag, cov = ex.marginals(src.data_ptr(), nrows, ncols, m)
        assert np.array_equal(diag, want_diag) and np.array_equal(cov, want_cov), m
    assert src.unchanged()


@pytest.mark.parametrize("fill", ["tenth", "full"])
@pytest.mark.parametrize("nrows,ncols,windows", [(3, 3077, [2, 1]), (70, 8200, [35, 8, 1])])
def test_insulation_of_a_long_band(ex, nrows, ncols, windows, fill):
    band = make_band(nrows, ncols, fill)
    src = Guarded(band)
    for m in (0, 2):
        want = prefix_insulation(band, nrows, ncols, windows, m)
        if fill == "full":  # every diamond of the largest window beyond column 1024 holds something
            assert windows[0] == max(windows) and want[0, 1024:ncols - windows[0]].all()
        d_out = GuardedOut(len(windows) * ncols)
        ex.insulation_into(src.data_ptr(), nrows, ncols, windows, m, d_out.data_ptr(), len(windows) * ncols)
        assert np.array_equal(d_out.sums(len(windows)), want), m
        assert d_out.guards_intact()
        assert np.array_equal(ex.insulation(src.data_ptr(), nrows, ncols, windows, m), want), m
    assert src.unchanged()


# (nrows, ncols, first, size, step, count): tiles beyond column 1024 that straddle 2048 (both) and 4096
DENSE = [(3, 3077, 1000, 1100, 900, 2), (70, 8200, 1990, 130, 2040, 3)]


@pytest.mark.parametrize("fill", ["tenth", "full"])
@pytest.mark.parametrize("nrows,ncols,first,size,step,count", DENSE)
def test_dense_regions_of_a_long_band(ex, nrows, ncols, first, size, step, count, fill):
    from modle_amd import pixels

    tiles = [(first + t * step, first + t * step + size) for t in range(count)]
    assert tiles[-1][1] <= ncols and all(hi > 1024 for _, hi in tiles)
    for mark in beyond(ncols, 2048, 4096):
        assert any(lo < mark < hi for lo, hi in tiles), mark
    band = make_band(nrows, ncols, fill, limit=2**31)
    ref = reference_dense(band, nrows, first, size, step, count)
    assert not (ref == POISON).any() and ref.any(axis=(1, 2)).all()
    assert pixels.tiles_fit(ncols, first, size, step) >= count
    n_words = count * size * size
    src, dst = Guarded(band), Guarded(np.full(n_words, POISON, dtype=np.uint32))
    ex.dense_tiles_into(src.data_ptr(), nrows, ncols, first, size, step, count, dst.data_ptr(), n_words)
    assert np.array_equal(words(dst).reshape(count, size, size), ref)
    assert dst.guards_intact()
    lo, hi = tiles[-1]
    assert np.array_equal(ex.dense(src.data_ptr(), nrows, ncols, lo, hi), ref[-1])
    assert src.unchanged()


def long_anchors(nrows, ncols, f):
    """anchors whose windows lie beyond column 1024, among them windows across the marks, and a few that are
    refused"""
    rng = np.random.default_rng([11, nrows, ncols, f])
    dmax = nrows - 1 - 2 * f
    m = 3000
    d = rng.integers(0, dmax + 1, size=m)
    a = 1024 + f + 1 + (rng.random(m) * (ncols - 1024 - 2 * f - 1 - d)).astype(np.int64)
    marks = [(x, x + min(dmax, 3)) for mark in beyond(ncols, 2048, 4096) for x in (mark - 1, mark, mark - f)]
    refused = [(-1, 5), (ncols - f, ncols - f), (2000, 1999), (1500, 1500 + dmax + 1)]
    a = np.concatenate([a, [p[0] for p in marks + refused]])
    b = np.concatenate([a[:m] + d, [p[1] for p in marks + refused]])
    order = rng.permutation(len(a))
    return a[order].astype(np.int64), b[order].astype(np.int64), len(marks), len(refused)


@pytest.mark.parametrize("fill", ["tenth", "full"])
@pytest.mark.parametrize("nrows,ncols,f", [(3, 3077, 1), (70, 8200, 32)])
def test_pileups_around_anchors_of_a_long_band(ex, nrows, ncols, f, fill):
    band = make_band(nrows, ncols, fill)
    a, b, n_marks, n_refused = long_anchors(nrows, ncols, f)
    ok = reference_accepts(nrows, ncols, f, a, b)
    assert int(ok.sum()) == len(a) - n_refused and (a[ok] - f > 1024).all()  # every window beyond column 1024
    for mark in beyond(ncols, 2048, 4096):  # windows with the mark inside their columns, and inside their rows
        assert ((b[ok] - f < mark) & (mark <= b[ok] + f)).any() and ((a[ok] - f < mark) & (mark <= a[ok] + f)).any()
    want, used = reference_pileup(band, nrows, ncols, f, a, b)
    assert used == int(ok.sum()) and want.all()
    src = Guarded(band)
    pile, n_used = run_pileup(ex, src, nrows, ncols, f, a, b)
    assert n_used == used and np.array_equal(pile, want)
    pile, n_used = ex.pileup(src.data_ptr(), nrows, ncols, f, a + 77, b + 77, bin_offset=77)
    assert n_used == used and np.array_equal(pile, want)
    assert src.unchanged()


# (45, 4200): the summed-area table of the restatement is ncols^2 words; (70, 8200) is its largest affordable
@pytest.mark.parametrize("nrows,ncols,w,p,min_diag", [(45, 4200, 5, 2, 2), (70, 8200, 5, 4, 0)])
def test_dots_of_a_long_band(ex, nrows, ncols, w, p, min_diag):
    band = make_band(nrows, ncols, "tenth", limit=2**31, seed=4)
    sums = sat_dot_sums(band, nrows, ncols, w, p, min_diag)
    valid = valid_mask(nrows, ncols, w, min_diag)
    for mark in beyond(ncols):  # valid pixels on either side of the marks, with something in their neighbourhoods
        assert valid[mark - 1].any() and valid[mark].any() and sums[0, mark - 1:mark + 1].any()
    src = Guarded(band)
    for n, table in enumerate(tables(nrows, w, p, 1)[0:3:2]):  # all zeros, and a seeded table
        want = reference_candidates(band, nrows, ncols, sums, table, w, min_diag, 1)
        b1, b2, cnt = candidate_pixels(want, nrows, ncols)
        assert len(b1) > 0
        if n == 0:  # candidates beyond every mark: the extraction of the candidate band carries, too
            assert all((b1 > mark).sum() > 10 for mark in beyond(ncols))
        d_cand, d_sums = cand_buffer(nrows, ncols), GuardedOut(4 * nrows * ncols)
        ex.dots_into(src.data_ptr(), nrows, ncols, w, p, min_diag, 1, table, d_cand.data_ptr(), d_sums.data_ptr())
        assert np.array_equal(d_sums.sums(4).reshape(4, ncols, nrows), sums), n
        assert np.array_equal(cand_words(d_cand), want), n
        assert d_cand.guards_intact() and d_sums.guards_intact()
        got = ex.dots(src.data_ptr(), nrows, ncols, w, p, min_diag, 1, table, bin_offset=11)
        assert np.array_equal(got.bin1, b1 + 11) and np.array_equal(got.bin2, b2 + 11)
        assert np.array_equal(got.count, cnt) and got.bin1_offset[-1] == len(b1) == got.stats.nnz
        assert np.array_equal(got.bin1_offset, np.searchsorted(b1, np.arange(ncols + 1), side="left"))
    assert src.unchanged()


@functools.lru_cache(maxsize=None)
def sampled_band(nrows, ncols):
    """a tenth of the pixels with 1 to 39 contacts -- ten blocks of Philox words at most, so that the restatement
    stays at a few hundred thousand blocks -- and, in columns beyond the marks, the trial counts around the tier
    boundary and one pixel of 2^18 + 3 contacts"""
    band = make_band(nrows, ncols, "tenth", limit=40, seed=3)
    for mark in beyond(ncols):
        for d, n in enumerate((T1 - 1, T1, T1 + 1, 4 * 64 + T1 + 1, 2**18 + 3)[:2 * nrows - 1]):
            band[(mark + 3 + d // nrows) * nrows + d % nrows] = n
    band.setflags(write=False)
    return band


@pytest.mark.parametrize("nrows,ncols", ANALYSED)
def test_sampling_of_a_long_band(ex, nrows, ncols):
    from modle_amd import pixels

    band = sampled_band(nrows, ncols)
    w, i, j = pixel_words(nrows, ncols)
    far = (band[w] != 0) & (j > 1024)
    assert int(far.sum()) >= 500 and int((band[w][far] > pixels.SAMPLE_TIER1_TRIALS).sum()) >= 1
    assert int(band[w].sum(dtype=np.uint64)) < 2_500_000  # (the restatement forms a quarter as many blocks)
    src, stats = Guarded(band), stats_of(band, nrows, ncols)
    assert ex.count(src.data_ptr(), nrows, ncols) == stats
    for threshold, seed, salt in ((2**31, 7, 0), (pixels.sample_threshold(0.1), 0x9E3779B97F4A7C15, 0xDEADBEEF)):
        want_kept, want_rest = reference_bands(band, nrows, ncols, threshold, seed, salt)
        assert 0 < int(want_kept.sum()) < stats.sum
        d_kept, d_rest = out_buffer(nrows, ncols), out_buffer(nrows, ncols)
        ex.sample_into(src.data_ptr(), nrows, ncols, threshold, seed, stats, d_kept.data_ptr(), d_rest.data_ptr(), salt)
        assert np.array_equal(words(d_kept), want_kept) and np.array_equal(words(d_rest), want_rest), threshold
        assert d_kept.guards_intact() and d_rest.guards_intact()
        # the host form: the extraction of the sampled band, whose scan carries
        b1, b2, cnt = candidate_pixels(want_kept, nrows, ncols)
        got = ex.sample(src.data_ptr(), nrows, ncols, threshold, seed, salt)
        assert np.array_equal(got.bin1, b1) and np.array_equal(got.bin2, b2) and np.array_equal(got.count, cnt)
        assert np.array_equal(got.bin1_offset, np.searchsorted(b1, np.arange(ncols + 1), side="left"))
    assert src.unchanged()


@pytest.mark.parametrize("fill", ["tenth", "ties"])
@pytest.mark.parametrize("nrows,ncols", ANALYSED)
def test_stripes_of_a_long_band(ex, nrows, ncols, fill):
    a, b = make_pair(nrows, ncols, fill)
    want = restate(a, b, nrows, ncols, 7)
    assert want[:, 1:3, ncols - nrows:].any()  # (the last stripes hold something)
    ref, tgt = Guarded(a), Guarded(b)
    for what in ROWS:
        n_words = 2 * ROWS[what] * ncols
        d_out = GuardedOut(n_words)
        ex.stripes_into(ref.data_ptr(), tgt.data_ptr(), nrows, ncols, what, d_out.data_ptr(), n_words)
        assert np.array_equal(d_out.sums(2 * ROWS[what]).reshape(2, ROWS[what], ncols), rows_of(want, what)), what
        assert d_out.guards_intact()
    assert np.array_equal(ex.stripes(ref.data_ptr(), tgt.data_ptr(), nrows, ncols, 7), want)
    assert ref.unchanged() and tgt.unchanged()


# ---- stripes_ranks at its real grid cap ------------------------------------------------------------------------

def test_the_rank_kernel_strides_beyond_its_grid_of_two_to_the_twenty(ex):
    """3 x (2^20 + 70): the workgroups 0 .. 69 of stripes_ranks take a second stripe each, reusing their keys in
    LDS; the moments are formed in the same call (their grids, a quarter and a 64th of the columns, stay below
    the cap: tests/test_gpu_pixels_smallgrid.py strides them).  The bands mix counts of 0 .. 2, which tie in
    most stripes, with counts up to 2^32 - 2."""
    from modle_amd import pixels

    nrows, ncols = 3, 2**20 + 70
    assert ncols > pixels.DEFAULT_BUILD_CAPS.stripes_grid and nrows <= 3
    ties, tenth = make_pair(nrows, ncols, "ties"), make_pair(nrows, ncols, "tenth", seed=1)
    a, b = (np.where(t != 0, t, s) for s, t in zip(ties, tenth))
    assert (a[-1], b[-1], a[1], b[2]) == (POISON,) * 4  # the trailing word and the triangle stay poisoned
    want = restate_shallow(a, b, nrows, ncols, 7)
    head = 300  # the vertical stripes of the first columns are those of the first columns alone: restate() once more
    assert np.array_equal(want[0, :, :head], restate(a[:nrows * head + 1], b[:nrows * head + 1], nrows, head, 7)[0])
    assert len(np.unique(want[:, 18:21, 2**20:])) > 3  # the second trip sees more than one kind of stripe
    ref, tgt = Guarded(a), Guarded(b)
    n_words = 2 * 21 * ncols
    d_out = GuardedOut(n_words)
    ex.stripes_into(ref.data_ptr(), tgt.data_ptr(), nrows, ncols, 7, d_out.data_ptr(), n_words)
    raw = d_out.read()  # (350 MB cross to the host once)
    assert (raw[:FRONT8] == POISON).all() and (raw[FRONT8 + d_out.n:] == POISON).all()
    got = raw[FRONT8:FRONT8 + d_out.n].view(np.uint64).reshape(2, 21, ncols)
    for block, name in ((slice(18, 21), "ranks"), (slice(0, 9), "moments"), (slice(9, 18), "masked moments")):
        diff = np.argwhere(got[:, block] != want[:, block])
        assert len(diff) == 0, (name, "first difference at (direction, row, column)", diff[0].tolist())
    assert ref.unchanged() and tgt.unchanged()
