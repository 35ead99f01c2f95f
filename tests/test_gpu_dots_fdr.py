"""The statistical test of the dot calling on the MI355X (include/modle_pixels.h: modle_pixels_dot_hist, _dot_hist_to_host,
_coarse_dot_hist_to_host, _dots_fdr, _dots_fdr_to_host, _coarse_dots_fdr_to_host; modle_amd/pixels.py; api.BandAnalyses
.dot_histogram, dot_histogram_tensor, dots(thresholds=), dots_fdr): the lambda-chunk histogram and the candidate band of
the threshold decision equal, word for word, the numpy restatement of tests/test_dots_fdr_outputs.py.  The input lies
between poisoned guard words, as in tests/test_gpu_dots.py; the table the histogram is added to holds 0xFF..FF in every
word, so the call must add to exactly those words (the sums wrap), and the candidate band and the pinned results are
poisoned before the call.  Counting is integer addition and the decision is one double product and comparisons on
both sides: nothing here has a tolerance."""
import itertools

import numpy as np
import pytest

from test_dots_fdr_outputs import reference_fdr_candidates, reference_hist
from test_dots_outputs import candidate_pixels, reference_candidates, sat_dot_sums, valid_mask
from test_gpu_dots import cand_buffer, cand_words, case, tables
from test_gpu_insulation import GuardedOut
from test_gpu_marginals import FRONT, Guarded, make_band, reference_coarsen, reference_marginals

pytestmark = pytest.mark.gpu

# (nrows, ncols, w, p, min_diag): one valid pixel; block edges (63, 65 and 2 * 64 + 2 w + 1 columns); the cap w = 20;
# many blocks in both grid directions
SHAPES = [(5, 5, 1, 0, 0), (40, 63, 3, 0, 0), (40, 65, 3, 1, 1), (100, 135, 3, 1, 2), (83, 201, 20, 7, 0),
          (200, 700, 5, 2, 2)]
FILLS = ["empty", "tenth", "full", "constant"]
N_OBS = (2, 33, 4096)  # below, across and above the 32 counts a workgroup keeps in LDS; the clip bin in all three
MINUS_ONE = np.uint64(0xFFFFFFFFFFFFFFFF)  # what a poisoned table holds


def band_and_sums(nrows, ncols, w, p, min_diag, fill):
    """`full` holds counts of 1 .. 40 (both sides of 32 and of the clip bin at 33), `tenth` counts up to 2^32"""
    return case(nrows, ncols, w, p, min_diag, fill, limit=41 if fill == "full" else 0xFFFFFFFF, seed=6)


def edge_tables(w, p):
    """one edge; HiCCUPS' 40; 63 edges that spread the lambdas of a band of counts up to 40 under a table around
    1 / area (test_gpu_dots.tables) over all chunks"""
    from modle_amd import pixels

    return [np.array([0.75]), pixels.dot_lambda_edges(), np.geomspace(0.05, 60.0, 63)]


def hist_words(buf, n_edges, n_obs):
    return buf.sums(1).reshape(4, n_edges + 1, n_obs)


@pytest.fixture(scope="module")
def ex():
    from modle_amd import pixels

    with pixels.Extractor(0) as e:
        yield e


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("nrows,ncols,w,p,min_diag", SHAPES)
def test_the_histogram_equals_the_definition(ex, nrows, ncols, w, p, min_diag, fill):
    band, sums = band_and_sums(nrows, ncols, w, p, min_diag, fill)
    n_valid = int(valid_mask(nrows, ncols, w, min_diag).sum())
    src = Guarded(band)
    lams = tables(nrows, w, p, 11)
    for n, (n_obs, edges) in enumerate(itertools.product(N_OBS, edge_tables(w, p))):
        lam = lams[(n + n // 3) % 4]
        want = reference_hist(band, nrows, ncols, sums, lam, edges, n_obs, w, min_diag)
        assert all(int(want[k].sum()) == n_valid for k in range(4))
        if fill == "full" and n_obs == 33 and n_valid > 1000 and len(edges) == 63:  # (a seeded table around 1 / area)
            assert np.count_nonzero(want[:, :, :32].sum(axis=2)) > 100 and want[:, :, 32].any()  # many chunks, both sides
        d_hist = GuardedOut(4 * (len(edges) + 1) * n_obs)
        ex.dot_hist_into(src.data_ptr(), nrows, ncols, w, p, min_diag, lam, edges, n_obs, d_hist.data_ptr())
        assert np.array_equal(hist_words(d_hist, len(edges), n_obs), want + MINUS_ONE), (n_obs, len(edges))
        if n % 4 == 0:  # two calls into one table give the sum of the two
            ex.dot_hist_into(src.data_ptr(), nrows, ncols, w, p, min_diag, lam, edges, n_obs, d_hist.data_ptr())
            assert np.array_equal(hist_words(d_hist, len(edges), n_obs), want + want + MINUS_ONE)
        assert d_hist.guards_intact()
        if n % 2 == 0:  # the one-call form zeroes a table of its own
            got = ex.dot_hist(src.data_ptr(), nrows, ncols, w, p, min_diag, lam, edges, n_obs)
            assert got.dtype == np.uint64 and np.array_equal(got, want)
    assert src.unchanged()


def seeded_thresholds(n_chunks, seed):
    rng = np.random.default_rng([seed, n_chunks])
    thr = rng.integers(1, 45, size=(4, n_chunks)).astype(np.uint32)
    thr[rng.random((4, n_chunks)) < 0.15] = 0
    thr[rng.random((4, n_chunks)) < 0.05] = 0xFFFFFFFF
    return thr


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("nrows,ncols,w,p,min_diag", SHAPES)
def test_the_candidates_equal_the_definition(ex, nrows, ncols, w, p, min_diag, fill):
    band, sums = band_and_sums(nrows, ncols, w, p, min_diag, fill)
    src = Guarded(band)
    lams, scales = tables(nrows, w, p, 12), tables(nrows, w, p, 13)
    n_called = 0
    for n, edges in enumerate(edge_tables(w, p)):
        n_chunks = len(edges) + 1
        for m, thr in enumerate((np.ones((4, n_chunks), dtype=np.uint32), np.zeros((4, n_chunks), dtype=np.uint32),
                                 seeded_thresholds(n_chunks, 14))):
            lam = lams[(n + m) % 4]
            for scale, min_count in ((None, 1), (scales[2 + (n + m) % 2], 1), (scales[0], 2)):
                want = reference_fdr_candidates(band, nrows, ncols, sums, lam, edges, thr, scale, w, min_diag, min_count)
                n_called += np.count_nonzero(want)
                if m == 1:
                    assert not want.any()
                d_cand = cand_buffer(nrows, ncols)
                ex.dots_fdr_into(src.data_ptr(), nrows, ncols, w, p, min_diag, min_count, lam, edges, thr, scale,
                                 d_cand.data_ptr())
                assert np.array_equal(cand_words(d_cand), want), (len(edges), m, min_count)
                assert d_cand.guards_intact()
                if m == 0 and scale is not None:  # thresholds of 1 with a scale table: the fold decision's own output
                    assert np.array_equal(want, reference_candidates(band, nrows, ncols, sums, scale, w, min_diag, min_count))
                    d_fold = cand_buffer(nrows, ncols)
                    ex.dots_into(src.data_ptr(), nrows, ncols, w, p, min_diag, min_count, scale, d_fold.data_ptr(), None)
                    assert np.array_equal(cand_words(d_fold), cand_words(d_cand))
    # (thresholds of 1 without a scale table call every valid pixel that is not zero)
    assert (n_called > 0) == bool(band[:nrows * ncols].reshape(ncols, nrows)[valid_mask(nrows, ncols, w, min_diag)].any())
    assert src.unchanged()


@pytest.mark.parametrize("nrows,ncols,w,p,min_diag", [SHAPES[0], SHAPES[3], SHAPES[5]])
def test_the_host_form_is_the_extraction_of_the_candidate_band(ex, nrows, ncols, w, p, min_diag):
    """counts below 2^31, which the extraction accepts; twice in a row: the same again"""
    from modle_amd import pixels

    band, sums = band_and_sums(nrows, ncols, w, p, min_diag, "full")
    src = Guarded(band)
    edges = edge_tables(w, p)[2]
    thr = seeded_thresholds(64, 15)
    lam = tables(nrows, w, p, 16)[3]
    for scale in (None, tables(nrows, w, p, 17)[2]):
        want = reference_fdr_candidates(band, nrows, ncols, sums, lam, edges, thr, scale, w, min_diag, 1)
        b1, b2, cnt = candidate_pixels(want, nrows, ncols)
        for _ in range(2):
            got = ex.dots_fdr(src.data_ptr(), nrows, ncols, w, p, min_diag, 1, lam, edges, thr, scale, bin_offset=11)
            assert got.bin1.dtype == got.bin2.dtype == np.int64 and got.count.dtype == np.int32
            assert np.array_equal(got.bin1, b1 + 11) and np.array_equal(got.bin2, b2 + 11) and np.array_equal(got.count, cnt)
            assert got.stats.nnz == len(b1) and len(got.bin1_offset) == ncols + 1 and got.bin1_offset[-1] == len(b1)
    assert src.unchanged()
    assert pixels.MAX_DOT_EDGES == 63 and pixels.MAX_DOT_OBS == 16384


def test_the_coarse_forms_are_those_of_the_coarse_band(ex):
    from modle_amd import pixels

    nrows, ncols, k, first_bin, w, p = 65, 130, 2, 1, 2, 1
    band = make_band(nrows, ncols, "tenth", limit=40, seed=3)
    coarse, nr, nc = reference_coarsen(band, nrows, ncols, k, first_bin)
    assert pixels.coarse_shape(nrows, ncols, k, first_bin) == (nr, nc) and 4 * w + 1 + 2 <= nr
    src = Guarded(band)
    sums = sat_dot_sums(coarse, nr, nc, w, p, 2)
    edges, thr = edge_tables(w, p)[2], seeded_thresholds(64, 18)
    for lam in tables(nr, w, p, 19)[2:]:
        want = reference_hist(coarse, nr, nc, sums, lam, edges, 33, w, 2)
        assert np.array_equal(ex.coarse_dot_hist(src.data_ptr(), nrows, ncols, k, first_bin, w, p, 2, lam, edges, 33), want)
        for scale in (None, tables(nr, w, p, 20)[3]):
            b1, b2, cnt = candidate_pixels(
                reference_fdr_candidates(coarse, nr, nc, sums, lam, edges, thr, scale, w, 2, 1), nr, nc)
            got = ex.coarse_dots_fdr(src.data_ptr(), nrows, ncols, k, first_bin, w, p, 2, 1, lam, edges, thr, scale)
            assert np.array_equal(got.bin1, b1) and np.array_equal(got.bin2, b2) and np.array_equal(got.count, cnt)
            assert len(got.bin1_offset) == nc + 1 and len(b1) > 0
    for call in (lambda: ex.coarse_dot_hist(src.data_ptr(), nrows, ncols, 1, 0, w, p, 2, np.zeros((4, nrows)), edges, 33),
                 lambda: ex.coarse_dots_fdr(src.data_ptr(), nrows, ncols, 1, 0, w, p, 2, 1, np.zeros((4, nrows)), edges, thr)):
        with pytest.raises(pixels.PixelsError) as e:  # a factor of 1
            call()
        assert e.value.code == pixels.ERR_ARG
    assert src.unchanged()


def test_invalid_calls_are_argument_errors_and_write_nothing(ex):
    from modle_amd import pixels

    nrows, ncols = 9, 12
    src = Guarded(make_band(nrows, ncols, "full", seed=8))
    edges = np.array([1.0, 2.0, 4.0])
    d_hist, d_cand = GuardedOut(4 * 4 * 8), cand_buffer(nrows, ncols)
    band, hist, cand = src.data_ptr(), d_hist.data_ptr(), d_cand.data_ptr()
    ok, thr = np.zeros((4, nrows)), np.ones((4, 4), dtype=np.uint32)
    nan, neg = ok.copy(), ok.copy()
    nan[2, 4], neg[0, 5] = np.nan, -1e-300
    inside = band + 4 * (nrows * ncols)  # the band's trailing word
    for what, args in [("no band", (None, nrows, ncols, 2, 1, 0, ok, edges, 8, hist)),
                       ("no table", (band, nrows, ncols, 2, 1, 0, ok, edges, 8, None)),
                       ("no lam", (band, nrows, ncols, 2, 1, 0, None, edges, 8, hist)),
                       ("nrows 0", (band, 0, ncols, 2, 1, 0, ok, edges, 8, hist)),
                       ("nrows > ncols", (band, ncols + 1, ncols, 2, 1, 0, np.zeros((4, ncols + 1)), edges, 8, hist)),
                       ("p == w", (band, nrows, ncols, 2, 2, 0, ok, edges, 8, hist)),
                       ("w == 0", (band, nrows, ncols, 0, 0, 0, ok, edges, 8, hist)),
                       ("w > 20", (band, nrows, ncols, 21, 0, 0, ok, edges, 8, hist)),
                       ("4w + 1 + min_diag > nrows", (band, nrows, ncols, 2, 0, 1, ok, edges, 8, hist)),
                       ("a NaN at a valid d", (band, nrows, ncols, 2, 1, 0, nan, edges, 8, hist)),
                       ("a negative entry at a valid d", (band, nrows, ncols, 1, 0, 0, neg, edges, 8, hist)),
                       ("no edge", (band, nrows, ncols, 2, 1, 0, ok, np.zeros(0), 8, hist)),
                       ("64 edges", (band, nrows, ncols, 2, 1, 0, ok, np.arange(1.0, 65.0), 8, hist)),
                       ("an edge of 0", (band, nrows, ncols, 2, 1, 0, ok, np.array([0.0, 1.0]), 8, hist)),
                       ("edges that do not rise", (band, nrows, ncols, 2, 1, 0, ok, np.array([1.0, 1.0]), 8, hist)),
                       ("an infinite edge", (band, nrows, ncols, 2, 1, 0, ok, np.array([1.0, np.inf]), 8, hist)),
                       ("a NaN edge", (band, nrows, ncols, 2, 1, 0, ok, np.array([np.nan]), 8, hist)),
                       ("n_obs 1", (band, nrows, ncols, 2, 1, 0, ok, edges, 1, hist)),
                       ("n_obs 16385", (band, nrows, ncols, 2, 1, 0, ok, edges, 16385, hist)),
                       ("a misaligned table", (band, nrows, ncols, 2, 1, 0, ok, edges, 8, hist + 4)),
                       ("the table overlaps the band", (band, nrows, ncols, 2, 1, 0, ok, edges, 8, inside - inside % 8))]:
        with pytest.raises(pixels.PixelsError) as e:
            ex.dot_hist_into(*args)
        assert e.value.code == pixels.ERR_ARG, what
    for what, args in [("no band", (None, nrows, ncols, 2, 1, 0, 1, ok, edges, thr, None, cand)),
                       ("no output", (band, nrows, ncols, 2, 1, 0, 1, ok, edges, thr, None, None)),
                       ("min_count 0", (band, nrows, ncols, 2, 1, 0, 0, ok, edges, thr, None, cand)),
                       ("p == w", (band, nrows, ncols, 2, 2, 0, 1, ok, edges, thr, None, cand)),
                       ("a NaN in lam", (band, nrows, ncols, 2, 1, 0, 1, nan, edges, thr, None, cand)),
                       ("a NaN in the scale", (band, nrows, ncols, 2, 1, 0, 1, ok, edges, thr, nan, cand)),
                       ("a negative scale", (band, nrows, ncols, 1, 0, 0, 1, ok, edges, thr, neg, cand)),
                       ("edges that fall", (band, nrows, ncols, 2, 1, 0, 1, ok, np.array([2.0, 1.0]), np.ones((4, 3), dtype=np.uint32), None, cand)),
                       ("d_cand overlaps the band", (band, nrows, ncols, 2, 1, 0, 1, ok, edges, thr, None, inside))]:
        with pytest.raises(pixels.PixelsError) as e:
            ex.dots_fdr_into(*args)
        assert e.value.code == pixels.ERR_ARG, what
    for bad_thr in (np.ones((4, 3), dtype=np.uint32), np.ones((3, 4), dtype=np.uint32), np.ones((4, 4)), -thr.astype(np.int64)):
        with pytest.raises(pixels.PixelsError) as e:  # refused by pixels.py
            ex.dots_fdr_into(band, nrows, ncols, 2, 1, 0, 1, ok, edges, bad_thr, None, cand)
        assert e.value.code == pixels.ERR_ARG
    for call in (lambda: ex.dot_hist(band, nrows, ncols, 2, 1, 0, nan, edges, 8),
                 lambda: ex.dot_hist(band, nrows, ncols, 2, 1, 0, ok, edges, 1),
                 lambda: ex.dot_hist(None, nrows, ncols, 2, 1, 0, ok, edges, 8),
                 lambda: ex.dots_fdr(band, nrows, ncols, 2, 1, 0, 0, ok, edges, thr),
                 lambda: ex.dots_fdr(band, nrows, ncols, 2, 1, 0, 1, ok, edges, thr, bin_offset=-1),
                 lambda: ex.dots_fdr(band, nrows, ncols, 3, 0, 0, 1, ok, edges, thr),
                 lambda: ex.coarse_dots_fdr(band, nrows, ncols, 2, 0, 2, 1, 0, 1, np.zeros((4, 5)), edges, thr)):  # nrows' is 5
        with pytest.raises(pixels.PixelsError) as e:
            call()
        assert e.value.code == pixels.ERR_ARG
    assert d_hist.unchanged() and d_cand.unchanged() and src.unchanged()  # (still poison)
    # entries outside the valid diagonals are not looked at
    outside = ok.copy()
    outside[:, :4], outside[:, 5:] = np.nan, -1.0  # w = 2, min_diag = 0: only d = 4 is read
    host_band = src.host[FRONT:FRONT + src.n]
    sums = sat_dot_sums(host_band, nrows, ncols, 2, 1, 0)
    ex.dot_hist_into(band, nrows, ncols, 2, 1, 0, outside, edges, 8, hist)
    assert np.array_equal(hist_words(d_hist, 3, 8), reference_hist(host_band, nrows, ncols, sums, ok, edges, 8, 2, 0) + MINUS_ONE)
    ex.dots_fdr_into(band, nrows, ncols, 2, 1, 0, 1, outside, edges, thr, outside, cand)
    assert np.array_equal(cand_words(d_cand),
                          reference_fdr_candidates(host_band, nrows, ncols, sums, ok, edges, thr, ok, 2, 0, 1))
    assert d_hist.guards_intact() and d_cand.guards_intact()


def test_simulator_forms_agree():
    """the interval of tests/test_gpu_dots.py's test of the same name (80 x 200, 4 cells): dot_histogram,
    dot_histogram_tensor, dots and dots_tensors with thresholds and dots_fdr give the restatement on the band copied to
    the host, at the bin size and at three times it"""
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
        folds = (1.1, 1.1, 1.05, 1.05)
        edges = np.geomspace(0.05, 20.0, 17)
        for factor, first_bin, w, p in ((1, 0, 5, 2), (3, 5, 3, 1)):
            b, nr, nc = (band, nrows, ncols) if factor == 1 else reference_coarsen(band, nrows, ncols, factor, first_bin)
            sums = sat_dot_sums(b, nr, nc, w, p, 2)
            diag_sum = reference_marginals(b, nr, nc, 0)[0]
            lam = pixels.dot_scales(diag_sum, nc, w, p, (1, 1, 1, 1), 2)
            scale = pixels.dot_scales(diag_sum, nc, w, p, folds, 2)
            pixel = np.arange(nc)[:, None] >= np.arange(nr)[None, :]  # (the words that are pixels)
            assert int(sim.contact_max(iid, factor, first_bin)) == int(b[:nr * nc].reshape(nc, nr)[pixel].max())
            n_obs = int(sim.contact_max(iid, factor, first_bin)) + 2
            want = reference_hist(b, nr, nc, sums, lam, edges, n_obs, w, 2)
            kw = dict(w=w, p=p, edges=edges, n_obs=n_obs, min_diag=2, factor=factor, first_bin=first_bin)
            got = sim.dot_histogram(iid, **kw)
            assert got.dtype == np.uint64 and np.array_equal(got, want)
            t = sim.dot_histogram_tensor(iid, **kw)
            assert t.dtype == torch.int64 and t.device == torch.device("cuda", 0) and tuple(t.shape) == want.shape
            assert sim.dot_histogram_tensor(iid, **kw, into=t) is t
            torch.cuda.synchronize()
            assert np.array_equal(t.cpu().numpy().view(np.uint64), want + want)
            driver.check_dot_hist(got, driver.dot_valid_pixels(nr, nc, w, 2))
            with pytest.raises(ValueError):
                sim.dot_histogram_tensor(iid, **kw, into=t[:, :, 1:])
            thr = pixels.dot_thresholds(want, edges, 0.2)
            b1, b2, cnt = candidate_pixels(
                reference_fdr_candidates(b, nr, nc, sums, lam, edges, thr, scale, w, 2, 1), nr, nc)
            loose = candidate_pixels(reference_candidates(b, nr, nc, sums, scale, w, 2, 1), nr, nc)[0]
            assert 0 < len(b1) < len(loose)
            kw = dict(w=w, p=p, min_count=1, folds=folds, min_diag=2, factor=factor, first_bin=first_bin)
            g1, g2, gc, ge = sim.dots(iid, **kw, thresholds=thr, edges=edges)
            assert np.array_equal(g1, b1) and np.array_equal(g2, b2) and np.array_equal(gc, cnt)
            assert np.array_equal(ge, (diag_sum.astype(np.float64) / (nc - np.arange(nr)))[b2 - b1])
            t1, t2, tc = sim.dots_tensors(iid, **kw, thresholds=thr, edges=edges)
            assert np.array_equal(t1.cpu().numpy(), b1) and np.array_equal(t2.cpu().numpy(), b2)
            assert np.array_equal(tc.cpu().numpy(), cnt)
            got_thr, per_id = sim.dots_fdr([iid], w, p, 0.2, 1, folds, 2, factor, [first_bin], edges, n_obs)
            assert np.array_equal(got_thr, thr) and list(per_id) == [iid]
            assert np.array_equal(per_id[iid][0], b1) and np.array_equal(per_id[iid][2], cnt)
        assert np.array_equal(sim.copy_outputs(iid)[0], band)
    finally:
        sim.close()
