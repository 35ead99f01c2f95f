"""The statistical test of the dot calling without a GPU (include/modle_pixels.h: modle_pixels_dot_hist, _dots_fdr;
modle_amd/pixels.py: dot_lambda_edges, poisson_tail, dot_thresholds; driver.check_dot_hist and the thresholds file;
the options --dots-fdr and --dots-lambda-chunks): the lambda-chunk histogram and the threshold decision restated
in numpy, sharing no code with the library and held to cases worked by hand; dot_thresholds against a second
restatement in 60-digit decimal arithmetic; the Poisson tail against the decimal one."""
import decimal
import functools
import os

import numpy as np
import pytest

from modle_amd import cli, driver, pixels
from test_dots_outputs import parse, prefix, run_preflight, sat_dot_sums, valid_mask  # noqa: F401 (prefix: a fixture)

D = decimal.Decimal


# ---- the definition, restated -------------------------------------------------------------------------

def reference_chunks(sums, lam, edges):
    """int [4, ncols, nrows]: the lambda chunk of every word for every neighbourhood -- np.float64(O_k) * lam, the
    number of edges strictly below it, a NaN in the top chunk (only the valid words mean anything)"""
    with np.errstate(invalid="ignore"):  # 0 * inf
        lambdas = sums.astype(np.float64) * np.asarray(lam, dtype=np.float64)[:, None, :]
    chunks = np.searchsorted(np.asarray(edges, dtype=np.float64), lambdas, side="left")
    chunks[np.isnan(lambdas)] = len(edges)
    return chunks


def reference_hist(band, nrows, ncols, sums, lam, edges, n_obs, w, min_diag):
    """uint64 [4, len(edges) + 1, n_obs]: one for every valid pixel and neighbourhood at [k][chunk][min(obs, n_obs - 1)]"""
    valid = valid_mask(nrows, ncols, w, min_diag)
    obs = band[:nrows * ncols].reshape(ncols, nrows)[valid].astype(np.int64)
    chunks = reference_chunks(sums, lam, edges)
    hist = np.zeros((4, len(edges) + 1, n_obs), dtype=np.uint64)
    for k in range(4):
        np.add.at(hist[k], (chunks[k][valid], np.minimum(obs, n_obs - 1)), np.uint64(1))
    return hist


def reference_fdr_candidates(band, nrows, ncols, sums, lam, edges, thr, scale, w, min_diag, min_count):
    """the candidate band of the threshold decision, uint32[nrows * ncols + 1]: obs where the pixel is valid, obs >=
    min_count, the threshold of its chunk is not 0 and obs reaches it for every k, and (with a scale table) the
    fold test holds for every k"""
    obs = band[:nrows * ncols].reshape(ncols, nrows)
    chunks = reference_chunks(sums, lam, edges)
    is_cand = valid_mask(nrows, ncols, w, min_diag) & (obs >= min_count)
    for k in range(4):
        t = np.asarray(thr, dtype=np.uint32)[k][chunks[k]]
        is_cand &= (t != 0) & (obs >= t)
        if scale is not None:
            with np.errstate(invalid="ignore"):
                is_cand &= obs.astype(np.float64) >= sums[k].astype(np.float64) * np.asarray(scale, dtype=np.float64)[k][None, :]
    out = np.zeros(nrows * ncols + 1, dtype=np.uint32)
    out[:-1] = np.where(is_cand, obs, 0).reshape(-1)
    return out


def band_of(matrix, nrows):
    """the band of a small symmetric matrix (its upper triangle up to diagonal nrows - 1), poison elsewhere"""
    ncols = len(matrix)
    band = np.full(nrows * ncols + 1, 0xFFFFFFFF, dtype=np.uint32)
    for j in range(ncols):
        for d in range(min(j, nrows - 1) + 1):
            band[j * nrows + d] = matrix[j - d][j]
    return band


def test_the_restatement_on_cases_worked_by_hand():
    """5 x 5, w = 1, p = 0, min_diag = 0: the one valid pixel is (1, 3), d = 2.  Its donut is the four corners (0, 2),
    (0, 4), (2, 2), (2, 4), its lower-left (2, 2), its horizontal (0 .. 2, 2) and (0 .. 2, 4), its vertical (0, 2 .. 4)
    and (2, 2 .. 4)."""
    m = np.zeros((5, 5), dtype=np.int64)
    m[0, 2], m[0, 4], m[2, 2], m[2, 4], m[1, 2], m[1, 4], m[0, 3], m[2, 3] = 1, 2, 3, 6, 10, 20, 100, 200
    edges = np.array([1.0, 3.0, 5.0])
    for obs, n_obs, at in ((7, 9, 7), (8, 9, 8), (2**32 - 1, 9, 8), (0, 2, 0), (5, 2, 1)):
        m[1, 3] = obs
        band = band_of(np.maximum(m, m.T), 5)
        sums = sat_dot_sums(band, 5, 5, 1, 0, 0)
        assert [int(s) for s in sums[:, 3, 2]] == [12, 3, 1 + 10 + 3 + 2 + 20 + 6, 1 + 100 + 2 + 3 + 200 + 6]
        lam = np.full((4, 5), np.nan)  # only d = 2 is read
        # 12 * 0.25 = 3.0 exactly, on the edge: the lower chunk (1, 3]; 3 * inf: the top; 42 * 0.1 = 4.2: chunk 2;
        # 312 * 0: lambda 0, chunk 0
        lam[:, 2] = 0.25, np.inf, 0.1, 0.0
        assert [int(c) for c in reference_chunks(sums, lam, edges)[:, 3, 2]] == [1, 3, 2, 0]
        hist = reference_hist(band, 5, 5, sums, lam, edges, n_obs, 1, 0)
        want = np.zeros((4, 4, n_obs), dtype=np.uint64)
        want[0, 1, at] = want[1, 3, at] = want[2, 2, at] = want[3, 0, at] = 1
        assert np.array_equal(hist, want), (obs, n_obs)
        # one ulp above the edge: the next chunk
        lam[0, 2] = np.nextafter(0.25, 1.0)
        assert int(reference_chunks(sums, lam, edges)[0, 3, 2]) == 2
        # the decision: every chunk's threshold is met at obs exactly, and missed one above it; a 0 never calls
        lam[0, 2] = 0.25
        thr = np.zeros((4, 4), dtype=np.uint32)
        thr[0, 1] = thr[1, 3] = thr[2, 2] = thr[3, 0] = max(obs, 1)
        called = reference_fdr_candidates(band, 5, 5, sums, lam, edges, thr, None, 1, 0, 1)
        assert int(called[3 * 5 + 2]) == obs and np.count_nonzero(called) == (obs != 0)
        if 0 < obs < 2**32 - 1:
            thr[2, 2] = obs + 1
            assert not reference_fdr_candidates(band, 5, 5, sums, lam, edges, thr, None, 1, 0, 1).any()
            thr[2, 2] = 0
            assert not reference_fdr_candidates(band, 5, 5, sums, lam, edges, thr, None, 1, 0, 1).any()
            thr[2, 2] = 1
            assert not reference_fdr_candidates(band, 5, 5, sums, lam, edges, thr, None, 1, 0, obs + 1).any()
            fold = np.zeros((4, 5))
            fold[2, 2] = obs / 42  # 42 * (obs / 42) against obs: numpy decides, as in the fold test's own file
            kept = reference_fdr_candidates(band, 5, 5, sums, lam, edges, thr, fold, 1, 0, 1).any()
            assert kept == (np.float64(obs) >= np.float64(42) * np.float64(obs / 42))
            fold[2, 2] = np.inf
            assert not reference_fdr_candidates(band, 5, 5, sums, lam, edges, thr, fold, 1, 0, 1).any()
    # 0 * inf is NaN: the top chunk
    m[:] = 0
    m[1, 3] = 4
    band = band_of(np.maximum(m, m.T), 5)
    sums = sat_dot_sums(band, 5, 5, 1, 0, 0)
    assert not sums.any()
    lam = np.full((4, 5), np.inf)
    assert [int(c) for c in reference_chunks(sums, lam, edges)[:, 3, 2]] == [3, 3, 3, 3]
    assert reference_hist(band, 5, 5, sums, lam, edges, 6, 1, 0)[:, 3, 4].tolist() == [1, 1, 1, 1]


def test_the_edges_are_those_of_hiccups():
    e = pixels.dot_lambda_edges()
    assert e.dtype == np.float64 and len(e) == 40 and e[0] == 1.0 and e[3] == 2.0 and e[39] == 8192.0
    assert np.array_equal(e, 2.0 ** (np.arange(40) / 3.0)) and (np.diff(e) > 0).all()
    assert len(pixels.dot_lambda_edges(1)) == 1 and len(pixels.dot_lambda_edges(63)) == 63
    for bad in (0, 64, -1):
        with pytest.raises(ValueError):
            pixels.dot_lambda_edges(bad)


# ---- the Poisson tail and the thresholds, in decimal ---------------------------------------------------

EDGES = pixels.dot_lambda_edges()
MEANS = [float(EDGES[i]) for i in (0, 10, 25, 39)]
N_OBS = 16384
# The largest relative error of pixels.poisson_tail against the decimal tail over t = 1, 8, 15, .. below N_OBS at the
# four means, wherever the exact tail is >= 1e-300, as measured (profiles/dots_fdr/poisson_tail_error.txt); the test
# allows 64 times that, for other builds of libm.
MEASURED_TAIL_ERROR = 5.137987060788686e-15


@functools.lru_cache(maxsize=None)
def decimal_tail(mean, n):
    """[P(Poisson(mean) >= t) for t < n] as 60-digit Decimals: the probabilities by their recurrence from exp(-mean),
    summed from far beyond n (where they are below 1e-600 of the last one wanted) downwards"""
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        mean_d = D(mean)
        top = n + int(mean) + 2200
        p, probs = (-mean_d).exp(), []
        for k in range(top + 1):
            probs.append(p)
            p = p * mean_d / (k + 1)
        tails, acc = [None] * n, D(0)
        for k in range(top, -1, -1):
            acc += probs[k]
            if k < n:
                tails[k] = acc
        return tails


def test_the_float_tail_is_the_decimal_tail():
    worst = 0.0
    for mean in MEANS:
        exact = decimal_tail(mean, N_OBS)
        got = pixels.poisson_tail(mean, N_OBS)
        assert got.dtype == np.float64 and got[0] == 1.0
        for t in range(1, N_OBS, 7):
            if exact[t] >= D("1e-300"):
                worst = max(worst, abs(float((D(float(got[t])) - exact[t]) / exact[t])))
    print(f"largest relative error of the Poisson tail: {worst!r}")
    assert worst <= 64 * MEASURED_TAIL_ERROR
    # what the naive form loses: exp(-1024) underflows, the tail at t = 1 is all but 1
    assert pixels.poisson_tail(1024.0, 2)[1] > 0.999999
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            pixels.poisson_tail(bad, 4)


def decimal_thresholds(hist, edges, fdr):
    """dot_thresholds restated: Python ints and Decimals, the rule as the header states it; asserts that every
    comparison it makes is decided with a relative margin of 1e-6"""
    n_obs = hist.shape[2]
    out = np.zeros(hist.shape[:2], dtype=np.uint32)
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        for c in range(len(edges)):
            tails = decimal_tail(float(edges[c]), n_obs)
            for k in range(4):
                counts = [int(x) for x in hist[k, c]]
                total = above = sum(counts)
                for t in range(1, n_obs):
                    above -= counts[t - 1]
                    if above == 0:
                        break
                    lhs, rhs = total * tails[t], D(fdr) * above
                    assert abs(lhs - rhs) >= D("1e-6") * max(lhs, rhs), (k, c, t)
                    if lhs <= rhs:
                        out[k, c] = t
                        break
    return out


@pytest.mark.parametrize("seed,fdr", [(1, 0.1), (2, 0.01), (3, 0.5)])
def test_the_thresholds_are_those_of_the_decimal_rule(seed, fdr):
    rng = np.random.default_rng(seed)
    hist = np.zeros((4, 41, N_OBS), dtype=np.uint64)
    for k in range(4):
        for c, share in ((0, 0.7), (10, 0.9), (25, 0.8), (39, 0.95)):
            mean = float(EDGES[c])
            draws = rng.poisson(share * mean, size=20_000 + 1000 * k)
            planted = rng.integers(int(mean + 6 * mean**0.5 + 6), int(mean + 12 * mean**0.5 + 24), size=30 + 10 * k)
            hist[k, c] = np.bincount(np.minimum(np.concatenate([draws, planted]), N_OBS - 1), minlength=N_OBS)
        # a chunk that never meets the rule: a Poisson law twice its edge has no enriched tail of its own ... and it
        # has, which is the rule's point; one that cannot: every pixel at 0
        hist[k, 5, 0] = 1000
        hist[k, 40, 3000] = 17  # the top chunk never calls
    hist[1, 10] = 0  # N = 0
    hist[2, 25, :] = 0
    hist[2, 25, N_OBS - 1] = 5  # everything in the clip bin: the rule is met where the tail itself falls to fdr
    got = pixels.dot_thresholds(hist, EDGES, fdr)
    want = decimal_thresholds(hist, EDGES, fdr)
    assert got.dtype == np.uint32 and got.shape == (4, 41)
    assert np.array_equal(got, want)
    assert not got[:, 5].any() and not got[:, 40].any() and got[1, 10] == 0
    assert float(EDGES[25]) - 40 < got[2, 25] < float(EDGES[25]) + 60
    for k, c in ((0, 0), (0, 10), (0, 25), (0, 39), (3, 39)):
        assert float(EDGES[c]) < got[k, c] < N_OBS - 1, (k, c)


def test_the_thresholds_refuse_nonsense():
    hist = np.zeros((4, 3, 5), dtype=np.uint64)
    assert not pixels.dot_thresholds(hist, [1.0, 2.0], 0.1).any()
    for args in ((hist, [1.0, 2.0, 3.0], 0.1), (hist[:3], [1.0, 2.0], 0.1), (hist.astype(np.float64), [1.0, 2.0], 0.1),
                 (hist, [1.0, 2.0], 0.0), (hist, [1.0, 2.0], 1.0), (hist, [1.0, 2.0], float("nan")),
                 (hist, [2.0, 1.0], 0.1), (hist, [0.0, 1.0], 0.1), (hist, [1.0, float("inf")], 0.1),
                 (hist[:, :, :1], [1.0, 2.0], 0.1)):
        with pytest.raises(ValueError):
            pixels.dot_thresholds(*args)


# ---- the options, the plan, the check and the file -----------------------------------------------------

def test_the_options_parse_and_preflight_plans_both_files(prefix):
    a = parse(prefix)
    assert a.dots_fdr is None and a.dots_lambda_chunks is None
    plain = run_preflight(prefix, "--dots").dots
    assert plain.fdr is None and plain.chunks == 40 and plain.thresholds_path is None
    assert plain == cli.Dots(prefix + "_dots.bedpe", 5000, 25_000, 10_000, 1, [1.75, 1.75, 1.5, 1.5], 2, 20_000)
    pre = run_preflight(prefix, "--dots", "--dots-fdr", "0.1")
    assert pre.dots == cli.Dots(prefix + "_dots.bedpe", 5000, 25_000, 10_000, 1, [1.75, 1.75, 1.5, 1.5], 2, 20_000, 0.1,
                                40, prefix + "_dots_thresholds.tsv")
    assert cli.dots_thresholds_path(prefix) == prefix + "_dots_thresholds.tsv"
    pre = run_preflight(prefix, "--dots", "--dots-fdr", "0.05", "--dots-lambda-chunks", "63", "--dots-folds", "1,1,1,1")
    assert (pre.dots.fdr, pre.dots.chunks, pre.dots.folds) == (0.05, 63, [1.0, 1.0, 1.0, 1.0])
    assert run_preflight(prefix, "--dots", "--dots-fdr", "0.1", "--dots-lambda-chunks", "1").dots.chunks == 1
    pre = run_preflight(prefix, "--dots", "--dots-fdr", "0.1", "--skip-output")
    assert pre.dots.path is None and pre.dots.thresholds_path is None and pre.dots.fdr == 0.1


@pytest.mark.parametrize("options,message", [
    (["--dots-fdr", "0.1"], "--dots-fdr needs --dots"),
    (["--dots-lambda-chunks", "40"], "--dots-lambda-chunks needs --dots"),
    (["--dots", "--dots-lambda-chunks", "40"], "--dots-lambda-chunks needs --dots-fdr"),
    (["--dots", "--dots-fdr", "0"], "--dots-fdr: 0.0 is not in (0, 1)"),
    (["--dots", "--dots-fdr", "1"], "--dots-fdr: 1.0 is not in (0, 1)"),
    (["--dots", "--dots-fdr", "-0.1"], "--dots-fdr: -0.1 is not in (0, 1)"),
    (["--dots", "--dots-fdr", "nan"], "--dots-fdr: nan is not in (0, 1)"),
    (["--dots", "--dots-fdr", "0.1", "--dots-lambda-chunks", "0"], "--dots-lambda-chunks: 0 is not in [1, 63]"),
    (["--dots", "--dots-fdr", "0.1", "--dots-lambda-chunks", "64"], "--dots-lambda-chunks: 64 is not in [1, 63]"),
])
def test_preflight_refuses_before_anything_is_made(prefix, options, message):
    with pytest.raises(SystemExit) as e:
        run_preflight(prefix, *options)
    assert str(e.value).startswith(message)
    assert not os.path.exists(os.path.dirname(prefix))


def test_the_thresholds_file_is_refused_to_be_overwritten(prefix):
    os.makedirs(os.path.dirname(prefix))
    with open(prefix + "_dots_thresholds.tsv", "wb") as fh:
        fh.write(b"precious")
    assert run_preflight(prefix, "--dots").dots.thresholds_path is None  # without the option: nobody's business
    with pytest.raises(SystemExit) as e:
        run_preflight(prefix, "--dots", "--dots-fdr", "0.1")
    assert str(e.value) == f"refusing to overwrite {prefix}_dots_thresholds.tsv: pass --force to overwrite"
    assert run_preflight(prefix, "--dots", "--dots-fdr", "0.1", "--force").dots.fdr == 0.1
    assert open(prefix + "_dots_thresholds.tsv", "rb").read() == b"precious"


def test_the_valid_pixels_of_a_band_in_closed_form():
    for nrows, ncols, w, min_diag in ((5, 5, 1, 0), (40, 63, 3, 0), (40, 65, 3, 1), (100, 135, 3, 2), (83, 201, 20, 0),
                                      (13, 13, 3, 0), (9, 12, 2, 0)):
        assert driver.dot_valid_pixels(nrows, ncols, w, min_diag) == int(valid_mask(nrows, ncols, w, min_diag).sum())


def test_the_histogram_is_checked_before_thresholds_are_taken():
    rng = np.random.default_rng(5)
    hist = np.zeros((4, 5, 7), dtype=np.uint64)
    obs = rng.integers(0, 7, size=300)
    for k in range(4):
        np.add.at(hist[k], (rng.integers(0, 5, size=300), obs), np.uint64(1))
    driver.check_dot_hist(hist, 300)
    driver.check_dot_hist(np.zeros((4, 2, 2), dtype=np.uint64), 0)
    with pytest.raises(RuntimeError) as e:
        driver.check_dot_hist(hist, 301)
    assert "the donut neighbourhood holds 300 pixels, the plan has 301 valid ones" in str(e.value)
    moved = hist.copy()  # one count moved to another count of the same chunk: the totals still hold
    c, o = np.argwhere(moved[2] > 0)[0]
    moved[2, c, o] -= 1
    moved[2, c, (o + 1) % 7] += 1
    with pytest.raises(RuntimeError) as e:
        driver.check_dot_hist(moved, 300)
    assert "horizontal" in str(e.value) and "donut" in str(e.value)
    lost = hist.copy()
    lost[3, c, np.argmax(lost[3, c])] -= 1
    with pytest.raises(RuntimeError) as e:
        driver.check_dot_hist(lost, 300)
    assert "the vertical neighbourhood holds 299 pixels" in str(e.value)
    within = hist.copy()  # moved to another chunk at the same count: the check cannot see it, and says nothing
    c1, o1 = np.argwhere(within[1] > 0)[0]
    within[1, c1, o1] -= 1
    within[1, (c1 + 1) % 5, o1] += 1
    driver.check_dot_hist(within, 300)


def test_the_lines_of_the_thresholds_file():
    assert driver.dot_thresholds_header() == "resolution\tneighbourhood\tchunk\tupper_edge\tpixels\tthreshold\n"
    hist = np.zeros((4, 3, 4), dtype=np.uint64)
    hist[0, 0], hist[0, 1], hist[3, 2, 3] = (5, 1, 0, 2), (0, 0, 7, 0), 2**40
    thr = np.zeros((4, 3), dtype=np.uint32)
    thr[0, 0], thr[0, 1] = 3, 2
    lines = driver.dot_thresholds_lines(10_000, [1.0, 2.0 ** (1 / 3)], hist, thr)
    assert len(lines) == 12
    assert lines[:3] == ["10000\tdonut\t0\t1.0\t8\t3\n", f"10000\tdonut\t1\t{2.0 ** (1 / 3)!r}\t7\t2\n",
                         "10000\tdonut\t2\tinf\t0\t0\n"]
    assert lines[3] == "10000\tlower_left\t0\t1.0\t0\t0\n" and lines[6].startswith("10000\thorizontal\t0\t")
    assert lines[11] == f"10000\tvertical\t2\tinf\t{2**40}\t0\n"
