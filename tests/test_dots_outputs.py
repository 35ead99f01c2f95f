"""Dot calling without a GPU: the definition of the four HiCCUPS neighbourhood sums restated twice (a brute
force over the footprint offsets and a summed-area form, which tests/test_gpu_dots.py holds the kernel
to), pixels.dot_areas and dot_scales, the candidate rule in numpy, api.cluster_dots, the lines of
<prefix>_dots.bedpe, what driver.check_dots and dots_misfit refuse and what cli.preflight refuses."""
import os
from fractions import Fraction

import numpy as np
import pytest

from modle_amd import api, cli, driver, pixels
from test_gpu_marginals import make_band, reference_marginals
from test_insulation_outputs import entry


# ---- the definition, twice ------------------------------------------------------------------------

def footprints(w, p):
    """the offsets (a, b) from (row i, column j) of the four neighbourhoods, written from their ranges"""
    donut = [(a, b) for a in range(-w, w + 1) for b in range(-w, w + 1)
             if not (abs(a) <= p and abs(b) <= p) and a != 0 and b != 0]
    lower_left = [(a, b) for a in range(1, w + 1) for b in range(-w, 0) if not (a <= p and b >= -p)]
    horizontal = [(a, b) for a in (-1, 0, 1) for b in list(range(-w, -p)) + list(range(p + 1, w + 1))]
    vertical = [(a, b) for a in list(range(-w, -p)) + list(range(p + 1, w + 1)) for b in (-1, 0, 1)]
    return [donut, lower_left, horizontal, vertical]


def valid_mask(nrows, ncols, w, min_diag):
    """[ncols, nrows] bool: whether word (j, d) is a valid pixel"""
    j, d = np.arange(ncols)[:, None], np.arange(nrows)[None, :]
    return (j - d >= w) & (j + w < ncols) & (d >= 2 * w + min_diag) & (d <= nrows - 1 - 2 * w)


def symmetric(band, nrows, ncols):
    """the pixels of the band as a dense symmetric uint64 matrix; the words that are no pixels are not read"""
    m = np.zeros((ncols, ncols), dtype=np.uint64)
    for j in range(ncols):
        for d in range(min(j, nrows - 1) + 1):
            m[j - d, j] = m[j, j - d] = band[j * nrows + d]
    return m


def brute_dot_sums(band, nrows, ncols, w, p, min_diag):
    """uint64 [4, ncols, nrows]: O_k at the valid pixels, by a loop over the offsets on the symmetric matrix"""
    m, out = symmetric(band, nrows, ncols), np.zeros((4, ncols, nrows), dtype=np.uint64)
    valid = valid_mask(nrows, ncols, w, min_diag)
    for k, offsets in enumerate(footprints(w, p)):
        for j, d in zip(*np.nonzero(valid)):
            out[k, j, d] = sum(int(m[j - d + a, j + b]) for a, b in offsets)
    return out


def sat_dot_sums(band, nrows, ncols, w, p, min_diag):
    """the same from a summed-area table of the upper triangle (the square of a valid pixel lies in it)"""
    upper = np.zeros((ncols, ncols), dtype=np.uint64)
    for d in range(nrows):
        j = np.arange(d, ncols)
        upper[j - d, j] = band[j * nrows + d]
    sat = np.zeros((ncols + 1, ncols + 1), dtype=np.uint64)
    sat[1:, 1:] = upper.cumsum(axis=0, dtype=np.uint64).cumsum(axis=1, dtype=np.uint64)
    out = np.zeros((4, ncols, nrows), dtype=np.uint64)
    J, D = np.nonzero(valid_mask(nrows, ncols, w, min_diag))
    i, j = J - D, J

    def rect(ra, rb, ca, cb):  # rows ra .. rb, columns ca .. cb, inclusive; uint64 arithmetic wraps and is exact
        return sat[rb + 1, cb + 1] - sat[ra, cb + 1] - sat[rb + 1, ca] + sat[ra, ca]

    out[0, J, D] = (rect(i - w, i + w, j - w, j + w) - rect(i - p, i + p, j - p, j + p)
                    - rect(i, i, j - w, j - p - 1) - rect(i, i, j + p + 1, j + w)
                    - rect(i - w, i - p - 1, j, j) - rect(i + p + 1, i + w, j, j))
    out[1, J, D] = rect(i + 1, i + w, j - w, j - 1) - rect(i + 1, i + p, j - p, j - 1)
    out[2, J, D] = rect(i - 1, i + 1, j - w, j - p - 1) + rect(i - 1, i + 1, j + p + 1, j + w)
    out[3, J, D] = rect(i - w, i - p - 1, j - 1, j + 1) + rect(i + p + 1, i + w, j - 1, j + 1)
    return out


def reference_candidates(band, nrows, ncols, sums, scale, w, min_diag, min_count):
    """the candidate band, uint32[nrows * ncols + 1]: obs where the pixel is valid, obs >= min_count and
    (double)obs >= (double)O_k * scale[k][d] for every k -- numpy's own double product and comparison"""
    obs = band[:nrows * ncols].reshape(ncols, nrows)
    is_cand = valid_mask(nrows, ncols, w, min_diag) & (obs >= min_count)
    with np.errstate(invalid="ignore"):  # 0 * inf is NaN, and a comparison with NaN is false
        for k in range(4):
            is_cand &= obs.astype(np.float64) >= sums[k].astype(np.float64) * np.asarray(scale, dtype=np.float64)[k][None, :]
    out = np.zeros(nrows * ncols + 1, dtype=np.uint32)
    out[:-1] = np.where(is_cand, obs, 0).reshape(-1)
    return out


def candidate_pixels(cand, nrows, ncols):
    """(bin1, bin2, count) of the non-zero words of a candidate band, in cooler order"""
    words = cand[:nrows * ncols].reshape(ncols, nrows)
    j, d = np.nonzero(words)
    order = np.lexsort((j, j - d))
    return (j - d)[order].astype(np.int64), j[order].astype(np.int64), words[j, d][order].astype(np.int32)


SMALL = [(5, 5, 1, 0, 0), (5, 4, 1, 0, 0), (9, 9, 2, 1, 0), (7, 30, 1, 0, 2), (13, 20, 3, 0, 0), (13, 20, 3, 2, 0),
         (15, 17, 3, 1, 2), (21, 26, 5, 4, 0)]


@pytest.mark.parametrize("nrows,ncols,w,p,min_diag", SMALL)
def test_the_brute_force_definition_and_the_summed_area_form_agree(nrows, ncols, w, p, min_diag):
    n_valid = int(valid_mask(nrows, ncols, w, min_diag).sum())
    if nrows == 5:
        assert n_valid == (1 if ncols == 5 else 0)  # exactly one valid pixel; none
    for fill in ("tenth", "full"):
        band = make_band(nrows, ncols, fill, seed=1)
        brute = brute_dot_sums(band, nrows, ncols, w, p, min_diag)
        assert np.array_equal(sat_dot_sums(band, nrows, ncols, w, p, min_diag), brute)
        assert not brute[:, ~valid_mask(nrows, ncols, w, min_diag)].any()
        if fill == "full" and n_valid:
            assert brute[0].max() > 0


@pytest.mark.parametrize("w,p", [(1, 0), (2, 0), (2, 1), (5, 2), (7, 4), (20, 0), (20, 19), (20, 7)])
def test_the_areas_count_the_offsets(w, p):
    assert pixels.dot_areas(w, p) == tuple(len(f) for f in footprints(w, p))
    assert pixels.dot_areas(w, p) == ((2 * w + 1) ** 2 - (2 * p + 1) ** 2 - 4 * (w - p), w * w - p * p, 6 * (w - p),
                                      6 * (w - p))
    assert [sorted(f) for f in pixels.dot_offsets(w, p)] == [sorted(f) for f in footprints(w, p)]
    assert pixels.dot_areas(20, 0)[0] + 1 + 80 == 1681  # the square of the cap: what bounds a sum below 2^43


def test_the_areas_refuse_a_peak_that_is_no_peak():
    for w, p in [(1, 1), (0, 0), (3, 5), (2, -1)]:
        with pytest.raises(ValueError):
            pixels.dot_areas(w, p)
        with pytest.raises(ValueError):
            pixels.dot_offsets(w, p)


@pytest.mark.parametrize("nrows,ncols,w,p,min_diag", SMALL)
def test_on_a_constant_band_every_sum_is_the_area_times_the_constant(nrows, ncols, w, p, min_diag):
    band = make_band(nrows, ncols, "empty")
    pixel = band == 0  # make_band poisons the words that are no pixels
    band[pixel] = 7
    sums = sat_dot_sums(band, nrows, ncols, w, p, min_diag)
    valid = valid_mask(nrows, ncols, w, min_diag)
    for k, area in enumerate(pixels.dot_areas(w, p)):
        assert (sums[k][valid] == 7 * area).all() and not sums[k][~valid].any()


@pytest.mark.parametrize("nrows,ncols,w,p,min_diag", [s for s in SMALL if s[:2] != (5, 4)] + [(90, 120, 20, 3, 2)])
def test_the_scales_are_the_folds_times_the_expected_over_the_expected_of_the_neighbourhood(nrows, ncols, w, p, min_diag):
    """exact rationals against float64: a sum of at most 1681 non-negative terms, one division and one
    multiplication keep the relative error below about 2e-13; the bound asked is 1e-12"""
    band = make_band(nrows, ncols, "full", limit=2**20, seed=3)
    diag_sum = reference_marginals(band, nrows, ncols, 0)[0]
    folds = (1.75, 1.25, 1.5, 3.0)
    got = pixels.dot_scales(diag_sum, ncols, w, p, folds, min_diag)
    assert got.dtype == np.float64 and got.shape == (4, nrows)
    e = [Fraction(int(diag_sum[d]), ncols - d) for d in range(nrows)]
    for k, offsets in enumerate(footprints(w, p)):
        for d in range(nrows):
            if not 2 * w + min_diag <= d <= nrows - 1 - 2 * w:
                assert got[k, d] == 0.0
                continue
            x = sum(e[d + b - a] for a, b in offsets)
            want = Fraction(folds[k]) * e[d] / x
            assert abs(Fraction(float(got[k, d])) - want) <= Fraction(1, 10**12) * want, (k, d)


def test_the_scales_are_infinite_where_nothing_is_expected_and_refuse_a_window_that_does_not_fit():
    diag_sum = np.zeros(9, dtype=np.uint64)
    got = pixels.dot_scales(diag_sum, 12, 2, 1, min_diag=0)
    assert np.isinf(got[:, 4]).all() and not got[:, :4].any() and not got[:, 5:].any()
    diag_sum[4] = 24  # only the donut holds pixels of diagonal 4, the two at (-2, -2) and (2, 2): 1.75 e / (2 e)
    got = pixels.dot_scales(diag_sum, 12, 2, 1, min_diag=0)
    assert got[:, 4].tolist() == [0.875, np.inf, np.inf, np.inf]
    assert np.array_equal(pixels.dot_scales(diag_sum, 12, 2, 1, pixels.DOT_FOLDS, 0), got)  # the default folds
    assert pixels.DOT_FOLDS == (1.75, 1.75, 1.5, 1.5)
    for bad in (dict(w=2, p=1, min_diag=1), dict(w=3, p=1, min_diag=0), dict(w=2, p=2, min_diag=0),
                dict(w=0, p=0, min_diag=0), dict(w=2, p=1, min_diag=-1)):
        with pytest.raises(ValueError):
            pixels.dot_scales(diag_sum, 12, bad["w"], bad["p"], min_diag=bad["min_diag"])
    with pytest.raises(ValueError):
        pixels.dot_scales(diag_sum, 12, 2, 1, (1.0, 1.0, float("nan"), 1.0), 0)
    with pytest.raises(ValueError):
        pixels.dot_scales(diag_sum, 8, 2, 1, min_diag=0)  # ncols < nrows


def test_the_candidate_rule_is_one_double_product_and_one_comparison():
    """on a constant band with w = 1, p = 0 the areas are 4, 1, 6, 6: with the table (0.25, 1, 0, 0) every
    threshold equals obs exactly and the pixel is a candidate; one ulp more on the donut and it is none"""
    nrows, ncols, c = 7, 12, 3
    band = make_band(nrows, ncols, "empty")
    band[band == 0] = c
    sums = sat_dot_sums(band, nrows, ncols, 1, 0, 0)
    valid = valid_mask(nrows, ncols, 1, 0)
    assert pixels.dot_areas(1, 0) == (4, 1, 6, 6) and valid.sum() > 10
    table = np.zeros((4, nrows))
    table[0], table[1] = 0.25, 1.0
    cand = reference_candidates(band, nrows, ncols, sums, table, 1, 0, 1)
    assert (cand[:-1].reshape(ncols, nrows)[valid] == c).all() and cand.sum() == c * valid.sum()
    assert not reference_candidates(band, nrows, ncols, sums, table, 1, 0, c + 1).any()  # min_count
    table[0] = np.nextafter(0.25, 1.0)
    assert not reference_candidates(band, nrows, ncols, sums, table, 1, 0, 1).any()
    table[0], table[3] = 0.25, np.inf  # 18 * inf: never reached
    assert not reference_candidates(band, nrows, ncols, sums, table, 1, 0, 1).any()
    band[band == c] = 0  # 0 * inf is NaN and obs = 0 is below min_count
    assert not reference_candidates(band, nrows, ncols, sat_dot_sums(band, nrows, ncols, 1, 0, 0), table, 1, 0, 1).any()
    b1, b2, cnt = candidate_pixels(cand, nrows, ncols)
    assert len(b1) == valid.sum() and (np.diff(b1) >= 0).all() and (cnt == c).all()
    assert all((b1[n], b2[n]) < (b1[n + 1], b2[n + 1]) for n in range(len(b1) - 1))


# ---- clustering -----------------------------------------------------------------------------------

def brute_cluster(bin1, bin2, count, radius):
    keep = []
    for n in range(len(bin1)):
        beaten = False
        for m in range(len(bin1)):
            if m == n or max(abs(bin1[m] - bin1[n]), abs(bin2[m] - bin2[n])) > radius:
                continue
            if count[m] > count[n] or (count[m] == count[n] and (bin1[m], bin2[m]) < (bin1[n], bin2[n])):
                beaten = True
        if not beaten:
            keep.append(n)
    return np.array(keep, dtype=np.intp)


@pytest.mark.parametrize("seed", range(4))
def test_clustering_keeps_the_local_maxima(seed):
    rng = np.random.default_rng(seed)
    cells = rng.choice(40 * 40, size=150, replace=False)
    bin1, bin2 = cells // 40, cells % 40 + 40
    count = rng.integers(1, 4, size=150)  # many ties
    for radius in (0, 1, 2, 5, 100):
        got = api.cluster_dots(bin1, bin2, count, radius)
        assert np.array_equal(got, brute_cluster(bin1, bin2, count, radius)), radius
        if radius == 0:
            assert len(got) == 150
        if radius == 100:
            assert len(got) == 1
    # the order of the input does not matter
    order = rng.permutation(150)
    got = api.cluster_dots(bin1[order], bin2[order], count[order], 2)
    assert sorted(order[got]) == list(api.cluster_dots(bin1, bin2, count, 2))


def test_clustering_breaks_ties_by_position_and_refuses_nonsense():
    assert list(api.cluster_dots([3, 3, 4], [9, 10, 10], [5, 5, 5], 1)) == [0]
    assert list(api.cluster_dots([3, 3, 4], [9, 10, 10], [5, 6, 5], 1)) == [1]
    assert list(api.cluster_dots([3, 5], [9, 9], [1, 9], 1)) == [0, 1]
    assert len(api.cluster_dots([], [], [], 3)) == 0
    with pytest.raises(ValueError):
        api.cluster_dots([1], [2], [3], -1)
    with pytest.raises(ValueError):
        api.cluster_dots([1, 2], [2], [3], 1)
    assert "not HiCCUPS" in api.cluster_dots.__doc__.replace("NOT", "not")


# ---- the file -------------------------------------------------------------------------------------

def test_the_header_and_the_rows_of_the_file(tmp_path):
    assert driver.dots_header() == "#chrom1\tstart1\tend1\tchrom2\tstart2\tend2\tcount\texpected\tobserved_over_expected\n"
    iv = {"name": "chrA", "size": 500_000, "start": 10_000, "end": 123_000}
    lines = driver.dots_lines(iv, 5000, 1, [2, 3], [10, 22], [6, 1], [1.5, 0.1])
    assert lines == ["chrA\t20000\t25000\tchrA\t60000\t65000\t6\t1.5\t4.0\n",
                     f"chrA\t25000\t30000\tchrA\t120000\t123000\t1\t0.1\t{1 / 0.1!r}\n"]
    # at twice the bin size the interval starts in the middle of coarse bin 1 of its chromosome
    iv2 = {"name": "chrA", "size": 500_000, "start": 15_000, "end": 128_000}
    rows = driver.dots_lines(iv2, 5000, 2, [0], [1], [4], [0.5])
    assert rows == ["chrA\t15000\t20000\tchrA\t20000\t30000\t4\t0.5\t8.0\n"]
    plan = [entry("chrA", 10_000, 123_000, 30, 23), entry("chrA", 130_000, 150_000, 3, 4, skipped=True),
            entry("chrB", 0, 10_000, 2, 2), entry("chrC", 0, 100_000, 20, 20)]
    calls = []

    def fed(k, factor, first_bin):
        calls.append((k, factor, first_bin))
        if k == 2:
            return None
        return ([2, 3], [10, 22], [6, 1], [1.5, 0.1]) if k == 0 else ([], [], [], [])

    path = str(tmp_path / "d.bedpe")
    driver.write_dots(path, plan, 5000, 5000, fed)
    assert calls == [(0, 1, 2), (2, 1, 0), (3, 1, 0)]
    assert open(path).readlines() == [driver.dots_header()] + lines


def test_the_candidates_are_checked_before_a_row_is_written():
    ok = ([5, 5, 6], [12, 13, 12], [3, 2, 2])
    driver.check_dots("chrA:0-100", 20, 40, 2, 2, 2, *ok)
    driver.check_dots("chrA:0-100", 20, 40, 2, 2, 2, [], [], [])
    for what, (b1, b2, c), message in [
            ("order", ([5, 5], [13, 12], [3, 3]), "does not follow"),
            ("twice", ([5, 5], [12, 12], [3, 3]), "does not follow"),
            ("left edge", ([1], [9], [3]), "no valid pixel"),
            ("right edge", ([30], [38], [3]), "no valid pixel"),
            ("near diagonal", ([5], [10], [3]), "no valid pixel"),
            ("band edge", ([5], [21], [3]), "no valid pixel"),
            ("count", ([5], [12], [1]), "has count 1, below 2")]:
        with pytest.raises(RuntimeError) as e:
            driver.check_dots("chrA:0-100", 20, 40, 2, 2, 2, b1, b2, c)
        assert str(e.value).startswith("chrA:0-100: the dot candidate") and message in str(e.value), what


class FakeSim:
    def __init__(self, result):
        self.result, self.calls = result, []

    def dots(self, interval_id, **kw):
        self.calls.append((interval_id, kw))
        return self.result


def test_the_output_stage_checks_and_clusters():
    plan = [entry("chrA", 0, 200_000, 20, 40), entry("chrB", 0, 200_000, 20, 40, skipped=True)]
    b1, b2 = np.array([5, 5, 6, 20]), np.array([12, 13, 12, 30])
    cnt, e = np.array([3, 4, 3, 2], dtype=np.int32), np.array([1.0, 0.5, 2.0, 0.25])
    sim = FakeSim((b1, b2, cnt, e))
    got = driver._interval_dots(sim, plan, [7, None], 2, 1, 2, [1, 1, 1, 1], 2, 1, 0, 1, 0)
    assert [list(x) for x in got] == [[5, 20], [13, 30], [4, 2], [0.5, 0.25]]
    assert sim.calls == [(7, dict(w=2, p=1, min_count=2, folds=[1, 1, 1, 1], min_diag=2, factor=1, first_bin=0))]
    assert driver._interval_dots(sim, plan, [7, None], 2, 1, 2, [1, 1, 1, 1], 2, 1, 1, 1, 0) is None
    assert [list(x) for x in driver._interval_dots(sim, plan, [7, None], 2, 1, 2, [1, 1, 1, 1], 2, 0, 0, 1, 0)][2] == [3, 4, 3, 2]
    with pytest.raises(RuntimeError):
        driver._interval_dots(FakeSim((b1, b2, cnt, e)), plan, [7, None], 2, 1, 3, [1, 1, 1, 1], 2, 1, 0, 1, 0)


def test_a_window_that_does_not_fit_the_band_is_named_with_the_largest_that_fits():
    plan = [entry("chrA", 0, 2_000_000, 40, 400), entry("chrB", 0, 500_000, 8, 100, skipped=True),
            entry("chrC", 25_000, 1_000_000, 39, 195)]
    assert driver.dots_misfit(plan, 5000, 5000, 45_000, 2) is None  # 4 * 9 + 1 + 2 = 39
    assert driver.dots_misfit(plan, 5000, 5000, 45_000, 3) == ("chrC:25000-1000000", 45_000, 9, 39, 40_000)
    assert driver.dots_misfit(plan, 5000, 5000, 50_000, 0) == ("chrA:0-2000000", 50_000, 10, 40, 45_000)
    # at twice the bin size the band of 40 diagonals has 21
    assert driver.dots_misfit(plan[:1], 5000, 10_000, 40_000, 2) is None  # 4 * 4 + 1 + 2 = 19
    assert driver.dots_misfit(plan[:1], 5000, 10_000, 50_000, 2) == ("chrA:0-2000000", 50_000, 5, 21, 40_000)
    assert driver.dots_misfit([entry("chrD", 0, 100_000, 4, 20)], 5000, 5000, 5000, 2) == ("chrD:0-100000", 5000, 1, 4, 0)


# ---- the options and preflight --------------------------------------------------------------------

@pytest.fixture
def prefix(tmp_path, monkeypatch):
    for name in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(name, raising=False)
    return str(tmp_path / "out" / "p")


def parse(prefix, *extra):
    return cli.build_parser().parse_args(["simulate", "-c", "g.chrom.sizes", "-b", "b.bed", "-o", prefix,
                                          "-r", "5kb", *extra])


def run_preflight(prefix, *extra):
    a = parse(prefix, *extra)
    return cli.preflight(a, cli.config_from_args(a))


def test_the_options_parse_and_preflight_plans_the_file(prefix):
    a = parse(prefix)
    assert not a.dots and a.dots_window is None and a.dots_folds is None
    pre = run_preflight(prefix, "--no-track-1d-lef-position")
    assert pre.dots is None and pre.insulation is None
    assert pre.outputs == cli.Outputs(prefix + ".cool", None, None, None)  # as before
    assert cli.Preflight([5000], pre.outputs, 0, 1, 0).dots is None  # the fields of before still make one
    pre = run_preflight(prefix, "--dots")
    assert pre.dots == cli.Dots(prefix + "_dots.bedpe", 5000, 25_000, 10_000, 1, [1.75, 1.75, 1.5, 1.5], 2, 20_000)
    assert cli.dots_path(prefix) == prefix + "_dots.bedpe"
    pre = run_preflight(prefix, "--dots", "--dots-resolution", "10kb", "--dots-window", "50kb", "--dots-peak", "10kb",
                        "--dots-min-count", "4", "--dots-folds", "1.2,1.3, 1.4,1", "--dots-ignore-diags", "0",
                        "--dots-cluster-radius", "0")
    assert pre.dots == cli.Dots(prefix + "_dots.bedpe", 10_000, 50_000, 10_000, 4, [1.2, 1.3, 1.4, 1.0], 0, 0)
    assert run_preflight(prefix, "--dots", "--dots-window", "100kb").dots.window == 100_000  # the cap is reached
    assert run_preflight(prefix, "--dots", "--dots-window", "5kb").dots.peak == 0
    assert run_preflight(prefix, "--dots", "--dots-resolution", "25kb").dots.radius == 25_000
    pre = run_preflight(prefix, "--dots", "--skip-output")
    assert pre.dots.path is None and pre.outputs == cli.Outputs(None, None, None, None)
    assert not os.path.exists(prefix + "_dots.bedpe")
    for bad in ("1,2,3", "1,2,3,4,5", "a,b,c,d", "1,2,3,-1", "1,2,3,inf", "1,2,3,nan", ""):
        with pytest.raises(Exception) as e:
            cli.fold_list(bad)
        assert e.type.__name__ == "ArgumentTypeError", bad


REFUSED = [
    (["--dots-window", "50kb"], "--dots-window needs --dots"),
    (["--dots-resolution", "10kb"], "--dots-resolution needs --dots"),
    (["--dots-peak", "10kb"], "--dots-peak needs --dots"),
    (["--dots-min-count", "3"], "--dots-min-count needs --dots"),
    (["--dots-folds", "1,1,1,1"], "--dots-folds needs --dots"),
    (["--dots-ignore-diags", "2", "--skip-output"], "--dots-ignore-diags needs --dots"),
    (["--dots-cluster-radius", "20kb"], "--dots-cluster-radius needs --dots"),
    (["--dots", "--dots-ignore-diags", "-1"], "--dots-ignore-diags: -1 is negative"),
    (["--dots", "--dots-min-count", "0"], "--dots-min-count: 0 is below 1"),
    (["--dots", "--dots-window", "12000"], "--dots-window: 12000 is not a positive multiple"),
    (["--dots", "--dots-window", "0"], "--dots-window: 0 is not a positive multiple"),
    (["--dots", "--dots-peak", "7000"], "--dots-peak: 7000 is not a multiple"),
    (["--dots", "--dots-cluster-radius", "7000"], "--dots-cluster-radius: 7000 is not a multiple"),
    (["--dots", "--dots-resolution", "10kb", "--dots-window", "25kb"], "--dots-window: 25000 is not a positive multiple"),
    (["--dots", "--dots-window", "50kb", "--dots-peak", "50kb"], "--dots-peak: 50000 is not below the window"),
    (["--dots", "--dots-window", "10kb", "--dots-peak", "15kb"], "--dots-peak: 15000 is not below the window"),
    (["--dots", "--dots-window", "105kb"], "--dots-window: 105000 is 21 bins"),
    (["--dots", "--dots-resolution", "12500"], "--dots-resolution: 12500 is not a multiple"),
    (["--dots", "--dots-resolution", "1kb"], "--dots-resolution: 1000 is not a multiple"),
]


@pytest.mark.parametrize("options,message", REFUSED)
def test_preflight_refuses_before_anything_is_made(prefix, options, message):
    with pytest.raises(SystemExit) as e:
        run_preflight(prefix, *options)
    assert str(e.value).startswith(message)
    assert not os.path.exists(os.path.dirname(prefix))


def test_the_dots_file_is_the_last_that_is_refused_to_be_overwritten(prefix):
    everything = ["--track-1d-lef-position", "--expected", "--insulation-windows", "100kb", "--dots"]
    os.makedirs(os.path.dirname(prefix))
    for which in ("_dots.bedpe", "_insulation.tsv"):  # each one is named before the one before it
        with open(prefix + which, "wb") as fh:
            fh.write(b"precious")
        with pytest.raises(SystemExit) as e:
            run_preflight(prefix, *everything)
        assert str(e.value) == f"refusing to overwrite {prefix + which}: pass --force to overwrite"
    assert run_preflight(prefix, *everything, "--force").dots.path == prefix + "_dots.bedpe"
    assert run_preflight(prefix, *everything, "--skip-output").dots.path is None
    os.remove(prefix + "_insulation.tsv")
    assert run_preflight(prefix, "--no-track-1d-lef-position").dots is None  # without the option: nobody's business
    assert open(prefix + "_dots.bedpe", "rb").read() == b"precious"
