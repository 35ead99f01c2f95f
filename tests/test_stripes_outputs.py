"""Two bands compared stripe by stripe, without a GPU: the numpy / Python-int restatement of the sums of
include/modle_pixels.h (modle_pixels_stripes) that the GPU tests compare against, cross-checked against an
O(n^2) brute-force form; pixels.stripe_scores on the restated sums against evaluate.compare; the rows per
mask and the argument refusals of the C entry points, which need no device; the lines of
<prefix>_stripes.tsv, driver.check_stripes, and what cli.preflight and driver.stripes_misfit refuse of
--compare-to.

The sums are integers and are compared exactly.  The scores are compared with evaluate.compare, whose
two-pass float64 form over at most 4096 terms is the only inexact side; the tolerance per metric is 64 times
the largest difference measured between the two on the inputs of this module (SCORE_SHAPES, seed 7):
    pearson    measured 5.551115123125783e-16  (absolute)                      tolerance 3.56e-14
    spearman   measured 1.1102230246251565e-16 (absolute)                      tolerance 7.11e-15
    rmse       measured 2.6482425481874274e-16 (relative to max(value, 1))     tolerance 1.70e-14
    eucl_dist  measured 2.2184876597836343e-16 (relative to max(value, 1))     tolerance 1.42e-14
(the issue expected 6.7e-16 for Pearson; stripe_scores forms it as the root of one correctly rounded quotient,
which came out a little closer).  NaNs must fall in the same places."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from modle_amd import cli, cooler, driver, evaluate, pixels

MOMENTS, MASKED, RANKS = 1, 2, 4
ROWS = {1: 9, 2: 9, 3: 18, 4: 3, 5: 12, 6: 12, 7: 21}
M64 = (1 << 64) - 1
TOLERANCE = {"pearson": 64 * 5.551115123125783e-16, "spearman": 64 * 1.1102230246251565e-16,
             "rmse": 64 * 2.6482425481874274e-16, "eucl_dist": 64 * 2.2184876597836343e-16}
SCORE_SHAPES = [(1, 1, 5), (5, 9, 4), (64, 70, 3), (129, 200, 50), (600, 640, 6), (300, 320, 2**32)]  # nrows, ncols, counts below


# ---- the restatement ---------------------------------------------------------------------------------------

def band_stripes(band, nrows, ncols, direction):
    """uint64 [ncols, nrows]: row c is the stripe of bin c, v[i] = M(c - i, c) or h[i] = M(c, c + i), with zeros
    where the matrix ends; the words of the band that are no pixels are not used"""
    b = np.asarray(band[:nrows * ncols], dtype=np.uint64).reshape(ncols, nrows)
    out = np.zeros((ncols, nrows), dtype=np.uint64)
    if direction == 0:
        keep = np.arange(nrows)[None, :] <= np.arange(ncols)[:, None]
        out[keep] = b[keep]
    else:
        for i in range(nrows):  # pixel (c, c + i) lies at b[c + i, i]
            out[:ncols - i, i] = b[i:, i]
    return out


def _sum_of_products(x, y):
    """per row the sum of x * y as Python ints: the low and the high halves of the uint64 products are summed
    apart and joined"""
    p = x * y
    lo = (p & np.uint64(0xFFFFFFFF)).sum(axis=1, dtype=np.uint64)
    hi = (p >> np.uint64(32)).sum(axis=1, dtype=np.uint64)
    return [int(l) + (int(h) << 32) for l, h in zip(lo, hi)]


def restate_moments(a, b, masked):
    """the nine rows n, Sa, Sb, Saa_lo, Saa_hi, Sbb_lo, Sbb_hi, Sab_lo, Sab_hi of the stripes a, b"""
    if masked:
        w = ((a != 0) & (b != 0)).astype(np.uint64)
        a, b, n = a * w, b * w, w.sum(axis=1, dtype=np.uint64)
    else:
        n = np.full(a.shape[0], a.shape[1], dtype=np.uint64)
    rows = [n, a.sum(axis=1, dtype=np.uint64), b.sum(axis=1, dtype=np.uint64)]
    for x, y in ((a, a), (b, b), (a, b)):
        s = _sum_of_products(x, y)
        rows.append(np.array([v & M64 for v in s], dtype=np.uint64))
        rows.append(np.array([v >> 64 for v in s], dtype=np.uint64))
    return np.stack(rows)


def doubled_ranks(x):
    """R2 = 2 * #{y < x} + #{y == x} + 1 within every row, from the sorted row"""
    s = np.sort(x, axis=1)
    out = np.empty(x.shape, dtype=np.uint64)
    for r in range(x.shape[0]):
        out[r] = np.searchsorted(s[r], x[r], "left") + np.searchsorted(s[r], x[r], "right") + 1
    return out


def restate_ranks(a, b):
    ra, rb = doubled_ranks(a), doubled_ranks(b)  # (at most 2 * 4096: the sums stay far below 2^64)
    return np.stack([(ra * ra).sum(axis=1, dtype=np.uint64), (rb * rb).sum(axis=1, dtype=np.uint64),
                     (ra * rb).sum(axis=1, dtype=np.uint64)])


def restate(band_a, band_b, nrows, ncols, what):
    """uint64 [2, rows(what), ncols]: what modle_pixels_stripes writes"""
    out = []
    for d in (0, 1):
        a, b = band_stripes(band_a, nrows, ncols, d), band_stripes(band_b, nrows, ncols, d)
        blocks = []
        if what & MOMENTS:
            blocks.append(restate_moments(a, b, False))
        if what & MASKED:
            blocks.append(restate_moments(a, b, True))
        if what & RANKS:
            blocks.append(restate_ranks(a, b))
        out.append(np.concatenate(blocks))
    return np.stack(out)


def brute(band_a, band_b, nrows, ncols, what):
    """the same from the definitions, entry by entry in Python ints"""
    def m(band, i, j):
        return int(band[j * nrows + (j - i)]) if 0 <= i <= j < ncols and j - i < nrows else 0

    out = np.zeros((2, ROWS[what], ncols), dtype=np.uint64)
    for d in (0, 1):
        for c in range(ncols):
            a = [m(band_a, c - i, c) if d == 0 else m(band_a, c, c + i) for i in range(nrows)]
            b = [m(band_b, c - i, c) if d == 0 else m(band_b, c, c + i) for i in range(nrows)]
            words = []
            for block in (MOMENTS, MASKED):
                if what & block:
                    pairs = [(x, y) for x, y in zip(a, b) if block == MOMENTS or (x != 0 and y != 0)]
                    s = [sum(x * x for x, _ in pairs), sum(y * y for _, y in pairs), sum(x * y for x, y in pairs)]
                    words += [len(pairs), sum(x for x, _ in pairs), sum(y for _, y in pairs)]
                    for v in s:
                        words += [v & M64, v >> 64]
            if what & RANKS:
                ra = [2 * sum(y < x for y in a) + sum(y == x for y in a) + 1 for x in a]
                rb = [2 * sum(y < x for y in b) + sum(y == x for y in b) + 1 for x in b]
                assert sum(ra) == sum(rb) == nrows * (nrows + 1)
                words += [sum(x * x for x in ra), sum(y * y for y in rb), sum(x * y for x, y in zip(ra, rb))]
            out[d, :, c] = words
    return out


def random_pair(nrows, ncols, below, seed=7):
    """two bands with about half of the words zero and counts below `below`; the words that are no pixels hold
    0xFFFFFFFF"""
    rng = np.random.default_rng([seed, nrows, ncols])
    bands = []
    for _ in range(2):
        x = rng.integers(0, below, size=nrows * ncols + 1, dtype=np.uint64)
        x[rng.random(x.size) < 0.5] = 0
        x = x.astype(np.uint32)
        for j in range(min(nrows, ncols)):
            x[j * nrows + j + 1:(j + 1) * nrows] = 0xFFFFFFFF
        x[nrows * ncols] = 0xFFFFFFFF
        bands.append(x)
    return bands


@pytest.mark.parametrize("nrows,ncols,below", [(1, 1, 5), (1, 7, 2**32), (5, 5, 3), (5, 9, 2**32), (33, 40, 3),
                                               (64, 64, 2**32), (64, 70, 4)])
def test_the_restatement_is_the_brute_force_definition(nrows, ncols, below):
    a, b = random_pair(nrows, ncols, below)
    for what in ROWS:
        got = restate(a, b, nrows, ncols, what)
        assert got.dtype == np.uint64 and got.shape == (2, ROWS[what], ncols)
        assert np.array_equal(got, brute(a, b, nrows, ncols, what)), what
    if below == 2**32 and nrows >= 5:
        assert restate(a, b, nrows, ncols, MOMENTS)[:, 4].any()  # a second moment beyond 2^64
    # the blocks of a mask are the rows of the single masks, in bit order
    all_ = restate(a, b, nrows, ncols, 7)
    assert np.array_equal(all_[:, :9], restate(a, b, nrows, ncols, MOMENTS))
    assert np.array_equal(all_[:, 9:18], restate(a, b, nrows, ncols, MASKED))
    assert np.array_equal(all_[:, 18:], restate(a, b, nrows, ncols, RANKS))


# ---- the scores ---------------------------------------------------------------------------------------------

def score_differences(nrows, ncols, below):
    """{metric: largest difference} between pixels.stripe_scores on the restated sums and evaluate.compare,
    over both directions and, where it is defined, the masked form; asserts that NaNs fall in the same places"""
    a, b = random_pair(nrows, ncols, below)
    rows = restate(a, b, nrows, ncols, 7)
    worst = {}
    for metric in pixels.STRIPE_METRICS:
        for d, direction in enumerate(("vertical", "horizontal")):
            for masked in (False, True):
                if metric == "spearman" and masked:
                    continue
                got = pixels.stripe_scores(rows[d], metric, masked)
                want = evaluate.compare(a, b, nrows, ncols, metric, direction, masked)[0]
                assert got.dtype == np.float64 and got.shape == (ncols,)
                assert np.array_equal(np.isnan(got), np.isnan(want)), (metric, direction, masked)
                ok = ~np.isnan(want)
                diff = np.abs(got[ok] - want[ok])
                if metric in ("rmse", "eucl_dist"):
                    diff = diff / np.maximum(want[ok], 1.0)
                worst[metric] = max(worst.get(metric, 0.0), float(diff.max()) if diff.size else 0.0)
    return worst


@pytest.mark.parametrize("nrows,ncols,below", SCORE_SHAPES)
def test_the_scores_are_evaluate_s(nrows, ncols, below):
    worst = score_differences(nrows, ncols, below)
    print({k: f"{v:.3g}" for k, v in worst.items()})
    for metric, diff in worst.items():
        assert diff <= TOLERANCE[metric], (metric, diff)


def test_the_scores_of_stripes_that_are_special():
    """hand-made rows: zeros score NaN for Pearson and 1 for Spearman, a stripe against itself 1, against its
    reverse -1, and no rounding leaves [-1, 1]"""
    nrows, ncols = 4, 6
    a = np.zeros(nrows * ncols + 1, dtype=np.uint32)
    b = a.copy()
    a[3 * nrows:4 * nrows] = [1, 2, 3, 4]  # the vertical stripe of bin 3
    b[3 * nrows:4 * nrows] = [4, 3, 2, 1]
    a[4 * nrows:5 * nrows] = b[4 * nrows:5 * nrows] = [7, 7, 9, 0]
    rows = restate(a, b, nrows, ncols, 7)[0]
    p, s = pixels.stripe_scores(rows, "pearson"), pixels.stripe_scores(rows, "spearman")
    assert np.isnan(p[:3]).all() and np.isnan(p[5]) and p[3] == -1.0 and p[4] == 1.0
    assert s.tolist() == [1.0, 1.0, 1.0, -1.0, 1.0, 1.0]
    assert pixels.stripe_scores(rows, "eucl_dist").tolist() == [0, 0, 0, math.sqrt(20), 0, 0]
    assert pixels.stripe_scores(rows, "rmse").tolist() == [0, 0, 0, math.sqrt(5), 0, 0]
    m = pixels.stripe_scores(rows, "rmse", masked=True)
    assert np.isnan(m[[0, 1, 2, 5]]).all() and m[3] == math.sqrt(5) and m[4] == 0.0  # no entry left: 0 / 0
    assert pixels.stripe_scores(rows, "eucl_dist", masked=True).tolist() == [0, 0, 0, math.sqrt(20), 0, 0]


def test_stripe_scores_reads_the_blocks_off_the_rows():
    a, b = random_pair(5, 9, 4)
    all_ = restate(a, b, 5, 9, 7)[1]
    for what in ROWS:
        rows = restate(a, b, 5, 9, what)[1]
        for metric in pixels.STRIPE_METRICS:
            for masked in (False, True):
                side = MASKED if masked else MOMENTS
                need = side | (RANKS if metric == "spearman" else 0)
                # 9 and 12 rows are MOMENTS or MASKED (and RANKS): taken as the block that is asked for
                taken = {3: RANKS, 9: side, 12: side | RANKS, 18: 3, 21: 7}[ROWS[what]]
                if metric == "spearman" and masked or taken & need != need:
                    with pytest.raises(ValueError):
                        pixels.stripe_scores(rows, metric, masked)
                elif what & need == need:
                    assert np.array_equal(pixels.stripe_scores(rows, metric, masked),
                                          pixels.stripe_scores(all_, metric, masked), equal_nan=True)
    for bad in (all_[:5], all_.astype(np.int64), all_[0], "rows"):
        with pytest.raises(ValueError):
            pixels.stripe_scores(bad, "pearson")
    with pytest.raises(ValueError):
        pixels.stripe_scores(all_, "kendall")


@pytest.mark.parametrize("nrows,ncols,below", [(1, 1, 5), (5, 9, 2**32), (64, 70, 3)])
def test_a_band_against_itself(nrows, ncols, below):
    a, _ = random_pair(nrows, ncols, below)
    both = restate(a, a, nrows, ncols, 7)
    for d in (0, 1):
        rows = both[d]
        for block in (0, 9):
            assert np.array_equal(rows[block + 1], rows[block + 2])
            for k in (0, 1):
                assert np.array_equal(rows[block + 3 + k], rows[block + 5 + k])
                assert np.array_equal(rows[block + 3 + k], rows[block + 7 + k])
        assert np.array_equal(rows[18], rows[19]) and np.array_equal(rows[18], rows[20])
        for masked in (False, True):
            p = pixels.stripe_scores(rows, "pearson", masked)
            assert ((p == 1.0) | np.isnan(p)).all()
            assert not pixels.stripe_scores(rows, "eucl_dist", masked).any()
            r = pixels.stripe_scores(rows, "rmse", masked)
            assert ((r == 0.0) | (np.isnan(r) & (rows[9 if masked else 0] == 0))).all()
        s = pixels.stripe_scores(rows, "spearman")
        assert ((s == 1.0) | np.isnan(s)).all()


# ---- the entry points that need no device -------------------------------------------------------------------

def test_the_rows_of_every_mask():
    for what, rows in ROWS.items():
        assert pixels.stripes_rows(what) == rows
    for what in (0, 8, 9, 15, 1 << 32, 1 << 63):
        with pytest.raises(pixels.PixelsError) as e:
            pixels.stripes_rows(what)
        assert e.value.code == pixels.ERR_ARG
    for what in (-1, 1 << 64):
        with pytest.raises(pixels.PixelsError):
            pixels.stripes_rows(what)
    assert (pixels.STRIPES_MOMENTS, pixels.STRIPES_MASKED, pixels.STRIPES_RANKS, pixels.MAX_STRIPE) == (1, 2, 4, 4096)
    assert pixels.STRIPE_METRICS == evaluate.METRICS == cli.COMPARE_METRICS
    assert {"modle_pixels_stripes", "modle_pixels_stripes_to_host", "modle_pixels_stripes_rows"} <= set(pixels.EXPORTS)


def test_what_the_entry_points_refuse_without_a_device():
    """every refusal comes before the handle or a band is touched: the handle here is host memory that names a
    device no machine has, and the bands and the output are addresses nobody owns"""
    lb = pixels.lib()
    handle = (C.c_uint64 * 512)()
    C.cast(handle, C.POINTER(C.c_int))[0] = 1 << 20  # modle_pixels_handle.device
    h = C.addressof(handle)
    ref, tgt, out = 0x10000000, 0x20000000, 0x30000000
    nrows, ncols = 5, 9
    words = 2 * 9 * ncols
    band = (nrows * ncols + 1) * 4
    err = C.create_string_buffer(512)
    cases = {
        "no handle": (None, ref, tgt, nrows, ncols, 1, out, words),
        "no reference": (h, None, tgt, nrows, ncols, 1, out, words),
        "no target": (h, ref, None, nrows, ncols, 1, out, words),
        "no output": (h, ref, tgt, nrows, ncols, 1, None, words),
        "what == 0": (h, ref, tgt, nrows, ncols, 0, out, words),
        "an unknown bit": (h, ref, tgt, nrows, ncols, 9, out, words),
        "only an unknown bit": (h, ref, tgt, nrows, ncols, 8, out, 0),
        "nrows 0": (h, ref, tgt, 0, ncols, 1, out, words),
        "both 0": (h, ref, tgt, 0, 0, 1, out, 0),
        "nrows > ncols": (h, ref, tgt, ncols + 1, ncols, 1, out, words),
        "ranks above the cap": (h, ref, tgt, 4097, 5000, 4, out, 2 * 3 * 5000),
        "ranks above the cap, among others": (h, ref, tgt, 4097, 5000, 7, out, 2 * 21 * 5000),
        "out_words too small": (h, ref, tgt, nrows, ncols, 1, out, words - 1),
        "out_words too large": (h, ref, tgt, nrows, ncols, 1, out, words + 1),
        "out_words of another mask": (h, ref, tgt, nrows, ncols, 3, out, words),
        "a misaligned output": (h, ref, tgt, nrows, ncols, 1, out + 4, words),
        "the output overlaps the reference": (h, ref, tgt, nrows, ncols, 1, ref + band - 8, words),
        "the output ends in the reference": (h, ref, tgt, nrows, ncols, 1, ref - 8 * words + 8, words),
        "the output overlaps the target": (h, ref, tgt, nrows, ncols, 1, tgt + 8, words),
        "the output is the one band of both": (h, ref, ref, nrows, ncols, 1, ref, words),
    }
    for name, args in cases.items():
        err.value = b""
        assert lb.modle_pixels_stripes(*args, None, err, len(err)) == pixels.ERR_ARG, name
        assert err.value.startswith(b"modle_pixels_stripes: "), name
    ptr = C.c_void_p(1)
    for name, args in cases.items():
        if "out" in name:
            continue
        ptr.value = 1
        assert lb.modle_pixels_stripes_to_host(*args[:6], C.byref(ptr), None, err, len(err)) == pixels.ERR_ARG, name
        assert ptr.value is None, name
    assert lb.modle_pixels_stripes_to_host(h, ref, tgt, nrows, ncols, 1, None, None, err, len(err)) == pixels.ERR_ARG


# ---- <prefix>_stripes.tsv -----------------------------------------------------------------------------------

def entry(name, start, end, nrows, ncols, size=None, skipped=False):
    return {"interval": {"name": name, "size": end if size is None else size, "start": start, "end": end},
            "nrows": nrows, "ncols": ncols, "tasks": None, "skipped": skipped}


def test_the_lines_of_the_file(tmp_path):
    assert driver.stripes_header("ref.mcool::/resolutions/10000", 10000, True, ["rmse", "pearson"]) == \
        "# reference=ref.mcool::/resolutions/10000 resolution=10000 exclude_zero_pixels=yes\n" \
        "chrom\tstart\tend\trmse_vertical\trmse_horizontal\tpearson_vertical\tpearson_horizontal\n"
    assert driver.stripes_header("r.cool", 5000, False, ["pearson"]).startswith(
        "# reference=r.cool resolution=5000 exclude_zero_pixels=no\nchrom\tstart\tend\tpearson_vertical\t")
    iv = {"name": "chrA", "start": 25_000, "end": 52_000}
    v, h = np.array([0.1, math.nan, -1.0]), np.array([1 / 3, 2.0, 1e-300])
    # at the bin size: bins count from the interval's start, the last one ends with it
    assert driver.stripes_lines(iv, 10_000, 1, [(v, h)]) == [
        "chrA\t25000\t35000\t0.1\t0.3333333333333333\n", "chrA\t35000\t45000\tnan\t2.0\n",
        "chrA\t45000\t52000\t-1.0\t1e-300\n"]
    # at twice the bin size of 5 kb: coarse bins are anchored at the chromosome's start (first_bin 5 is odd)
    assert driver.stripes_lines(iv, 5_000, 2, [(v, h), (h, v)]) == [
        "chrA\t25000\t30000\t0.1\t0.3333333333333333\t0.3333333333333333\t0.1\n",
        "chrA\t30000\t40000\tnan\t2.0\t2.0\tnan\n", "chrA\t40000\t50000\t-1.0\t1e-300\t1e-300\t-1.0\n"]
    assert driver.stripes_lines(iv, 5_000, 1, []) == []
    plan = [entry("chrA", 0, 20_000, 3, 4), entry("chrB", 0, 9_000, 2, 2, skipped=True), entry("chrC", 5_000, 15_000, 2, 2)]
    calls = []

    def scores(k, factor, first_bin):
        calls.append((k, factor, first_bin))
        n = 2 if k == 0 else 1
        return None if k == 2 and factor == 1 else [(np.full(n, 0.5), np.full(n, math.nan))]

    path = str(tmp_path / "p_stripes.tsv")
    driver.write_stripes(path, plan, 5_000, "r.cool", 10_000, False, ["pearson"], scores)
    assert calls == [(0, 2, 0), (2, 2, 1)]
    assert open(path).read() == ("# reference=r.cool resolution=10000 exclude_zero_pixels=no\n"
                                 "chrom\tstart\tend\tpearson_vertical\tpearson_horizontal\n"
                                 "chrA\t0\t10000\t0.5\tnan\nchrA\t10000\t20000\t0.5\tnan\nchrC\t5000\t10000\t0.5\tnan\n")
    calls.clear()
    driver.write_stripes(path, plan, 5_000, "r.cool", 5_000, False, ["pearson"], scores)  # an entry without a matrix
    assert calls == [(0, 1, 0), (2, 1, 1)] and len(open(path).readlines()) == 2 + 2


def test_check_stripes_ties_the_sums_to_the_bands():
    nrows, ncols = 5, 9
    a, b = random_pair(nrows, ncols, 50)
    rows = restate(a, b, nrows, ncols, 7)
    sum_a = int(band_stripes(a, nrows, ncols, 0).sum())
    sum_b = int(band_stripes(b, nrows, ncols, 1).sum())
    assert sum_a != sum_b
    driver.check_stripes("chrA:0-45000", rows, nrows, sum_a, sum_b)
    driver.check_stripes("chrA:0-45000", rows[:, :9], nrows, sum_a, sum_b)
    for ref_sum, run_sum, message in ((sum_a + 1, sum_b, "the vertical stripes of the reference add up to"),
                                      (sum_a, sum_b - 1, "the vertical stripes of the run add up to"),
                                      (sum_b, sum_a, "the vertical stripes of the reference add up to")):
        with pytest.raises(RuntimeError) as e:
            driver.check_stripes("chrA:0-45000", rows, nrows, ref_sum, run_sum)
        assert str(e.value).startswith("chrA:0-45000: " + message)
    bad = rows.copy()
    bad[1, 1, 4] += np.uint64(1)  # one Sa of the horizontal direction
    with pytest.raises(RuntimeError) as e:
        driver.check_stripes("x", bad, nrows, sum_a, sum_b)
    assert "the horizontal stripes of the reference add up to" in str(e.value)
    bad = rows.copy()
    bad[0, 0, 8] = np.uint64(4)  # an n
    with pytest.raises(RuntimeError) as e:
        driver.check_stripes("x", bad, nrows, sum_a, sum_b)
    assert "a vertical stripe counts 4 entries, the band has 5 diagonals" in str(e.value)
    assert driver.stripes_what(["pearson"], False) == 1 and driver.stripes_what(["rmse", "spearman"], False) == 5
    assert driver.stripes_what(["eucl_dist"], True) == 3


# ---- the options and what is refused before anything is simulated -------------------------------------------

CHROMS = [("chrA", 100_000), ("chrB", 40_000)]


@pytest.fixture
def prefix(tmp_path, monkeypatch):
    for name in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(name, raising=False)
    return str(tmp_path / "out" / "p")


@pytest.fixture
def refs(tmp_path):
    """a .cool at 5 kb and an .mcool at 5 and 10 kb of CHROMS, without a pixel"""
    cool, mcool = str(tmp_path / "ref.cool"), str(tmp_path / "ref.mcool")
    with cooler.CoolerWriter(cool, CHROMS, 5000), cooler.McoolWriter(mcool, CHROMS, [5000, 10000]):
        pass
    return cool, mcool


def parse(prefix, *extra):
    return cli.build_parser().parse_args(["simulate", "-c", "g.chrom.sizes", "-b", "b.bed", "-o", prefix,
                                          "-r", "5kb", "--no-track-1d-lef-position", *extra])


def run_preflight(prefix, *extra):
    a = parse(prefix, *extra)
    return cli.preflight(a, cli.config_from_args(a))


def run_plan(prefix, *extra):
    """what the output stage is handed: the `stripes` of the plan, after preflight has accepted the arguments"""
    a = parse(prefix, *extra)
    pre = cli.preflight(a, cli.config_from_args(a))
    assert pre.outputs.cooler == prefix + ".cool"
    return pre.stripes


def test_the_options_parse_and_preflight_plans_the_file(prefix, refs):
    cool, mcool = refs
    a = parse(prefix)
    assert (a.compare_to, a.compare_metrics, a.compare_resolution, a.compare_exclude_zero_pixels) == (None,) * 4
    assert run_plan(prefix) is None
    assert run_plan(prefix, "--compare-to", cool) == cli.Stripes(prefix + "_stripes.tsv", cool, 5000, ["pearson"], False, 5000, CHROMS)
    assert cli.stripes_path(prefix) == prefix + "_stripes.tsv" and not os.path.exists(prefix + "_stripes.tsv")
    uri = mcool + "::/resolutions/10000"
    got = run_plan(prefix, "--compare-to", uri, "--compare-metrics", "rmse, spearman,pearson",
                   "--compare-resolution", "10kb")
    assert got == cli.Stripes(prefix + "_stripes.tsv", uri, 10000, ["rmse", "spearman", "pearson"], False, 10000, CHROMS)
    got = run_plan(prefix, "--compare-to", mcool + "::/resolutions/5000", "--compare-exclude-zero-pixels",
                   "--compare-metrics", "eucl_dist")
    assert got.exclude_zero is True and got.metrics == ["eucl_dist"]
    assert cli.metric_list("pearson,spearman,rmse,eucl_dist") == list(cli.COMPARE_METRICS)
    for bad in ("", "pearson,", "kendall", "rmse,rmse"):
        with pytest.raises(Exception) as e:
            cli.metric_list(bad)
        assert e.type.__name__ == "ArgumentTypeError", bad
    with pytest.raises(SystemExit):
        parse(prefix, "--compare-to", cool, "--compare-metrics", "kendall")
    # analyze takes the same options
    a = cli.build_parser().parse_args(["analyze", cool, "-o", prefix, "--compare-to", cool, "--compare-metrics", "rmse"])
    assert a.compare_to == cool and a.compare_metrics == ["rmse"]
    # the file is refused to be overwritten like the others
    os.makedirs(os.path.dirname(prefix), exist_ok=True)
    with open(prefix + "_stripes.tsv", "w") as fh:
        fh.write("precious")
    with pytest.raises(SystemExit) as e:
        run_preflight(prefix, "--compare-to", cool)
    assert str(e.value) == f"refusing to overwrite {prefix}_stripes.tsv: pass --force to overwrite"
    assert run_preflight(prefix, "--compare-to", cool, "--force").outputs.cooler == prefix + ".cool"
    assert run_preflight(prefix).outputs.cooler == prefix + ".cool" and open(prefix + "_stripes.tsv").read() == "precious"


def test_preflight_refuses_before_anything_is_made(prefix, refs, tmp_path):
    cool, mcool = refs
    junk = str(tmp_path / "junk.cool")
    with open(junk, "w") as fh:
        fh.write("no hdf5")
    refused = [
        (["--compare-metrics", "rmse"], "--compare-metrics needs --compare-to"),
        (["--compare-resolution", "10kb"], "--compare-resolution needs --compare-to"),
        (["--compare-exclude-zero-pixels"], "--compare-exclude-zero-pixels needs --compare-to"),
        (["--compare-exclude-zero-pixels", "--skip-output"], "--compare-exclude-zero-pixels needs --compare-to"),
        (["--compare-to", cool, "--skip-output"], "--compare-to needs the output stage: it excludes --skip-output"),
        (["--compare-to", cool, "--compare-metrics", "rmse,spearman", "--compare-exclude-zero-pixels"],
         "--compare-exclude-zero-pixels: spearman"),
        (["--compare-to", str(tmp_path / "absent.cool")], f"--compare-to: {tmp_path / 'absent.cool'} is no file"),
        (["--compare-to", str(tmp_path / "absent.mcool") + "::/resolutions/5000"],
         f"--compare-to: {tmp_path / 'absent.mcool'} is no file"),
        (["--compare-to", junk], f"--compare-to: cannot read {junk}"),
        (["--compare-to", mcool + "::/resolutions/25000"], f"--compare-to: cannot read {mcool}::/resolutions/25000"),
        (["--compare-to", mcool + "::/resolutions/10000"],
         f"--compare-to: {mcool}::/resolutions/10000 has a bin size of 10000, the comparison runs at 5000"),
        (["--compare-to", cool, "--compare-resolution", "10kb"],
         f"--compare-to: {cool} has a bin size of 5000, the comparison runs at 10000"),
        (["--compare-to", cool, "--compare-resolution", "7500"], "--compare-resolution: 7500 is not a multiple"),
        (["--compare-to", cool, "--compare-resolution", "1kb"], "--compare-resolution: 1000 is not a multiple"),
    ]
    for options, message in refused:
        with pytest.raises(SystemExit) as e:
            run_preflight(prefix, *options)
        assert str(e.value).startswith(message), (options, str(e.value))
        assert not os.path.exists(os.path.dirname(prefix))


def test_what_the_plan_refuses(prefix, refs):
    cool, mcool = refs
    plan = [entry("chrA", 0, 100_000, 8, 20), entry("chrB", 0, 40_000, 8, 8, skipped=True)]
    misfit = driver.stripes_misfit
    assert misfit(plan, 5000, 5000, ["pearson", "spearman"], 5000, CHROMS) is None
    assert misfit(plan, 5000, 10000, ["pearson"], 10000, CHROMS, CHROMS) is None
    assert misfit(plan, 5000, 5000, ["pearson"], 5000, CHROMS[:1]) is None  # chrB is skipped: not compared
    assert misfit(plan, 5000, 10000, ["pearson"], 5000, CHROMS) == \
        "the file has a bin size of 5000, the comparison runs at 10000"
    assert misfit(plan, 5000, 5000, ["pearson"], 5000, [("chrX", 100_000)]) == "the file has no chromosome chrA"
    assert misfit(plan, 5000, 5000, ["pearson"], 5000, [("chrA", 99_999)]) == \
        "chromosome chrA has 99999 bp in the file and 100000 in the run"
    assert misfit(plan, 5000, 5000, ["pearson"], 5000, CHROMS, [("chrA", 120_000)]) == \
        "chromosome chrA has 100000 bp in the file and 120000 in the run"
    # an interval that is a part of its chromosome is compared by the chromosome's length
    part = [entry("chrA", 20_000, 60_000, 8, 8, size=100_000)]
    assert misfit(part, 5000, 5000, ["rmse"], 5000, CHROMS) is None
    deep = [entry("chrA", 0, 100_000, 4097, 5000)]
    assert misfit(deep, 5000, 5000, ["pearson", "rmse", "eucl_dist"], 5000, CHROMS) is None
    assert misfit(deep, 5000, 5000, ["rmse", "spearman"], 5000, CHROMS) == \
        "spearman ranks stripes of at most 4096 entries, the band of chrA:0-100000 has 4097 diagonals at 5000"
    assert misfit([entry("chrA", 0, 100_000, 4096, 5000)], 5000, 5000, ["spearman"], 5000, CHROMS) is None
    assert misfit(deep, 5000, 10000, ["spearman"], 10000, CHROMS) is None  # 2049 diagonals at 10 kb
    # cli.check_plan turns it into the end of the run
    a = parse(prefix, "--compare-to", cool, "--compare-metrics", "spearman")
    cfg = cli.config_from_args(a)
    pre = cli.preflight(a, cfg)
    assert cli.check_plan(a, cfg, pre, plan, CHROMS) == []
    for bad_plan, chroms, message in ((deep, CHROMS, "spearman ranks stripes of at most 4096 entries"),
                                      (plan, [("chrA", 100_001), ("chrB", 40_000)], "chromosome chrA has 100000 bp in "
                                       "the file and 100001 in the run"),
                                      ([entry("chrC", 0, 50_000, 8, 10)], [("chrC", 50_000)],
                                       "the file has no chromosome chrC")):
        with pytest.raises(SystemExit) as e:
            cli.check_plan(a, cfg, pre, bad_plan, chroms)
        assert str(e.value).startswith(f"--compare-to {cool}: {message}")
