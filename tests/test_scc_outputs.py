"""Two bands compared diagonal by diagonal, without a GPU: the numpy / Python-int restatement of the sums of
include/modle_pixels.h (modle_pixels_scc) that the GPU tests compare against, cross-checked against the
definition written as loops; pixels.scc_scores on the restated sums, its special cases and a float path that
shares nothing with it; the argument refusals of the C entry points, which need no device; the lines of
<prefix>_scc.tsv, driver.check_scc, and what cli.scc_options and driver.scc_misfit refuse of --scc.

The sums are integers and are compared exactly.  The float path forms the box sums by adding shifted float64
slices -- exact while every box sum is below 2^53, which holds for SCORE_SHAPES, so its non-zero mask is exact
too -- and correlates every stratum with np.corrcoef, whose float64 sums are the only inexact side.  The
tolerance of the SCC and of every stratum's correlation is 64 times the largest absolute difference measured
between the two on SCORE_SHAPES (seed 11, both sample conventions):
    measured 1.4432899320127035e-15        tolerance 9.24e-14
(at (300, 320, 10, 2^20), whose box sums reach 2^28 and their products 2^56: np.corrcoef rounds there; the
issue's scratch run had 2.3e-16 with another generator).  NaNs must fall in the same places.  A weight is
n (1 + 1 / n) (1 - 1 / n) / 12 in four float64 operations on the float side and one correctly rounded quotient
of integers in scc_scores: they differ by at most 4 roundings, and 8 * 2^-52 relative is asked for."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from modle_amd import cli, cooler, driver, pixels

M64 = (1 << 64) - 1
MEASURED = 1.4432899320127035e-15
TOLERANCE = 64 * MEASURED
WEIGHT_RTOL = 8 * 2.0**-52
# nrows, ncols, h, counts below
SCORE_SHAPES = [(5, 9, 0, 4), (9, 12, 2, 4), (64, 70, 1, 3), (70, 130, 3, 50), (129, 200, 5, 1000),
                (300, 320, 10, 2**20), (130, 150, 20, 2**32)]


# ---- the restatement ---------------------------------------------------------------------------------------

def dense_ints(band, nrows, ncols):
    """the symmetric matrix of a band as Python integers, object [ncols, ncols]; the words of the band that are
    no pixels are not used"""
    b = np.asarray(band[:nrows * ncols]).reshape(ncols, nrows)
    m = np.zeros((ncols, ncols), dtype=object)
    for d in range(nrows):
        at = np.arange(ncols - d)
        vals = np.array([int(x) for x in b[d:, d]], dtype=object)
        m[at, at + d] = vals
        m[at + d, at] = vals
    return m


def box_sums(m, h):
    """X(i, j) = the sum of m over |di| <= h, |dj| <= h, zeros outside: by a padded cumulative sum"""
    n = m.shape[0]
    z = np.zeros((n + 2 * h, n + 2 * h), dtype=object)
    z[h:h + n, h:h + n] = m
    s = np.zeros((n + 2 * h + 1, n + 2 * h + 1), dtype=object)
    s[1:, 1:] = z.cumsum(axis=0).cumsum(axis=1)
    k = 2 * h + 1
    return s[k:, k:] - s[:n, k:] - s[k:, :n] + s[:n, :n]


def restate(a, b, nrows, ncols, h, lo, hi):
    """uint64 [11, nrows]: what modle_pixels_scc writes for the bands `a` (reference) and `b`"""
    assert 0 <= lo <= hi and hi + 2 * h <= nrows - 1 <= ncols - 1
    xa, xb = box_sums(dense_ints(a, nrows, ncols), h), box_sums(dense_ints(b, nrows, ncols), h)
    out = np.zeros((11, nrows), dtype=np.uint64)
    for d in range(lo, hi + 1):
        sa, sb = [int(x) for x in np.diagonal(xa, d)], [int(x) for x in np.diagonal(xb, d)]
        assert len(sa) == ncols - d
        sums = (sum(sa), sum(sb), sum(x * x for x in sa), sum(y * y for y in sb), sum(x * y for x, y in zip(sa, sb)))
        out[0, d] = sum(1 for x, y in zip(sa, sb) if x or y)
        for k, v in enumerate(sums):
            assert v < 1 << 128
            out[1 + 2 * k, d], out[2 + 2 * k, d] = v & M64, v >> 64
    return out


def wide(rows, d):
    """(n, Sa, Sb, Saa, Sbb, Sab) of stratum d as Python integers"""
    w = [int(rows[k][d]) for k in range(11)]
    return (w[0],) + tuple(w[k] | (w[k + 1] << 64) for k in (1, 3, 5, 7, 9))


def random_pair(nrows, ncols, below, seed=11, density=0.4):
    """two bands with counts in [0, below) at `density` of the pixels; the words that are no pixels hold
    0xFFFFFFFF"""
    rng = np.random.default_rng([seed, nrows, ncols])
    n = nrows * ncols
    bands = []
    for _ in range(2):
        band = np.zeros(n + 1, dtype=np.uint32)
        mask = rng.random(n) < density
        band[:-1][mask] = rng.integers(0, below, size=int(mask.sum()), dtype=np.int64)
        for j in range(min(nrows, ncols)):
            band[j * nrows + j + 1:(j + 1) * nrows] = 0xFFFFFFFF
        band[n] = 0xFFFFFFFF
        bands.append(band)
    return bands


def cell(band, nrows, ncols, x, y):
    if not (0 <= x < ncols and 0 <= y < ncols) or abs(x - y) >= nrows:
        return 0
    return int(band[max(x, y) * nrows + abs(x - y)])


@pytest.mark.parametrize("nrows,ncols,h,lo,hi", [(1, 1, 0, 0, 0), (5, 5, 0, 0, 4), (5, 9, 1, 0, 2), (9, 12, 2, 1, 4),
                                                 (7, 7, 3, 0, 0), (12, 14, 1, 3, 5)])
def test_the_restatement_is_the_definition_written_as_loops(nrows, ncols, h, lo, hi):
    a, b = random_pair(nrows, ncols, 2**32)
    got = restate(a, b, nrows, ncols, h, lo, hi)
    assert got.shape == (11, nrows) and got.dtype == np.uint64
    for d in range(nrows):
        if not lo <= d <= hi:
            assert not got[:, d].any()
            continue
        ent = [tuple(sum(cell(band, nrows, ncols, i + di, i + d + dj) for di in range(-h, h + 1)
                         for dj in range(-h, h + 1)) for band in (a, b)) for i in range(ncols - d)]
        assert wide(got, d) == (sum(1 for x, y in ent if x or y), sum(x for x, _ in ent), sum(y for _, y in ent),
                                sum(x * x for x, _ in ent), sum(y * y for _, y in ent), sum(x * y for x, y in ent))


def test_the_sums_pass_64_bits():
    nrows, ncols, h = 41, 41, 20
    full = np.full(nrows * ncols + 1, 0xFFFFFFFF, dtype=np.uint32)
    rows = restate(full, full, nrows, ncols, h, 0, 0)
    n, sa, _, saa, _, sab = wide(rows, 0)
    assert n == ncols and saa == sab and saa >> 64 and sa < 1 << 64
    # every box is clipped on all sides: the largest one is the whole matrix
    assert max(int(x) for x in np.diagonal(box_sums(dense_ints(full, nrows, ncols), h))) == 41 * 41 * 0xFFFFFFFF


# ---- the scores ----------------------------------------------------------------------------------------------

def float_scores(a, b, nrows, ncols, h, lo, hi, include_zeros):
    """(scc, rho, weight) by a path that shares nothing with scc_scores or restate: float64 matrices, box sums
    as sums of shifted slices, np.corrcoef per stratum"""
    mats = []
    for band in (a, b):
        m = np.zeros((ncols + 2 * h, ncols + 2 * h))
        for j in range(ncols):
            for d in range(min(j + 1, nrows)):
                m[h + j - d, h + j] = m[h + j, h + j - d] = float(band[j * nrows + d])
        x = np.zeros((ncols, ncols))
        for di in range(2 * h + 1):
            for dj in range(2 * h + 1):
                x += m[di:di + ncols, dj:dj + ncols]
        assert x.max() < 2.0**53
        mats.append(x)
    rho, weight = np.full(hi - lo + 1, math.nan), np.zeros(hi - lo + 1)
    for d in range(lo, hi + 1):
        x, y = np.diagonal(mats[0], d), np.diagonal(mats[1], d)
        if not include_zeros:
            keep = (x != 0) | (y != 0)
            x, y = x[keep], y[keep]
        n = len(x)
        if n >= 2:
            weight[d - lo] = n * (1 + 1 / n) * (1 - 1 / n) / 12
            if x.min() != x.max() and y.min() != y.max():
                rho[d - lo] = np.corrcoef(x, y)[0, 1]
    total = weight.sum()
    scc = float(np.where(np.isfinite(rho), rho, 0.0) @ weight / total) if total > 0 else math.nan
    return scc, rho, weight


def score_differences(nrows, ncols, h, below):
    """the largest absolute difference of the SCC and of a stratum's correlation between scc_scores and the
    float path, over both sample conventions; the NaNs and the weights are held here"""
    a, b = random_pair(nrows, ncols, below)
    lo, hi = 1, nrows - 1 - 2 * h
    rows = restate(a, b, nrows, ncols, h, lo, hi)
    worst = 0.0
    for include_zeros in (False, True):
        scc, rho, weight = pixels.scc_scores(rows, ncols, lo, hi, include_zeros)
        want_scc, want_rho, want_weight = float_scores(a, b, nrows, ncols, h, lo, hi, include_zeros)
        assert rho.dtype == weight.dtype == np.float64 and rho.shape == weight.shape == (hi - lo + 1,)
        assert np.array_equal(np.isnan(rho), np.isnan(want_rho)) and math.isnan(scc) == math.isnan(want_scc)
        assert (np.abs(weight - want_weight) <= WEIGHT_RTOL * want_weight).all()
        ok = ~np.isnan(rho)
        worst = max([worst, abs(scc - want_scc) if scc == scc else 0.0] + list(np.abs(rho[ok] - want_rho[ok])))
    return worst


@pytest.mark.parametrize("nrows,ncols,h,below", SCORE_SHAPES)
def test_the_scores_are_those_of_a_float_path(nrows, ncols, h, below):
    worst = score_differences(nrows, ncols, h, below)
    print(f"scc_scores against the float path at {(nrows, ncols, h, below)}: {worst!r}")
    assert worst <= TOLERANCE


def rows_of(strata, nrows):
    """uint64 [11, nrows] from {d: [(a, b), ...]}: hand-made strata"""
    out = np.zeros((11, nrows), dtype=np.uint64)
    for d, ent in strata.items():
        sums = (sum(x for x, _ in ent), sum(y for _, y in ent), sum(x * x for x, _ in ent), sum(y * y for _, y in ent),
                sum(x * y for x, y in ent))
        out[0, d] = sum(1 for x, y in ent if x or y)
        for k, v in enumerate(sums):
            out[1 + 2 * k, d], out[2 + 2 * k, d] = v & M64, v >> 64
    return out


def test_the_scores_of_strata_that_are_special():
    # a band against itself scores 1.0 exactly, or NaN where nothing varies
    for nrows, ncols, h, below in ((5, 9, 0, 4), (64, 70, 1, 2**32), (130, 150, 20, 2**32)):
        a, _ = random_pair(nrows, ncols, below)
        hi = nrows - 1 - 2 * h
        scc, rho, weight = pixels.scc_scores(restate(a, a, nrows, ncols, h, 0, hi), ncols, 0, hi)
        assert ((rho == 1.0) | np.isnan(rho)).all() and (rho == 1.0).any()
        # (a stratum without a correlation counts as 0 and keeps its weight: only without one the SCC is 1)
        assert scc == sum(w for w, r in zip(weight, rho) if r == 1.0) / sum(weight) and (below < 2**32 or scc == 1.0)
    full = np.full(5 * 9 + 1, 7, dtype=np.uint32)
    scc, rho, weight = pixels.scc_scores(restate(full, full, 5, 9, 0, 1, 4), 9, 1, 4)
    assert scc == 0.0 and np.isnan(rho).all() and (weight > 0).all()
    # a stratum of constant a: rho is NaN, it counts as 0 and keeps its weight
    big = 3 << 40
    rows = rows_of({1: [(5, 1), (5, 2), (5, 9)], 2: [(1, 2), (2, 4), (4, 8), (big, 2 * big)]}, 4)
    scc, rho, weight = pixels.scc_scores(rows, 10, 1, 2)
    assert math.isnan(rho[0]) and rho[1] == 1.0
    assert weight[0] == (9 - 1) / 36 and weight[1] == (16 - 1) / 48
    assert scc == weight[1] / (weight[0] + weight[1])
    # n < 2: weight 0 and rho NaN; all weights 0: the SCC is NaN
    rows = rows_of({1: [(3, 4), (0, 0)], 2: [(0, 0), (0, 0)], 3: [(1, 2), (2, 1)]}, 4)
    scc, rho, weight = pixels.scc_scores(rows, 10, 1, 3)
    assert list(weight) == [0.0, 0.0, 3 / 24] and math.isnan(rho[0]) and math.isnan(rho[1]) and rho[2] == -1.0
    assert scc == -1.0
    scc, rho, weight = pixels.scc_scores(rows, 10, 1, 2)
    assert math.isnan(scc) and not weight.any() and np.isnan(rho).all()
    # include_zeros changes n only: the sums of the strata of 10 - d entries, of which the zeros are not listed
    rows = rows_of({1: [(1, 2), (2, 1), (3, 3)], 2: [(1, 1), (2, 3)]}, 3)
    scc, rho, weight = pixels.scc_scores(rows, 10, 1, 2, include_zeros=True)
    for d, ent in ((1, [(1, 2), (2, 1), (3, 3)] + [(0, 0)] * 6), (2, [(1, 1), (2, 3)] + [(0, 0)] * 6)):
        n = len(ent)
        assert n == 10 - d and weight[d - 1] == (n * n - 1) / (12 * n)
        assert abs(rho[d - 1] - np.corrcoef(*np.array(ent, dtype=float).T)[0, 1]) <= TOLERANCE
    plain = pixels.scc_scores(rows, 10, 1, 2)
    assert list(plain[2]) == [8 / 36, 3 / 24] and plain[1][1] == 1.0 and plain[1][0] != rho[0]
    # what is no [11, nrows] of uint64, and strata the rows do not hold
    for bad in (rows[:10], rows.astype(np.int64), rows[0]):
        with pytest.raises(ValueError):
            pixels.scc_scores(bad, 10, 1, 2)
    for lo, hi, ncols in ((2, 1, 10), (0, 3, 10), (-1, 2, 10), (1, 2, 2)):
        with pytest.raises(ValueError):
            pixels.scc_scores(rows, ncols, lo, hi)
    assert pixels.SCC_ROWS == 11 and pixels.MAX_SCC_SMOOTH == 20 == pixels.MAX_DOT_WINDOW


def test_what_the_entry_points_refuse_without_a_device():
    """every refusal comes before the handle or a band is touched: the handle here is host memory that names a
    device no machine has, and the bands and the output are addresses nobody owns"""
    lb = pixels.lib()
    assert pixels.scc_groups() == 128 or os.environ.get("MODLE_PIXELS_LIB")
    handle = (C.c_uint64 * 512)()
    C.cast(handle, C.POINTER(C.c_int))[0] = 1 << 20  # modle_pixels_handle.device
    h = C.addressof(handle)
    ref, tgt, out = 0x10000000, 0x20000000, 0x30000000
    nrows, ncols = 50, 90
    words = 11 * nrows
    band = (nrows * ncols + 1) * 4
    err = C.create_string_buffer(512)
    cases = {
        "no handle": (None, ref, tgt, nrows, ncols, 0, 1, 49, out, words),
        "no reference": (h, None, tgt, nrows, ncols, 0, 1, 49, out, words),
        "no target": (h, ref, None, nrows, ncols, 0, 1, 49, out, words),
        "no output": (h, ref, tgt, nrows, ncols, 0, 1, 49, None, words),
        "nrows 0": (h, ref, tgt, 0, ncols, 0, 0, 0, out, 0),
        "nrows > ncols": (h, ref, tgt, ncols + 1, ncols, 0, 1, 49, out, 11 * (ncols + 1)),
        "a smoothing above 20": (h, ref, tgt, nrows, ncols, 21, 1, 7, out, words),
        "a smoothing that wraps": (h, ref, tgt, nrows, ncols, (1 << 63) + 1, 1, 7, out, words),
        "min_diag > max_diag": (h, ref, tgt, nrows, ncols, 0, 5, 4, out, words),
        "max_diag beyond the band": (h, ref, tgt, nrows, ncols, 0, 1, 50, out, words),
        "a max_diag that wraps": (h, ref, tgt, nrows, ncols, 1, 1, M64, out, words),
        "a box beyond the band": (h, ref, tgt, nrows, ncols, 3, 1, 44, out, words),
        "the widest box beyond the band": (h, ref, tgt, nrows, ncols, 20, 1, 10, out, words),
        "out_words too small": (h, ref, tgt, nrows, ncols, 0, 1, 49, out, words - 1),
        "out_words too large": (h, ref, tgt, nrows, ncols, 0, 1, 49, out, words + 1),
        "a misaligned output": (h, ref, tgt, nrows, ncols, 0, 1, 49, out + 4, words),
        "the output overlaps the reference": (h, ref, tgt, nrows, ncols, 0, 1, 49, ref + band - 8, words),
        "the output ends in the reference": (h, ref, tgt, nrows, ncols, 0, 1, 49, ref - 8 * words + 8, words),
        "the output overlaps the target": (h, ref, tgt, nrows, ncols, 0, 1, 49, tgt + 8, words),
        "the output is the one band of both": (h, ref, ref, nrows, ncols, 0, 1, 49, ref, words),
    }
    for name, args in cases.items():
        err.value = b""
        assert lb.modle_pixels_scc(*args, None, err, len(err)) == pixels.ERR_ARG, name
        assert err.value.startswith(b"modle_pixels_scc: "), name
    ptr = C.c_void_p(1)
    for name, args in cases.items():
        if "out" in name:
            continue
        ptr.value = 1
        assert lb.modle_pixels_scc_to_host(*args[:8], C.byref(ptr), None, err, len(err)) == pixels.ERR_ARG, name
        assert ptr.value is None, name
    assert lb.modle_pixels_scc_to_host(h, ref, tgt, nrows, ncols, 0, 1, 49, None, None, err, len(err)) == pixels.ERR_ARG
    # the python forms refuse what ctypes would wrap
    for strata in ((-1, 1, 4), (0, -1, 4), (0, 1, 1 << 64)):
        with pytest.raises(pixels.PixelsError) as e:
            pixels._strata(*strata)
        assert e.value.code == pixels.ERR_ARG


# ---- <prefix>_scc.tsv ----------------------------------------------------------------------------------------

def entry(name, start, end, nrows, ncols, size=None, skipped=False):
    return {"interval": {"name": name, "size": end if size is None else size, "start": start, "end": end},
            "nrows": nrows, "ncols": ncols, "tasks": None, "skipped": skipped}


def test_the_lines_of_the_file(tmp_path):
    assert driver.scc_header("ref.mcool::/resolutions/10000", 10000, 20000, True) == \
        "# reference=ref.mcool::/resolutions/10000 resolution=10000 smooth=20000 include_zeros=yes\n" \
        "distance\tn\trho\tweight\n"
    iv = {"name": "chrA", "start": 25_000, "end": 75_000}
    rows = rows_of({1: [(1, 2), (2, 1), (3, 3)], 2: [(1, 1), (2, 3)], 3: [(4, 4)]}, 5)
    scc, rho, weight = pixels.scc_scores(rows, 10, 1, 3)
    assert math.isnan(rho[2]) and weight[2] == 0.0
    assert driver.scc_lines(iv, 5_000, 1, 10, 0, 1, 3, rows, False) == [
        f"# chrom=chrA start=25000 end=75000 bin_size=5000 smooth_bins=0 min_diag=1 max_diag=3 scc={scc:.17g}\n",
        f"5000\t3\t{rho[0]:.17g}\t{weight[0]:.17g}\n", f"10000\t2\t1\t{weight[1]:.17g}\n", "15000\t1\tnan\t0\n"]
    # with the zeros and at twice the bin size: n is the length of the diagonal, the distances are coarse bins
    scc0, rho0, weight0 = pixels.scc_scores(rows, 10, 2, 2, True)
    assert driver.scc_lines(iv, 5_000, 2, 10, 1, 2, 2, rows, True) == [
        f"# chrom=chrA start=25000 end=75000 bin_size=10000 smooth_bins=1 min_diag=2 max_diag=2 scc={scc0:.17g}\n",
        f"20000\t8\t{rho0[0]:.17g}\t{weight0[0]:.17g}\n"]
    empty = np.zeros((11, 5), dtype=np.uint64)
    assert driver.scc_lines(iv, 5_000, 1, 10, 0, 1, 1, empty, False) == [
        "# chrom=chrA start=25000 end=75000 bin_size=5000 smooth_bins=0 min_diag=1 max_diag=1 scc=nan\n", "5000\t0\tnan\t0\n"]
    plan = [entry("chrA", 0, 50_000, 5, 10), entry("chrB", 0, 9_000, 2, 2, skipped=True), entry("chrC", 5_000, 55_000, 5, 10)]
    asked = []

    def taken(k):
        asked.append(k)
        return None if k == 2 else (10, 0, 1, 3, rows)

    path = str(tmp_path / "p_scc.tsv")
    driver.write_scc(path, plan, 5_000, "r.cool", 5_000, 0, False, taken)
    assert asked == [0, 2]  # an entry that is skipped is not asked for, one without a matrix writes nothing
    assert open(path).read() == driver.scc_header("r.cool", 5_000, 0, False) + \
        "".join(driver.scc_lines(plan[0]["interval"], 5_000, 1, 10, 0, 1, 3, rows, False))


def diag_sums(band, nrows, ncols):
    b = np.asarray(band[:nrows * ncols], dtype=np.uint64).reshape(ncols, nrows)
    return np.array([int(b[d:, d].sum()) for d in range(nrows)], dtype=np.uint64)


@pytest.mark.parametrize("nrows,ncols,h", [(5, 9, 0), (9, 12, 2), (64, 70, 1), (70, 130, 3), (129, 200, 5),
                                           (300, 320, 10), (130, 150, 20)])
def test_check_scc_ties_the_sums_to_the_bands(nrows, ncols, h):
    a, b = random_pair(nrows, ncols, 1000)
    lo, hi = 0, nrows - 1 - 2 * h
    rows = restate(a, b, nrows, ncols, h, lo, hi)
    da, db = diag_sums(a, nrows, ncols), diag_sums(b, nrows, ncols)
    driver.check_scc("chrA:0-45000", rows, ncols, h, lo, hi, da, db)
    d = hi // 2
    if h == 0:
        assert [wide(rows, x)[1] for x in range(nrows)] == [int(x) for x in da]  # equality without smoothing
        for bump in (1, -1):
            bad = rows.copy()
            bad[1, d] = np.uint64((int(bad[1, d]) + bump) & M64)
            with pytest.raises(RuntimeError) as e:
                driver.check_scc("chrA:0-45000", bad, ncols, h, lo, hi, da, db)
            assert str(e.value).startswith(f"chrA:0-45000: diagonal {d} of the reference adds up to")
    bad = rows.copy()
    bad[2, d] += np.uint64(1)  # 2^64 more in Sa: beyond what the diagonals hold
    with pytest.raises(RuntimeError) as e:
        driver.check_scc("x", bad, ncols, h, lo, hi, da, db)
    assert f"diagonal {d} of the reference adds up to" in str(e.value)
    bad = rows.copy()
    bad[4, hi] += np.uint64(1)  # the same in Sb
    with pytest.raises(RuntimeError) as e:
        driver.check_scc("x", bad, ncols, h, lo, hi, da, db)
    assert f"diagonal {hi} of the run adds up to" in str(e.value)
    bad = rows.copy()
    bad[0, d] = np.uint64(ncols - d + 1)  # an n
    with pytest.raises(RuntimeError) as e:
        driver.check_scc("x", bad, ncols, h, lo, hi, da, db)
    assert f"diagonal {d} counts {ncols - d + 1} entries, it has {ncols - d} pixels" in str(e.value)
    _, _, _, saa, sbb, _ = wide(rows, d)
    beyond = math.isqrt(saa * sbb) + 1  # an Sab beyond Cauchy-Schwarz
    bad = rows.copy()
    bad[9, d], bad[10, d] = beyond & M64, beyond >> 64
    with pytest.raises(RuntimeError) as e:
        driver.check_scc("x", bad, ncols, h, lo, hi, da, db)
    assert f"diagonal {d} has Sab^2" in str(e.value)


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


def test_the_plan_of_before_has_no_scc():
    assert cli.Preflight._fields[-1] == "scc" and cli.Preflight._fields[:8] == (
        "bin_sizes", "outputs", "rank", "world", "device", "insulation", "dots", "pileup")
    outputs = cli.Outputs(None, None, None, None)
    for n_fields in (5, 11):  # the positional five, and every field of before
        pre = cli.Preflight(*([None, outputs, 0, 1, 0] + [None] * (n_fields - 5)))
        assert pre.scc is None and pre.outputs is outputs
    assert cli.Preflight(None, outputs, 0, 1, 0).coverage_min_diag == 0
    assert cli.Scc._fields == ("path", "smooth", "max_distance", "min_diag", "include_zeros")


def test_the_options_parse_and_preflight_plans_the_file(prefix, refs):
    cool, mcool = refs
    a = parse(prefix)
    assert (a.scc, a.scc_smooth, a.scc_max_distance, a.scc_ignore_diags, a.scc_include_zeros) == (None,) * 5
    assert run_preflight(prefix).scc is None and run_preflight(prefix, "--compare-to", cool).scc is None
    pre = run_preflight(prefix, "--compare-to", cool, "--scc")
    assert pre.scc == cli.Scc(prefix + "_scc.tsv", 0, None, 1, False) and pre.stripes.path == prefix + "_stripes.tsv"
    assert cli.scc_path(prefix) == prefix + "_scc.tsv" and not os.path.exists(prefix + "_scc.tsv")
    uri = mcool + "::/resolutions/10000"
    pre = run_preflight(prefix, "--compare-to", uri, "--compare-resolution", "10kb", "--scc", "--scc-smooth", "20kb",
                        "--scc-max-distance", "50kb", "--scc-ignore-diags", "0", "--scc-include-zeros")
    assert pre.scc == cli.Scc(prefix + "_scc.tsv", 20_000, 50_000, 0, True)
    assert run_preflight(prefix, "--compare-to", cool, "--scc", "--scc-smooth", "100kb").scc.smooth == 100_000  # 20 bins
    # analyze takes the same options
    a = cli.build_parser().parse_args(["analyze", cool, "-o", prefix, "--compare-to", cool, "--scc", "--scc-smooth", "5kb"])
    assert a.scc is True and a.scc_smooth == 5000
    # the file is refused to be overwritten like the others
    os.makedirs(os.path.dirname(prefix), exist_ok=True)
    with open(prefix + "_scc.tsv", "w") as fh:
        fh.write("precious")
    with pytest.raises(SystemExit) as e:
        run_preflight(prefix, "--compare-to", cool, "--scc")
    assert str(e.value) == f"refusing to overwrite {prefix}_scc.tsv: pass --force to overwrite"
    assert run_preflight(prefix, "--compare-to", cool, "--scc", "--force").scc.path == prefix + "_scc.tsv"
    assert run_preflight(prefix, "--compare-to", cool).scc is None and open(prefix + "_scc.tsv").read() == "precious"


def test_preflight_refuses_before_anything_is_made(prefix, refs):
    cool, mcool = refs
    both = ["--compare-to", cool, "--scc"]
    refused = [
        (["--scc-smooth", "5kb"], "--scc-smooth needs --scc"),
        (["--scc-max-distance", "50kb"], "--scc-max-distance needs --scc"),
        (["--scc-ignore-diags", "2"], "--scc-ignore-diags needs --scc"),
        (["--scc-include-zeros"], "--scc-include-zeros needs --scc"),
        (["--compare-to", cool, "--scc-smooth", "5kb"], "--scc-smooth needs --scc"),
        (["--scc"], "--scc needs --compare-to"),
        (["--scc", "--scc-smooth", "5kb"], "--scc needs --compare-to"),
        (both + ["--skip-output"], "--compare-to needs the output stage"),
        (both + ["--scc-smooth", "7500"], "--scc-smooth: 7500 is not a multiple of the resolution of the comparison (5000)"),
        (both + ["--scc-smooth", "105kb"], "--scc-smooth: 105000 is 21 bins of 5000: at most 20"),
        (["--compare-to", mcool + "::/resolutions/10000", "--compare-resolution", "10kb", "--scc", "--scc-smooth", "5kb"],
         "--scc-smooth: 5000 is not a multiple of the resolution of the comparison (10000)"),
        (both + ["--scc-max-distance", "12kb"], "--scc-max-distance: 12000 is not a multiple"),
        (both + ["--scc-ignore-diags", "-1"], "--scc-ignore-diags: -1 is negative"),
    ]
    for options, message in refused:
        with pytest.raises(SystemExit) as e:
            run_preflight(prefix, *options)
        assert str(e.value).startswith(message), (options, str(e.value))
        assert not os.path.exists(os.path.dirname(prefix))


def test_what_the_plan_refuses(prefix, refs):
    cool, _ = refs
    plan = [entry("chrA", 0, 100_000, 8, 20), entry("chrB", 0, 40_000, 4, 8, skipped=True)]
    assert driver.scc_strata(8, 5000, 0, None, 1) == (0, 1, 7)
    assert driver.scc_strata(8, 5000, 10_000, None, 1) == (2, 1, 3)
    assert driver.scc_strata(8, 5000, 10_000, 10_000, 0) == (2, 0, 2)
    assert driver.scc_strata(8, 5000, 5_000, 100_000, 1) == (1, 1, 5)  # no further than the band allows
    misfit = driver.scc_misfit
    assert misfit(plan, 5000, 5000, 0, None, 1) is None
    assert misfit(plan, 5000, 5000, 15_000, None, 1) is None  # 7 - 6: the one stratum 1; chrB is skipped
    assert misfit(plan, 5000, 5000, 15_000, None, 2) == \
        "no diagonal is left in the band of chrA:0-100000 (8 diagonals at 5000): with a smoothing of 3 bins the " \
        "last one is 1, the first one 2"
    assert misfit(plan, 5000, 5000, 20_000, None, 0).startswith("no diagonal is left in the band of chrA:0-100000")
    assert misfit(plan, 5000, 5000, 0, 5_000, 2).startswith("no diagonal is left in the band of chrA:0-100000")
    assert misfit(plan, 5000, 10000, 20_000, None, 1) is not None  # 5 diagonals at 10 kb: the one stratum 0
    assert misfit(plan, 5000, 10000, 20_000, None, 0) is None
    second = plan + [entry("chrB", 0, 40_000, 3, 8)]
    assert misfit(second, 5000, 5000, 5_000, None, 1).startswith("no diagonal is left in the band of chrB:0-40000")
    # cli.check_plan turns it into the end of the run
    a = parse(prefix, "--compare-to", cool, "--scc", "--scc-smooth", "15kb", "--scc-ignore-diags", "2")
    cfg = cli.config_from_args(a)
    pre = cli.preflight(a, cfg)
    with pytest.raises(SystemExit) as e:
        cli.check_plan(a, cfg, pre, plan, CHROMS)
    assert str(e.value).startswith("--scc: no diagonal is left in the band of chrA:0-100000")
    a = parse(prefix, "--compare-to", cool, "--scc", "--scc-smooth", "15kb")
    cfg = cli.config_from_args(a)
    assert cli.check_plan(a, cfg, cli.preflight(a, cfg), plan, CHROMS) == []
