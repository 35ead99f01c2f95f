"""Rescaled pileups without a GPU: the Python-int restatement of the definition in include/modle_pixels.h
(reference_rescale, reference_rescale_accepts: a triple loop that shares no code with the library) with the
properties the definition promises; rescale_blocks, the same sums formed per distinct window with numpy, which
tests/test_gpu_rescale.py holds the kernel to on shapes the triple loop would take minutes for, checked here
against the triple loop; the host-only acceptance rule of the library and every refusal; api.rescaled_expected
and api.domain_strength against their restatements; and what `simulate --domains-at` does around the kernel:
the BED reader and the placement of the domains, the option checks and the refusals, the checks before a row is
written and <prefix>_domains.tsv byte for byte."""
import math
import os

import numpy as np
import pytest

from test_gpu_marginals import make_band, reference_marginals
from test_pileup_outputs import I64_MAX, I64_MIN, plan_entry, reference_pileup

MAX_R = 128


def reference_rescale_accepts(nrows, ncols, r, start, end, bin_offset=0):
    """the rule in Python ints, which cannot overflow"""
    out = []
    for x, y in zip(start, end):
        s, e = int(x) - int(bin_offset), int(y) - int(bin_offset)
        out.append(0 <= s < e <= ncols and r <= e - s <= nrows)
    return np.array(out, dtype=bool)


def reference_rescale(band, nrows, ncols, r, start, end):
    """(pile, area as Python-int lists of lists [r][r], n_used) of windows that are already relative to the band:
    for every accepted window, every x and every y the word M(s + x, s + y) goes to the cell
    (floor(x r / W), floor(y r / W)), and the cell's area grows by one"""
    pile = [[0] * r for _ in range(r)]
    area = [[0] * r for _ in range(r)]
    n_used = 0
    for s, e in zip((int(x) for x in start), (int(x) for x in end)):
        if not (0 <= s < e <= ncols and r <= e - s <= nrows):
            continue
        n_used += 1
        w = e - s
        for x in range(w):
            for y in range(w):
                i, j = min(s + x, s + y), max(s + x, s + y)
                assert j - i < nrows and j - i <= j
                pile[x * r // w][y * r // w] += int(band[j * nrows + (j - i)])
                area[x * r // w][y * r // w] += 1
    return pile, area, n_used


def window_blocks(band, nrows, r, s, e):
    """(pile, area) of the one window [s, e), uint64 [r, r]: the W x W square of the symmetric matrix, gathered
    with numpy, and its rows and columns added up block by block (every block is a run: the label
    floor(x r / W) does not decrease, and W >= r leaves none empty)"""
    w = e - s
    x = np.arange(s, e, dtype=np.int64)
    i, j = np.minimum(x[:, None], x[None, :]), np.maximum(x[:, None], x[None, :])
    square = band[j * nrows + (j - i)].astype(np.uint64)
    label = np.arange(w, dtype=np.int64) * r // w
    first = np.flatnonzero(np.diff(label, prepend=-1))
    assert len(first) == r
    ones = np.ones((w, w), dtype=np.uint64)
    add = lambda m: np.add.reduceat(np.add.reduceat(m, first, axis=0), first, axis=1)
    return add(square), add(ones)


def rescale_blocks(band, nrows, ncols, r, start, end, cache=None):
    """(pile, area as uint64 [r, r], n_used): reference_rescale's sums, formed once per distinct window
    (`cache`: {(s, e): window_blocks}) and added with the number of times the window is listed; exact while
    the sums stay below 2^64"""
    start, end = np.asarray(start, dtype=np.int64).reshape(-1), np.asarray(end, dtype=np.int64).reshape(-1)
    ok = reference_rescale_accepts(nrows, ncols, r, start, end)
    pile, area = np.zeros((r, r), dtype=np.uint64), np.zeros((r, r), dtype=np.uint64)
    cache = {} if cache is None else cache
    if ok.any():
        wins, times = np.unique(np.stack([start[ok], end[ok]], axis=1), axis=0, return_counts=True)
        for (s, e), k in zip(wins.tolist(), times.tolist()):
            if (s, e) not in cache:
                cache[(s, e)] = window_blocks(band, nrows, r, s, e)
            pile += cache[(s, e)][0] * np.uint64(k)
            area += cache[(s, e)][1] * np.uint64(k)
    return pile, area, int(ok.sum())


def ragged_windows(nrows, ncols, r, n, seed):
    rng = np.random.default_rng([seed, nrows, ncols, r])
    w = rng.integers(r, nrows + 1, size=n)
    s = (rng.random(n) * (ncols - w + 1)).astype(np.int64)
    return s, s + w


# ---- the definition and its properties ------------------------------------------------------------------

def test_the_restatement_on_a_band_small_enough_to_do_by_hand():
    nrows, ncols = 3, 4
    band = np.zeros(nrows * ncols + 1, dtype=np.uint32)
    m = {(0, 0): 1, (0, 1): 2, (1, 1): 3, (0, 2): 4, (1, 2): 5, (2, 2): 6, (1, 3): 7, (2, 3): 8, (3, 3): 9}
    for (i, j), v in m.items():
        band[j * nrows + (j - i)] = v
    # the window [0, 3) on a grid of 2: blocks {0, 1} and {2} (floor(x * 2 / 3) = 0, 0, 1)
    pile, area, used = reference_rescale(band, nrows, ncols, 2, [0], [3])
    assert used == 1 and pile == [[1 + 2 + 2 + 3, 4 + 5], [4 + 5, 6]] and area == [[4, 2], [2, 1]]
    pile, area, used = reference_rescale(band, nrows, ncols, 2, [2, 0, -1, 3], [4, 4, 2, 3])
    assert used == 1 and pile == [[6, 8], [8, 9]] and area == [[1, 1], [1, 1]]  # W = 4 > nrows, s < 0, s == e
    pile, area, used = reference_rescale(band, nrows, ncols, 1, [1, 1], [4, 4])
    assert used == 2 and pile == [[2 * (3 + 6 + 9 + 2 * (5 + 7 + 8))]] and area == [[18]]


@pytest.mark.parametrize("nrows,ncols,r", [(9, 20, 3), (12, 30, 5), (7, 7, 7), (40, 90, 13)])
def test_windows_of_the_grid_s_own_width_are_the_on_diagonal_pileup(nrows, ncols, r):
    assert r % 2 == 1
    band = make_band(nrows, ncols, "full", limit=1000, seed=3)
    rng = np.random.default_rng([1, nrows, ncols, r])
    s = rng.integers(0, ncols - r + 1, size=30)
    pile, area, used = reference_rescale(band, nrows, ncols, r, s, s + r)
    want, n = reference_pileup(band, nrows, ncols, r // 2, s + r // 2, s + r // 2)
    assert used == n == 30 and np.array_equal(np.array(pile, dtype=np.uint64), want)
    assert area == [[30] * r for _ in range(r)]


@pytest.mark.parametrize("nrows,ncols,r,k", [(12, 30, 4, 3), (40, 90, 13, 3), (10, 10, 5, 2)])
def test_an_exact_multiple_sums_k_by_k_blocks(nrows, ncols, r, k):
    band = make_band(nrows, ncols, "full", limit=1000, seed=4)
    w = k * r
    assert w <= nrows
    for s in (0, ncols - w, (ncols - w) // 2):
        pile, area, used = reference_rescale(band, nrows, ncols, r, [s], [s + w])
        assert used == 1 and area == [[k * k] * r for _ in range(r)]
        for u in range(r):
            for v in range(r):
                block = 0
                for x in range(u * k, (u + 1) * k):
                    for y in range(v * k, (v + 1) * k):
                        i, j = min(s + x, s + y), max(s + x, s + y)
                        block += int(band[j * nrows + (j - i)])
                assert pile[u][v] == block


def test_symmetry_the_total_and_positive_areas_on_ragged_widths():
    nrows, ncols, r = 40, 90, 13
    band = make_band(nrows, ncols, "full", limit=1000, seed=5)
    start, end = ragged_windows(nrows, ncols, r, 60, 2)
    assert len(set((end - start).tolist())) > 15 and (end - start).min() >= r and (end - start).max() <= nrows
    pile, area, used = reference_rescale(band, nrows, ncols, r, start, end)
    assert used == 60
    assert all(pile[u][v] == pile[v][u] and area[u][v] == area[v][u] for u in range(r) for v in range(r))
    assert all(area[u][v] > 0 for u in range(r) for v in range(r))
    total = 0
    for s, e in zip(start.tolist(), end.tolist()):
        for i in range(s, e):
            for j in range(i, e):
                total += int(band[j * nrows + (j - i)]) * (1 if i == j else 2)
    assert sum(map(sum, pile)) == total
    assert sum(map(sum, area)) == sum((e - s) ** 2 for s, e in zip(start.tolist(), end.tolist()))
    # the numpy form the GPU tests use is the triple loop
    p2, a2, u2 = rescale_blocks(band, nrows, ncols, r, start, end)
    assert u2 == used and p2.tolist() == pile and a2.tolist() == area
    both = rescale_blocks(band, nrows, ncols, r, np.concatenate([start, start[:7], [-1, 80]]),
                          np.concatenate([end, end[:7], [20, 91]]))
    again = reference_rescale(band, nrows, ncols, r, start[:7], end[:7])
    assert both[2] == 67 and both[0].tolist() == [[pile[u][v] + again[0][u][v] for v in range(r)] for u in range(r)]


def test_the_api_s_closed_forms_of_the_blocks_and_the_area():
    from modle_amd import api

    for w, r in [(13, 13), (40, 13), (27, 4), (5, 1), (129, 128), (600, 60)]:
        lo = api.rescaled_block_edges(w, r)
        label = [x * r // w for x in range(w)]
        assert lo[0] == 0 and lo[r] == w and all(label[lo[u]:lo[u + 1]] == [u] * (lo[u + 1] - lo[u]) for u in range(r))
    nrows, ncols, r = 40, 90, 13
    start, end = ragged_windows(nrows, ncols, r, 50, 6)
    band = make_band(nrows, ncols, "empty")
    _, area, _ = rescale_blocks(band, nrows, ncols, r, start, end)
    hist = np.bincount(end - start, minlength=nrows + 1)
    got = api.rescaled_area(hist, r)
    assert got.dtype == np.uint64 and np.array_equal(got, area)
    assert not api.rescaled_area(np.zeros(nrows + 1), r).any()


# ---- the host-only acceptance rule ----------------------------------------------------------------------

def edge_windows(nrows, ncols, r):
    """(start, end) relative to the band: both sides of every edge of the rule and the int64 extremes in every
    position"""
    pairs = [(0, r), (0, r - 1), (0, nrows), (0, nrows + 1), (-1, r - 1), (-1, r), (ncols - r, ncols), (ncols - r + 1, ncols + 1),
             (ncols - nrows, ncols), (ncols - nrows - 1, ncols), (ncols - 1, ncols), (ncols, ncols), (ncols, ncols + 1),
             (5, 5), (5, 4), (0, 0), (0, 1), (0, ncols), (1, ncols + 1),
             (I64_MIN, I64_MIN), (I64_MAX, I64_MAX), (I64_MIN, I64_MAX), (I64_MAX, I64_MIN), (0, I64_MAX), (I64_MIN, r),
             (I64_MIN, 0), (I64_MAX, 0), (0, I64_MIN), (r, I64_MIN), (I64_MAX - 1, I64_MAX), (I64_MIN, I64_MIN + 1)]
    return np.array([p[0] for p in pairs], dtype=object), np.array([p[1] for p in pairs], dtype=object)


@pytest.mark.parametrize("nrows,ncols,r", [(1, 1, 1), (3, 3, 1), (7, 30, 3), (40, 65, 9), (65, 65, 65), (130, 300, 128),
                                           (40, 90, 13), (5, 9, 7)])
def test_accepts_equal_the_rule_at_every_edge_and_for_any_int64(nrows, ncols, r):
    from modle_amd import pixels

    start, end = edge_windows(nrows, ncols, r)
    want = reference_rescale_accepts(nrows, ncols, r, start, end)
    got = pixels.rescale_accepts(nrows, ncols, r, start.astype(np.int64), end.astype(np.int64))
    assert got.dtype == bool and np.array_equal(got, want)
    assert want.any() == (r <= nrows)
    for off in (7, -7, 2**61, -2**61, I64_MIN, I64_MAX, 1, -1):
        # the same windows shifted (where the shift stays an int64), and unshifted against the offset
        fits = np.array([I64_MIN <= int(x) + off <= I64_MAX and I64_MIN <= int(y) + off <= I64_MAX for x, y in zip(start, end)])
        s2 = np.array([int(x) + off for x in start[fits]], dtype=np.int64)
        e2 = np.array([int(x) + off for x in end[fits]], dtype=np.int64)
        assert np.array_equal(pixels.rescale_accepts(nrows, ncols, r, s2, e2, off), want[fits]), off
        assert np.array_equal(pixels.rescale_accepts(nrows, ncols, r, start.astype(np.int64), end.astype(np.int64), off),
                              reference_rescale_accepts(nrows, ncols, r, start, end, off)), off
    rng = np.random.default_rng([nrows, ncols, r])
    s = rng.integers(-3, ncols + 3, size=500)
    e = s + rng.integers(-2, nrows + 4, size=500)
    assert np.array_equal(pixels.rescale_accepts(nrows, ncols, r, s, e), reference_rescale_accepts(nrows, ncols, r, s, e))
    assert pixels.rescale_accepts(nrows, ncols, r, [], []).shape == (0,)


def test_accepts_refuses_what_the_kernel_refuses():
    from modle_amd import pixels

    assert pixels.MAX_RESCALE == MAX_R and pixels.rescale_groups() >= 1
    ok = pixels.rescale_accepts
    ok(40, 90, 128, [0], [40])  # a grid above the band: nothing is accepted, nothing is refused
    assert not ok(40, 90, 128, [0], [40]).any()
    for what, args in [("size == 0", (40, 90, 0, [0], [40])), ("size > 128", (200, 900, 129, [0], [150])),
                       ("a negative size", (40, 90, -1, [0], [40])), ("nrows == 0", (0, 90, 3, [0], [40])),
                       ("nrows > ncols", (91, 90, 3, [0], [40])), ("a negative shape", (-1, 90, 3, [0], [40])),
                       ("starts and ends of two lengths", (40, 90, 3, [0, 1], [40]))]:
        with pytest.raises(pixels.PixelsError) as e:
            ok(*args)
        assert e.value.code == pixels.ERR_ARG, what
    # n * ceil(min(nrows, ncols) / size)^2 >= 2^32, on both sides of its edge
    zeros = lambda n: (np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64))
    for nrows, r, n_fits in [(2**15, 1, 3), (65535, 1, 1), (2**15 + 1, 2, 15), (2**14 * 128, 128, 15), (2**14 * 128 - 127, 128, 15),
                             (2**14 * 128 + 1, 128, 15), (2**14 * 128 + 1, 127, 15), (1000, 3, 38500)]:
        c = -(-nrows // r)
        assert n_fits * c * c < 2**32 <= (n_fits + 1) * c * c, (nrows, r)
        assert ok(nrows, nrows + 5, r, *zeros(n_fits)).shape == (n_fits,)
        with pytest.raises(pixels.PixelsError) as e:
            ok(nrows, nrows + 5, r, *zeros(n_fits + 1))
        assert e.value.code == pixels.ERR_ARG
    assert ok(65536, 65536, 1, [], []).shape == (0,)  # n == 0: the product is 0
    with pytest.raises(pixels.PixelsError):
        ok(65536, 65536, 1, [0], [1])  # ceil^2 alone is 2^32
    with pytest.raises(pixels.PixelsError):
        ok(2**20, 2**20, 1, [0], [1])  # ceil^2 is 2^40: judged without forming n * ceil^2 in 64 bits the wrong way
    import ctypes as C

    big = pixels.lib().modle_pixels_rescale_accepts
    one = (C.c_int64 * 1)(0)
    out = (C.c_uint8 * 1)()
    assert big(40, 90, 3, 0, one, one, 2**31, out) == pixels.ERR_ARG  # n == 2^31, before an entry is read
    assert big(40, 90, 3, 0, None, one, 1, out) == pixels.ERR_ARG and big(40, 90, 3, 0, one, one, 1, None) == pixels.ERR_ARG
    assert big(40, 90, 3, 0, None, None, 0, None) == 0


# ---- the expected pile and the strength -----------------------------------------------------------------

def restated_expected(width_hist, diag_sum, ncols, r):
    """per pixel: every (x, y) of every width counts one for its cell and its distance"""
    cnt = [[{} for _ in range(r)] for _ in range(r)]
    for w, k in enumerate(int(x) for x in width_hist):
        for x in range(w if k else 0):
            for y in range(w):
                cell = cnt[x * r // w][y * r // w]
                cell[abs(y - x)] = cell.get(abs(y - x), 0) + k
    out = np.zeros((r, r))
    for u in range(r):
        for v in range(r):
            out[u, v] = math.fsum(float(cnt[u][v][d]) * (float(int(diag_sum[d])) / float(ncols - d)) for d in sorted(cnt[u][v]))
    return out, cnt


@pytest.mark.parametrize("nrows,ncols,r", [(12, 30, 5), (40, 90, 13), (9, 9, 1), (20, 20, 20)])
def test_rescaled_expected_equals_its_restatement_bit_for_bit(nrows, ncols, r):
    from modle_amd import api

    band = make_band(nrows, ncols, "full", limit=0xFFFFFFFF, seed=7)
    diag_sum = reference_marginals(band, nrows, ncols, 0)[0]
    start, end = ragged_windows(nrows, ncols, r, 40, 8)
    hist = np.bincount(end - start, minlength=nrows + 1).astype(np.uint64)
    hist[nrows] += 3
    want, cnt = restated_expected(hist, diag_sum, ncols, r)
    got = api.rescaled_expected(hist, diag_sum, ncols, r)
    assert got.dtype == np.float64 and got.shape == (r, r) and np.array_equal(got, want) and (got > 0).all()
    counts = api.rescaled_expected_counts(hist, r)
    for u in range(r):
        for v in range(u, r):
            row = counts[v * (v + 1) // 2 + u]
            assert {int(d): int(row[d]) for d in np.flatnonzero(row)} == cnt[u][v] == cnt[v][u]
    terms = api.rescaled_expected_terms(hist, diag_sum, ncols, r)
    assert len(terms) == r * r and [math.fsum(t) for t in terms] == want.reshape(-1).tolist()
    # the area is the number of pairs
    assert np.array_equal(api.rescaled_area(hist, r).astype(np.int64),
                          np.array([[sum(cnt[u][v].values()) for v in range(r)] for u in range(r)]))
    assert not api.rescaled_expected(np.zeros(nrows + 1), diag_sum, ncols, r).any()
    with pytest.raises(ValueError):
        api.rescaled_expected(np.ones(nrows + 2), diag_sum, ncols, max(r, 2))  # a width below the grid (and one above the band)
    with pytest.raises(ValueError):
        api.rescaled_expected([0] * (nrows + 1) + [1], diag_sum, ncols, r)  # W = nrows + 1


def test_domain_strength_on_a_hand_made_pile():
    from modle_amd import api

    assert api.domain_strength_blocks(6, 100) == (2, 4) and api.domain_strength_blocks(60, 100) == (20, 40)
    assert api.domain_strength_blocks(60, 0) == (0, 60) and api.domain_strength_blocks(7, 50) == (2, 5)  # 1.75 up, 5.25 down
    assert api.domain_strength_blocks(128, 200) == (52, 76) and api.domain_strength_blocks(1, 100) == (1, 0)
    pile = np.arange(36, dtype=np.uint64).reshape(6, 6) + np.uint64(2**63)
    expected = np.full((6, 6), 0.1)
    expected[2, 3] = 1e20
    within = [(2, 2), (2, 3), (3, 3)]
    between = [(0, 2), (0, 3), (1, 2), (1, 3), (2, 4), (2, 5), (3, 4), (3, 5)]
    ow, ob = sum(2**63 + 6 * u + v for u, v in within), sum(2**63 + 6 * u + v for u, v in between)
    ew, eb = math.fsum([0.1, 1e20, 0.1]), math.fsum([0.1] * 8)
    got = api.domain_strength(pile, expected, 6, 100)
    assert got == (float(ow) / ew) / (float(ob) / eb) and got > 0
    flat = api.domain_strength(np.ones((6, 6), dtype=np.uint64), np.ones((6, 6)), 6, 100)
    assert flat == 1.0
    nan = lambda *a: math.isnan(api.domain_strength(*a))
    assert nan(pile, expected, 6, 0)                                   # no flank: nothing to compare with
    assert nan(np.ones((1, 1)), np.ones((1, 1)), 1, 100)               # no cell within
    assert nan(np.ones((2, 2)), np.ones((2, 2)), 2, 100)               # g0 = 1, g1 = 1
    zero = np.ones((6, 6))
    for cell in within:
        zero[cell] = 0.0
    assert nan(pile, zero, 6, 100)                                     # nothing expected within
    zero = np.ones((6, 6))
    for cell in between:
        zero[cell] = 0.0
    assert nan(pile, zero, 6, 100) and nan(zero, np.ones((6, 6)), 6, 100)  # nothing expected, nothing observed between
    with pytest.raises(ValueError):
        api.domain_strength(pile, expected, 5, 100)


# ---- the domains of `simulate --domains-at` -------------------------------------------------------------

BED = ("#chrom\tstart\tend\tname\n"
       "chrA\t100000\t150000\tfirst\t.\n"     # bins 20 .. 29 of 5 kb: columns 17 .. 27 of an interval from bin 3
       "\n"
       "chrA\t100000\t150001\n"               # one base into bin 30: the end rounds up
       "# a remark\n"
       "chrA\t102000\t103000\n"               # inside one bin: one bin wide
       "chrA 200000 200000\n"                 # blanks instead of tabs, empty: one bin wide
       "chrA\t15000\t30000\n"                 # at the interval's start: the padding leaves the band
       "chrA\t10000\t30000\n"                 # starts before the interval
       "chrA\t590000\t600001\n"               # ends after it
       "chrB\t0\t5000\n"                      # chrB is skipped
       "chrC\t0\t10\n"                        # not simulated
       "chrD\t5000\t15000\n"                  # spans two intervals
       "chrD\t12000\t50000\n")


def test_the_bed_reader_and_the_placement(tmp_path):
    from modle_amd import driver

    path = str(tmp_path / "tads.bed")
    with open(path, "w") as fh:
        fh.write(BED)
    domains = driver.read_bed(path)
    assert domains == [("chrA", 100000, 150000), ("chrA", 100000, 150001), ("chrA", 102000, 103000), ("chrA", 200000, 200000),
                       ("chrA", 15000, 30000), ("chrA", 10000, 30000), ("chrA", 590000, 600001), ("chrB", 0, 5000),
                       ("chrC", 0, 10), ("chrD", 5000, 15000), ("chrD", 12000, 50000)]
    plan = [plan_entry("chrA", 15_000, 600_000, 40, 117), plan_entry("chrB", 0, 10_000, 2, 2, skipped=True),
            plan_entry("chrD", 0, 10_000, 2, 2), plan_entry("chrD", 10_000, 50_000, 8, 8)]
    placed, unplaced = driver.place_domains(plan, 5000, 5000, 100, domains)
    assert unplaced == 5 and sorted(placed) == [0, 3]
    assert placed[0][0].dtype == placed[0][1].dtype == np.int64
    # [17, 27) padded by 10, [17, 28) by 11, [17, 18) by 1, [37, 38) by 1, [0, 3) by 3: not clipped
    assert placed[0][0].tolist() == [7, 6, 16, 36, -3] and placed[0][1].tolist() == [37, 39, 19, 39, 6]
    assert placed[3][0].tolist() == [-8] and placed[3][1].tolist() == [16]  # [0, 8) padded by 8
    placed, unplaced = driver.place_domains(plan, 5000, 5000, 0, domains)
    assert placed[0][0].tolist() == [17, 17, 17, 37, 0] and placed[0][1].tolist() == [27, 28, 18, 38, 3]
    placed, unplaced = driver.place_domains(plan, 5000, 5000, 55, domains)  # 10 * 55 // 100 = 5, 11 * 55 // 100 = 6, 0, 0, 1
    assert placed[0][0].tolist() == [12, 11, 17, 37, -1] and placed[0][1].tolist() == [32, 34, 18, 38, 4]
    # at twice the bin size the interval starts in coarse bin 1 of its chromosome
    placed, unplaced = driver.place_domains(plan, 5000, 10_000, 100, domains)
    assert unplaced == 5
    assert placed[0][0].tolist() == [4, 3, 8, 18, -2] and placed[0][1].tolist() == [19, 21, 11, 21, 4]
    assert driver.place_domains(plan, 5000, 5000, 100, []) == ({}, 0)
    # the rule rejects what leaves the band: nothing is clipped into it
    from modle_amd import pixels

    placed, _ = driver.place_domains(plan, 5000, 5000, 100, domains)
    assert pixels.rescale_accepts(40, 117, 3, *placed[0]).tolist() == [True, True, True, True, False]
    # what cannot be read
    for text, why in [("chrA\t1\n", "line 1: fewer than three columns"), ("#x\nchrA\t1\tx\n", "line 2: invalid literal"),
                      ("chrA\t5\t2\n", "line 1: a negative start or an end before its start"),
                      ("chrA\t-5\t2\n", "line 1: a negative start")]:
        bad = str(tmp_path / "bad.bed")
        with open(bad, "w") as fh:
            fh.write(text)
        with pytest.raises(ValueError) as e:
            driver.read_bed(bad)
        assert str(e.value).startswith(f"{bad}, {why}"), text
    with pytest.raises(OSError):
        driver.read_bed(str(tmp_path / "missing.bed"))


def test_a_size_no_window_reaches_and_a_file_that_cannot_be_read_are_named(tmp_path):
    from modle_amd import driver

    plan = [plan_entry("chrA", 0, 2_000_000, 40, 400), plan_entry("chrB", 0, 500_000, 80, 100, skipped=True),
            plan_entry("chrC", 25_000, 1_000_000, 39, 195)]
    assert driver.domains_misfit(plan, 5000, 5000, 40) is None
    assert driver.domains_misfit(plan, 5000, 5000, 41) == ("size", 41, 40)  # (the skipped band does not count)
    assert driver.domains_misfit(plan[1:], 5000, 5000, 40) == ("size", 40, 39)
    assert driver.domains_misfit(plan[:1], 5000, 10_000, 21) is None  # at twice the bin size 40 diagonals are 21
    assert driver.domains_misfit(plan[:1], 5000, 10_000, 22) == ("size", 22, 21)
    assert driver.domains_misfit(plan[1:2], 5000, 5000, 128) is None  # no matrix: nothing to say
    good, bad, missing = str(tmp_path / "good.bed"), str(tmp_path / "bad.bed"), str(tmp_path / "missing.bed")
    with open(good, "w") as fh:
        fh.write(BED)
    with open(bad, "w") as fh:
        fh.write("chrA\t1\n")
    assert driver.domains_misfit(plan, 5000, 5000, 40, [good]) is None
    assert driver.domains_misfit(plan, 5000, 5000, 41, [good, bad, missing]) == ("bed", bad, f"{bad}, line 1: fewer than three columns")
    got = driver.domains_misfit(plan, 5000, 5000, 40, [missing])
    assert got[:2] == ("bed", missing) and "No such file" in got[2]


# ---- the options and preflight --------------------------------------------------------------------------

@pytest.fixture
def prefix(tmp_path, monkeypatch):
    for name in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(name, raising=False)
    return str(tmp_path / "out" / "p")


def run_preflight(prefix, *extra, command="simulate"):
    from modle_amd import cli

    head = ["simulate", "-c", "g.chrom.sizes", "-b", "b.bed"] if command == "simulate" else ["analyze", "in.cool"]
    a = cli.build_parser().parse_args([*head, "-o", prefix, *(["-r", "5kb"] if command == "simulate" else []), *extra])
    cfg = cli.config_from_args(a) if command == "simulate" else __import__("modle_amd").api.make_config(bin_size=5000)
    return cli.preflight(a, cfg)


def test_the_options_parse_and_preflight_plans_the_file(prefix):
    from modle_amd import cli

    pre = run_preflight(prefix, "--no-track-1d-lef-position")
    assert pre.domains is None and pre.outputs == cli.Outputs(prefix + ".cool", None, None, None)  # as before
    # the field, between the two it was put between; the constructions of before still make a plan
    assert cli.Preflight._fields[-3:] == ("coverage_min_diag", "domains", "scc") and len(cli.Preflight._fields) == 13
    assert cli.Preflight._fields[:8] == ("bin_sizes", "outputs", "rank", "world", "device", "insulation", "dots", "pileup")
    five = cli.Preflight([5000], pre.outputs, 0, 1, 0)
    assert five.domains is None and five.scc is None and five.coverage_min_diag == 0
    eleven = cli.Preflight([5000], pre.outputs, 0, 1, 0, None, None, None, None, None, 2)
    assert eleven.coverage_min_diag == 2 and eleven.domains is None and eleven.scc is None
    assert cli.Domains._fields == ("path", "resolution", "size", "flank_percent", "sources")
    pre = run_preflight(prefix, "--domains-at", "tads.bed")
    assert pre.domains == cli.Domains(prefix + "_domains.tsv", 5000, 60, 100, ["tads.bed"])
    assert cli.domains_path(prefix) == prefix + "_domains.tsv"
    pre = run_preflight(prefix, "--domains-at", "x/a.bed", "--domains-at", "b.bed", "--domains-at", "x/a.bed", "--domains-size", "128",
                        "--domains-flank-percent", "0", "--domains-resolution", "25kb")
    assert pre.domains == cli.Domains(prefix + "_domains.tsv", 25_000, 128, 0, ["x/a.bed", "b.bed", "x/a.bed"])
    assert run_preflight(prefix, "--domains-at", "t.bed", "--domains-size", "1", "--domains-flank-percent", "200").domains[2:4] == (1, 200)
    pre = run_preflight(prefix, "--domains-at", "tads.bed", "--skip-output")
    assert pre.domains.path is None and pre.domains.sources == ["tads.bed"]
    assert not os.path.exists(prefix + "_domains.tsv")
    # analyze takes the same options through the same function
    pre = run_preflight(prefix, "--domains-at", "tads.bed", "--domains-size", "30", command="analyze")
    assert pre.domains == cli.Domains(prefix + "_domains.tsv", 5000, 30, 100, ["tads.bed"])


REFUSED = [
    (["--domains-size", "30"], "--domains-size needs --domains-at"),
    (["--domains-flank-percent", "50"], "--domains-flank-percent needs --domains-at"),
    (["--domains-resolution", "10kb", "--skip-output"], "--domains-resolution needs --domains-at"),
    (["--domains-at", "t.bed", "--domains-size", "0"], "--domains-size: 0 is not in [1, 128]"),
    (["--domains-at", "t.bed", "--domains-size", "129"], "--domains-size: 129 is not in [1, 128]"),
    (["--domains-at", "t.bed", "--domains-flank-percent", "201"], "--domains-flank-percent: 201 is not in [0, 200]"),
    (["--domains-at", "t.bed", "--domains-flank-percent", "-1"], "--domains-flank-percent: -1 is not in [0, 200]"),
    (["--domains-at", "t.bed", "--domains-resolution", "12500"], "--domains-resolution: 12500 is not a multiple"),
    (["--domains-at", "t.bed", "--domains-resolution", "1kb"], "--domains-resolution: 1000 is not a multiple"),
]


@pytest.mark.parametrize("options,message", REFUSED)
def test_preflight_refuses_before_anything_is_made(prefix, options, message):
    with pytest.raises(SystemExit) as e:
        run_preflight(prefix, *options)
    assert str(e.value).startswith(message)
    assert not os.path.exists(os.path.dirname(prefix))


def test_the_domains_file_is_refused_to_be_overwritten_after_the_pileup_file(prefix):
    everything = ["--no-track-1d-lef-position", "--pileup-at", "barriers", "--domains-at", "t.bed", "--subsample-frac", "0.5"]
    os.makedirs(os.path.dirname(prefix))
    for which in ("_sampled.cool", "_domains.tsv", "_pileup.tsv"):  # each one is named before the one before it
        with open(prefix + which, "wb") as fh:
            fh.write(b"precious")
        with pytest.raises(SystemExit) as e:
            run_preflight(prefix, *everything)
        assert str(e.value) == f"refusing to overwrite {prefix + which}: pass --force to overwrite"
    assert run_preflight(prefix, *everything, "--force").domains.path == prefix + "_domains.tsv"
    os.remove(prefix + "_pileup.tsv"), os.remove(prefix + "_sampled.cool")
    assert run_preflight(prefix, "--no-track-1d-lef-position").domains is None  # without the option: nobody's business
    assert open(prefix + "_domains.tsv", "rb").read() == b"precious"


def test_the_plan_refuses_a_size_and_a_file_before_anything_is_simulated(tmp_path, prefix):
    """plan_run's messages, on a genome of one chromosome: -w 200kb at 5 kb is a band of 40 diagonals"""
    from modle_amd import cli

    sizes, bed, tads = str(tmp_path / "g.chrom.sizes"), str(tmp_path / "b.bed"), str(tmp_path / "tads.bed")
    with open(sizes, "w") as fh:
        fh.write("chrA\t2000000\n")
    with open(bed, "w") as fh:
        fh.write("chrA\t41000\t41019\t.\t0.8\t+\nchrA\t141000\t141019\t.\t0.8\t-\n")
    with open(tads, "w") as fh:
        fh.write("chrA\t100000\t150000\n")

    def plan(*extra):
        a = cli.build_parser().parse_args(["simulate", "-c", sizes, "-b", bed, "-o", prefix, "-r", "5kb", "-w", "200kb",
                                           *extra])
        cfg = cli.config_from_args(a)
        return cli.plan_run(a, cfg, cli.preflight(a, cfg), lambda *x: None)

    assert len(plan("--domains-at", tads, "--domains-size", "40")[1]) == 1
    with pytest.raises(SystemExit) as e:
        plan("--domains-at", tads, "--domains-size", "41")
    assert str(e.value) == "--domains-size: no window reaches 41 bins of 5000: the deepest band has 40 diagonals"
    assert len(plan("--domains-at", tads, "--domains-size", "21", "--domains-resolution", "10kb")[1]) == 1
    with pytest.raises(SystemExit) as e:
        plan("--domains-at", tads, "--domains-size", "22", "--domains-resolution", "10kb")
    assert str(e.value) == "--domains-size: no window reaches 22 bins of 10000: the deepest band has 21 diagonals"
    with open(tads, "w") as fh:
        fh.write("chrA\t100000\n")
    with pytest.raises(SystemExit) as e:
        plan("--domains-at", tads)
    assert str(e.value) == f"--domains-at {tads}: the file cannot be read as BED: {tads}, line 1: fewer than three columns"
    with pytest.raises(SystemExit) as e:
        plan("--domains-at", str(tmp_path / "none.bed"))
    assert str(e.value).startswith(f"--domains-at {tmp_path / 'none.bed'}: the file cannot be read as BED: ")
    assert len(plan("--domains-at", str(tmp_path / "none.bed"), "--skip-output")[1]) == 1  # no file is planned: none is read


# ---- the checks and the file ----------------------------------------------------------------------------

def test_the_header_and_the_rows_of_a_block():
    from modle_amd import driver

    assert driver.domains_header("a b.bed", 5000, 2, 100, 41, 40, 38, 1 / 3) == (
        f"#source=a b.bed\tresolution=5000\tsize=2\tflank_percent=100\tgiven=41\tplaced=40\tused=38\tstrength={1 / 3!r}\n")
    assert driver.domains_header("t.bed", 10_000, 60, 0, 0, 0, 0, math.nan).endswith("\tused=0\tstrength=nan\n")
    assert driver.domains_lines(2, [2**64 + 1, 0, 3, 4], [2**65, 1, 2, 3], [0.1, 0.0, 1e300, 1 / 3]) == [
        "0\t0\t18446744073709551617\t36893488147419103232\t0.1\n", "0\t1\t0\t1\t0.0\n", "1\t0\t3\t2\t1e+300\n",
        f"1\t1\t4\t3\t{1 / 3!r}\n"]


def test_a_rescaled_pile_is_checked_before_a_row_is_written():
    from modle_amd import driver

    nrows, ncols, r = 12, 30, 4
    band = make_band(nrows, ncols, "full", limit=1000, seed=2)
    start, end = [2, 5, 5, 18], [10, 17, 17, 30]
    pile, area, used = rescale_blocks(band, nrows, ncols, r, start, end)
    hist = np.bincount(np.array(end) - np.array(start), minlength=nrows + 1).astype(np.uint64)
    alone = lambda s, e: rescale_blocks(band, nrows, ncols, r, [s], [e])[0]
    totals = [int(alone(s, e).sum()) for s, e in zip(start, end)]
    wins = list(zip(start, end))
    driver.check_rescaled("chrA:0-100", "t.bed", r, pile, area, used, hist, wins, totals, alone)
    driver.check_rescaled("chrA:0-100", "t.bed", r, np.zeros((r, r)), np.zeros((r, r)), 0, np.zeros(nrows + 1))
    lopsided, wrong_area = pile.copy(), area.copy()
    lopsided[1, 2] += 1
    wrong_area[0, 0] += 1
    for what, args, message in [
            ("the count", (r, pile, area, used + 1, hist, wins, totals, alone), "used 5 windows, their widths count 4"),
            ("the area", (r, pile, wrong_area, used, hist, wins, totals, alone), "cell (0, 0) of the rescaled pileup at t.bed took"),
            ("the symmetry", (r, lopsided, area, used, hist, wins, totals, alone),
             "the pile of the rescaled pileup at t.bed is not symmetric"),
            ("a window", (r, pile, area, used, hist, wins, [totals[0], totals[1] + 1], alone),
             "the window [5, 17) of the rescaled pileup at t.bed piles"),
            ("the shape", (r + 1, pile, area, used, hist, wins, totals, alone), "not 5 x 5")]:
        with pytest.raises(RuntimeError) as e:
            driver.check_rescaled("chrA:0-100", "t.bed", *args)
        assert str(e.value).startswith("chrA:0-100: ") and message in str(e.value), what


def test_the_total_of_a_window_from_the_pixels():
    from modle_amd import driver
    from test_cooler_pixels import reference_pixels

    from modle_amd import pixels

    nrows, ncols = 12, 30
    band = make_band(nrows, ncols, "tenth", limit=1000, seed=9)
    band[5 * nrows] = 7  # a diagonal pixel
    b1, b2, cn, index = reference_pixels(band, nrows, ncols, 0)
    px = pixels.Pixels(b1, b2, cn, index, None)
    for s, e in [(0, 12), (3, 9), (18, 30), (5, 6), (0, 1)]:
        assert driver.window_total(px, s, e) == int(rescale_blocks(band, nrows, ncols, 1, [s], [e])[0][0, 0]), (s, e)


class FakeSim:
    """what the file stage asks of a simulator for a cooler and the domains file: one band, held in numpy"""
    device = 0

    def __init__(self, band, nrows, ncols, iid):
        self.band, self.nrows, self.ncols, self.iid, self.calls = band, nrows, ncols, iid, []

    def copy_outputs(self, interval_id, want_contacts=True):
        assert interval_id == self.iid and not want_contacts
        return None, 0, None

    def outputs(self, interval_id):
        return 0x1000, None, self.nrows, self.ncols

    def pixels(self, interval_id, bin_offset=0, stream=None, factor=1, first_bin=0):
        from test_cooler_pixels import reference_pixels

        from modle_amd import pixels

        assert (interval_id, factor, first_bin) == (self.iid, 1, 0)
        self.calls.append("pixels")
        b1, b2, cn, index = reference_pixels(self.band, self.nrows, self.ncols, bin_offset)
        return pixels.Pixels(b1, b2, cn, index, pixels.Stats(len(cn), int(cn.sum()), int(cn.max())))

    def marginals(self, interval_id, min_diag=0, factor=1, first_bin=0):
        self.calls.append("marginals")
        return reference_marginals(self.band, self.nrows, self.ncols, min_diag)

    def rescaled_pileup(self, interval_id, start, end, size, factor=1, first_bin=0, bin_offset=0):
        assert (interval_id, factor, first_bin, bin_offset) == (self.iid, 1, 0, 0)
        self.calls.append(("rescaled_pileup", len(start)))
        pile, area, used = rescale_blocks(self.band, self.nrows, self.ncols, size, start, end)
        ok = reference_rescale_accepts(self.nrows, self.ncols, size, start, end)
        w = (np.asarray(end, dtype=np.int64) - np.asarray(start, dtype=np.int64))[ok]
        return pile, area, used, np.bincount(w, minlength=self.nrows + 1).astype(np.uint64)


def test_the_file_stage_writes_the_domains_file(tmp_path):
    from modle_amd import api, cli, driver

    nrows, ncols, iid, r, percent = 12, 30, 7, 4, 50
    band = make_band(nrows, ncols, "full", limit=1000, seed=11)
    cfg = api.make_config(bin_size=5000)
    chroms = [("chrA", 150_000), ("chrB", 150_000)]
    plan = [plan_entry("chrA", 0, 150_000, nrows, ncols), plan_entry("chrB", 0, 150_000, nrows, ncols, skipped=True)]
    ids = [iid, None]  # chrB has no matrix
    tads, none = str(tmp_path / "tads.bed"), str(tmp_path / "none.bed")
    with open(tads, "w") as fh:  # [4, 8) padded by 2, twice; [10, 16) by 3; [0, 4) leaves the band; chrB and chrC
        fh.write("chrA\t20000\t40000\nchrA\t20000\t40000\nchrA\t50000\t80000\nchrA\t0\t20000\nchrB\t0\t20000\nchrC\t0\t5\n")
    with open(none, "w") as fh:
        fh.write("# no domain\n")
    p = str(tmp_path / "p")
    pre = cli.Preflight(None, cli.Outputs(p + ".cool", None, None, None), 0, 1, 0,
                        domains=cli.Domains(cli.domains_path(p), 5000, r, percent, [tads, none, tads]))
    sim, said = FakeSim(band, nrows, ncols, iid), []
    driver.write_outputs(sim, cfg, plan, ids, None, pre, (), said.append, chroms=chroms)
    assert said == [f"written {p}.cool", f"--domains-at {tads}: 2 domains lie in no simulated interval", f"written {p}_domains.tsv"]
    assert sim.calls[:3] == ["pixels", ("rescaled_pileup", 4), "pixels"]  # the cooler's, then the band's own columns
    assert sim.calls.count("pixels") == 2 and sim.calls.count("marginals") == 1  # extracted and summed once for the three blocks
    assert sim.calls.count(("rescaled_pileup", 1)) == 3 + 3  # the accepted windows, each alone, per block with windows
    start, end = [2, 2, 7, -2], [10, 10, 19, 6]
    pile, area, used = reference_rescale(band, nrows, ncols, r, start, end)
    assert used == 3
    hist = np.bincount([8, 8, 12], minlength=nrows + 1)
    diag_sum = reference_marginals(band, nrows, ncols, 0)[0]
    expected = restated_expected(hist, diag_sum, ncols, r)[0]
    strength = api.domain_strength(np.array(pile, dtype=object), expected, r, percent)
    assert strength > 0
    block = [driver.domains_header(tads, 5000, r, percent, 6, 4, 3, strength)] + \
        driver.domains_lines(r, sum(pile, []), sum(area, []), expected.reshape(-1).tolist())
    empty = [driver.domains_header(none, 5000, r, percent, 0, 0, 0, math.nan)] + driver.domains_lines(r, [0] * 16, [0] * 16, [0.0] * 16)
    got = open(p + "_domains.tsv").readlines()
    assert got == block + empty + block and len(got) == 3 * (1 + r * r)
    assert got[0].startswith(f"#source={tads}\tresolution=5000\tsize=4\tflank_percent=50\tgiven=6\tplaced=4\tused=3\tstrength=")
    assert got[1].split("\t")[:2] == ["0", "0"] and got[6].split("\t")[:2] == ["1", "1"] and len(got[1].split("\t")) == 5
    # without the record no such file is written, and another rank writes nothing
    (tmp_path / "plain").mkdir()
    q = str(tmp_path / "plain" / "p")
    driver.write_outputs(FakeSim(band, nrows, ncols, iid), cfg, plan, ids, None,
                         cli.Preflight(None, cli.Outputs(q + ".cool", None, None, None), 0, 1, 0), (), said.append, chroms=chroms)
    assert os.listdir(tmp_path / "plain") == ["p.cool"]
