"""Pileups without a GPU: the numpy / Python-int restatement of the definition in include/modle_pixels.h
(reference_pileup, reference_accepts: what tests/test_gpu_pileup.py holds the kernel to), the host-only
acceptance rule of the library against it, api.pileup_expected and api.apa_scores against their
restatements, and what `simulate --pileup-at` does around the kernel: the BEDPE reader and the placement
of its pairs, the lines of <prefix>_pileup.tsv byte for byte, the option checks and the refusals."""
import math
import os

import numpy as np
import pytest

I64_MIN, I64_MAX = -2**63, 2**63 - 1


def reference_accepts(nrows, ncols, f, bin1, bin2, bin_offset=0):
    """the rule in Python ints, which cannot overflow"""
    out = []
    for x, y in zip(bin1, bin2):
        a, b = int(x) - int(bin_offset), int(y) - int(bin_offset)
        out.append(a <= b and a >= f and b + f <= ncols - 1 and (b - a) + 2 * f <= nrows - 1)
    return np.array(out, dtype=bool)


def reference_pileup(band, nrows, ncols, f, a, b):
    """(pile as uint64 [S, S], n_used) of anchors that are already relative to the band: for every accepted
    anchor and every cell the word M(x, y) = band[max(x, y) * nrows + |x - y|].  An anchor listed k times
    enters as k times its word; the sums are formed in uint64, which is exact while they stay below 2^64
    (fewer than 2^31 words below 2^32)"""
    s = 2 * f + 1
    a, b = np.asarray(a, dtype=np.int64).reshape(-1), np.asarray(b, dtype=np.int64).reshape(-1)
    ok = reference_accepts(nrows, ncols, f, a, b)
    assert len(a) < 2**31
    pairs, times = np.unique(np.stack([a[ok], b[ok]], axis=1), axis=0, return_counts=True)
    aa, bb, times = pairs[:, 0], pairs[:, 1], times.astype(np.uint64)
    pile = np.zeros((s, s), dtype=np.uint64)
    for r in range(s):
        for c in range(s):
            x, y = aa - f + r, bb - f + c
            i, j = np.minimum(x, y), np.maximum(x, y)
            assert ((i >= 0) & (j < ncols) & (j - i < nrows)).all()
            pile[r, c] = (band[j * nrows + (j - i)].astype(np.uint64) * times).sum(dtype=np.uint64)
    return pile, int(ok.sum())


def edge_anchors(nrows, ncols, f):
    """(bin1, bin2) relative to the band: both sides of every edge of the rule, the int64 extremes, a > b"""
    dmax = nrows - 1 - 2 * f
    pairs = [(f, f), (f - 1, f), (f - 1, f - 1), (ncols - 1 - f, ncols - 1 - f), (ncols - 1 - f - dmax, ncols - 1 - f),
             (ncols - f - dmax, ncols - f), (ncols - f, ncols - f), (f, f + dmax), (f, f + dmax + 1), (f + 1, f),
             (f + dmax, f), (I64_MIN, I64_MIN), (I64_MAX, I64_MAX), (I64_MIN, I64_MAX), (I64_MAX, I64_MIN), (f, I64_MAX),
             (I64_MIN, f), (-1, f), (0, 0), (-f, f), (f, -f)]
    return np.array([p[0] for p in pairs], dtype=object), np.array([p[1] for p in pairs], dtype=object)


@pytest.mark.parametrize("nrows,ncols,f", [(1, 1, 0), (3, 3, 1), (7, 30, 1), (40, 65, 7), (65, 65, 32), (70, 300, 32),
                                           (200, 700, 10)])
def test_accepts_equal_the_rule_at_every_edge_and_for_any_int64(nrows, ncols, f):
    from modle_amd import pixels

    rng = np.random.default_rng([nrows, ncols, f])
    e1, e2 = edge_anchors(nrows, ncols, f)
    assert reference_accepts(nrows, ncols, f, e1[:1], e2[:1]).all()  # (f, f) fits every shape here
    for off in (0, 5, -7, I64_MAX, I64_MIN, 2**62, -2**62):
        b1, b2 = [], []
        for x, y in zip(e1, e2):  # the edges, shifted where the shift stays an int64, and raw
            for u, v in ((int(x) + off, int(y) + off), (int(x), int(y))):
                if I64_MIN <= u <= I64_MAX and I64_MIN <= v <= I64_MAX:
                    b1.append(u), b2.append(v)
        m = 300
        r1 = rng.integers(-3, ncols + 3, size=m)
        r2 = r1 + rng.integers(-2, nrows + 2, size=m)
        for u, v in zip(r1, r2):
            if I64_MIN <= int(u) + off <= I64_MAX and I64_MIN <= int(v) + off <= I64_MAX:
                b1.append(int(u) + off), b2.append(int(v) + off)
        b1, b2 = np.array(b1, dtype=np.int64), np.array(b2, dtype=np.int64)
        want = reference_accepts(nrows, ncols, f, b1, b2, off)
        got = pixels.pileup_accepts(nrows, ncols, f, b1, b2, off)
        assert got.dtype == bool and np.array_equal(got, want), off
        if off in (0, 5, -7):
            assert want.any() and not want.all()
    assert len(pixels.pileup_accepts(nrows, ncols, f, [], [])) == 0


def test_accepts_refuses_what_the_kernel_refuses():
    from modle_amd import pixels

    for args in [(0, 5, 0), (6, 5, 0), (70, 80, 33), (4, 9, 2), (9, 9, -1), (-1, 9, 0)]:
        with pytest.raises(pixels.PixelsError) as e:
            pixels.pileup_accepts(*args, [1], [2])
        assert e.value.code == pixels.ERR_ARG, args
    with pytest.raises(pixels.PixelsError):
        pixels.pileup_accepts(9, 9, 1, [1, 2], [2])


def test_reference_pileup_on_a_band_small_enough_to_do_by_hand():
    """nrows 3, ncols 4: M = [[1,2,3,0],[2,4,5,6],[3,5,7,8],[0,6,8,9]] (the (0, 3) pixel is outside the band)"""
    nrows, ncols = 3, 4
    band = np.zeros(nrows * ncols + 1, dtype=np.uint32)
    m = {(0, 0): 1, (0, 1): 2, (0, 2): 3, (1, 1): 4, (1, 2): 5, (1, 3): 6, (2, 2): 7, (2, 3): 8, (3, 3): 9}
    for (i, j), v in m.items():
        band[j * nrows + (j - i)] = v
    pile, used = reference_pileup(band, nrows, ncols, 1, [1, 2, 1, 0, 2], [1, 2, 2, 1, 1])
    assert used == 2  # (1, 1) and (2, 2); (1, 2) needs d + 2 <= 2
    assert pile.tolist() == [[1 + 4, 2 + 5, 3 + 6], [2 + 5, 4 + 7, 5 + 8], [3 + 6, 5 + 8, 7 + 9]]
    pile, used = reference_pileup(band, nrows, ncols, 0, [0, 1, 1, 3, 1], [2, 3, 3, 3, 0])
    assert used == 4 and pile.tolist() == [[3 + 6 + 6 + 9]]


def restated_expected(dist_hist, diag_sum, ncols, f):
    s = 2 * f + 1
    out = np.zeros((s, s), dtype=np.float64)
    for r in range(s):
        for c in range(s):
            terms = []
            for d in reversed(range(len(dist_hist))):  # (another order: fsum does not care)
                if int(dist_hist[d]) != 0:
                    k = abs(d + c - r)
                    terms.append(float(int(dist_hist[d])) * (float(int(diag_sum[k])) / float(ncols - k)))
            out[r, c] = math.fsum(terms)
    return out


def test_pileup_expected_equals_its_restatement_bit_for_bit():
    from modle_amd import api

    rng = np.random.default_rng(11)
    for nrows, ncols, f in ((40, 65, 7), (9, 9, 0), (70, 300, 32), (5, 8, 2)):
        diag = rng.integers(0, 2**40, size=nrows, dtype=np.int64).astype(np.uint64)
        hist = np.zeros(nrows, dtype=np.uint64)
        top = nrows - 2 * f
        hist[:top] = rng.integers(0, 4, size=top)
        hist[0] = 3
        got = api.pileup_expected(hist, diag, ncols, f)
        assert got.dtype == np.float64 and got.shape == (2 * f + 1, 2 * f + 1)
        assert np.array_equal(got.view(np.uint64), restated_expected(hist, diag, ncols, f).view(np.uint64))
        terms = api.pileup_expected_terms(hist, diag, ncols, f)
        assert len(terms) == (2 * f + 1) ** 2 and all(len(t) == np.count_nonzero(hist) for t in terms)
        assert not api.pileup_expected(np.zeros(nrows, dtype=np.uint64), diag, ncols, f).any()
    with pytest.raises(ValueError):
        api.pileup_expected([0, 0, 1], [1, 2, 3], 5, 1)  # distance 2 with a flank of 1 needs diagonal 4


def test_apa_scores_on_a_hand_made_pile():
    from modle_amd import api

    pile = np.zeros((7, 7), dtype=np.uint64)
    pile[3, 3] = 40
    pile[5:, :2] = [[1, 2], [3, 6]]   # lower-left: mean 3, variance (4 + 1 + 0 + 9) / 4 = 3.5
    pile[:2, :2] = 5                  # upper-left: mean 5
    pile[:2, 5:] = [[8, 0], [0, 0]]   # upper-right: mean 2
    got = api.apa_scores(pile, 2)     # lower-right: all zero
    assert set(got) == {"peak", "p2ll", "p2ul", "p2ur", "p2lr", "z_ll"} and all(type(v) is float for v in got.values())
    assert got["peak"] == 40.0 and got["p2ll"] == 40.0 / 3.0 and got["p2ul"] == 8.0 and got["p2ur"] == 20.0
    assert math.isnan(got["p2lr"])
    assert got["z_ll"] == (40.0 - 3.0) / math.sqrt(3.5)
    one = api.apa_scores(pile, 1)
    assert one["p2ll"] == 40.0 / 3.0 and one["p2ul"] == 8.0 and math.isnan(one["p2ur"]) and math.isnan(one["z_ll"])
    three = api.apa_scores(pile, 3)
    assert three["p2ll"] == 40.0 / (12.0 / 9.0) and three["p2ul"] == 40.0 / (20.0 / 9.0)
    for corner in (0, 4, -1):
        with pytest.raises(ValueError):
            api.apa_scores(pile, corner)
    with pytest.raises(ValueError):
        api.apa_scores(np.zeros((4, 4)), 1)
    with pytest.raises(ValueError):
        api.apa_scores(np.zeros((1, 1)), 1)  # f = 0 has no corner


# ---- the anchors of `simulate --pileup-at` ----------------------------------------------------------

def plan_entry(name, start, end, nrows, ncols, skipped=False, bar_pos=()):
    return {"interval": {"name": name, "size": end, "start": start, "end": end,
                         "bar_pos": np.array(bar_pos, dtype=np.uint64)},
            "nrows": nrows, "ncols": ncols, "tasks": None, "skipped": skipped}


BEDPE = ("#chrom1\tstart1\tend1\tchrom2\tstart2\tend2\tname\n"
         "chrA\t100000\t110001\tchrA\t200000\t205000\tfirst\t.\n"   # midpoints 105000 and 202500
         "\n"
         "chrA\t300000\t300010\tchrA\t120000\t120002\n"               # listed right side first: swapped
         "# a remark\n"
         "chrA\t100000\t110000\tchrB\t1000\t2000\n"                   # trans
         "chrC\t0\t10\tchrC\t20\t30\n"                                # a chromosome that is not simulated
         "chrA\t0\t10000\tchrA\t150000\t160000\n"                     # the left midpoint lies before the interval
         "chrA\t119999\t120000\tchrA\t599999\t600001\n"               # the right midpoint is the interval's end
         "chrA 500000 500001 chrA 599998 599999\n"                    # blanks instead of tabs
         "chrB\t0\t9999\tchrB\t5000\t5001\n"                          # chrB is skipped
         "chrD\t12000\t12001\tchrD\t49999\t50000\n")


def test_the_bedpe_reader_and_the_placement(tmp_path):
    from modle_amd import driver

    path = str(tmp_path / "loops.bedpe")
    with open(path, "w") as fh:
        fh.write(BEDPE)
    pairs = driver.read_bedpe(path)
    assert pairs == [("chrA", 105000, "chrA", 202500), ("chrA", 300005, "chrA", 120001), ("chrA", 105000, "chrB", 1500),
                     ("chrC", 5, "chrC", 25), ("chrA", 5000, "chrA", 155000), ("chrA", 119999, "chrA", 600000),
                     ("chrA", 500000, "chrA", 599998), ("chrB", 4999, "chrB", 5000), ("chrD", 12000, "chrD", 49999)]
    plan = [plan_entry("chrA", 15_000, 600_000, 40, 117), plan_entry("chrB", 0, 10_000, 2, 2, skipped=True),
            plan_entry("chrD", 0, 10_000, 2, 2), plan_entry("chrD", 10_000, 50_000, 8, 8)]
    placed, trans, outside = driver.place_pairs(plan, 5000, 5000, pairs)
    assert (trans, outside) == (1, 4) and sorted(placed) == [0, 3]
    assert placed[0][0].dtype == placed[0][1].dtype == np.int64
    assert placed[0][0].tolist() == [18, 21, 97] and placed[0][1].tolist() == [37, 57, 116]  # bins 21, 40, ... less 3
    assert placed[3][0].tolist() == [0] and placed[3][1].tolist() == [7]
    # at twice the bin size the interval starts in coarse bin 1 of its chromosome
    placed, trans, outside = driver.place_pairs(plan, 5000, 10_000, pairs)
    assert (trans, outside) == (1, 4)
    assert placed[0][0].tolist() == [9, 11, 49] and placed[0][1].tolist() == [19, 29, 58]
    assert driver.place_pairs(plan, 5000, 5000, []) == ({}, 0, 0)
    # what cannot be read
    for text, why in [("chrA\t1\t2\tchrA\t3\n", "line 1: fewer than six columns"),
                      ("#x\nchrA\t1\t2\tchrA\t3\tx\n", "line 2: invalid literal"),
                      ("chrA\t5\t2\tchrA\t3\t4\n", "line 1: a negative start or an end before its start"),
                      ("chrA\t-5\t2\tchrA\t3\t4\n", "line 1: a negative start")]:
        bad = str(tmp_path / "bad.bedpe")
        with open(bad, "w") as fh:
            fh.write(text)
        with pytest.raises(ValueError) as e:
            driver.read_bedpe(bad)
        assert str(e.value).startswith(f"{bad}, {why}"), text
    with pytest.raises(OSError):
        driver.read_bedpe(str(tmp_path / "missing.bedpe"))


def test_the_barriers_become_anchors_on_the_diagonal():
    from modle_amd import driver

    iv = plan_entry("chrA", 15_000, 600_000, 40, 117, bar_pos=[599_999, 15_000, 41_010, 44_999])["interval"]
    a, b = driver.barrier_anchors(iv, 5000, 5000)
    assert a.dtype == b.dtype == np.int64 and a.tolist() == b.tolist() == [0, 5, 5, 116]
    a, b = driver.barrier_anchors(iv, 5000, 10_000)
    assert a.tolist() == b.tolist() == [0, 3, 3, 58]


def test_a_flank_that_does_not_fit_and_a_file_that_cannot_be_read_are_named(tmp_path):
    from modle_amd import driver

    plan = [plan_entry("chrA", 0, 2_000_000, 40, 400), plan_entry("chrB", 0, 500_000, 8, 100, skipped=True),
            plan_entry("chrC", 25_000, 1_000_000, 39, 195)]
    assert driver.pileup_misfit(plan, 5000, 5000, 95_000) is None  # 2 * 19 + 1 = 39
    assert driver.pileup_misfit(plan, 5000, 5000, 100_000) == ("flank", "chrA:0-2000000", 100_000, 20, 40, 95_000)
    assert driver.pileup_misfit(plan[1:], 5000, 5000, 100_000) == ("flank", "chrC:25000-1000000", 100_000, 20, 39, 95_000)
    # at twice the bin size the band of 40 diagonals has 21
    assert driver.pileup_misfit(plan[:1], 5000, 10_000, 100_000) is None
    assert driver.pileup_misfit(plan[:1], 5000, 10_000, 110_000) == ("flank", "chrA:0-2000000", 110_000, 11, 21, 100_000)
    good, bad, missing = str(tmp_path / "good.bedpe"), str(tmp_path / "bad.bedpe"), str(tmp_path / "missing.bedpe")
    with open(good, "w") as fh:
        fh.write(BEDPE)
    with open(bad, "w") as fh:
        fh.write("chrA\t1\t2\n")
    assert driver.pileup_misfit(plan, 5000, 5000, 95_000, ["dots", good, "barriers"]) is None
    got = driver.pileup_misfit(plan, 5000, 5000, 100_000, ["dots", good, bad, missing])  # the file comes first
    assert got == ("bedpe", bad, f"{bad}, line 1: fewer than six columns")
    got = driver.pileup_misfit(plan, 5000, 5000, 95_000, [missing])
    assert got[:2] == ("bedpe", missing) and "No such file" in got[2]


# ---- the file ---------------------------------------------------------------------------------------

SCORES = {"peak": 40.0, "p2ll": 40.0 / 3.0, "p2ul": 8.0, "p2ur": 20.0, "p2lr": math.nan, "z_ll": 0.1}


def test_the_header_and_the_rows_of_a_block():
    from modle_amd import driver

    assert driver.pileup_header("barriers", 5000, 15_000, 5000, 41, 40, 38, SCORES) == (
        "#source=barriers\tresolution=5000\tflank=15000\tcorner=5000\tgiven=41\tplaced=40\tused=38"
        f"\tpeak=40.0\tp2ll={40.0 / 3.0!r}\tp2ul=8.0\tp2ur=20.0\tp2lr=nan\tz_ll=0.1\n")
    lines = driver.pileup_lines("a b.bedpe", 10_000, 10_000, [2**64 + 1, 0, 3, 4, 5, 6, 7, 8, 9],
                                [0.1, 0.0, 1e300, 4.5, 5.0, 6.0, 7.0, 8.0, 1 / 3])
    assert lines == ["a b.bedpe\t-10000\t-10000\t18446744073709551617\t0.1\n", "a b.bedpe\t-10000\t0\t0\t0.0\n",
                     "a b.bedpe\t-10000\t10000\t3\t1e+300\n", "a b.bedpe\t0\t-10000\t4\t4.5\n", "a b.bedpe\t0\t0\t5\t5.0\n",
                     "a b.bedpe\t0\t10000\t6\t6.0\n", "a b.bedpe\t10000\t-10000\t7\t7.0\n", "a b.bedpe\t10000\t0\t8\t8.0\n",
                     f"a b.bedpe\t10000\t10000\t9\t{1 / 3!r}\n"]


def test_the_file_sums_the_intervals_and_keeps_the_order_of_the_sources(tmp_path):
    from modle_amd import api, driver

    plan = [plan_entry("chrA", 10_000, 123_000, 30, 23), plan_entry("chrA", 130_000, 150_000, 3, 4, skipped=True),
            plan_entry("chrB", 0, 10_000, 2, 2), plan_entry("chrC", 0, 100_000, 20, 20)]
    piles = {0: np.arange(9, dtype=np.uint64).reshape(3, 3) + 2**63, 3: np.arange(9, dtype=np.uint64).reshape(3, 3) + 2**63}
    terms = {0: [[0.1, 0.2]] * 9, 3: [[0.3, 1e-20, 1e20, -1e20]] * 9}
    calls = []

    def anchors(name, k, factor, first_bin):
        calls.append(("anchors", name, k, factor, first_bin))
        if k == 2:
            return None
        return (np.arange(k + 2), np.arange(k + 2)) if name != "x.bedpe" else (np.zeros(0, np.int64), np.zeros(0, np.int64))

    def pileup(name, k, factor, first_bin, a, b):
        calls.append(("pileup", name, k, factor, first_bin, len(a)))
        if name == "x.bedpe":
            return np.zeros((3, 3), dtype=np.uint64), 0, [[] for _ in range(9)]
        return piles[k], k + 1, terms[k]

    path = str(tmp_path / "p.tsv")
    done = driver.write_pileup(path, plan, 5000, 10_000, 10_000, 10_000, ["barriers", "x.bedpe"], anchors, pileup,
                               {"x.bedpe": 4})
    assert done == [("barriers", 7, 7, 5), ("x.bedpe", 4, 0, 0)]
    assert calls == [("anchors", "barriers", 0, 2, 2), ("pileup", "barriers", 0, 2, 2, 2),
                     ("anchors", "barriers", 2, 2, 0),
                     ("anchors", "barriers", 3, 2, 0), ("pileup", "barriers", 3, 2, 0, 5),
                     ("anchors", "x.bedpe", 0, 2, 2), ("pileup", "x.bedpe", 0, 2, 2, 0),
                     ("anchors", "x.bedpe", 2, 2, 0),
                     ("anchors", "x.bedpe", 3, 2, 0), ("pileup", "x.bedpe", 3, 2, 0, 0)]
    observed = [2 * (2**63 + q) for q in range(9)]  # beyond 64 bits: summed in Python ints
    expected = [math.fsum([0.1, 0.2, 0.3, 1e-20, 1e20, -1e20])] * 9
    assert expected[0] != 0.1 + 0.2 + 0.3 + 1e-20 + 1e20 - 1e20
    scores = api.apa_scores(np.array(observed, dtype=np.float64).reshape(3, 3), 1)
    zero = api.apa_scores(np.zeros((3, 3)), 1)
    assert zero["peak"] == 0.0 and all(math.isnan(zero[k]) for k in zero if k != "peak")
    assert open(path).readlines() == (
        [driver.pileup_header("barriers", 10_000, 10_000, 10_000, 7, 7, 5, scores)]
        + driver.pileup_lines("barriers", 10_000, 10_000, observed, expected)
        + [driver.pileup_header("x.bedpe", 10_000, 10_000, 10_000, 4, 0, 0, zero)]
        + driver.pileup_lines("x.bedpe", 10_000, 10_000, [0] * 9, [0.0] * 9))


def test_a_pile_is_checked_before_a_row_is_written():
    from modle_amd import driver

    pile = np.array([[1, 2, 3], [4, 50, 6], [7, 8, 9]], dtype=np.uint64)
    driver.check_pileup("chrA:0-100", "barriers", 1, pile, 2, [2, 0, 0], 25, centre=50)
    driver.check_pileup("chrA:0-100", "dots", 1, pile, 2, [0, 1, 1], 5)  # 90 <= 2 * 9 * 5
    driver.check_pileup("chrA:0-100", "dots", 1, np.zeros((3, 3)), 0, [0, 0, 0], 0)
    for what, args, kw, message in [
            ("the count", (1, pile, 3, [2, 0, 0], 25), {}, "used 3 anchors, their distances count 2"),
            ("the bound", (1, pile, 2, [0, 2, 0], 4), {}, "sums to 90, above 2 windows of 9 pixels of at most 4"),
            ("the centre", (1, pile, 2, [2, 0, 0], 25), {"centre": 49}, "the centre of the pileup at barriers is 50"),
            ("the shape", (2, pile, 2, [2, 0, 0], 25), {}, "has 9 cells, not 5 x 5")]:
        with pytest.raises(RuntimeError) as e:
            driver.check_pileup("chrA:0-100", "barriers", *args, **kw)
        assert str(e.value).startswith("chrA:0-100: ") and message in str(e.value), what


class FakeSim:
    """what _interval_pileup asks of a simulator: the pileup and the pixels of one band"""

    def __init__(self, band, nrows, ncols):
        self.band, self.nrows, self.ncols, self.calls = band, nrows, ncols, []

    def pileup(self, interval_id, bin1, bin2, flank, factor=1, first_bin=0, bin_offset=0):
        self.calls.append(("pileup", interval_id, flank, factor, first_bin))
        pile, used = reference_pileup(self.band, self.nrows, self.ncols, flank, bin1, bin2)
        ok = reference_accepts(self.nrows, self.ncols, flank, bin1, bin2)
        d = (np.asarray(bin2) - np.asarray(bin1))[ok]
        return pile, used, np.bincount(d, minlength=self.nrows).astype(np.uint64)

    def pixels(self, interval_id, bin_offset=0, stream=None, factor=1, first_bin=0):
        from modle_amd import pixels

        self.calls.append(("pixels", interval_id, factor, first_bin))
        j, d = np.divmod(np.arange(self.nrows * self.ncols), self.nrows)
        keep = (d <= j) & (self.band[:-1] != 0)
        order = np.lexsort((j[keep], (j - d)[keep]))
        b1, b2, cnt = (j - d)[keep][order], j[keep][order], self.band[:-1][keep][order].astype(np.int32)
        return pixels.Pixels(b1, b2, cnt, None, pixels.Stats(len(cnt), int(cnt.sum()), int(cnt.max())))


def test_the_output_stage_checks_the_pile_against_the_pixels():
    from modle_amd import api, driver
    from test_gpu_marginals import make_band, reference_marginals

    nrows, ncols, f = 12, 30, 2
    band = make_band(nrows, ncols, "full", limit=1000, seed=2)
    sim = FakeSim(band, nrows, ncols)
    plan = [plan_entry("chrA", 0, 150_000, nrows, ncols), plan_entry("chrB", 0, 1, 1, 1, skipped=True)]
    diag_sum = reference_marginals(band, nrows, ncols, 0)[0]
    cache = {}
    call = lambda name, k, a, b: driver._interval_pileup(sim, plan, [7, None], lambda k, factor, first_bin: (diag_sum, None),
                                                         cache, f, name, k, 1, 0, np.array(a), np.array(b))
    a, b = [2, 5, 5, 1, 27, 28], [2, 5, 5, 1, 27, 28]
    pile, used, terms = call("barriers", 0, a, b)
    want, n = reference_pileup(band, nrows, ncols, f, a, b)
    assert used == n == 4 and np.array_equal(pile, want)
    hist = np.zeros(nrows, dtype=np.uint64)
    hist[0] = 4
    assert terms == api.pileup_expected_terms(hist, diag_sum, ncols, f)
    pile, used, terms = call("dots", 0, [3, 4], [9, 12])  # d = 6 and 8: 8 + 4 > 11
    assert used == 1 and sim.calls == [("pileup", 7, f, 1, 0), ("pixels", 7, 1, 0), ("pileup", 7, f, 1, 0)]  # extracted once
    assert call("barriers", 1, a, b) is None
    # a pile that does not hold what the pixels hold is refused
    sim.band = band.copy()
    sim.band[5 * nrows] += 1  # pixel (5, 5)
    with pytest.raises(RuntimeError) as e:
        call("barriers", 0, a, b)
    assert "the centre of the pileup at barriers" in str(e.value)
    call("dots", 0, a, b)  # (not tied to the diagonal)


# ---- the options and preflight ----------------------------------------------------------------------

@pytest.fixture
def prefix(tmp_path, monkeypatch):
    for name in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(name, raising=False)
    return str(tmp_path / "out" / "p")


def run_preflight(prefix, *extra):
    from modle_amd import cli

    a = cli.build_parser().parse_args(["simulate", "-c", "g.chrom.sizes", "-b", "b.bed", "-o", prefix, "-r", "5kb", *extra])
    return cli.preflight(a, cli.config_from_args(a))


def test_the_options_parse_and_preflight_plans_the_file(prefix):
    from modle_amd import cli

    pre = run_preflight(prefix, "--no-track-1d-lef-position")
    assert pre.pileup is None and pre.dots is None
    assert pre.outputs == cli.Outputs(prefix + ".cool", None, None, None)  # as before
    assert cli.Preflight([5000], pre.outputs, 0, 1, 0).pileup is None  # the fields of before still make one
    assert cli.Preflight([5000], pre.outputs, 0, 1, 0, None, None).pileup is None
    assert cli.Preflight._fields[:8] == ("bin_sizes", "outputs", "rank", "world", "device", "insulation", "dots", "pileup")
    pre = run_preflight(prefix, "--pileup-at", "barriers")
    assert pre.pileup == cli.Pileup(prefix + "_pileup.tsv", 5000, 50_000, 15_000, ["barriers"])
    assert cli.pileup_path(prefix) == prefix + "_pileup.tsv"
    pre = run_preflight(prefix, "--dots", "--dots-resolution", "10kb", "--pileup-at", "x/loops.bedpe", "--pileup-at", "dots",
                        "--pileup-at", "barriers", "--pileup-at", "dots", "--pileup-resolution", "10kb", "--pileup-flank",
                        "20kb", "--pileup-corner", "20kb")
    assert pre.pileup == cli.Pileup(prefix + "_pileup.tsv", 10_000, 20_000, 20_000, ["x/loops.bedpe", "dots", "barriers", "dots"])
    assert run_preflight(prefix, "--pileup-at", "barriers", "--pileup-flank", "160kb").pileup.corner == 50_000  # the cap
    assert run_preflight(prefix, "--pileup-at", "barriers", "--pileup-flank", "5kb").pileup.corner == 5000
    assert run_preflight(prefix, "--pileup-at", "barriers", "--pileup-resolution", "25kb").pileup.flank == 250_000
    pre = run_preflight(prefix, "--pileup-at", "barriers", "--skip-output")
    assert pre.pileup.path is None and pre.pileup.sources == ["barriers"]
    assert not os.path.exists(prefix + "_pileup.tsv")


REFUSED = [
    (["--pileup-flank", "25kb"], "--pileup-flank needs --pileup-at"),
    (["--pileup-resolution", "10kb"], "--pileup-resolution needs --pileup-at"),
    (["--pileup-corner", "10kb", "--skip-output"], "--pileup-corner needs --pileup-at"),
    (["--pileup-at", "dots"], "--pileup-at dots needs --dots"),
    (["--pileup-at", "barriers", "--pileup-at", "dots", "--pileup-flank", "25kb"], "--pileup-at dots needs --dots"),
    (["--dots", "--dots-resolution", "10kb", "--pileup-at", "dots"],
     "--pileup-at dots: the pileup resolution (5000) is not the dots resolution (10000)"),
    (["--dots", "--pileup-at", "dots", "--pileup-resolution", "10kb"],
     "--pileup-at dots: the pileup resolution (10000) is not the dots resolution (5000)"),
    (["--pileup-at", "barriers", "--pileup-flank", "165kb"], "--pileup-flank: 165000 is 33 bins of 5000: at most 32"),
    (["--pileup-at", "barriers", "--pileup-flank", "12000"], "--pileup-flank: 12000 is not a positive multiple"),
    (["--pileup-at", "barriers", "--pileup-flank", "0"], "--pileup-flank: 0 is not a positive multiple"),
    (["--pileup-at", "barriers", "--pileup-resolution", "10kb", "--pileup-flank", "25kb"],
     "--pileup-flank: 25000 is not a positive multiple of the pileup resolution (10000)"),
    (["--pileup-at", "barriers", "--pileup-resolution", "12500"], "--pileup-resolution: 12500 is not a multiple"),
    (["--pileup-at", "barriers", "--pileup-resolution", "1kb"], "--pileup-resolution: 1000 is not a multiple"),
    (["--pileup-at", "barriers", "--pileup-corner", "7000"], "--pileup-corner: 7000 is not a positive multiple"),
    (["--pileup-at", "barriers", "--pileup-corner", "0"], "--pileup-corner: 0 is not a positive multiple"),
    (["--pileup-at", "barriers", "--pileup-flank", "10kb", "--pileup-corner", "15kb"],
     "--pileup-corner: 15000 is above the flank (10000)"),
]


@pytest.mark.parametrize("options,message", REFUSED)
def test_preflight_refuses_before_anything_is_made(prefix, options, message):
    with pytest.raises(SystemExit) as e:
        run_preflight(prefix, *options)
    assert str(e.value).startswith(message)
    assert not os.path.exists(os.path.dirname(prefix))


def test_the_pileup_file_is_the_last_that_is_refused_to_be_overwritten(prefix):
    everything = ["--track-1d-lef-position", "--expected", "--insulation-windows", "100kb", "--dots", "--pileup-at", "dots"]
    os.makedirs(os.path.dirname(prefix))
    for which in ("_pileup.tsv", "_dots.bedpe"):  # each one is named before the one before it
        with open(prefix + which, "wb") as fh:
            fh.write(b"precious")
        with pytest.raises(SystemExit) as e:
            run_preflight(prefix, *everything)
        assert str(e.value) == f"refusing to overwrite {prefix + which}: pass --force to overwrite"
    assert run_preflight(prefix, *everything, "--force").pileup.path == prefix + "_pileup.tsv"
    assert run_preflight(prefix, *everything, "--skip-output").pileup.path is None
    os.remove(prefix + "_dots.bedpe")
    assert run_preflight(prefix, "--no-track-1d-lef-position").pileup is None  # without the option: nobody's business
    assert open(prefix + "_pileup.tsv", "rb").read() == b"precious"


def test_the_plan_refuses_a_flank_and_a_file_before_anything_is_simulated(tmp_path, prefix):
    """plan_run's messages, on a genome of one chromosome: -w 200kb at 5 kb is a band of 40 diagonals"""
    from modle_amd import cli

    sizes, bed = str(tmp_path / "g.chrom.sizes"), str(tmp_path / "b.bed")
    with open(sizes, "w") as fh:
        fh.write("chrA\t2000000\n")
    with open(bed, "w") as fh:
        fh.write("chrA\t41000\t41019\t.\t0.8\t+\nchrA\t141000\t141019\t.\t0.8\t-\n")

    def plan(*extra):
        a = cli.build_parser().parse_args(["simulate", "-c", sizes, "-b", bed, "-o", prefix, "-r", "5kb", "-w", "200kb",
                                           *extra])
        cfg = cli.config_from_args(a)
        return cli.plan_run(a, cfg, cli.preflight(a, cfg), lambda *x: None)

    assert len(plan("--pileup-at", "barriers", "--pileup-flank", "95kb")[1]) == 1
    with pytest.raises(SystemExit) as e:
        plan("--pileup-at", "barriers", "--pileup-flank", "100kb")
    assert str(e.value) == ("--pileup-flank: the flank of 100000 (20 bins of 5000) does not fit the band of "
                            "chrA:0-2000000 (40 diagonals): the largest flank that fits is 95000 (19 bins)")
    missing = str(tmp_path / "missing.bedpe")
    with pytest.raises(SystemExit) as e:
        plan("--pileup-at", "barriers", "--pileup-at", missing)
    assert str(e.value).startswith(f"--pileup-at {missing}: the file cannot be read as BEDPE: ") and "No such file" in str(e.value)
    assert len(plan("--pileup-at", missing, "--pileup-flank", "100kb", "--skip-output")[1]) == 1  # nothing is written: not looked at
