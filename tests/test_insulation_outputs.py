"""`simulate --insulation-windows` without a GPU: the numpy restatement of the insulation sums that the
GPU tests compare against (the brute-force definition and the per-column prefix form, which must agree),
the host-only number of pixels of a diamond (modle_pixels_insulation_n_valid), the identity that ties the
sums to the diagonal sums (driver.check_insulation), the float rule (api.insulation_score), the options and
what cli.preflight and driver.insulation_misfit refuse for them, and the lines of <prefix>_insulation.tsv."""
import math
import os

import numpy as np
import pytest

from modle_amd import api, cli, driver
from test_gpu_marginals import POISON, make_band, reference_marginals


# ---- the restatement ----------------------------------------------------------------------------

def brute_insulation(band, nrows, ncols, w, min_diag):
    """the definition: for bin b the pixels (a, c), b - w + 1 <= a <= b <= c <= b + w - 1, a >= 0,
    c < ncols, c - a >= min_diag; (ins_sum, n_valid) as lists of ints"""
    assert 2 * w - 1 <= nrows
    sums, counts = [], []
    for b in range(ncols):
        s = n = 0
        for a in range(max(0, b - w + 1), b + 1):
            for c in range(b, min(ncols, b + w)):
                if c - a >= min_diag:
                    s += int(band[c * nrows + (c - a)])
                    n += 1
        sums.append(s)
        counts.append(n)
    return sums, counts


def prefix_insulation(band, nrows, ncols, windows, min_diag):
    """the per-column form: column j = b + t, 0 <= t < w, gives bin b the words d in [max(t, min_diag),
    min(t + w - 1, j)] = P_j[min(t + w - 1, j) + 1] - P_j[max(t, min_diag)] with the exclusive prefix sums
    P_j of the column's pixel words; uint64 [len(windows), ncols]"""
    out = np.zeros((len(windows), ncols), dtype=np.uint64)
    for j in range(ncols):
        depth = min(j, nrows - 1) + 1  # the pixel words of column j
        prefix = np.zeros(depth + 1, dtype=np.uint64)
        np.cumsum(band[j * nrows:j * nrows + depth], dtype=np.uint64, out=prefix[1:])
        for k, w in enumerate(windows):
            assert 2 * w - 1 <= nrows
            t = np.arange(0, min(w, j + 1), dtype=np.int64)
            lo, hi = np.maximum(t, min_diag), np.minimum(t + w - 1, j)
            keep = lo <= hi
            out[k, j - t[keep]] += prefix[hi[keep] + 1] - prefix[lo[keep]]
    return out


def brute_n_valid(ncols, w, min_diag):
    return [sum(1 for a in range(max(0, b - w + 1), b + 1) for c in range(b, min(ncols, b + w)) if c - a >= min_diag)
            for b in range(ncols)]


def identity_rhs(diag_sum, w, min_diag):
    """sum over d = min_diag .. 2w - 2 of min(d + 1, 2w - 1 - d) * diag_sum[d]"""
    return sum(min(d + 1, 2 * w - 1 - d) * int(diag_sum[d]) for d in range(min_diag, 2 * w - 1))


# (nrows, ncols, windows): a band one word wide, all triangle, windows that fill the band exactly, odd sizes
SMALL = [(1, 1, [1]), (1, 7, [1]), (5, 5, [1, 2, 3]), (5, 9, [2, 3]), (3, 4, [2, 1]), (9, 9, [5, 1]), (9, 30, [5, 2, 4]),
         (11, 17, [6, 3])]


@pytest.mark.parametrize("nrows,ncols,windows", SMALL)
def test_the_brute_force_definition_and_the_prefix_form_agree(nrows, ncols, windows):
    for fill in ("tenth", "full"):
        band = make_band(nrows, ncols, fill)  # the words that are no pixels hold POISON
        assert band[nrows * ncols] == POISON
        wmax = max(windows)
        for m in (0, 1, 2, 2 * wmax - 1, 2 * wmax + 3):
            got = prefix_insulation(band, nrows, ncols, windows, m)
            assert got.dtype == np.uint64 and got.shape == (len(windows), ncols)
            for k, w in enumerate(windows):
                sums, counts = brute_insulation(band, nrows, ncols, w, m)
                assert got[k].tolist() == sums, (fill, m, w)
                assert counts == brute_n_valid(ncols, w, m)
                if m >= 2 * w - 1:
                    assert not any(sums) and not any(counts)
        # a poisoned word would show: every sum is below what the pixels alone can give
        pixels_total = int(reference_marginals(band, nrows, ncols, 0)[0].sum())
        assert int(prefix_insulation(band, nrows, ncols, [1], 0).sum()) == int(reference_marginals(band, nrows, ncols, 0)[0][0])
        assert all(int(x) <= pixels_total for x in prefix_insulation(band, nrows, ncols, windows, 0).ravel())


@pytest.mark.parametrize("ncols", [1, 2, 7, 30])
@pytest.mark.parametrize("w", [1, 2, 5])
def test_n_valid_is_the_number_of_pixels_of_the_diamond(ncols, w):
    from modle_amd import pixels

    for m in (0, 1, 2, 2 * w - 1, 2 * w + 3):
        got = pixels.insulation_n_valid(ncols, w, m)
        assert got.dtype == np.uint64 and got.tolist() == brute_n_valid(ncols, w, m), (ncols, w, m)
    if ncols >= 2 * w - 1:  # a bin in the middle sees the whole diamond
        assert int(pixels.insulation_n_valid(ncols, w, 0)[w - 1]) == w * w
    assert pixels.insulation_n_valid(0, w).shape == (0,)


def test_n_valid_refuses_a_window_that_is_no_window():
    from modle_amd import pixels

    for window in (0, 1025, -1):
        with pytest.raises(pixels.PixelsError) as e:
            pixels.insulation_n_valid(9, window, 2)
        assert e.value.code == pixels.ERR_ARG
    assert int(pixels.insulation_n_valid(3000, 1024, 0)[1500]) == 1024 * 1024


@pytest.mark.parametrize("nrows,ncols,windows", SMALL)
def test_the_sums_add_up_to_the_weighted_diagonal_sums(nrows, ncols, windows):
    band = make_band(nrows, ncols, "full", seed=1)
    diag_sum = reference_marginals(band, nrows, ncols, 0)[0]
    for m in (0, 1, 2, 2 * max(windows) - 1, 2 * max(windows) + 3):
        ins = prefix_insulation(band, nrows, ncols, windows, m)
        for k, w in enumerate(windows):
            assert sum(int(x) for x in ins[k]) == identity_rhs(diag_sum, w, m), (m, w)
        driver.check_insulation("chrA:0-5000", windows, m, ins, diag_sum)
    ins = prefix_insulation(band, nrows, ncols, windows, 0)
    for k in range(len(windows)):
        doctored = ins.copy()
        doctored[k, ncols // 2] += np.uint64(1)  # one word changed
        with pytest.raises(RuntimeError) as e:
            driver.check_insulation("chrA:0-5000", windows, 0, doctored, diag_sum)
        assert "chrA:0-5000" in str(e.value) and f"window of {windows[k]} bins" in str(e.value)
    with pytest.raises(RuntimeError) as e:  # the sums of another number of diagonals
        driver.check_insulation("chrA:0-5000", windows, 1, ins, diag_sum)
    assert "chrA:0-5000" in str(e.value) or not int(diag_sum[0])


# ---- the score ----------------------------------------------------------------------------------

def test_the_score_is_the_log2_of_the_mean_over_the_median_of_the_valid_bins():
    #          a bin without pixels; a zero sum; means 2, 8, 4 and 32
    ins_sum = np.array([[7, 0, 8, 16, 4, 64]], dtype=np.uint64)
    n_valid = np.array([[0, 3, 4, 2, 1, 2]], dtype=np.uint64)
    got = api.insulation_score(ins_sum, n_valid)
    assert got.dtype == np.float64 and got.shape == (1, 6)
    # the median is over the five bins with n_valid > 0, the zero mean included: of 0, 2, 8, 4, 32 it is 4
    assert math.isnan(got[0, 0]) and math.isnan(got[0, 1])
    assert got[0, 2:].tolist() == [-1.0, 1.0, 0.0, 3.0]
    # (were the bin without pixels counted with its sum, or the median taken over all six, it would differ)
    assert api.insulation_score(ins_sum[0], n_valid[0]).tolist()[2:] == [-1.0, 1.0, 0.0, 3.0]
    # a value that is no power of two
    got = api.insulation_score(np.array([3, 5, 10], dtype=np.uint64), np.array([1, 1, 1], dtype=np.uint64))
    assert got.tolist() == [pytest.approx(math.log2(3 / 5), rel=1e-15), 0.0, 1.0]
    # a zero median: every bin is nan
    got = api.insulation_score(np.array([[0, 0, 9], [1, 2, 3]], dtype=np.uint64), np.array([[1, 1, 1], [1, 1, 1]], dtype=np.uint64))
    assert np.isnan(got[0]).all() and got[1].tolist() == [-1.0, 0.0, pytest.approx(math.log2(1.5), rel=1e-15)]  # every window its own median
    # no valid bin at all
    assert np.isnan(api.insulation_score(np.array([5, 5], dtype=np.uint64), np.array([0, 0], dtype=np.uint64))).all()
    # sums beyond 2^53 keep their quotient
    big = api.insulation_score(np.array([2**60, 2**61], dtype=np.uint64), np.array([2, 2], dtype=np.uint64))
    assert big.tolist() == [pytest.approx(math.log2(1 / 1.5), rel=1e-15), pytest.approx(math.log2(2 / 1.5), rel=1e-15)]
    with pytest.raises(ValueError):
        api.insulation_score(np.zeros(3, dtype=np.uint64), np.zeros(4, dtype=np.uint64))


# ---- the options and preflight ------------------------------------------------------------------

SUFFIXES = {"cool": ".cool", "bw": "_lef_1d_occupancy.bw", "npz": "_dense.npz", "expected": "_expected.tsv",
            "bedgraph": "_coverage.bedgraph", "insulation": "_insulation.tsv"}
WINDOWS = ["--insulation-windows", "100kb,250kb"]


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


def test_the_options_parse_and_are_absent_by_default(prefix):
    a = parse(prefix)
    assert (a.insulation_windows, a.insulation_resolution, a.insulation_ignore_diags) == (None, None, None)
    a = parse(prefix, "--insulation-windows", "100kb, 1.5mb,20000", "--insulation-resolution", "10kb",
              "--insulation-ignore-diags", "3")
    assert (a.insulation_windows, a.insulation_resolution, a.insulation_ignore_diags) == ([100_000, 1_500_000, 20_000],
                                                                                         10_000, 3)
    assert cli.window_list("5kb") == [5000]
    assert len(cli.window_list(",".join(["5kb"] * 8))) == 8
    for bad in ("", "5kb,,10kb", "5kb,", "five", ",".join(["5kb"] * 9)):
        with pytest.raises(Exception) as e:
            cli.window_list(bad)
        assert e.type.__name__ == "ArgumentTypeError", bad
    with pytest.raises(SystemExit):
        parse(prefix, "--insulation-windows", ",".join(["5kb"] * 9))
    with pytest.raises(SystemExit):
        parse(prefix, *WINDOWS, "--insulation-ignore-diags", "two")


def test_preflight_plans_the_file_and_nothing_else_changes(prefix):
    pre = run_preflight(prefix, "--track-1d-lef-position")
    assert pre.insulation is None
    assert pre.outputs == cli.Outputs(prefix + ".cool", prefix + "_lef_1d_occupancy.bw", None, None)  # as before
    assert cli.Preflight([5000], pre.outputs, 0, 1, 0).insulation is None  # the five fields of before still make one
    pre = run_preflight(prefix, "--no-track-1d-lef-position", *WINDOWS)
    assert pre.outputs == cli.Outputs(prefix + ".cool", None, None, None)
    assert pre.insulation == cli.Insulation(prefix + "_insulation.tsv", 5000, [100_000, 250_000], 2)  # cooltools' default
    pre = run_preflight(prefix, *WINDOWS, "--insulation-resolution", "50kb", "--insulation-ignore-diags", "0")
    assert pre.insulation == cli.Insulation(prefix + "_insulation.tsv", 50_000, [100_000, 250_000], 0)
    assert cli.insulation_path(prefix) == prefix + "_insulation.tsv"
    # the cap of 1024 bins is reached, not passed
    assert run_preflight(prefix, "--insulation-windows", "5120kb").insulation.windows == [5_120_000]
    pre = run_preflight(prefix, *WINDOWS, "--skip-output")
    assert pre.insulation.path is None and pre.outputs == cli.Outputs(None, None, None, None)
    assert not os.path.exists(prefix + "_insulation.tsv")


REFUSED = [
    (["--insulation-resolution", "10kb"], "--insulation-resolution needs --insulation-windows"),
    (["--insulation-ignore-diags", "2"], "--insulation-ignore-diags needs --insulation-windows"),
    (["--insulation-ignore-diags", "0", "--skip-output"], "--insulation-ignore-diags needs --insulation-windows"),
    (WINDOWS + ["--insulation-ignore-diags", "-1"], "--insulation-ignore-diags: -1 is negative"),
    (["--insulation-windows", "100kb,0"], "--insulation-windows: 0 is not a positive multiple"),
    (["--insulation-windows", "100kb,12000"], "--insulation-windows: 12000 is not a positive multiple"),
    (WINDOWS + ["--insulation-resolution", "20kb"], "--insulation-windows: 250000 is not a positive multiple"),
    (["--insulation-windows", "5125kb"], "--insulation-windows: 5125000 is 1025 bins"),
    (WINDOWS + ["--insulation-resolution", "12500"], "--insulation-resolution: 12500 is not a multiple"),
    (WINDOWS + ["--insulation-resolution", "1kb"], "--insulation-resolution: 1000 is not a multiple"),
]


@pytest.mark.parametrize("options,message", REFUSED)
def test_preflight_refuses_before_anything_is_made(prefix, options, message):
    with pytest.raises(SystemExit) as e:
        run_preflight(prefix, *options)
    assert str(e.value).startswith(message)
    assert not os.path.exists(os.path.dirname(prefix))


def test_the_insulation_file_is_the_last_that_is_refused_to_be_overwritten(prefix):
    everything = ["--track-1d-lef-position", "--dense-region", "chrA", "--expected", "--coverage", *WINDOWS]
    os.makedirs(os.path.dirname(prefix))
    order = ["insulation", "bedgraph", "expected", "npz", "bw", "cool"]  # each one is named before those to its left
    for n, which in enumerate(order):
        with open(prefix + SUFFIXES[which], "wb") as fh:
            fh.write(b"precious")
        with pytest.raises(SystemExit) as e:
            run_preflight(prefix, *everything)
        assert str(e.value) == f"refusing to overwrite {prefix + SUFFIXES[which]}: pass --force to overwrite", n
    assert run_preflight(prefix, *everything, "--force").insulation.path == prefix + "_insulation.tsv"
    assert run_preflight(prefix, *everything, "--skip-output").insulation.path is None
    for which in order:  # without the option the file is nobody's business
        if which != "insulation":
            os.remove(prefix + SUFFIXES[which])
    assert run_preflight(prefix, "--no-track-1d-lef-position").insulation is None
    assert open(prefix + "_insulation.tsv", "rb").read() == b"precious"


# ---- what the plan refuses ----------------------------------------------------------------------

def entry(name, start, end, nrows, ncols, skipped=False):
    return {"interval": {"name": name, "size": end, "start": start, "end": end}, "nrows": nrows, "ncols": ncols,
            "tasks": None, "skipped": skipped}


def test_the_coarse_shape_is_the_library_s():
    from modle_amd import pixels

    for nrows, ncols, first_bin, k in [(80, 200, 5, 3), (600, 700, 7, 25), (5, 9, 0, 2), (40, 400, 0, 2), (1, 1, 3, 4)]:
        assert driver.insulation_shape(nrows, ncols, first_bin, k) == pixels.coarse_shape(nrows, ncols, k, first_bin)
    assert driver.insulation_shape(80, 200, 5, 1) == (80, 200)


def test_a_window_whose_diamond_leaves_the_band_is_named_with_the_largest_that_fits():
    plan = [entry("chrA", 0, 2_000_000, 40, 400), entry("chrB", 0, 500_000, 40, 100, skipped=True),
            entry("chrC", 25_000, 1_000_000, 39, 195)]
    assert driver.insulation_misfit(plan, 5000, 5000, [100_000, 5000]) is None  # 2 * 20 - 1 = 39 diagonals
    assert driver.insulation_misfit(plan, 5000, 5000, [5000, 105_000]) == ("chrA:0-2000000", 105_000, 21, 40, 100_000)
    plan[0]["nrows"] = 41
    assert driver.insulation_misfit(plan, 5000, 5000, [105_000]) == ("chrC:25000-1000000", 105_000, 21, 39, 100_000)
    # at twice the bin size the band of 40 diagonals has 21: windows up to 11 coarse bins fit
    plan = [entry("chrA", 0, 2_000_000, 40, 400)]
    assert driver.insulation_shape(40, 400, 0, 2) == (21, 200)
    assert driver.insulation_misfit(plan, 5000, 10_000, [110_000]) is None
    assert driver.insulation_misfit(plan, 5000, 10_000, [120_000]) == ("chrA:0-2000000", 120_000, 12, 21, 110_000)
    # a skipped entry has no matrix: nothing is asked of it
    assert driver.insulation_misfit([entry("chrB", 0, 500_000, 3, 100, skipped=True)], 5000, 5000, [100_000]) is None


# ---- the lines ----------------------------------------------------------------------------------

def test_the_header_and_the_rows_of_the_file(tmp_path):
    assert driver.insulation_header([10_000, 25_000]) == (
        "chrom\tstart\tend\tsum_10000\tn_valid_10000\tlog2_insulation_score_10000"
        "\tsum_25000\tn_valid_25000\tlog2_insulation_score_25000\n")
    iv = {"name": "chrA", "size": 50_000, "start": 10_000, "end": 23_000}
    # means 4, 0, 2^40 (median 4) and 2, 2, none (median 2): every score is exact
    ins_sum = np.array([[8, 0, 2**40], [2, 2, 4]], dtype=np.uint64)
    n_valid = np.array([[2, 1, 1], [1, 1, 0]], dtype=np.uint64)
    score = api.insulation_score(ins_sum, n_valid)
    lines = driver.insulation_lines(iv, 5000, 1, ins_sum, n_valid, score)
    assert lines == ["chrA\t10000\t15000\t8\t2\t0.0\t2\t1\t0.0\n",
                     "chrA\t15000\t20000\t0\t1\tnan\t2\t1\t0.0\n",
                     "chrA\t20000\t23000\t1099511627776\t1\t38.0\t4\t0\tnan\n"]
    # at twice the bin size the interval starts in the middle of coarse bin 1 of its chromosome: the fine
    # bins 2, 3, 4 (from 10 kb) fall into the coarse bins 1 (one fine bin) and 2 (two, clipped at the end)
    iv = {"name": "chrA", "size": 50_000, "start": 15_000, "end": 28_000}
    rows = driver.insulation_lines(iv, 5000, 2, ins_sum[:, :2], n_valid[:, :2], score[:, :2])
    assert [r.split("\t")[:3] for r in rows] == [["chrA", "15000", "20000"], ["chrA", "20000", "28000"]]
    # the writer: the header, plan order, a skipped entry and one without a matrix write no row
    plan = [entry("chrA", 10_000, 23_000, 3, 3), entry("chrA", 30_000, 50_000, 3, 4, skipped=True),
            entry("chrB", 0, 10_000, 2, 2), entry("chrC", 0, 15_000, 3, 3)]
    calls = []

    def fed(k, factor, first_bin):
        calls.append((k, factor, first_bin))
        return None if k == 2 else (ins_sum, n_valid)

    path = str(tmp_path / "i.tsv")
    driver.write_insulation(path, plan, 5000, 5000, [10_000, 25_000], fed)
    got = open(path).readlines()
    assert calls == [(0, 1, 2), (2, 1, 0), (3, 1, 0)]
    assert got[0] == driver.insulation_header([10_000, 25_000]) and got[1:4] == lines and len(got) == 7
    assert [r.split("\t")[:3] for r in got[4:]] == [["chrC", "0", "5000"], ["chrC", "5000", "10000"],
                                                      ["chrC", "10000", "15000"]]


class FakeSim:
    """api.Simulator.insulation from a table"""

    def __init__(self, table):
        self.table, self.calls = table, []

    def insulation(self, interval_id, windows, min_diag=2, factor=1, first_bin=0):
        self.calls.append((interval_id, list(windows), min_diag, factor, first_bin))
        return self.table[interval_id]


def test_the_output_stage_checks_what_it_writes_and_names_the_interval_and_the_window():
    nrows, ncols, windows = 9, 30, [5, 2]
    band = make_band(nrows, ncols, "full", seed=2)
    diag_sum = reference_marginals(band, nrows, ncols, 0)[0]
    ins = prefix_insulation(band, nrows, ncols, windows, 2)
    n_valid = np.array([brute_n_valid(ncols, w, 2) for w in windows], dtype=np.uint64)
    plan = [entry("chrA", 0, 150_000, nrows, ncols), entry("chrB", 0, 150_000, nrows, ncols, skipped=True)]
    asked = []

    def marginals(k, factor, first_bin):
        asked.append((k, factor, first_bin))
        return diag_sum, None

    sim = FakeSim({11: (ins, n_valid)})
    got = driver._interval_insulation(sim, plan, [11, None], windows, 2, marginals, 0, 1, 0)
    assert got[0] is ins and got[1] is n_valid
    assert sim.calls == [(11, windows, 2, 1, 0)] and asked == [(0, 1, 0)]
    assert driver._interval_insulation(sim, plan, [11, None], windows, 2, marginals, 1, 1, 0) is None
    assert len(sim.calls) == 1
    doctored = ins.copy()
    doctored[1, 7] -= np.uint64(1)
    with pytest.raises(RuntimeError) as e:
        driver._interval_insulation(FakeSim({11: (doctored, n_valid)}), plan, [11, None], windows, 2, marginals, 0, 1, 0)
    assert "chrA:0-150000" in str(e.value) and "window of 2 bins" in str(e.value)
