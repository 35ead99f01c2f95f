"""`simulate --dots --dots-fdr` end to end, on the genome and the options of tests/test_gpu_simulate_dots.py (without
clustering, so that the dots are the candidates): <prefix>_dots_thresholds.tsv and <prefix>_dots.bedpe are what the
numpy restatement of tests/test_dots_fdr_outputs.py computes from the pixel table read back out of the .mcool the same
run wrote -- the histogram over both chromosomes, pixels.dot_thresholds, the threshold decision with the fold test
on; the rows are a subset of those of the run without the option; and `analyze` of the run's .mcool writes both files
byte for byte.  Two rates: 0.1, at which no pixel of this 3.5 Mb genome clears the thresholds of all four
neighbourhoods (the file of the dots is the header alone, and must be), and 0.5, at which a dozen do, so that every
check also sees rows.  Each run is a fresh child process, made once per module, one at a time."""
import os

import numpy as np
import pytest

import test_gpu_simulate_dots as dots
import test_gpu_simulate_ranks as ranks
from test_dots_fdr_outputs import reference_fdr_candidates, reference_hist
from test_dots_outputs import candidate_pixels, sat_dot_sums, valid_mask
from test_gpu_analyze import analyze
from test_gpu_marginals import reference_marginals
from test_gpu_simulate_marginals import CHROMS, SIMULATED, pixels_of

from modle_amd import driver, pixels

pytestmark = pytest.mark.gpu

RATES = (0.1, 0.5)
CALLS = {0.1: False, 0.5: True}  # whether the restatement calls a dot at the rate (it prints how many)
ANALYSIS = ["--mcool-resolutions", "10kb", "--dots", "--dots-window", "15kb", "--dots-peak", "5kb", "--dots-min-count",
            str(dots.MIN_COUNT), "--dots-folds", ",".join(map(str, dots.FOLDS)), "--dots-cluster-radius", "0"]
# (a contact density above the other end-to-end tests': counts that a Poisson tail can tell from noise)
RUN = ["--ncells", str(ranks.NCELLS), "--no-track-1d-lef-position", "--target-contact-density", "20"]


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("dots_fdr"))


@pytest.fixture(scope="module")
def plain(workdir):
    return ranks.simulate(workdir, "plain", 1, 0, RUN + ANALYSIS)[0]


@pytest.fixture(scope="module", params=RATES)
def tested(request, workdir, plain):  # (after the run without the option has ended): (rate, prefix)
    rate = request.param
    return rate, ranks.simulate(workdir, f"tested{rate}", 1, 0, RUN + ANALYSIS + ["--dots-fdr", str(rate)])[0]


def test_the_files_of_the_runs(plain, tested):
    assert ranks.files_of(plain) == ["run.mcool", "run_dots.bedpe"]
    assert ranks.files_of(tested[1]) == ["run.mcool", "run_dots.bedpe", "run_dots_thresholds.tsv"]


def test_the_rows_are_a_subset_of_those_of_the_run_without_the_option(plain, tested):
    rate, run = tested
    with open(plain + "_dots.bedpe") as a, open(run + "_dots.bedpe") as b:
        loose, strict = a.readlines(), b.readlines()
    assert strict[0] == loose[0] == driver.dots_header()
    assert set(strict) <= set(loose) and len(strict) < len(loose)
    assert (len(strict) > 1) == CALLS[rate]
    at = [loose.index(row) for row in strict]
    assert at == sorted(at)  # in the same order


def test_both_files_are_the_restatement_s_on_the_mcool_s_pixels(tested):
    """with the options of this module the restatement finds, over chrA and chrC, 16 822 valid pixels with counts up
    to 148; at a rate of 0.1 18 chunks have a threshold and no pixel clears those of all four neighbourhoods, at 0.5
    34 chunks have one and 12 pixels do, of the 6 091 the fold test alone calls (printed by the test).  Every row of
    the file is a pixel the restatement calls, and every such pixel is a row."""
    FDR, tested = tested
    level = pixels_of(tested + ".mcool", dots.BASE)
    nrows, w, p, min_diag = dots.NROWS, dots.W, dots.P, dots.MIN_DIAG
    edges = pixels.dot_lambda_edges()
    bands = {}
    for name in SIMULATED:  # plan order
        ncols, b1, b2, cn = level[name]
        band = np.zeros(nrows * ncols + 1, dtype=np.uint32)
        band[b2 * nrows + (b2 - b1)] = cn
        diag_sum = reference_marginals(band, nrows, ncols, 0)[0]
        bands[name] = (band, ncols, diag_sum, sat_dot_sums(band, nrows, ncols, w, p, min_diag),
                       pixels.dot_scales(diag_sum, ncols, w, p, (1.0, 1.0, 1.0, 1.0), min_diag))
    n_obs = min(max(int(band.max()) for band, *_ in bands.values()) + 2, 16384)
    hist = sum(reference_hist(band, nrows, ncols, sums, lam, edges, n_obs, w, min_diag)
               for band, ncols, _, sums, lam in bands.values())
    n_valid = sum(int(valid_mask(nrows, ncols, w, min_diag).sum()) for _, ncols, *_ in bands.values())
    driver.check_dot_hist(hist, n_valid)
    thr = pixels.dot_thresholds(hist, edges, FDR)
    with open(tested + "_dots_thresholds.tsv") as fh:
        assert fh.readlines() == [driver.dot_thresholds_header()] + driver.dot_thresholds_lines(dots.BASE, edges, hist, thr)
    want, n_dots = [driver.dots_header()], 0
    for name in SIMULATED:
        band, ncols, diag_sum, sums, lam = bands[name]
        size = dict(CHROMS)[name]
        scale = pixels.dot_scales(diag_sum, ncols, w, p, dots.FOLDS, min_diag)
        c1, c2, cc = candidate_pixels(reference_fdr_candidates(band, nrows, ncols, sums, lam, edges, thr, scale, w, min_diag,
                                                               dots.MIN_COUNT), nrows, ncols)
        e = diag_sum.astype(np.float64) / (ncols - np.arange(nrows))
        n_dots += len(c1)
        for i, j, c in zip(map(int, c1), map(int, c2), map(int, cc)):
            x = float(e[j - i])
            want.append(f"{name}\t{i * dots.BASE}\t{min((i + 1) * dots.BASE, size)}\t{name}\t{j * dots.BASE}\t"
                        f"{min((j + 1) * dots.BASE, size)}\t{c}\t{x!r}\t{c / x!r}\n")
    print(f"valid pixels {n_valid}, counts up to {n_obs - 2}, {np.count_nonzero(thr)} thresholds, dots {n_dots}")
    assert (n_dots > 0) == CALLS[FDR]
    with open(tested + "_dots.bedpe") as fh:
        assert fh.readlines() == want


def test_analyze_of_the_run_s_mcool_writes_both_files_byte_for_byte(workdir, tested):
    FDR, tested = tested
    out = os.path.join(workdir, f"analyzed{FDR}", "run")
    analyze([f"{tested}.mcool::/resolutions/{dots.BASE}", "-o", out, "-w", ranks.DIAGONAL_WIDTH] + ANALYSIS
            + ["--dots-fdr", str(FDR)])
    assert ranks.files_of(out) == ["run.mcool", "run_dots.bedpe", "run_dots_thresholds.tsv"]
    for tail in ("_dots.bedpe", "_dots_thresholds.tsv"):
        with open(tested + tail, "rb") as a, open(out + tail, "rb") as b:
            ours = a.read()
            assert ours == b.read(), tail
            assert tail != "_dots.bedpe" or (ours.count(b"\n") > 1) == CALLS[FDR]
