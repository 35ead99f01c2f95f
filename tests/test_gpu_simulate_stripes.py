"""`simulate --compare-to` end to end, on the genome, the cell count and the options of
tests/test_gpu_simulate_ranks.py: a first run writes an .mcool at 5 and 10 kb; a second run with another seed
is compared with its 5 kb level, and every row of <prefix>_stripes.tsv is pixels.stripe_scores of the sums that
api.BandAnalyses.stripe_moments forms here from the two files' pixels, and agrees with evaluate.compare on host
bands within the tolerance of tests/test_stripes_outputs.py; a third run is compared at twice its bin size with
the 10 kb level, its band coarsened on the device; a run with the first run's seed scores an RMSE of 0 on every
bin; and `analyze` of the second run's .cool with the same options writes the file byte for byte.  Each run is
a fresh child process, made once per module; one process has the GPU open at a time besides this one."""
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_simulate_ranks as ranks
from test_gpu_simulate_marginals import CHROMS, SIMULATED
from test_stripes_outputs import TOLERANCE

from modle_amd import api, cooler, driver, evaluate, pixels

pytestmark = pytest.mark.gpu

BASE, RES = 5000, 10000
NROWS = 40  # -w 200kb at 5 kb
BASIC = ["--ncells", str(ranks.NCELLS), "--no-track-1d-lef-position"]
METRICS = ["pearson", "spearman", "rmse"]
COARSE_METRICS = ["rmse", "pearson"]


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("stripes"))


@pytest.fixture(scope="module")
def first(workdir):
    return ranks.simulate(workdir, "first", 1, 0, BASIC + ["--mcool-resolutions", "10kb"])[0] + ".mcool"


def compare_options(first, res, metrics, *more):
    return ["--compare-to", f"{first}::/resolutions/{res}", "--compare-metrics", ",".join(metrics), *more]


@pytest.fixture(scope="module")
def second(workdir, first):
    return ranks.simulate(workdir, "second", 1, 0, BASIC + ["--seed", "6"] + compare_options(first, BASE, METRICS))[0]


@pytest.fixture(scope="module")
def third(workdir, first, second):
    return ranks.simulate(workdir, "third", 1, 0, BASIC + ["--seed", "6"] + compare_options(
        first, RES, COARSE_METRICS, "--compare-resolution", "10kb", "--compare-exclude-zero-pixels"))[0]


def band_pixels(uri, name, nrows):
    """(bin1, bin2, count, first bin, bins) of a chromosome of a cooler, as the file holds them, and its dense
    host band of `nrows` diagonals"""
    with cooler.CoolerReader(uri) as r:
        bin1, bin2, count, first = r.pixels(name)
        ncols = r.n_bins(name)
    i, j = bin1 - first, bin2 - first
    keep = (j < ncols) & (j - i < nrows)
    band = np.zeros(nrows * ncols + 1, dtype=np.uint32)
    band[j[keep] * nrows + (j[keep] - i[keep])] = count[keep]
    return (bin1, bin2, count, first, ncols), band


def expected_file(ref_uri, run_cool, res, metrics, exclude_zero):
    """(the lines of <prefix>_stripes.tsv, {chromosome: (reference band, run band, nrows, ncols)} on the host at
    `res`): the reference's pixels at `res` and the run's at the base bin size go to bands on the device, the
    run's is coarsened there, and the scores are pixels.stripe_scores of api.stripe_moments"""
    factor = res // BASE
    lines = [driver.stripes_header(ref_uri, res, exclude_zero, metrics)]
    host = {}
    what = driver.stripes_what(metrics, exclude_zero)
    with api.LoadedBands(0) as refs, api.LoadedBands(0) as runs:
        for name in SIMULATED:  # plan order; chrB has no barrier and no pixel
            size = dict(CHROMS)[name]
            (b1, b2, cn, off, ncols), run_band = band_pixels(run_cool, name, NROWS)
            assert ncols == -(-size // BASE) and int(run_band.sum()) > 1000
            nr, nc = pixels.band_shape(NROWS, ncols, factor, 0)
            tid, _ = runs.load_pixels(b1, b2, cn, NROWS, ncols, off)
            (b1, b2, cn, off, ref_cols), ref_band = band_pixels(ref_uri, name, nr)
            assert ref_cols == nc and int(ref_band.sum()) > 1000
            rid, _ = refs.load_pixels(b1, b2, cn, nr, nc, off)
            rows = runs.stripe_moments(tid, refs, rid, what, factor=factor, first_bin=0)
            assert rows.shape == (2, pixels.stripes_rows(what), nc)
            scores = [tuple(pixels.stripe_scores(rows[d], m, exclude_zero) for d in (0, 1)) for m in metrics]
            iv = {"name": name, "start": 0, "end": size}
            lines += driver.stripes_lines(iv, BASE, factor, scores)
            host[name] = (ref_band, rows, scores, nr, nc)
    return "".join(lines), host


def test_the_files_of_the_runs(first, second, third):
    assert ranks.files_of(first) == ["run.mcool"]
    assert ranks.files_of(second) == ["run.cool", "run_stripes.tsv"]
    assert ranks.files_of(third) == ["run.cool", "run_stripes.tsv"]


def test_every_row_is_the_score_of_the_sums_formed_here(first, second):
    uri = f"{first}::/resolutions/{BASE}"
    want, host = expected_file(uri, second + ".cool", BASE, METRICS, False)
    got = open(second + "_stripes.tsv").read()
    assert got == want
    assert len(got.splitlines()) == 2 + 400 + 300
    assert got.splitlines()[1] == "chrom\tstart\tend\tpearson_vertical\tpearson_horizontal\tspearman_vertical\t" \
                                  "spearman_horizontal\trmse_vertical\trmse_horizontal"
    # the same against evaluate.compare on dense host bands
    for name in SIMULATED:
        ref_band, _, scores, nr, nc = host[name]
        _, run_band = band_pixels(second + ".cool", name, NROWS)
        assert not np.array_equal(ref_band, run_band)  # another seed
        for (v, h), metric in zip(scores, METRICS):
            for mine, direction in ((v, "vertical"), (h, "horizontal")):
                theirs = evaluate.compare(ref_band, run_band, nr, nc, metric, direction)[0]
                assert np.array_equal(np.isnan(mine), np.isnan(theirs)), (name, metric, direction)
                ok = ~np.isnan(theirs)
                scale = np.maximum(theirs[ok], 1.0) if metric == "rmse" else 1.0
                assert (np.abs(mine[ok] - theirs[ok]) / scale <= TOLERANCE[metric]).all(), (name, metric, direction)
                assert ok.sum() > nc // 2


def test_a_comparison_at_twice_the_bin_size_coarsens_the_run_on_the_device(first, third):
    uri = f"{first}::/resolutions/{RES}"
    want, host = expected_file(uri, third + ".cool", RES, COARSE_METRICS, True)
    got = open(third + "_stripes.tsv").read()
    assert got == want
    assert got.startswith(f"# reference={uri} resolution=10000 exclude_zero_pixels=yes\nchrom\tstart\tend\trmse_vertical\t")
    assert len(got.splitlines()) == 2 + 200 + 150
    assert host["chrA"][3:] == (21, 200)  # (40 - 1 + 1) // 2 + 1 diagonals at 10 kb


def test_a_run_with_the_seed_of_the_reference_is_at_distance_zero(workdir, first, third):
    same = ranks.simulate(workdir, "same", 1, 0, BASIC + compare_options(first, BASE, ["rmse", "eucl_dist", "pearson"]))[0]
    rows = [l.split("\t") for l in open(same + "_stripes.tsv").read().splitlines()[2:]]
    assert len(rows) == 400 + 300
    assert all(r[3:7] == ["0.0"] * 4 for r in rows)
    assert all(r[7] in ("1.0", "nan") and r[8] in ("1.0", "nan") for r in rows) and sum(r[7] == "1.0" for r in rows) > 350


def test_analyze_of_the_run_s_cooler_writes_the_same_file(workdir, first, second, third):
    prefix = os.path.join(workdir, "analyzed", "run")
    p = subprocess.run([sys.executable, "-m", "modle_amd", "analyze", second + ".cool", "-o", prefix, "-w",
                        ranks.DIAGONAL_WIDTH, *compare_options(first, BASE, METRICS)], cwd=ranks.ROOT,
                       capture_output=True, text=True, timeout=300,
                       env={k: v for k, v in os.environ.items() if k not in ("MODLE_HIP_LIB", "MODLE_PIXELS_LIB")})
    assert p.returncode == 0, p.stderr[-3000:]
    assert "run_stripes.tsv" in ranks.files_of(prefix)
    with open(prefix + "_stripes.tsv", "rb") as a, open(second + "_stripes.tsv", "rb") as b:
        theirs = b.read()
        assert a.read() == theirs and len(theirs) > 10_000
