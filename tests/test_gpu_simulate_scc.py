"""`simulate --compare-to REF --scc` end to end, on the genome, the cell count and the options of
tests/test_gpu_simulate_ranks.py: a first run writes the reference .cool; a second run with another seed is
compared with it under a smoothing of 2 bins, and every row of <prefix>_scc.tsv is pixels.scc_scores of the
restatement of tests/test_scc_outputs.py on the two files read back, within its tolerance (n exactly); the
stripes file is byte for byte what the same run writes without --scc; and `analyze` of the second run's .cool
with the same options writes <prefix>_scc.tsv byte for byte.  Each run is a fresh child process, made once per
module; one process has the GPU open at a time besides this one."""
import math
import os
import subprocess
import sys

import pytest

import test_gpu_simulate_ranks as ranks
from test_gpu_simulate_marginals import CHROMS, SIMULATED
from test_gpu_simulate_stripes import BASE, BASIC, NROWS, band_pixels
from test_scc_outputs import TOLERANCE, restate

from modle_amd import driver, pixels

pytestmark = pytest.mark.gpu

H = 2
SMOOTH = H * BASE
LO, HI = 1, NROWS - 1 - 2 * H


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("scc"))


@pytest.fixture(scope="module")
def first(workdir):
    return ranks.simulate(workdir, "first", 1, 0, BASIC)[0] + ".cool"


def scc_options(first):
    return ["--compare-to", first, "--scc", "--scc-smooth", str(SMOOTH)]


@pytest.fixture(scope="module")
def second(workdir, first):
    return ranks.simulate(workdir, "second", 1, 0, BASIC + ["--seed", "6"] + scc_options(first))[0]


@pytest.fixture(scope="module")
def plain(workdir, first, second):
    return ranks.simulate(workdir, "plain", 1, 0, BASIC + ["--seed", "6", "--compare-to", first])[0]


def test_the_files_of_the_runs(first, second, plain):
    assert ranks.files_of(first) == ["run.cool"]
    assert ranks.files_of(second) == ["run.cool", "run_scc.tsv", "run_stripes.tsv"]
    assert ranks.files_of(plain) == ["run.cool", "run_stripes.tsv"]


def test_every_row_is_the_score_of_the_restated_sums(first, second):
    got = open(second + "_scc.tsv").read().splitlines()
    assert got[0] == f"# reference={first} resolution={BASE} smooth={SMOOTH} include_zeros=no"
    assert got[1] == "distance\tn\trho\tweight"
    at = 2
    for name in SIMULATED:  # plan order; chrB has no barrier and no pixel
        size = dict(CHROMS)[name]
        (_, _, _, _, ncols), run_band = band_pixels(second + ".cool", name, NROWS)
        (_, _, _, _, ref_cols), ref_band = band_pixels(first, name, NROWS)
        assert ncols == ref_cols == -(-size // BASE) and int(run_band.sum()) > 1000 and int(ref_band.sum()) > 1000
        rows = restate(ref_band, run_band, NROWS, ncols, H, LO, HI)
        scc, rho, weight = pixels.scc_scores(rows, ncols, LO, HI)
        head = dict(kv.split("=") for kv in got[at][2:].split(" "))
        assert got[at].startswith("# ") and {k: v for k, v in head.items() if k != "scc"} == {
            "chrom": name, "start": "0", "end": str(size), "bin_size": str(BASE), "smooth_bins": str(H),
            "min_diag": str(LO), "max_diag": str(HI)}
        assert abs(float(head["scc"]) - scc) <= TOLERANCE and 0.0 < scc < 1.0  # another seed, the same model
        for d in range(LO, HI + 1):
            dist, n, r, w = got[at + 1 + d - LO].split("\t")
            assert int(dist) == d * BASE and int(n) == int(rows[0][d])
            assert abs(float(w) - weight[d - LO]) <= TOLERANCE * weight[d - LO]
            assert math.isnan(float(r)) == math.isnan(rho[d - LO])
            assert math.isnan(float(r)) or abs(float(r) - rho[d - LO]) <= TOLERANCE
        assert int(rows[0][LO]) > ncols // 2  # the first diagonal is well filled
        assert got[at:at + 2 + HI - LO] == [l.rstrip("\n") for l in driver.scc_lines(
            {"name": name, "start": 0, "end": size}, BASE, 1, ncols, H, LO, HI, rows, False)]  # the same digits, too
        at += 2 + HI - LO
    assert at == len(got)


def test_the_stripes_file_is_that_of_a_run_without_scc(second, plain):
    with open(second + "_stripes.tsv", "rb") as a, open(plain + "_stripes.tsv", "rb") as b:
        theirs = b.read()
        assert a.read() == theirs and len(theirs) > 10_000


def test_analyze_of_the_run_s_cooler_writes_the_same_file(workdir, first, second, plain):
    prefix = os.path.join(workdir, "analyzed", "run")
    p = subprocess.run([sys.executable, "-m", "modle_amd", "analyze", second + ".cool", "-o", prefix, "-w",
                        ranks.DIAGONAL_WIDTH, *scc_options(first)], cwd=ranks.ROOT,
                       capture_output=True, text=True, timeout=300,
                       env={k: v for k, v in os.environ.items() if k not in ("MODLE_HIP_LIB", "MODLE_PIXELS_LIB")})
    assert p.returncode == 0, p.stderr[-3000:]
    assert {"run_scc.tsv", "run_stripes.tsv"} <= set(ranks.files_of(prefix))
    for name in ("_scc.tsv", "_stripes.tsv"):
        with open(prefix + name, "rb") as a, open(second + name, "rb") as b:
            theirs = b.read()
            assert a.read() == theirs and len(theirs) > 2_000, name
