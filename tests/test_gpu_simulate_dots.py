"""`simulate --dots` end to end, on the genome, the cell count and the options of
tests/test_gpu_simulate_ranks.py: every row of <prefix>_dots.bedpe is what the numpy restatement of
tests/test_dots_outputs.py computes from the pixel table read back out of the .mcool the same run wrote --
the diagonal sums, pixels.dot_scales, the candidate rule, api.cluster_dots; a window that does not fit the
band ends the run before anything is simulated; a run without the option writes no such file; and two
ranks that share this GPU (--dist-backend gloo) write the file byte for byte as the single rank does.  Each
run is a fresh child process, made once per module; at most two processes have the GPU open at a time."""
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_simulate_ranks as ranks
from test_dots_outputs import candidate_pixels, reference_candidates, sat_dot_sums, valid_mask
from test_gpu_marginals import reference_marginals
from test_gpu_simulate_marginals import CHROMS, SIMULATED, pixels_of

from modle_amd import api, driver, pixels

pytestmark = pytest.mark.gpu

BASE = 5000
NROWS = 40            # -w 200kb at 5 kb
W, P, MIN_DIAG = 3, 1, 2  # bins: 4 * 3 + 1 + 2 = 15 diagonals are needed
# chosen for this test (the defaults ask for 1.75 / 1.5 times a neighbourhood that is mostly empty at 5
# cells): the counts they give are in the docstring of the test below
FOLDS, MIN_COUNT, RADIUS = (1.0, 1.0, 1.0, 1.0), 2, 2
BASIC = ["--ncells", str(ranks.NCELLS), "--no-track-1d-lef-position", "--mcool-resolutions", "10kb"]
OPTIONS = BASIC + ["--dots", "--dots-window", "15kb", "--dots-peak", "5kb", "--dots-min-count", str(MIN_COUNT),
                   "--dots-folds", ",".join(map(str, FOLDS)), "--dots-cluster-radius", "10kb"]


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("dots"))


@pytest.fixture(scope="module")
def one(workdir):
    return ranks.simulate(workdir, "one", 1, 0, OPTIONS)[0]


@pytest.fixture(scope="module")
def two(workdir, one):  # (after the single-rank run has ended)
    return ranks.simulate(workdir, "two", 2, ranks.PORT + 5, OPTIONS)[0]


def test_the_files_of_the_run(one):
    assert ranks.files_of(one) == ["run.mcool", "run_dots.bedpe"]


def test_every_row_of_the_file_is_a_clustered_candidate_of_the_mcool_s_pixels(one):
    """with the folds and the smallest count of this module the restatement finds, over chrA and chrC, 178
    candidates among 16 822 valid pixels and 141 dots after clustering (printed by the test): at least 10
    dots, and fewer than half of the valid pixels, are asserted"""
    want = [driver.dots_header()]
    level = pixels_of(one + ".mcool", BASE)
    n_valid = n_candidates = n_dots = 0
    for name in SIMULATED:  # plan order
        size = dict(CHROMS)[name]
        ncols, b1, b2, cn = level[name]
        assert len(cn) > 50 and (b2 - b1).max() < NROWS and (b2 - b1).min() == 0
        band = np.zeros(NROWS * ncols + 1, dtype=np.uint32)
        band[b2 * NROWS + (b2 - b1)] = cn
        diag_sum = reference_marginals(band, NROWS, ncols, 0)[0]
        table = pixels.dot_scales(diag_sum, ncols, W, P, FOLDS, MIN_DIAG)
        sums = sat_dot_sums(band, NROWS, ncols, W, P, MIN_DIAG)
        c1, c2, cc = candidate_pixels(reference_candidates(band, NROWS, ncols, sums, table, W, MIN_DIAG, MIN_COUNT),
                                      NROWS, ncols)
        keep = api.cluster_dots(c1, c2, cc, RADIUS)
        e = diag_sum.astype(np.float64) / (ncols - np.arange(NROWS))
        n_valid += int(valid_mask(NROWS, ncols, W, MIN_DIAG).sum())
        n_candidates += len(c1)
        n_dots += len(keep)
        for n in keep:
            i, j, c, x = int(c1[n]), int(c2[n]), int(cc[n]), float(e[c2[n] - c1[n]])
            want.append(f"{name}\t{i * BASE}\t{min((i + 1) * BASE, size)}\t{name}\t{j * BASE}\t{min((j + 1) * BASE, size)}"
                        f"\t{c}\t{x!r}\t{c / x!r}\n")
    print(f"valid pixels {n_valid}, candidates {n_candidates}, dots {n_dots}")
    assert n_dots >= 10 and 2 * n_candidates < n_valid
    with open(one + "_dots.bedpe") as fh:
        got = fh.readlines()
    assert got == want


def test_a_window_that_does_not_fit_ends_the_run_before_the_launch(workdir):
    os.makedirs(os.path.join(workdir, "in"), exist_ok=True)
    sizes, bed = ranks.genome_files(os.path.join(workdir, "in"))
    prefix = os.path.join(workdir, "misfit", "run")
    options = BASIC + ["--dots", "--dots-window", "50kb"]  # 4 * 10 + 1 + 2 > 40
    p = subprocess.run([sys.executable, "-m", "modle_amd", "simulate", "-c", sizes, "-b", bed, "-o", prefix,
                        *ranks.COMMON, *options], cwd=ranks.ROOT, capture_output=True, text=True, timeout=120,
                       env={k: v for k, v in os.environ.items() if k not in ("MODLE_HIP_LIB", "MODLE_PIXELS_LIB")})
    assert p.returncode != 0
    last = p.stderr.strip().splitlines()[-1]
    assert last.startswith("--dots-window: the window of 50000 (10 bins of 5000) with 2 diagonals ignored does not fit "
                           "the band of chrA:0-2000000 (40 diagonals)") and "45000 (9 bins)" in last, p.stderr[-2000:]
    assert "simulating" not in p.stderr and "simulation kernel" not in p.stderr
    assert not ranks.files_of(prefix)  # no file


def test_a_run_without_the_option_writes_no_such_file(workdir, one):
    plain = ranks.simulate(workdir, "plain", 1, 0, BASIC)[0]
    assert ranks.files_of(plain) == ["run.mcool"]


def test_two_ranks_write_the_file_byte_for_byte(one, two):
    assert ranks.files_of(two) == ["run.mcool", "run_dots.bedpe"]
    with open(one + "_dots.bedpe", "rb") as a, open(two + "_dots.bedpe", "rb") as b:
        single = a.read()
        assert b.read() == single and len(single) > 500
