"""`simulate --insulation-windows` end to end, on the genome, the cell count and the options of
tests/test_gpu_simulate_ranks.py, at twice the bin size and with an .mcool that holds that size: every sum
and every n_valid of <prefix>_insulation.tsv is what the numpy restatement of tests/test_insulation_outputs.py
computes from the pixel table read back out of the .mcool the same run wrote, and every score is
api.insulation_score of them; a window whose diamond does not fit the band ends the run before anything is
simulated; a run without the options writes no such file; and two ranks that share this GPU
(--dist-backend gloo) write the file byte for byte as the single rank does.  Each run is a fresh child
process, made once per module; at most two processes have the GPU open at a time."""
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_simulate_ranks as ranks
from test_gpu_simulate_marginals import CHROMS, SIMULATED, pixels_of
from test_insulation_outputs import brute_n_valid, prefix_insulation

from modle_amd import api, driver

pytestmark = pytest.mark.gpu

BASE, RES = 5000, 10000
NROWS = 21              # -w 200kb at 5 kb is 40 diagonals: (40 - 1 + 1) // 2 + 1 at 10 kb
WINDOWS = (50_000, 110_000)  # 5 and 11 bins: the diamond of the second fills the band exactly
MIN_DIAG = 1
BASIC = ["--ncells", str(ranks.NCELLS), "--no-track-1d-lef-position", "--mcool-resolutions", "10kb,25kb"]
OPTIONS = BASIC + ["--insulation-windows", "50kb,110kb", "--insulation-resolution", "10kb",
                   "--insulation-ignore-diags", str(MIN_DIAG)]


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("insulation"))


@pytest.fixture(scope="module")
def one(workdir):
    return ranks.simulate(workdir, "one", 1, 0, OPTIONS)[0]


@pytest.fixture(scope="module")
def two(workdir, one):  # (after the single-rank run has ended)
    return ranks.simulate(workdir, "two", 2, ranks.PORT + 4, OPTIONS)[0]


def test_the_files_of_the_run(one):
    assert ranks.files_of(one) == ["run.mcool", "run_insulation.tsv"]


def test_every_row_of_the_file_is_the_diamond_sum_of_the_mcool_s_pixels(one):
    want = [driver.insulation_header(WINDOWS)]
    bins = [w // RES for w in WINDOWS]
    level = pixels_of(one + ".mcool", RES)
    assert not level["chrB"][3].size
    for name in SIMULATED:  # plan order
        size = dict(CHROMS)[name]
        ncols, b1, b2, cn = level[name]
        assert len(cn) > 50 and (b2 - b1).max() < NROWS and (b2 - b1).min() == 0
        band = np.zeros(NROWS * ncols + 1, dtype=np.uint32)
        band[b2 * NROWS + (b2 - b1)] = cn
        ins_sum = prefix_insulation(band, NROWS, ncols, bins, MIN_DIAG)
        n_valid = np.array([brute_n_valid(ncols, w, MIN_DIAG) for w in bins], dtype=np.uint64)
        assert int(ins_sum[0].sum()) > 1000 and int(ins_sum[1].sum()) > int(ins_sum[0].sum())
        assert int(n_valid[1][ncols // 2]) == 11 * 11 - 1 and int(n_valid[1][0]) == 11 - 1
        score = api.insulation_score(ins_sum, n_valid)
        assert np.isfinite(score[1]).sum() > ncols // 2
        for c in range(ncols):
            want.append(f"{name}\t{c * RES}\t{min((c + 1) * RES, size)}" + "".join(
                f"\t{int(ins_sum[k][c])}\t{int(n_valid[k][c])}\t{float(score[k][c])!r}" for k in range(2)) + "\n")
    with open(one + "_insulation.tsv") as fh:
        got = fh.readlines()
    assert len(got) == len(want) == 1 + 200 + 150
    assert got == want


def test_a_window_that_does_not_fit_ends_the_run_before_the_launch(workdir):
    os.makedirs(os.path.join(workdir, "in"), exist_ok=True)
    sizes, bed = ranks.genome_files(os.path.join(workdir, "in"))
    prefix = os.path.join(workdir, "misfit", "run")
    options = BASIC + ["--insulation-windows", "50kb,120kb", "--insulation-resolution", "10kb"]  # 2 * 12 - 1 > 21
    p = subprocess.run([sys.executable, "-m", "modle_amd", "simulate", "-c", sizes, "-b", bed, "-o", prefix,
                        *ranks.COMMON, *options], cwd=ranks.ROOT, capture_output=True, text=True, timeout=120,
                       env={k: v for k, v in os.environ.items() if k not in ("MODLE_HIP_LIB", "MODLE_PIXELS_LIB")})
    assert p.returncode != 0
    last = p.stderr.strip().splitlines()[-1]
    assert last.startswith("--insulation-windows: the diamond of 120000 (12 bins of 10000) does not fit the band of "
                           "chrA:0-2000000 (21 diagonals)") and "110000 (11 bins)" in last, p.stderr[-2000:]
    assert "simulating" not in p.stderr and "simulation kernel" not in p.stderr
    assert not ranks.files_of(prefix)  # no file


def test_a_run_without_the_options_writes_no_such_file(workdir, one):
    plain = ranks.simulate(workdir, "plain", 1, 0, BASIC)[0]
    assert ranks.files_of(plain) == ["run.mcool"]


def test_two_ranks_write_the_file_byte_for_byte(one, two):
    assert ranks.files_of(two) == ["run.mcool", "run_insulation.tsv"]
    with open(one + "_insulation.tsv", "rb") as a, open(two + "_insulation.tsv", "rb") as b:
        single = a.read()
        assert b.read() == single and len(single) > 1000
