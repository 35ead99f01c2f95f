"""`simulate --expected --coverage` end to end, on the genome, the cell count and the options of
tests/test_gpu_simulate_ranks.py and with an .mcool of two coarse levels: every row of
<prefix>_expected.tsv and every line of <prefix>_coverage.bedgraph is what numpy computes from the pixel
tables read back out of the .mcool the same run wrote, resolution by resolution; and two ranks that share
this GPU (--dist-backend gloo, launched the way that module launches its ranks) write both files byte for
byte as the single rank does.  Each run is a fresh child process, made once per module; at most two
processes have the GPU open at a time."""
import numpy as np
import pytest

import test_gpu_simulate_ranks as ranks
from test_mcool_writer import read_group

pytestmark = pytest.mark.gpu

BASE, BIN_SIZES = 5000, (5000, 10000, 25000)
NROWS = 40       # -w 200kb at 5 kb
MIN_DIAG = 2
CHROMS = [("chrA", 2_000_000), ("chrB", 500_000), ("chrC", 1_500_000)]  # chrB has no barrier: it is skipped
SIMULATED = ("chrA", "chrC")
OPTIONS = ["--ncells", str(ranks.NCELLS), "--no-track-1d-lef-position", "--mcool-resolutions", "10kb,25kb",
           "--expected", "--coverage", "--coverage-ignore-diags", str(MIN_DIAG)]
HEADER = "chrom\tstart\tend\tbin_size\tdist\tdist_bp\tn_valid\tcount_sum\tcount_avg\n"


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("marginals"))


@pytest.fixture(scope="module")
def one(workdir):
    return ranks.simulate(workdir, "one", 1, 0, OPTIONS)[0]


@pytest.fixture(scope="module")
def two(workdir, one):  # (after the single-rank run has ended)
    return ranks.simulate(workdir, "two", 2, ranks.PORT + 3, OPTIONS)[0]


def pixels_of(mcool, bin_size):
    """{chromosome: (bins, bin1, bin2, count)} of one resolution, the ids relative to the chromosome"""
    group = read_group(mcool, f"/resolutions/{bin_size}")
    assert group["attrs"]["bin-size"] == bin_size
    out = {}
    for c, (name, size) in enumerate(CHROMS):
        px = np.array(group["pixels_by_chrom"][name], dtype=np.int64).reshape(-1, 3)
        out[name] = (-(-size // bin_size), px[:, 0] - group["chrom_offset"][c], px[:, 1] - group["chrom_offset"][c],
                     px[:, 2])
    return out


def test_the_files_of_the_run(one):
    assert ranks.files_of(one) == ["run.mcool", "run_coverage.bedgraph", "run_expected.tsv"]


def test_every_row_of_the_expected_file_is_the_sum_of_a_diagonal_of_the_mcool(one):
    want, totals = [HEADER], []
    per_level = {b: pixels_of(one + ".mcool", b) for b in BIN_SIZES}
    for name in SIMULATED:  # plan order, then ascending bin size, then ascending diagonal
        size = dict(CHROMS)[name]
        for b in BIN_SIZES:
            k = b // BASE
            ncols, b1, b2, cn = per_level[b][name]
            nrows = min(ncols, (NROWS - 1 + k - 1) // k + 1)
            assert len(cn) > 50 and (b2 - b1).max() < nrows and (b2 - b1).min() == 0
            diag_sum = np.zeros(nrows, dtype=np.int64)
            np.add.at(diag_sum, b2 - b1, cn)
            totals.append(int(diag_sum.sum()))
            for d in range(nrows):
                s, n = int(diag_sum[d]), ncols - d
                want.append(f"{name}\t0\t{size}\t{b}\t{d}\t{d * b}\t{n}\t{s}\t{s / n!r}\n")
    assert not per_level[BASE]["chrB"][3].size
    assert totals[0] == totals[1] == totals[2] > 1000 and totals[3] == totals[4] == totals[5] > 1000
    with open(one + "_expected.tsv") as fh:
        got = fh.readlines()
    assert len(got) == len(want) == 1 + 2 * (40 + 21 + 9)
    assert got == want


def test_every_line_of_the_coverage_file_is_a_row_sum_of_the_base_resolution(one):
    want = []
    for name in SIMULATED:
        size = dict(CHROMS)[name]
        ncols, b1, b2, cn = pixels_of(one + ".mcool", BASE)[name]
        d = b2 - b1
        coverage = np.zeros(ncols, dtype=np.int64)
        np.add.at(coverage, b2[d >= MIN_DIAG], cn[d >= MIN_DIAG])            # the column part
        np.add.at(coverage, b1[d >= max(MIN_DIAG, 1)], cn[d >= max(MIN_DIAG, 1)])  # the row part
        assert coverage.sum() == 2 * cn[d >= MIN_DIAG].sum() > 1000 and cn[d < MIN_DIAG].sum() > 0
        want += [f"{name}\t{i * BASE}\t{min((i + 1) * BASE, size)}\t{int(c)}\n" for i, c in enumerate(coverage)]
    with open(one + "_coverage.bedgraph") as fh:
        got = fh.readlines()
    assert len(got) == len(want) == 400 + 300
    assert got == want


def test_two_ranks_write_both_files_byte_for_byte(one, two):
    assert ranks.files_of(two) == ["run.mcool", "run_coverage.bedgraph", "run_expected.tsv"]
    for suffix in ("_expected.tsv", "_coverage.bedgraph"):
        with open(one + suffix, "rb") as a, open(two + suffix, "rb") as b:
            single = a.read()
            assert b.read() == single and len(single) > 1000, suffix
