"""`simulate --domains-at` end to end, on the genome and the cell count of tests/test_gpu_simulate_ranks.py: every
header and every row of <prefix>_domains.tsv is what the API (api.LoadedBands.rescaled_pileup and marginals,
api.rescaled_expected_terms, api.domain_strength) and the restatement of tests/test_rescale_outputs.py compute
from the pixels read back out of the .cool the same run wrote, over the domains of a small BED file written here
(the stretches between neighbouring barriers), at twice the bin size of the run; `analyze` of that .cool with the
same options writes the file byte for byte; a run without the option writes no such file.  Each run is a fresh
child process; one process has the GPU open at a time besides this one."""
import math
import os

import numpy as np
import pytest

import test_gpu_simulate_ranks as ranks
from test_gpu_analyze import analyze
from test_gpu_marginals import reference_coarsen
from test_gpu_simulate_pileup import barrier_positions
from test_rescale_outputs import rescale_blocks

from modle_amd import api, cooler, driver

pytestmark = pytest.mark.gpu

BASE, NROWS = 5000, 40  # -r 5kb, -w 200kb
RES, R, PERCENT = 10_000, 6, 50  # 21 diagonals of 10 kb; a domain of about 8 bins is padded by 4 on either side
CHROMS = dict([("chrA", 2_000_000), ("chrB", 500_000), ("chrC", 1_500_000)])
OPTIONS = ["--ncells", str(ranks.NCELLS), "--no-track-1d-lef-position"]


def bed_file(path):
    """the 20 + 12 stretches between neighbouring barriers of chrA and chrC, then a domain on the chromosome that
    is skipped and one on a chromosome that is not there, one whose window is deeper than the band and one whose
    padding leaves the matrix on the left: (given, placed, used) = (36, 34, 32)"""
    rows = ["#chrom\tstart\tend\tname\n"]
    for name, count in (("chrA", 20), ("chrC", 12)):
        pos = barrier_positions(name)
        rows += [f"{name}\t{pos[i]}\t{pos[i + 1]}\ttad{i}\n" for i in range(count)]
    rows += ["# what is not used\n", "chrB\t100000\t200000\n", "chrZ\t0\t1000\n", "chrA\t400000\t700000\n", "chrA\t10000\t60000\n"]
    with open(path, "w") as fh:
        fh.writelines(rows)
    return 36, 34, 32


def windows_of(path, name):
    """the windows of the domains of `name`, restated: whole chromosomes, bins of RES from 0"""
    s, e = [], []
    for line in open(path):
        c = line.split("\t")
        if not line.startswith("#") and c[0] == name:
            a = int(c[1]) // RES
            b = max(a + 1, -(-int(c[2]) // RES))
            pad = (b - a) * PERCENT // 100
            s.append(a - pad), e.append(b + pad)
    return np.array(s, dtype=np.int64), np.array(e, dtype=np.int64)


def domain_options(path):
    return ["--domains-at", path, "--domains-size", str(R), "--domains-flank-percent", str(PERCENT), "--domains-resolution",
            str(RES)]


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("domains"))


@pytest.fixture(scope="module")
def bed(workdir):
    path = os.path.join(workdir, "tads.bed")
    return path, bed_file(path)


@pytest.fixture(scope="module")
def one(workdir, bed):
    return ranks.simulate(workdir, "one", 1, 0, OPTIONS + domain_options(bed[0]))


def test_the_blocks_of_the_file_are_the_api_s_results(one, bed):
    prefix, _, stderr = one
    path, triple = bed
    assert ranks.files_of(prefix) == ["run.cool", "run_domains.tsv"]
    assert "run_domains.tsv" in stderr.splitlines()[-2]  # written last, before `done`
    observed, area, terms, placed, used = [0] * (R * R), [0] * (R * R), [[] for _ in range(R * R)], 0, 0
    with cooler.CoolerReader(prefix + ".cool") as reader, api.LoadedBands(0) as bands:
        assert reader.bin_size == BASE
        for name in ("chrA", "chrC"):  # plan order; chrB has no barriers and is skipped
            ncols = -(-CHROMS[name] // BASE)
            b1, b2, cn, first = reader.pixels(name)
            bid, st = bands.load_pixels(b1, b2, cn, NROWS, ncols, first)
            assert st.n_in == len(cn) > 0
            s, e = windows_of(path, name)
            pile, ar, n_used, hist = bands.rescaled_pileup(bid, s, e, R, factor=RES // BASE, first_bin=0)
            # the restatement, on the band at twice the bin size
            band = np.zeros(NROWS * ncols + 1, dtype=np.uint32)
            band[(b2 - first) * NROWS + (b2 - b1)] = cn
            coarse, nr, nc = reference_coarsen(band, NROWS, ncols, RES // BASE, 0)
            assert nr == 21
            want, want_area, want_used = rescale_blocks(coarse, nr, nc, R, s, e)
            assert n_used == want_used and np.array_equal(pile, want) and np.array_equal(ar, want_area)
            assert np.array_equal(hist, np.bincount((e - s)[(s >= 0) & (e - s <= nr)], minlength=nr + 1))
            diag_sum = bands.marginals(bid, 0, RES // BASE, 0)[0]
            placed += len(s)
            used += n_used
            for q in range(R * R):
                observed[q] += int(pile.reshape(-1)[q])
                area[q] += int(ar.reshape(-1)[q])
            for q, t in enumerate(api.rescaled_expected_terms(hist, diag_sum, nc, R)):
                terms[q] += t
    assert (placed + 2, placed, used) == triple
    expected = [math.fsum(t) for t in terms]
    strength = api.domain_strength(np.array(observed, dtype=object).reshape(R, R), np.array(expected).reshape(R, R), R, PERCENT)
    print(f"strength {strength!r}")
    assert strength > 0 and sum(observed) > 0 and min(area) > 0
    want = [driver.domains_header(path, RES, R, PERCENT, *triple, strength)] + driver.domains_lines(R, observed, area, expected)
    with open(prefix + "_domains.tsv") as fh:
        got = fh.readlines()
    assert len(got) == 1 + R * R and got[0] == want[0]
    assert got == want
    assert f"--domains-at {path}: 2 domains lie in no simulated interval" in stderr


def test_analyze_of_the_run_s_cooler_writes_the_file_byte_for_byte(one, bed, workdir):
    prefix = one[0]
    out = os.path.join(workdir, "an", "run")
    analyze([prefix + ".cool", "-o", out, "-w", ranks.DIAGONAL_WIDTH] + domain_options(bed[0]))
    assert ranks.files_of(out) == ["run.cool", "run_domains.tsv"]
    with open(prefix + "_domains.tsv", "rb") as a, open(out + "_domains.tsv", "rb") as b:
        single = a.read()
        assert b.read() == single and len(single) > 500


def test_a_run_without_the_option_writes_no_such_file(workdir, one):
    plain = ranks.simulate(workdir, "plain", 1, 0, OPTIONS)[0]
    assert ranks.files_of(plain) == ["run.cool"]
