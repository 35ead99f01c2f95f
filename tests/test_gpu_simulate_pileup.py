"""`simulate --pileup-at` end to end, on the genome, the cell count and the dots options of
tests/test_gpu_simulate_dots.py: every header and every row of <prefix>_pileup.tsv is what the restatement
of tests/test_pileup_outputs.py computes from the pixel table read back out of the .mcool the same run
wrote, around the rows of the run's own <prefix>_dots.bedpe, around the barriers of the genome and around
the pairs of a small BEDPE file written here; a flank that does not fit the band ends the run before
anything is simulated; a run without the option writes no such file; and two ranks that share this GPU
(--dist-backend gloo) write the file byte for byte as the single rank does.  Each run is a fresh child
process, made once per module; at most two processes have the GPU open at a time."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_simulate_dots as dots
import test_gpu_simulate_ranks as ranks
from test_gpu_marginals import reference_marginals
from test_gpu_simulate_marginals import CHROMS, SIMULATED, pixels_of
from test_pileup_outputs import reference_accepts, reference_pileup

from modle_amd import api, driver

pytestmark = pytest.mark.gpu

BASE, NROWS = dots.BASE, dots.NROWS  # 5 kb, -w 200kb: 40 diagonals
F = 5                                # --pileup-flank 25kb: windows of 11 x 11, anchors up to d = 29
CORNER = 1                           # the default: max(1, 5 // 3) bins


def barrier_positions(name):
    """the midpoints of the barriers ranks.genome_files writes: (start + end + 1) / 2 of p .. p + 19"""
    first, step, n = {"chrA": (41_000, 80_000, 24), "chrC": (63_000, 83_000, 17)}[name]
    return [first + i * step + (i * 37 % 11) * 1000 + 10 for i in range(n)]


def bedpe_file(path):
    """ten pairs of neighbouring barriers (one per chromosome listed right side first), then a trans pair, a
    pair on the chromosome that is not simulated, a pair 60 bins apart, whose window leaves the band, and a
    pair whose window leaves the matrix on the left: (given, placed, used) = (14, 12, 10)"""
    rows = ["#chrom1\tstart1\tend1\tchrom2\tstart2\tend2\n"]
    for name, count in (("chrA", 6), ("chrC", 4)):
        pos = barrier_positions(name)
        for i in range(count):
            left, right = (name, pos[2 * i] - 500, pos[2 * i] + 500), (name, pos[2 * i + 1] - 2000, pos[2 * i + 1] + 1000)
            if i == 1:
                left, right = right, left
            rows.append("\t".join(map(str, left + right)) + "\tloop\n")
    rows += ["# what is not used\n", "chrA\t100000\t105000\tchrC\t400000\t405000\n", "chrB\t100000\t105000\tchrB\t200000\t205000\n",
             "chrA\t100000\t105000\tchrA\t400000\t405000\n", "chrA\t5000\t10000\tchrA\t50000\t55000\n"]
    with open(path, "w") as fh:
        fh.writelines(rows)
    return 14, 12, 10


def bedpe_anchors(path, name):
    """the columns of the cis pairs of `name`, restated: midpoints, bins of 5 kb (the intervals are whole
    chromosomes), a <= b"""
    a, b = [], []
    for line in open(path):
        if line.startswith("#"):
            continue
        c = line.split("\t")
        if c[0] == c[3] == name:
            x, y = sorted(((int(c[1]) + int(c[2])) // 2 // BASE, (int(c[4]) + int(c[5])) // 2 // BASE))
            a.append(x), b.append(y)
    return np.array(a, dtype=np.int64), np.array(b, dtype=np.int64)


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("pileup"))


@pytest.fixture(scope="module")
def bedpe(workdir):
    path = os.path.join(workdir, "loops.bedpe")
    return path, bedpe_file(path)


def options(path):
    return dots.OPTIONS + ["--pileup-at", "dots", "--pileup-at", "barriers", "--pileup-at", path, "--pileup-flank", "25kb"]


@pytest.fixture(scope="module")
def one(workdir, bedpe):
    return ranks.simulate(workdir, "one", 1, 0, options(bedpe[0]))


@pytest.fixture(scope="module")
def two(workdir, bedpe, one):  # (after the single-rank run has ended)
    return ranks.simulate(workdir, "two", 2, ranks.PORT + 6, options(bedpe[0]))[0]


def test_the_files_of_the_run(one):
    assert ranks.files_of(one[0]) == ["run.mcool", "run_dots.bedpe", "run_pileup.tsv"]
    assert "run_pileup.tsv" in one[2].splitlines()[-2]  # written last, before `done`


def test_every_header_and_row_of_the_file_is_the_restatement(one, bedpe):
    """with the asked flank of 25 kb = 5 bins the windows reach d + 10 <= 39: of the 141 dots of the dots test
    137 are used, and all 41 barriers (printed by the test); at least 10 of each are asserted"""
    prefix, _, stderr = one
    path, triple = bedpe
    level = pixels_of(prefix + ".mcool", BASE)
    dot_rows = [l.split("\t") for l in open(prefix + "_dots.bedpe") if not l.startswith("#")]
    assert len(dot_rows) >= 10
    want, counts = [], {}
    for source in ("dots", "barriers", path):
        observed, terms, given, used = [0] * (2 * F + 1) ** 2, [[] for _ in range((2 * F + 1) ** 2)], 0, 0
        for name in SIMULATED:  # plan order
            ncols, b1, b2, cn = level[name]
            assert ncols == -(-dict(CHROMS)[name] // BASE)
            band = np.zeros(NROWS * ncols + 1, dtype=np.uint32)
            band[b2 * NROWS + (b2 - b1)] = cn
            if source == "dots":
                a = np.array([int(r[1]) // BASE for r in dot_rows if r[0] == name], dtype=np.int64)
                b = np.array([int(r[4]) // BASE for r in dot_rows if r[0] == name], dtype=np.int64)
            elif source == "barriers":
                a = b = np.array(sorted(p // BASE for p in barrier_positions(name)), dtype=np.int64)
            else:
                a, b = bedpe_anchors(path, name)
            given += len(a)
            pile, n_used = reference_pileup(band, NROWS, ncols, F, a, b)
            ok = reference_accepts(NROWS, ncols, F, a, b)
            hist = np.bincount((b - a)[ok], minlength=NROWS)
            diag_sum = reference_marginals(band, NROWS, ncols, 0)[0]
            used += n_used
            for q in range(len(observed)):
                r, c = divmod(q, 2 * F + 1)
                observed[q] += int(pile[r, c])
                terms[q] += [float(int(hist[d])) * (float(int(diag_sum[abs(d + c - r)])) / float(ncols - abs(d + c - r)))
                             for d in range(NROWS) if hist[d]]
            if source == "barriers":  # the centre is the barriers' own diagonal pixels
                assert int(pile[F, F]) == sum(int(band[x * NROWS]) for x in a[ok])
        placed = given
        if source == path:
            given += 2  # the trans pair and the pair on chrB
        counts[source] = (given, placed, used)
        scores = api.apa_scores(np.array(observed, dtype=np.float64).reshape(2 * F + 1, 2 * F + 1), CORNER)
        want.append(driver.pileup_header(source, BASE, F * BASE, CORNER * BASE, given, placed, used, scores))
        want += driver.pileup_lines(source, BASE, F * BASE, observed, [math.fsum(t) for t in terms])
        assert sum(observed) > 0 and scores["peak"] > 0
    print(f"(given, placed, used): {counts}")
    assert counts["dots"][2] >= 10 and counts["barriers"][2] >= 10
    assert counts["dots"][0] == counts["dots"][1] == len(dot_rows) and counts["barriers"][:2] == (41, 41)
    assert counts[path] == triple
    with open(prefix + "_pileup.tsv") as fh:
        got = fh.readlines()
    assert len(got) == 3 * (1 + (2 * F + 1) ** 2)
    assert [l for l in got if l.startswith("#")] == [l for l in want if l.startswith("#")]
    assert got == want
    assert f"--pileup-at {path}: 2 pairs are not placed (1 between two chromosomes, 1 in no simulated interval)" in stderr


def test_a_flank_that_does_not_fit_ends_the_run_before_the_launch(workdir):
    os.makedirs(os.path.join(workdir, "in"), exist_ok=True)
    sizes, bed = ranks.genome_files(os.path.join(workdir, "in"))
    prefix = os.path.join(workdir, "misfit", "run")
    extra = dots.BASIC + ["--pileup-at", "barriers", "--pileup-flank", "100kb"]  # 2 * 20 + 1 > 40
    p = subprocess.run([sys.executable, "-m", "modle_amd", "simulate", "-c", sizes, "-b", bed, "-o", prefix,
                        *ranks.COMMON, *extra], cwd=ranks.ROOT, capture_output=True, text=True, timeout=120,
                       env={k: v for k, v in os.environ.items() if k not in ("MODLE_HIP_LIB", "MODLE_PIXELS_LIB")})
    assert p.returncode != 0
    last = p.stderr.strip().splitlines()[-1]
    assert last == ("--pileup-flank: the flank of 100000 (20 bins of 5000) does not fit the band of chrA:0-2000000 "
                    "(40 diagonals): the largest flank that fits is 95000 (19 bins)"), p.stderr[-2000:]
    assert "simulating" not in p.stderr and "simulation kernel" not in p.stderr
    assert not ranks.files_of(prefix)  # no file


def test_a_run_without_the_option_writes_no_such_file(workdir, one):
    plain = ranks.simulate(workdir, "plain", 1, 0, dots.OPTIONS)[0]
    assert ranks.files_of(plain) == ["run.mcool", "run_dots.bedpe"]
    with open(plain + "_dots.bedpe", "rb") as a, open(one[0] + "_dots.bedpe", "rb") as b:
        assert a.read() == b.read()  # the pileup leaves the dots as they were


def test_two_ranks_write_the_file_byte_for_byte(one, two):
    assert ranks.files_of(two) == ["run.mcool", "run_dots.bedpe", "run_pileup.tsv"]
    with open(one[0] + "_pileup.tsv", "rb") as a, open(two + "_pileup.tsv", "rb") as b:
        single = a.read()
        assert b.read() == single and len(single) > 5000
