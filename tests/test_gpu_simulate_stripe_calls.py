"""`simulate --call-stripes` end to end, on the genome, the cell count and the options of
tests/test_gpu_simulate_ranks.py: every row of <prefix>_stripe_calls.bedpe is re-derived from the .cool the same
run wrote, loaded into a band on the device and called through api.LoadedBands.call_stripes; `analyze` of the
run's cooler with the same options writes the file byte for byte; and a profile that does not add up to the
diagonals ends the output stage before a row is written.  Each run is a fresh child process, made once per
module; one process has the GPU open at a time besides this one."""
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_simulate_ranks as ranks
from test_gpu_simulate_marginals import CHROMS, SIMULATED
from test_gpu_simulate_stripes import BASE, BASIC, NROWS, band_pixels

from modle_amd import api, cli, driver

pytestmark = pytest.mark.gpu

# 10, 20 and 30 bins, a flank of 3: 33 of the 40 diagonals; the fold and the count are low enough for 5 cells
CALLS = cli.StripeCalls(None, BASE, [50_000, 100_000, 150_000], 15_000, BASE, 1.25, 4, 3, 15_000)
OPTIONS = ["--call-stripes", "--call-stripes-lengths", "50kb,100kb,150kb", "--call-stripes-flank", "15kb",
           "--call-stripes-fold", "1.25", "--call-stripes-min-count", "4"]


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("stripe_calls"))


@pytest.fixture(scope="module")
def one(workdir):
    return ranks.simulate(workdir, "one", 1, 0, BASIC + OPTIONS)[0]


def load(lb, cool, name):
    import torch

    (_, _, _, _, ncols), band = band_pixels(cool, name, NROWS)
    return lb.add_band(torch.from_numpy(band.view(np.int32)).to("cuda:0"), NROWS, ncols), ncols


def test_every_row_is_derived_again_from_the_cooler(one):
    assert ranks.files_of(one) == ["run.cool", "run_stripe_calls.bedpe"]
    m, h, lengths, d0, radius = driver.stripe_calls_bins(CALLS)
    assert (m, h, lengths, d0, radius) == (3, 0, [10, 20, 30], 3, 3)
    want = driver.stripe_calls_header(CALLS).splitlines(keepends=True)
    directions = set()
    with api.LoadedBands(0) as lb:
        for name in SIMULATED:  # plan order; chrB has no barrier and no pixel
            bid, ncols = load(lb, one + ".cool", name)
            rows = lb.call_stripes(bid, m, lengths, d0, h, CALLS.fold, CALLS.min_count, radius)
            assert rows and all(r.centre >= 4 and r.enrichment >= 1.25 and m <= r.bin < ncols - m for r in rows)
            directions |= {r.direction for r in rows}
            iv = {"name": name, "start": 0, "end": dict(CHROMS)[name]}
            want += driver.stripe_calls_lines(iv, BASE, 1, h, d0, rows)
    assert directions == {0, 1}
    with open(one + "_stripe_calls.bedpe") as fh:
        got = fh.readlines()
    assert got == want and len(got) > 2 + 4
    for line in got[2:]:
        chrom, lo1, hi1, chrom2, lo2, hi2, direction, length = line.split("\t")[:8]
        assert chrom == chrom2 and int(hi1) - int(lo1) == BASE and int(length) in CALLS.lengths
        # the extent lies before the anchor of a stripe that runs upstream, behind it downstream
        assert (int(hi2) == int(lo1) - 2 * BASE) if direction == "up" else (int(lo2) == int(hi1) + 2 * BASE)
        assert int(hi2) - int(lo2) == int(length) - 3 * BASE


def test_analyze_of_the_run_s_cooler_writes_the_same_file(workdir, one):
    prefix = os.path.join(workdir, "analyzed", "run")
    p = subprocess.run([sys.executable, "-m", "modle_amd", "analyze", one + ".cool", "-o", prefix, "-w",
                        ranks.DIAGONAL_WIDTH, *OPTIONS], cwd=ranks.ROOT, capture_output=True, text=True, timeout=300,
                       env={k: v for k, v in os.environ.items() if k not in ("MODLE_HIP_LIB", "MODLE_PIXELS_LIB")})
    assert p.returncode == 0, p.stderr[-3000:]
    assert "run_stripe_calls.bedpe" in ranks.files_of(prefix)
    with open(prefix + "_stripe_calls.bedpe", "rb") as a, open(one + "_stripe_calls.bedpe", "rb") as b:
        theirs = b.read()
        assert a.read() == theirs and len(theirs) > 500


def test_a_band_too_narrow_ends_the_run_before_the_launch(workdir):
    os.makedirs(os.path.join(workdir, "in"), exist_ok=True)
    sizes, bed = ranks.genome_files(os.path.join(workdir, "in"))
    prefix = os.path.join(workdir, "misfit", "run")
    options = BASIC + ["--call-stripes", "--call-stripes-lengths", "50kb,190kb", "--call-stripes-flank", "15kb"]
    p = subprocess.run([sys.executable, "-m", "modle_amd", "simulate", "-c", sizes, "-b", bed, "-o", prefix,
                        *ranks.COMMON, *options], cwd=ranks.ROOT, capture_output=True, text=True, timeout=120,
                       env={k: v for k, v in os.environ.items() if k not in ("MODLE_HIP_LIB", "MODLE_PIXELS_LIB")})
    assert p.returncode != 0
    last = p.stderr.strip().splitlines()[-1]
    assert last == ("--call-stripes-lengths: the length of 190000 with the flank of 15000 needs 41 diagonals of 5000, the "
                    "band of chrA:0-2000000 has 40: widen the band with -w"), p.stderr[-2000:]
    assert "simulating" not in p.stderr and "simulation kernel" not in p.stderr
    assert not ranks.files_of(prefix)  # no file


def test_a_tampered_sum_fails_loudly_before_a_row_is_written(one, tmp_path, monkeypatch):
    name = SIMULATED[0]
    calls = CALLS._replace(path=str(tmp_path / "t_stripe_calls.bedpe"))
    with api.LoadedBands(0) as lb:
        bid, ncols = load(lb, one + ".cool", name)
        plan = [{"interval": {"name": name, "start": 0, "end": dict(CHROMS)[name]}, "nrows": NROWS, "ncols": ncols,
                 "skipped": False}]

        def marginals(k, factor, first_bin):
            return lb.marginals(bid, 0, factor, first_bin)

        shared = (lb, api.make_config(bin_size=BASE), plan, [bid], {}, marginals, lambda _: None)
        driver.stripe_calls_file(*shared, calls)  # as it is, the file is the run's part for this chromosome
        with open(calls.path) as fh, open(one + "_stripe_calls.bedpe") as run:
            mine = fh.readlines()
            assert len(mine) > 3 and mine == run.readlines()[:len(mine)]
        os.remove(calls.path)
        true_profiles = lb.stripe_profiles

        def tampered(*args, **kw):
            prof, n_valid = true_profiles(*args, **kw)
            prof[1, 2, 3, ncols // 2] += np.uint64(1)  # one contact more in one word of one centre
            return prof, n_valid

        monkeypatch.setattr(lb, "stripe_profiles", tampered)
        with pytest.raises(RuntimeError) as e:
            driver.stripe_calls_file(*shared, calls)
        assert str(e.value).startswith(f"{name}:0-{dict(CHROMS)[name]}: the downstream profiles of length 30 at offset 0 add up to")
        assert open(calls.path).read() == driver.stripe_calls_header(calls)  # the header, and no row
