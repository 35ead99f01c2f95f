"""`simulate --call-domains --domains-at called` end to end, on the genome, the cell count and the options of
tests/test_gpu_simulate_ranks.py (a small genome with barriers): the run writes <prefix>_domain_calls.bed and,
from the domains it has just called, <prefix>_domains.tsv; `analyze` of the run's cooler with the same options
writes both byte for byte; the domains are disjoint, inside their chromosome and within the width limits; and the
score and the strength of every row are recomputed on the host from the triangle sums of the band the .cool
holds.  Each run is a fresh child process, made once per module; one process has the GPU open at a time besides
this one."""
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_simulate_ranks as ranks
from test_gpu_simulate_marginals import CHROMS, SIMULATED
from test_gpu_simulate_stripes import BASE, BASIC, NROWS, band_pixels

from modle_amd import api, cli, driver, pixels

pytestmark = pytest.mark.gpu

# the defaults: 2 Mb, which the band of 40 diagonals clamps to 40 bins; 3 bins; gamma 1; two diagonals ignored
CALLS = cli.DomainCalls(None, BASE, 2_000_000, 3 * BASE, 1.0, 2)
OPTIONS = ["--call-domains", "--domains-at", "called", "--domains-size", "10", "--insulation-windows", "25kb,50kb"]


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("domain_calls"))


@pytest.fixture(scope="module")
def one(workdir):
    return ranks.simulate(workdir, "one", 1, 0, BASIC + OPTIONS)[0]


def load(lb, cool, name):
    import torch

    (_, _, _, _, ncols), band = band_pixels(cool, name, NROWS)
    return lb.add_band(torch.from_numpy(band.view(np.int32)).to("cuda:0"), NROWS, ncols), ncols


def test_both_files_are_written_and_every_row_is_derived_again_from_the_cooler(one):
    assert ranks.files_of(one) == ["run.cool", "run_domain_calls.bed", "run_domains.tsv", "run_insulation.tsv"]
    width, least, d0 = driver.domain_calls_bins(CALLS)
    assert (width, least, d0) == (400, 3, 2)
    with open(one + "_domain_calls.bed") as fh:
        got = fh.readlines()
    assert "".join(got[:2]) == driver.domain_calls_header(CALLS)
    want = got[:2]
    with api.LoadedBands(0) as lb:
        for name in SIMULATED:  # plan order; chrB has no barrier and no pixel
            bid, ncols = load(lb, one + ".cool", name)
            size = dict(CHROMS)[name]
            table = lb.triangle_sums(bid, NROWS, d0)  # the largest width, clamped to the band
            rows = lb.call_domains(bid, NROWS, d0)
            assert len(rows) >= 3
            iv = {"name": name, "start": 0, "end": size}
            lines = driver.domain_calls_lines(iv, BASE, 1, rows)
            want += lines
            # disjoint, inside the chromosome, within the width limits
            last = 0
            for r, line in zip(rows, lines):
                assert last <= r.start < r.end <= ncols and least <= r.width == r.end - r.start <= NROWS
                last = r.end
                chrom, lo, hi, label, score, strength = line.rstrip("\n").split("\t")
                assert chrom == name and 0 <= int(lo) == r.start * BASE < int(hi) == min(r.end * BASE, size)
                assert label == f"{name}:{lo}-{hi}"
                # the score and the strength again, from the table, in the order the decision fixes
                k, n = r.width - 1, ncols - r.width + 1
                total = sum(int(x) for x in table[k, :n])
                mu = total / n
                t = float(int(table[k, r.start]))
                assert score == "%.17g" % (t - 1.0 * mu) and strength == "%.17g" % (t / mu)
                assert float(score) > 0 and float(strength) > 1
    assert got == want and len(got) > 2 + 6
    # the average domain is that of the domains just called: every one is given, placed and used or refused
    cols = [line.split("\t") for line in got[2:]]
    assert driver.read_bed(one + "_domain_calls.bed") == [(c[0], int(c[1]), int(c[2])) for c in cols]
    with open(one + "_domains.tsv") as fh:
        head = fh.readline()
    fields = dict(f.split("=") for f in head[1:].rstrip("\n").split("\t"))
    assert fields["source"] == "called" and int(fields["given"]) == len(got) - 2 == int(fields["placed"])
    assert int(fields["used"]) <= int(fields["placed"])


def test_analyze_of_the_run_s_cooler_writes_the_same_files(workdir, one):
    prefix = os.path.join(workdir, "analyzed", "run")
    p = subprocess.run([sys.executable, "-m", "modle_amd", "analyze", one + ".cool", "-o", prefix, "-w",
                        ranks.DIAGONAL_WIDTH, *OPTIONS], cwd=ranks.ROOT, capture_output=True, text=True, timeout=300,
                       env={k: v for k, v in os.environ.items() if k not in ("MODLE_HIP_LIB", "MODLE_PIXELS_LIB")})
    assert p.returncode == 0, p.stderr[-3000:]
    assert {"run_domain_calls.bed", "run_domains.tsv"} <= set(ranks.files_of(prefix))
    for tail, least in (("_domain_calls.bed", 300), ("_domains.tsv", 1000)):
        with open(prefix + tail, "rb") as a, open(one + tail, "rb") as b:
            theirs = b.read()
            assert a.read() == theirs and len(theirs) > least, tail


def test_a_tampered_word_fails_loudly_before_a_row_is_written(one, tmp_path, monkeypatch):
    name = SIMULATED[0]
    calls = CALLS._replace(path=str(tmp_path / "t_domain_calls.bed"))
    with api.LoadedBands(0) as lb:
        bid, ncols = load(lb, one + ".cool", name)
        plan = [{"interval": {"name": name, "start": 0, "end": dict(CHROMS)[name]}, "nrows": NROWS, "ncols": ncols,
                 "skipped": False}]

        def marginals(k, factor, first_bin):
            return lb.marginals(bid, 0, factor, first_bin)

        shared = (lb, api.make_config(bin_size=BASE), plan, [bid], {}, marginals, lambda _: None)
        driver.domain_calls_file(*shared, calls)  # as it is, the file is the run's part for this chromosome
        with open(calls.path) as fh, open(one + "_domain_calls.bed") as run:
            mine = fh.readlines()
            assert len(mine) > 3 and mine == run.readlines()[:len(mine)]
        os.remove(calls.path)
        true_sums = lb.triangle_sums

        def tampered(*args, **kw):
            table = true_sums(*args, **kw)
            table[17, ncols // 2] += np.uint64(1)  # one contact more in one window
            return table

        monkeypatch.setattr(lb, "triangle_sums", tampered)
        with pytest.raises(RuntimeError) as e:
            driver.domain_calls_file(*shared, calls)
        assert str(e.value).startswith(f"{name}:0-{dict(CHROMS)[name]}: the windows of 18 bins hold ")
        assert open(calls.path).read() == driver.domain_calls_header(calls)  # the header, and no row
    assert pixels.DOMAIN_MIN_WIDTH == 3
