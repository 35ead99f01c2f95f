"""`python -m modle_amd analyze` on the MI355X: the analyses of a file are the analyses of the band it was
written from.  One `simulate` with every analysis at once writes its files; `analyze` of the run's .mcool at the
base resolution, with the same options, must write the same files: the texts byte for byte, the arrays and the
coolers (read with cooler.CoolerReader) entry for entry.  A second file, which the simulator cannot write -- wider
than the band that is loaded -- is held against the restatement of tests/test_band_outputs.py.  Every run is a
fresh child process, one at a time; nothing here has a tolerance."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_simulate_dots as dots
import test_gpu_simulate_insulation as insulation
import test_gpu_simulate_marginals as marginals
import test_gpu_simulate_ranks as ranks
from test_band_outputs import reference_band
from test_cooler_pixels import random_band
from test_gpu_marginals import reference_marginals
from test_gpu_simulate_pileup import bedpe_file

from modle_amd import api, cooler

pytestmark = pytest.mark.gpu

ROOT = ranks.ROOT
SEED = ranks.COMMON[ranks.COMMON.index("--seed") + 1]
RESOLUTIONS = [5000, 10000, 25000]
TEXTS = ["_expected.tsv", "_coverage.bedgraph", "_insulation.tsv", "_dots.bedpe", "_pileup.tsv"]
LOG = re.compile(r"^(\S+): (\d+) pixels in the band \((\d+) contacts\), beyond the band (\d+) pixels \((\d+) contacts\), "
                 r"outside (\d+) pixels \((\d+) contacts\)$")


def analysis_options(bedpe):
    """the options of the existing test_gpu_simulate_* modules, all at once (without their --ncells and
    --mcool-resolutions, which differ between them, and without --pileup-at barriers, which a file cannot serve)"""
    own = lambda opts, basic: [o for o in opts[len(basic):]]
    return (["--mcool-resolutions", "10kb,25kb", "--expected", "--coverage", "--coverage-ignore-diags",
             str(marginals.MIN_DIAG)] + own(insulation.OPTIONS, insulation.BASIC) + own(dots.OPTIONS, dots.BASIC) +
            ["--subsample-frac", "0.5", "--subsample-split", "--pileup-at", "dots", "--pileup-at", bedpe,
             "--pileup-flank", "25kb", "--dense-region", "chrC:200kb-900kb", "--dense-region", "chrA"])


def analyze(args, expect_ok=True):
    if ranks._failed:
        pytest.fail(f"not started: the run {ranks._failed[0]} failed before")
    env = {k: v for k, v in os.environ.items() if k not in ("MODLE_HIP_LIB", "MODLE_PIXELS_LIB")}
    try:
        p = subprocess.run([sys.executable, "-m", "modle_amd", "analyze", *args], cwd=ROOT, env=env,
                           capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        ranks._failed.append("analyze")
        raise
    if expect_ok and p.returncode != 0:
        ranks._failed.append("analyze")
    assert (p.returncode == 0) == expect_ok, f"exit code {p.returncode}\n{p.stderr[-3000:]}"
    return p


def assert_same_coolers(path_a, path_b, bin_sizes):
    for b in bin_sizes:
        group = f"::/resolutions/{b}" if len(bin_sizes) > 1 else ""
        with cooler.CoolerReader(path_a + group) as ra, cooler.CoolerReader(path_b + group) as rb:
            assert ra.bin_size == rb.bin_size == b and ra.chroms == rb.chroms
            assert ra.chrom_offset == rb.chrom_offset and np.array_equal(ra.bin1_offset(), rb.bin1_offset())
            n = 0
            for name, _ in ra.chroms:
                pa, pb = ra.pixels(name), rb.pixels(name)
                assert pa[3] == pb[3] and all(np.array_equal(x, y) for x, y in zip(pa[:3], pb[:3])), (path_a, b, name)
                assert name != "chrB" or len(pa[0]) == 0
                n += len(pa[0])
            assert n > 0, (path_a, b)


def test_analyze_of_a_run_s_mcool_is_the_run_s_analysis(tmp_path):
    d = str(tmp_path)
    bedpe = os.path.join(d, "loops.bedpe")
    bedpe_file(bedpe)
    options = analysis_options(bedpe)
    sim, _, _ = ranks.simulate(d, "sim", 1, 0, ["--ncells", str(ranks.NCELLS), "--no-track-1d-lef-position"] + options)
    out = os.path.join(d, "an", "run")
    p = analyze([f"{sim}.mcool::/resolutions/5000", "-o", out, "-w", ranks.DIAGONAL_WIDTH, "--subsample-seed", SEED]
                + options)
    assert sorted(os.listdir(os.path.dirname(out))) == sorted(os.listdir(os.path.dirname(sim)))
    for tail in TEXTS:
        a, b = open(sim + tail, "rb").read(), open(out + tail, "rb").read()
        assert a == b and len(a) > 200, tail
        # (the pileup is one pile per source: it names no chromosome)
        assert b"chrB" not in b and (tail == "_pileup.tsv" or (b"chrA" in b and b"chrC" in b)), tail
    with np.load(sim + "_dense.npz") as za, np.load(out + "_dense.npz") as zb:
        assert sorted(za.files) == sorted(zb.files) and len(za.files) == 2
        for key in za.files:
            assert za[key].dtype == zb[key].dtype and np.array_equal(za[key], zb[key]) and za[key].any(), key
    for tail in (".mcool", "_sampled.mcool", "_sampled_rest.mcool"):
        assert_same_coolers(sim + tail, out + tail, RESOLUTIONS)
    # the file holds what the band held: nothing beyond it, nothing outside
    lines = [LOG.match(l) for l in p.stderr.splitlines()]
    seen = {m.group(1): [int(x) for x in m.groups()[1:]] for m in lines if m}
    assert sorted(seen) == ["chrA", "chrB", "chrC"] and seen["chrB"] == [0] * 6
    for name in ("chrA", "chrC"):
        assert seen[name][0] > 0 and seen[name][2:] == [0] * 4
    # a second run onto the same prefix is refused without --force, and nothing changes
    before = {f: os.path.getmtime(os.path.join(os.path.dirname(out), f)) for f in os.listdir(os.path.dirname(out))}
    q = analyze([f"{sim}.mcool::/resolutions/5000", "-o", out, "-w", ranks.DIAGONAL_WIDTH, "--expected"], expect_ok=False)
    assert "refusing to overwrite" in q.stderr
    assert before == {f: os.path.getmtime(os.path.join(os.path.dirname(out), f)) for f in os.listdir(os.path.dirname(out))}


CHROMS = [("chrA", 1_003_000), ("chrQuiet", 42_000), ("chrB", 600_000)]
WIDE = {"chrA": (60, 201, 0.3), "chrB": (45, 120, 0.5)}  # nrows, ncols, density: wider than -w 100kb (20 diagonals)


def test_a_file_wider_than_the_band(tmp_path):
    rng = np.random.default_rng(5)
    src, out = str(tmp_path / "wide.cool"), str(tmp_path / "out" / "run")
    with cooler.CoolerWriter(src, CHROMS, 5000) as w:
        for name, (nrows, ncols, density) in WIDE.items():
            w.append(name, random_band(rng, nrows, ncols, density), nrows, ncols)
    p = analyze([src, "-o", out, "-w", "100kb", "--expected"])
    cfg = api.make_config(bin_size=5000, diagonal_width=100_000)
    seen = {m.group(1): [int(x) for x in m.groups()[1:]] for m in map(LOG.match, p.stderr.splitlines()) if m}
    assert sorted(seen) == ["chrA", "chrB", "chrQuiet"] and seen["chrQuiet"] == [0] * 6
    rows = [l.rstrip("\n").split("\t") for l in open(out + "_expected.tsv")][1:]
    with cooler.CoolerReader(src) as r, cooler.CoolerReader(out + ".cool") as got:
        assert got.chroms == CHROMS and got.bin_size == 5000 and len(got.pixels("chrQuiet")[0]) == 0
        for name, size in CHROMS:
            if name == "chrQuiet":
                continue
            nrows, ncols = api.matrix_shape(cfg, size)
            assert (nrows, ncols) == (20, WIDE[name][1])
            b1, b2, cn, b0 = r.pixels(name)
            band, st = reference_band(nrows, ncols, b1, b2, cn, b0)
            assert st["n_beyond"] > 0 and st["first_bad"] == -1
            assert seen[name] == [st["n_in"], st["sum_in"], st["n_beyond"], st["sum_beyond"], st["n_outside"],
                                  st["sum_outside"]]
            diag_sum, _ = reference_marginals(band, nrows, ncols, 0)
            mine = [c for c in rows if c[0] == name]
            assert [int(c[4]) for c in mine] == list(range(nrows))
            assert [int(c[7]) for c in mine] == [int(x) for x in diag_sum]
            assert [int(c[6]) for c in mine] == [ncols - d for d in range(nrows)]
            # the rewritten cooler holds exactly the in-pixels
            i, j = b1 - b0, b2 - b0
            keep = (j - i < nrows) & (j < ncols)
            g1, g2, gc, g0 = got.pixels(name)
            assert g0 == b0 and np.array_equal(g1, b1[keep]) and np.array_equal(g2, b2[keep]) and \
                np.array_equal(gc, cn[keep])
    assert not any(c[0] == "chrQuiet" for c in rows)


def test_a_list_out_of_order_names_the_file_the_chromosome_and_the_pixel(tmp_path):
    """api.LoadedBands on a list with a duplicate, the way cli.load_bands reports it"""
    from modle_amd import cli, pixels

    class Reader:
        uri = "broken.cool"

        def pixels(self, name):
            return (np.array([3, 3, 4], dtype=np.int64), np.array([3, 3, 5], dtype=np.int64),
                    np.array([1, 1, 1], dtype=np.int32), 0)

    plan = [{"interval": {"name": "chrZ"}, "nrows": 4, "ncols": 9, "skipped": False}]
    with api.LoadedBands(0) as bands:
        with pytest.raises(SystemExit) as e:
            cli.load_bands(bands, Reader(), plan, lambda *a: None)
    assert "broken.cool: chromosome chrZ: pixel 1 of its 3" in str(e.value)
    assert pixels.ERR_ORDER == -4
