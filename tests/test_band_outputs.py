"""Pixels to band without a GPU: the numpy / Python-int restatement of the definition in include/modle_pixels.h
(reference_classes, reference_band, reference_order: they share no code with the library and serve the GPU tests
as well), modle_pixels_band_classify against it, the cooler reader of include/modle_cooler_read.h against the
writers and against modle_cool_read_band, and the refusals of `python -m modle_amd analyze` that need no device.
Everything is exact integers; nothing has a tolerance."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from modle_amd import cooler, evaluate, pixels
from test_cooler_pixels import H5PY_PYTHON, random_band, reference_pixels
from test_gpu_marginals import reference_coarsen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64_MIN, I64_MAX = -2**63, 2**63 - 1
IN, BEYOND, OUTSIDE = 0, 1, 2
OK, ERR_RANGE, ERR_ORDER = 0, -3, -4


def reference_classes(nrows, ncols, bin1, bin2, bin_offset=0):
    """IN: 0 <= i <= j < ncols and j - i < nrows; BEYOND: 0 <= i <= j < ncols and j - i >= nrows; OUTSIDE: the rest
    -- in Python ints, which cannot overflow"""
    out = []
    for a, b in zip(np.asarray(bin1).tolist(), np.asarray(bin2).tolist()):
        i, j = a - int(bin_offset), b - int(bin_offset)
        out.append((IN if j - i < nrows else BEYOND) if 0 <= i <= j < ncols else OUTSIDE)
    return np.array(out, dtype=np.uint8)


def reference_order(bin1, bin2, count):
    """(code, first_bad): the smallest index whose pixel is not after its predecessor (ERR_ORDER) or whose count
    is negative (ERR_RANGE; ORDER where one index is both), or (OK, -1)"""
    pairs = list(zip(np.asarray(bin1).tolist(), np.asarray(bin2).tolist()))
    for t, c in enumerate(np.asarray(count).tolist()):
        if t > 0 and not pairs[t - 1] < pairs[t]:
            return ERR_ORDER, t
        if c < 0:
            return ERR_RANGE, t
    return OK, -1


def reference_band(nrows, ncols, bin1, bin2, count, bin_offset=0):
    """(band, stats): the band of the list, uint32[nrows * ncols + 1] with 0 wherever no IN pixel lies, and the
    fields of modle_pixels_band_stats as a dict (a negative count enters no sum)"""
    cls = reference_classes(nrows, ncols, bin1, bin2, bin_offset)
    band = np.zeros(nrows * ncols + 1, dtype=np.uint32)
    st = dict(n_in=0, sum_in=0, nnz_in=0, n_beyond=0, sum_beyond=0, n_outside=0, sum_outside=0, max_count=0)
    for a, b, c, k in zip(np.asarray(bin1).tolist(), np.asarray(bin2).tolist(), np.asarray(count).tolist(),
                          cls.tolist()):
        v = max(c, 0)
        what = ("in", "beyond", "outside")[k]
        st["n_" + what] += 1
        st["sum_" + what] += v
        if k == IN:
            i, j = a - int(bin_offset), b - int(bin_offset)
            band[j * nrows + (j - i)] = c & 0xFFFFFFFF
            st["nnz_in"] += v > 0
            st["max_count"] = max(st["max_count"], v)
    st["first_bad"] = reference_order(bin1, bin2, count)[1]
    return band, st


# ---- the rule ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nrows,ncols", [(1, 1), (3, 3), (7, 30), (40, 65), (65, 65), (200, 700)])
@pytest.mark.parametrize("bin_offset", [-7, 0, 2**40])
def test_band_classify_on_seeded_lists(nrows, ncols, bin_offset):
    rng = np.random.default_rng([nrows, ncols, abs(bin_offset)])
    n = 4000
    bin1 = rng.integers(-3, ncols + 4, size=n) + bin_offset
    bin2 = bin1 + rng.integers(-2, nrows + 3, size=n)
    want = reference_classes(nrows, ncols, bin1, bin2, bin_offset)
    assert set(want.tolist()) == ({IN, BEYOND, OUTSIDE} if nrows < ncols else {IN, OUTSIDE})
    assert np.array_equal(pixels.band_classify(nrows, ncols, bin1, bin2, bin_offset), want)


@pytest.mark.parametrize("bin_offset", [I64_MIN, I64_MIN + 1, -7, 0, 5, 2**40, I64_MAX - 3, I64_MAX])
def test_band_classify_at_the_int64_extremes(bin_offset):
    """every pair of I64_MIN, I64_MAX, the offset and its neighbours, in both positions: no overflow anywhere"""
    near = [bin_offset + d for d in range(-3, 12) if I64_MIN <= bin_offset + d <= I64_MAX]
    values = sorted(set([I64_MIN, I64_MIN + 1, -1, 0, 1, I64_MAX - 1, I64_MAX] + near))
    bin1 = np.array([a for a in values for _ in values], dtype=np.int64)
    bin2 = np.array([b for _ in values for b in values], dtype=np.int64)
    for nrows, ncols in [(1, 1), (3, 8), (8, 8)]:
        want = reference_classes(nrows, ncols, bin1, bin2, bin_offset)
        assert np.array_equal(pixels.band_classify(nrows, ncols, bin1, bin2, bin_offset), want), (nrows, ncols)
    if bin_offset < I64_MAX - 12:
        assert IN in want.tolist()


def test_band_classify_refuses_bad_arguments():
    one = np.zeros(1, dtype=np.int64)
    for nrows, ncols in [(3, 2), (0, 2), (2, 0)]:
        with pytest.raises(pixels.PixelsError) as e:
            pixels.band_classify(nrows, ncols, one, one)
        assert e.value.code == pixels.ERR_ARG
    assert pixels.band_classify(0, 0, one, one).tolist() == [OUTSIDE]
    assert len(pixels.band_classify(3, 5, [], [])) == 0


def test_the_new_symbols_are_exported():
    header = open(os.path.join(ROOT, "include", "modle_cooler_read.h")).read()
    names = set(re.findall(r"\b(modle_cool_reader_[a-z_]+)\s*\(", header))
    assert names == {"modle_cool_reader_open", "modle_cool_reader_info", "modle_cool_reader_chrom",
                     "modle_cool_reader_indexes", "modle_cool_reader_pixels", "modle_cool_reader_close"}
    for name in names:
        assert hasattr(cooler.lib(), name)
    declared = set(re.findall(r"\b(modle_pixels_band_[a-z_]+)\s*\(",
                              open(os.path.join(ROOT, "include", "modle_pixels.h")).read()))
    assert declared == {"modle_pixels_band_classify", "modle_pixels_band_check", "modle_pixels_band_fill",
                        "modle_pixels_band_from_host"}
    for name in declared:
        assert name in pixels.EXPORTS and hasattr(pixels.lib(), name)
    assert (pixels.BAND_TILE_COLS, pixels.BAND_TILE_DIAGS, pixels.ERR_ORDER) == (64, 128, -4)
    text = open(os.path.join(ROOT, "include", "modle_pixels.h")).read()
    assert f"#define MODLE_PIXELS_BAND_TILE_COLS {pixels.BAND_TILE_COLS}\n" in text
    assert f"#define MODLE_PIXELS_BAND_TILE_DIAGS {pixels.BAND_TILE_DIAGS}\n" in text


# ---- the reader ----------------------------------------------------------------------------------------------

BASE, BIN_SIZES = 5000, [5000, 10000, 25000]
CHROMS = [("chrA", 1_003_000), ("chrQuiet", 42_000), ("chrB", 600_000)]  # chrQuiet: no contacts
BANDS = {"chrA": (40, 201, 0.3), "chrB": (25, 120, 0.5)}  # nrows, ncols (every bin of the chromosome), density


def chrom_first_bins(bin_size):
    first, out = 0, {}
    for name, size in CHROMS:
        out[name] = first
        first += -(-size // bin_size)
    out[None] = first
    return out


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """(path of a .cool, path of an .mcool, {bin size: {chromosome: (bin1, bin2, count)}}): both written from
    seeded bands, the pixels per resolution from the numpy references of the writers' tests"""
    rng = np.random.default_rng(77)
    tmp = tmp_path_factory.mktemp("band_outputs")
    cool, mcool = str(tmp / "in.cool"), str(tmp / "in.mcool")
    table = {b: {name: (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int32)) for name, _ in CHROMS}
             for b in BIN_SIZES}
    with cooler.CoolerWriter(cool, CHROMS, BASE) as wc, cooler.McoolWriter(mcool, CHROMS, BIN_SIZES) as wm:
        for name, (nrows, ncols, density) in BANDS.items():
            band = random_band(rng, nrows, ncols, density)
            wc.append(name, band, nrows, ncols)
            for b in BIN_SIZES:
                k = b // BASE
                cb, nr, nc = (band, nrows, ncols) if k == 1 else reference_coarsen(band, nrows, ncols, k, 0)
                b1, b2, cn, off = reference_pixels(cb, nr, nc, chrom_first_bins(b)[name])
                wm.resolution(b).append_pixels(name, nc, b1, b2, cn, bin1_offset=off)
                table[b][name] = (b1, b2, cn)
    return cool, mcool, table


def test_the_reader_returns_what_the_writers_wrote(files):
    cool, mcool, table = files
    for uri, b in [(cool, BASE)] + [(f"{mcool}::/resolutions/{b}", b) for b in BIN_SIZES]:
        first = chrom_first_bins(b)
        with cooler.CoolerReader(uri) as r:
            assert r.bin_size == b and r.chroms == CHROMS
            assert r.chrom_offset == [first[name] for name, _ in CHROMS] + [first[None]]
            index = r.bin1_offset()
            assert len(index) == first[None] + 1 and index[0] == 0
            total = 0
            for cid, (name, _) in enumerate(CHROMS):
                b1, b2, cn, b0 = r.pixels(name)
                w1, w2, wc = table[b][name]
                assert b0 == first[name]
                assert (b1.dtype, b2.dtype, cn.dtype) == (np.int64, np.int64, np.int32)
                assert np.array_equal(b1, w1) and np.array_equal(b2, w2) and np.array_equal(cn, wc), (uri, name)
                assert all(np.array_equal(x, y) for x, y in zip(r.pixels(cid)[:3], (b1, b2, cn)))
                assert index[first[name]] == total
                total += len(b1)
            assert index[-1] == total > 100
            assert len(r.pixels("chrQuiet")[0]) == 0
            with pytest.raises(KeyError):
                r.pixels("chrNone")


@pytest.mark.parametrize("width_bins", [1, 7, 25, 40, 300])
def test_the_band_of_the_reader_s_pixels_is_read_band_s(files, width_bins):
    """modle_cool_read_band, the evaluator's host reader, is the independent reference: same band word for
    word, and its `missed` is the sum beyond the band"""
    cool = files[0]
    with cooler.CoolerReader(cool) as r:
        for name, _ in CHROMS:
            want, nrows, ncols, bs, missed = evaluate.read_cooler_band(cool, name, width_bins * BASE)
            b1, b2, cn, b0 = r.pixels(name)
            assert (bs, ncols) == (BASE, r.n_bins(name)) and nrows == min(width_bins, ncols)
            band, st = reference_band(nrows, ncols, b1, b2, cn, b0)
            assert np.array_equal(band[:-1], want[:-1]), (name, width_bins)
            assert st["sum_beyond"] == missed and st["n_outside"] == 0 and st["first_bad"] == -1
            assert np.array_equal(pixels.band_classify(nrows, ncols, b1, b2, b0),
                                  reference_classes(nrows, ncols, b1, b2, b0))
    assert missed == 0 or width_bins < 25


def spoil(src, tmp_path, what, group="/"):
    assert os.path.exists(H5PY_PYTHON), f"{H5PY_PYTHON} (h5py) is missing"
    path = str(tmp_path / f"{what}{os.path.splitext(src)[1]}")
    shutil.copy(src, path)
    env = {k: v for k, v in os.environ.items() if not k.startswith("PYTHON")}
    out = subprocess.run([H5PY_PYTHON, os.path.join(ROOT, "tests", "h5py_cooler_spoil.py"), path, what, group],
                         capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stderr
    return path


def test_the_reader_s_refusals(files, tmp_path):
    cool, mcool, _ = files
    for uri, code, words in [
            (str(tmp_path / "none.cool"), -2, ["unable to open"]),
            (f"{mcool}::/resolutions/7000", -1, ["/resolutions/7000", "10000, 25000, 5000"]),
            (mcool, -1, ["no cooler", "10000", "25000", "5000"]),
            (f"{cool}::/resolutions/5000", -1, ["no group", "none"]),
            (spoil(cool, tmp_path, "bin-type"), -1, ["bin-type", "variable", "fixed"]),
            (spoil(cool, tmp_path, "float-count"), -1, ["pixels/count", "integer"]),
            (spoil(cool, tmp_path, "short-index"), -1, ["bin1_offset", "entries"]),
            (spoil(mcool, tmp_path, "bin-type", "/resolutions/10000") + "::/resolutions/10000", -1, ["bin-type"])]:
        with pytest.raises(cooler.CoolerError) as e:
            cooler.CoolerReader(uri)
        assert e.value.code == code, uri
        for w in words:
            assert w in str(e.value), (uri, str(e.value))
    # (the other resolutions of the spoilt .mcool still open)
    with cooler.CoolerReader(str(tmp_path / "bin-type.mcool") + "::/resolutions/5000") as r:
        assert r.bin_size == 5000


# ---- analyze: what is refused before a device is touched -----------------------------------------------------

def run_analyze(args, env=None):
    full = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    full["HIP_VISIBLE_DEVICES"] = full["CUDA_VISIBLE_DEVICES"] = ""  # a device that is touched is an error here
    full.update(env or {})
    return subprocess.run([sys.executable, "-m", "modle_amd", "analyze"] + args, cwd=ROOT, capture_output=True,
                          text=True, env=full)


def test_analyze_refuses_before_a_device_is_touched(files, tmp_path):
    cool, mcool, _ = files
    out = tmp_path / "out"
    out.mkdir()
    prefix = str(out / "run")
    existing = out / "run_expected.tsv"
    cases = [
        ([cool, "-o", prefix, "--pileup-at", "barriers"], None, "--pileup-at barriers: a file has no barriers"),
        ([cool, "-o", prefix], {"WORLD_SIZE": "2"}, "WORLD_SIZE"),
        ([cool, "-o", prefix, "--chromosomes", "chrA,chrZ"], None, "chrZ is not a chromosome"),
        ([str(tmp_path / "none.cool"), "-o", prefix], None, "cannot read"),
        ([f"{mcool}::/resolutions/7000", "-o", prefix], None, "10000, 25000, 5000"),
        ([mcool, "-o", prefix], None, "no cooler"),
        ([cool, "-o", prefix, "--expected"], None, f"refusing to overwrite {existing}: pass --force"),
        ([cool, "-o", prefix, "--insulation-resolution", "10kb"], None, "needs --insulation-windows"),
    ]
    existing.write_text("kept\n")
    for args, env, message in cases:
        p = run_analyze(args, env)
        assert p.returncode != 0, args
        assert message in p.stderr, (args, p.stderr)
        assert sorted(os.listdir(out)) == ["run_expected.tsv"] and existing.read_text() == "kept\n", args
    p = run_analyze(["--help"])
    assert p.returncode == 0 and "--diagonal-width" in p.stdout and "--insulation-windows" in p.stdout


def test_simulate_s_help_is_what_it_was():
    """the options of the analyses moved into a function both subcommands call: the text of `simulate --help`
    is the parent commit's, stored in tests/golden/simulate_help.txt (80 columns)"""
    env = dict(os.environ, COLUMNS="80")
    p = subprocess.run([sys.executable, "-m", "modle_amd", "simulate", "--help"], cwd=ROOT, capture_output=True,
                       text=True, env=env)
    assert p.returncode == 0
    assert p.stdout == open(os.path.join(ROOT, "tests", "golden", "simulate_help.txt")).read()


def test_a_job_that_does_not_fit_names_its_remedies():
    """bands plus four times the largest (coarse, dot candidates, kept, rest) against the free device memory"""
    from modle_amd import cli

    plan = [{"nrows": 10, "ncols": 100}, {"nrows": 20, "ncols": 300}]
    sizes = [(10 * 100 + 1) * 4, (20 * 300 + 1) * 4]
    need = sum(sizes) + cli.ANALYSIS_SCRATCH_BANDS * sizes[1]
    assert cli.ANALYSIS_SCRATCH_BANDS == 4
    cli.check_band_memory(plan, need)
    cli.check_band_memory([], 0)
    with pytest.raises(SystemExit) as e:
        cli.check_band_memory(plan, need - 1)
    assert "-w" in str(e.value) and "--chromosomes" in str(e.value) and str(need) in str(e.value)
