"""`simulate --call-domains` without a GPU: the numpy restatement of the triangle sums that the GPU tests compare
against (pixels.triangle_sums_host, held against the definition written as loops of Python integers), the
host-only number of pixels of a window (modle_pixels_triangle_cells), what the entry points refuse before a device
is touched, the identity that turns three triangles into a diamond of the insulation
(api.insulation_from_triangles), the decision (pixels.domain_calls, held against an exhaustive search in
Fractions), the identity that ties the table to the diagonal sums (driver.check_triangles), the options and what
cli.preflight refuses for them, and the lines of <prefix>_domain_calls.bed, which the reader of --domains-at
reads."""
import ctypes as C
import math
import os
from fractions import Fraction

import numpy as np
import pytest

from modle_amd import api, cli, driver, pixels
from test_gpu_marginals import make_band
from test_insulation_outputs import prefix_insulation

M64 = (1 << 64) - 1


# ---- the restatement ------------------------------------------------------------------------------------------

def loops(band, nrows, ncols, width, d0):
    """the definition: T[k][s] = the sum of M(a, c) = band[c * nrows + (c - a)] over s <= a <= c < min(s + k + 1,
    ncols), c - a >= d0, in Python integers; (sums, cells) as lists of lists"""
    sums, cells = [], []
    for k in range(width):
        sums.append([]), cells.append([])
        for s in range(ncols):
            t = n = 0
            for a in range(s, min(s + k + 1, ncols)):
                for c in range(a, min(s + k + 1, ncols)):
                    if c - a >= d0:
                        assert c - a < nrows
                        t += int(band[c * nrows + (c - a)])
                        n += 1
            sums[-1].append(t), cells[-1].append(n)
    return sums, cells


def diag_sums(band, nrows, ncols):
    return [sum(int(band[c * nrows + d]) for c in range(d, ncols)) for d in range(nrows)]


def band_of(matrix, nrows):
    """the band of the first `nrows` diagonals of the symmetric `matrix`"""
    n = len(matrix)
    band = np.zeros(nrows * n + 1, dtype=np.uint32)
    for c in range(n):
        for d in range(min(c, nrows - 1) + 1):
            band[c * nrows + d] = matrix[c - d][c]
    return band


@pytest.mark.parametrize("d0", [0, 1, 2, 6, 7, 9])
@pytest.mark.parametrize("width", [1, 4, 7])
def test_the_restatement_is_the_definition_written_as_loops(width, d0):
    nrows, ncols = 7, 11
    band = make_band(nrows, ncols, "full")  # (the words that are no pixels hold 0xFFFFFFFF: reading one shows)
    want, cells = loops(band, nrows, ncols, width, d0)
    got = pixels.triangle_sums_host(band, nrows, ncols, width, d0)
    assert got.dtype == np.uint64 and got.shape == (width, ncols)
    assert [[int(x) for x in row] for row in got] == want
    assert int(got.max()) > 2**32 or d0 >= width - 1  # (one pixel per window at d0 == width - 1)
    if d0 >= width:
        assert not got.any()
    got_cells = pixels.triangle_cells(ncols, width, d0)
    assert got_cells.dtype == np.uint64 and [[int(x) for x in row] for row in got_cells] == cells
    for bad in ((0, 0), (8, 0), (3, -1)):
        with pytest.raises(ValueError):
            pixels.triangle_sums_host(band, nrows, ncols, *bad)


@pytest.mark.parametrize("ncols,width,d0", [(1, 1, 0), (5, 5, 0), (11, 7, 2), (64, 9, 9), (70, 65, 3), (3, 10, 1)])
def test_the_cells_match_the_closed_form(ncols, width, d0):
    got = pixels.triangle_cells(ncols, width, d0)
    for k in range(width):
        for s in range(ncols):
            w = min(k + 1, ncols - s)
            assert int(got[k, s]) == (0 if w <= d0 else (w - d0) * (w - d0 + 1) // 2)
    assert pixels.triangle_cells(0, 3, 0).shape == (3, 0)
    for args in ((5, 0, 0), (5, pixels.MAX_TRIANGLE_WIDTH + 1, 0), (5, -1, 0), (5, 2, -1), (-1, 2, 0), (5, 1 << 64, 0)):
        with pytest.raises(pixels.PixelsError) as e:
            pixels.triangle_cells(*args)
        assert e.value.code == pixels.ERR_ARG
    assert pixels.lib().modle_pixels_triangle_cells(5, 2, 0, None) == pixels.ERR_ARG


# ---- the symbols and the refusals ---------------------------------------------------------------------------------

def test_the_symbols_are_exported_and_declared():
    names = ["modle_pixels_triangles", "modle_pixels_triangles_to_host", "modle_pixels_coarse_triangles_to_host",
             "modle_pixels_triangle_cells"]
    here = os.path.dirname(os.path.abspath(__file__))
    header = open(os.path.join(here, "..", "include", "modle_pixels.h")).read()
    for name in names:
        assert name in pixels.EXPORTS and getattr(pixels.lib(), name) is not None and name + "(" in header
    assert "#define MODLE_PIXELS_MAX_TRIANGLE_WIDTH 65535" in header and pixels.MAX_TRIANGLE_WIDTH == 65535
    assert 4096 <= pixels.MAX_TRIANGLE_WIDTH and 65535 * 65536 // 2 * 0xFFFFFFFF < 1 << 64
    for name in ("triangles_into", "triangles_to_host", "coarse_triangles_to_host"):
        assert callable(getattr(pixels, name)) and callable(getattr(pixels.Extractor, name))
    for name in ("triangle_sums", "triangle_sums_tensor", "call_domains"):
        assert callable(getattr(api.BandAnalyses, name)) and callable(getattr(api.Simulator, name))


def test_what_the_entry_points_refuse_without_a_device():
    """every refusal comes before the handle, the band or the output is touched: the handle here is host memory
    that names a device no machine has, and the band and the output are addresses nobody owns, so nothing can
    have been written; the message names the rule that was broken"""
    lb = pixels.lib()
    handle = (C.c_uint64 * 512)()
    C.cast(handle, C.POINTER(C.c_int))[0] = 1 << 20  # modle_pixels_handle.device
    h = C.addressof(handle)
    band, out = 0x10000000, 0x30000000
    nrows, ncols = 50, 90
    band_bytes = (nrows * ncols + 1) * 4
    err = C.create_string_buffer(512)
    # handle, band, nrows, ncols, max_width, min_diag, out, out_words
    accepted = {
        "W == 1": (h, band, nrows, ncols, 1, 0, out, ncols),
        "W == nrows": (h, band, nrows, ncols, nrows, 2, out, nrows * ncols),
        "min_diag beyond W": (h, band, nrows, ncols, 10, M64, out, 10 * ncols),
        "more words than needed": (h, band, nrows, ncols, 10, 0, out, 10 * ncols + 7),
        "the square whole matrix": (h, band, ncols, ncols, ncols, 0, out, ncols * ncols),
        "the output ends where the band begins": (h, band, nrows, ncols, 3, 0, band - 8 * 3 * ncols, 3 * ncols),
        "the output begins where the band ends": (h, band + 4, nrows, ncols, 3, 0, band + 4 + band_bytes, 3 * ncols),
    }
    refused = {
        "no handle": ((None, band, nrows, ncols, 5, 0, out, 5 * ncols), b"no null pointer"),
        "no band": ((h, None, nrows, ncols, 5, 0, out, 5 * ncols), b"no null pointer"),
        "no output": ((h, band, nrows, ncols, 5, 0, None, 5 * ncols), b"no null pointer"),
        "nrows 0": ((h, band, 0, ncols, 1, 0, out, ncols), b"0 < nrows <= ncols"),
        "an empty band": ((h, band, 0, 0, 1, 0, out, 0), b"0 < nrows <= ncols"),
        "nrows > ncols": ((h, band, ncols + 1, ncols, 5, 0, out, 5 * ncols), b"0 < nrows <= ncols"),
        "W == 0": ((h, band, nrows, ncols, 0, 0, out, 0), b"1 <= max_width <= nrows"),
        "W == nrows + 1": ((h, band, nrows, ncols, nrows + 1, 0, out, (nrows + 1) * ncols), b"1 <= max_width <= nrows"),
        "a W that wraps": ((h, band, nrows, ncols, M64, 0, out, M64), b"1 <= max_width <= nrows"),
        "W above the cap": ((h, 1 << 44, 70_000, 70_000, 65536, 0, 1 << 45, 65536 * 70_000), b"max_width <= 65535"),
        "out_words too small": ((h, band, nrows, ncols, 5, 0, out, 5 * ncols - 1), b"out_words >= max_width * ncols"),
        "a misaligned output": ((h, band, nrows, ncols, 5, 0, out + 4, 5 * ncols), b"8-byte aligned"),
        "the output overlaps the band": ((h, band, nrows, ncols, 5, 0, band + band_bytes - 4, 5 * ncols), b"overlaps the band"),
        "the output ends in the band": ((h, band, nrows, ncols, 5, 0, band - 8 * 5 * ncols + 8, 5 * ncols), b"overlaps the band"),
        "the output is the band": ((h, band, nrows, ncols, 5, 0, band, 5 * ncols), b"overlaps the band"),
    }
    for name, (args, rule) in refused.items():
        err.value = b""
        assert lb.modle_pixels_triangles(*args, None, err, len(err)) == pixels.ERR_ARG, name
        assert err.value.startswith(b"modle_pixels_triangles: ") and rule in err.value, (name, err.value)
    for name, args in accepted.items():  # past the argument checks: the device of the handle does not exist
        err.value = b""
        assert lb.modle_pixels_triangles(*args, None, err, len(err)) == pixels.ERR_DEVICE, name
    # the cap at the cap: accepted
    assert lb.modle_pixels_triangles(h, 1 << 44, 70_000, 70_000, 65535, 0, 1 << 45, 65535 * 70_000, None, err,
                                     len(err)) == pixels.ERR_DEVICE
    ptr = C.c_void_p(1)
    for name, (args, rule) in refused.items():
        if "out" in name:
            continue
        for fn, extra in ((lb.modle_pixels_triangles_to_host, ()), (lb.modle_pixels_coarse_triangles_to_host, (1, 0))):
            # (the coarse form at a factor of 1, which it refuses whatever the rest)
            ptr.value = 1
            assert fn(*args[:4], *extra, *args[4:6], C.byref(ptr), None, err, len(err)) == pixels.ERR_ARG, name
            assert ptr.value is None, name
            if not extra:
                assert rule in err.value, (name, err.value)
    # the rule holds against the coarse shape: 50 diagonals by 5 are 11
    assert pixels.coarse_shape(nrows, ncols, 5, 0) == (11, 18)
    ptr.value = 1
    assert lb.modle_pixels_coarse_triangles_to_host(h, band, nrows, ncols, 5, 0, 12, 0, C.byref(ptr), None, err,
                                                    len(err)) == pixels.ERR_ARG
    assert ptr.value is None and b"of the coarse band" in err.value and b"1 <= max_width <= nrows" in err.value
    assert lb.modle_pixels_coarse_triangles_to_host(h, band, nrows, ncols, 5, 0, 11, 0, C.byref(ptr), None, err,
                                                    len(err)) == pixels.ERR_DEVICE
    assert lb.modle_pixels_triangles_to_host(h, band, nrows, ncols, 5, 0, None, None, err, len(err)) == pixels.ERR_ARG
    # the python forms refuse what ctypes would wrap
    for args in ((-1, 0), (5, -1), (1 << 64, 0), (5, 1 << 64)):
        with pytest.raises(pixels.PixelsError) as e:
            pixels._triangle_args(*args)
        assert e.value.code == pixels.ERR_ARG


# ---- three triangles are a diamond ----------------------------------------------------------------------------------

@pytest.mark.parametrize("d0", [0, 2, 5])
@pytest.mark.parametrize("nrows,ncols", [(21, 40), (9, 9), (13, 70)])
def test_the_insulation_is_a_difference_of_three_triangles(nrows, ncols, d0):
    band = make_band(nrows, ncols, "full")
    table = pixels.triangle_sums_host(band, nrows, ncols, nrows, d0)
    windows = [w for w in (1, 2, 5, 7, 11) if 2 * w - 1 <= nrows]
    got = api.insulation_from_triangles(table, windows)
    assert got.dtype == np.uint64 and np.array_equal(got, prefix_insulation(band, nrows, ncols, windows, d0))
    with pytest.raises(ValueError):
        api.insulation_from_triangles(table, [nrows // 2 + 2])  # 2 w - 1 > W
    with pytest.raises(ValueError):
        api.insulation_from_triangles(table, [0])
    with pytest.raises(ValueError):
        api.insulation_from_triangles(table.astype(np.int64), [1])


# ---- the decision ---------------------------------------------------------------------------------------------------

def exhaustive(table, gamma, lo, hi):
    """the best and the second best set of disjoint windows [s, s + w), lo <= w <= hi, wholly in the chromosome,
    by the sum of Q(s, w) = T[w - 1][s] - gamma * mu_w in Fractions: ((score, windows), (score, windows))"""
    width, ncols = table.shape
    hi = min(hi, width, ncols)
    gamma = Fraction(gamma)
    mu = {w: Fraction(sum(int(x) for x in table[w - 1, :ncols - w + 1]), ncols - w + 1) for w in range(lo, hi + 1)}
    found = []

    def walk(e, score, taken):
        if e == ncols:
            found.append((score, tuple(taken)))
            return
        walk(e + 1, score, taken)  # bin e stays outside
        for w in range(lo, hi + 1):
            if e + w <= ncols:
                walk(e + w, score + int(table[w - 1, e]) - gamma * mu[w], taken + [(e, w)])

    walk(0, Fraction(0), [])
    found.sort(key=lambda f: f[0], reverse=True)
    return found[0], found[1], mu


def blocks_matrix(n, blocks, inside, outside, rng):
    m = np.full((n, n), outside, dtype=np.int64)
    for a, b in blocks:
        m[a:b, a:b] = inside
    m += rng.integers(0, 3, size=(n, n))
    return np.triu(m) + np.triu(m, 1).T


@pytest.mark.parametrize("n,blocks,gamma,lo,d0", [
    (12, [(0, 4), (4, 9), (9, 12)], 1, 3, 0), (12, [(1, 5), (7, 12)], 1, 3, 2), (11, [(0, 3), (3, 6), (6, 11)], 0.5, 2, 1),
    (10, [(2, 8)], 1.5, 3, 0), (12, [(0, 6), (6, 12)], 1, 1, 0), (9, [(2, 7)], 1, 3, 2)])
def test_the_calls_are_those_of_an_exhaustive_search_in_fractions(n, blocks, gamma, lo, d0):
    rng = np.random.default_rng([n, len(blocks), d0])
    matrix = blocks_matrix(n, blocks, 1000, 10, rng)
    band = band_of(matrix, n)
    table = pixels.triangle_sums_host(band, n, n, n, d0)
    cells = pixels.triangle_cells(n, n, d0)
    (best, windows), (second, _), mu = exhaustive(table, gamma, lo, n)
    assert best - second >= 1  # the optimum is unique by a margin that no rounding reaches
    calls = pixels.domain_calls(table, cells, gamma=gamma, min_width=lo, max_width=n)
    assert [(c.start, c.width) for c in calls] == list(windows)
    for c in calls:
        assert c.end == c.start + c.width and c.sum == int(table[c.width - 1, c.start])
        assert c.cells == int(cells[c.width - 1, c.start])
        q = c.sum - Fraction(gamma) * mu[c.width]
        assert abs(Fraction(c.score) - q) <= abs(q) * Fraction(1, 2**50)
        assert abs(Fraction(c.strength) - c.sum / mu[c.width]) <= Fraction(c.sum, 2**50) / mu[c.width]
    assert sum(Fraction(c.score) for c in calls) == pytest.approx(float(best))
    # a narrower largest width: the search agrees again
    (best2, windows2), (second2, _), _ = exhaustive(table, gamma, lo, max(lo, n // 2))
    if best2 - second2 >= 1:
        narrow = pixels.domain_calls(table, cells, gamma=gamma, min_width=lo, max_width=max(lo, n // 2))
        assert [(c.start, c.width) for c in narrow] == list(windows2)


def test_a_block_diagonal_matrix_gives_its_blocks():
    n, blocks = 60, [(0, 7), (7, 20), (20, 24), (30, 41), (41, 60)]  # the bins 24 .. 29 belong to no block
    matrix = np.zeros((n, n), dtype=np.int64)
    for a, b in blocks:
        matrix[a:b, a:b] = 50
    nrows = 25
    band = band_of(matrix, nrows)
    for d0 in (0, 2):
        table = pixels.triangle_sums_host(band, nrows, n, nrows, d0)
        calls = pixels.domain_calls(table, pixels.triangle_cells(n, nrows, d0), gamma=1, min_width=3)
        assert [(c.start, c.end) for c in calls] == blocks, d0
        assert all(c.score > 0 and c.strength > 1 for c in calls)
    # the defaults are those of the module
    assert (pixels.DOMAIN_GAMMA, pixels.DOMAIN_MIN_WIDTH) == (1.0, 3)
    assert pixels.domain_calls(table, pixels.triangle_cells(n, nrows, 2)) == calls


def test_ties_leave_a_bin_out_and_then_take_the_shorter_width():
    # an empty table: every window scores 0, which only equals leaving its bins out
    table = np.zeros((5, 9), dtype=np.uint64)
    cells = pixels.triangle_cells(9, 5, 0)
    assert pixels.domain_calls(table, cells, gamma=1, min_width=1) == []
    # gamma 0 and one contact at (4, 4): every window that holds bin 4 scores 1; the shortest is taken
    table = pixels.triangle_sums_host(band_of(np.diag([0, 0, 0, 0, 1, 0, 0, 0, 0]), 5), 5, 9, 5, 0)
    calls = pixels.domain_calls(table, cells, gamma=0, min_width=2)
    assert [(c.start, c.end) for c in calls] == [(3, 5)] and calls[0].score == 1.0
    assert math.isnan(pixels.domain_calls(table, cells, gamma=0, min_width=5, max_width=5)[0].strength) is False


def test_what_the_decision_refuses():
    table = np.zeros((4, 9), dtype=np.uint64)
    cells = pixels.triangle_cells(9, 4, 0)
    table[3, 2] = 1 << 53
    with pytest.raises(ValueError) as e:
        pixels.domain_calls(table, cells, gamma=1, min_width=3)
    assert "2^53" in str(e.value)
    table[3, 2] = (1 << 53) - 1
    assert [(c.start, c.end) for c in pixels.domain_calls(table, cells, gamma=1, min_width=3)] == [(2, 6)]
    for bad in (dict(min_width=0), dict(gamma=math.nan), dict(gamma=math.inf)):
        with pytest.raises(ValueError):
            pixels.domain_calls(table, cells, **{"gamma": 1, "min_width": 3, **bad})
    with pytest.raises(ValueError):
        pixels.domain_calls(table.astype(np.int64), cells)
    with pytest.raises(ValueError):
        pixels.domain_calls(table, cells[:3])
    assert pixels.domain_calls(table, cells, gamma=1, min_width=5) == []  # no width is left


# ---- the table against the diagonal sums ------------------------------------------------------------------------------

@pytest.mark.parametrize("nrows,ncols,width,d0", [(7, 11, 7, 0), (7, 11, 5, 2), (21, 40, 21, 2), (9, 9, 9, 1), (6, 30, 1, 0),
                                                  (6, 30, 4, 4)])
def test_the_table_adds_up_to_the_diagonal_sums(nrows, ncols, width, d0):
    band = make_band(nrows, ncols, "full")
    table = pixels.triangle_sums_host(band, nrows, ncols, width, d0)
    diag = diag_sums(band, nrows, ncols)
    windows = [w for w in (1, 2, 4) if 2 * w - 1 <= nrows]
    ins = prefix_insulation(band, nrows, ncols, windows, d0)
    driver.check_triangles("chrA:0-10", table, d0, diag)
    driver.check_triangles("chrA:0-10", table, d0, diag, windows, ins)
    for k, s in ((0, 0), (width - 1, ncols - 1), (width // 2, ncols // 2), (width - 1, 0)):
        for step in (1, -1):
            if step == -1 and table[k, s] == 0:
                continue
            wrong = table.copy()
            wrong[k, s] = np.uint64(int(table[k, s]) + step)
            with pytest.raises(RuntimeError) as e:
                driver.check_triangles("chrA:0-10", wrong, d0, diag)
            assert str(e.value).startswith("chrA:0-10: the windows of ")
    if windows and 2 * windows[-1] - 1 <= width:
        wrong = ins.copy()
        wrong[len(windows) - 1, ncols // 2] += np.uint64(1)
        with pytest.raises(RuntimeError) as e:
            driver.check_triangles("chrA:0-10", table, d0, diag, windows, wrong)
        assert "difference of three triangles" in str(e.value)
    with pytest.raises(RuntimeError):
        driver.check_triangles("chrA:0-10", table, d0, diag[:width - 1])


# ---- <prefix>_domain_calls.bed ---------------------------------------------------------------------------------------

def entry(name, start, end, nrows, ncols, skipped=False):
    return {"interval": {"name": name, "size": end, "start": start, "end": end}, "nrows": nrows, "ncols": ncols,
            "tasks": None, "skipped": skipped}


def test_the_lines_of_the_file_and_the_reader_of_domains_at(tmp_path):
    calls = cli.DomainCalls(str(tmp_path / "p_domain_calls.bed"), 5000, 2_000_000, 15_000, 1.0, 2)
    assert cli.DomainCalls._fields == ("path", "resolution", "max_width", "min_width", "gamma", "min_diag")
    assert driver.domain_calls_bins(calls) == (400, 3, 2)
    header = driver.domain_calls_header(calls)
    assert header == ("# resolution=5000 max_width=2000000 min_width=15000 gamma=1.0 ignore_diags=2\n"
                      "#chrom\tstart\tend\tname\tscore\tstrength\n")
    iv = {"name": "chrA", "start": 25_000, "end": 523_000}
    rows = [pixels.DomainCall(2, 10, 8, 500, 21, 12.5, 1 / 3), pixels.DomainCall(90, 100, 10, 7, 36, 0.25, math.nan)]
    lines = driver.domain_calls_lines(iv, 5000, 1, rows)
    assert lines == ["chrA\t35000\t75000\tchrA:35000-75000\t12.5\t0.33333333333333331\n",
                     "chrA\t475000\t523000\tchrA:475000-523000\t0.25\tnan\n"]  # the last bin is clipped to the interval
    assert driver.domain_calls_lines(iv, 5000, 2, rows[:1]) == ["chrA\t40000\t120000\tchrA:40000-120000\t12.5\t0.33333333333333331\n"]
    plan = [entry("chrA", 25_000, 523_000, 40, 100), entry("chrB", 0, 9_000, 2, 2, skipped=True), entry("chrC", 0, 500_000, 40, 100)]
    asked = []

    def each(k, factor, first_bin):
        asked.append((k, factor, first_bin))
        return None if k == 2 else rows

    driver.write_domain_calls(calls.path, plan, 5000, calls, each)
    assert asked == [(0, 1, 5), (2, 1, 0)]  # an entry that is skipped is not asked for, one without a matrix writes nothing
    assert open(calls.path).read() == header + "".join(lines)
    # six columns, and the reader of --domains-at takes the file as it is
    assert all(len(line.split("\t")) == 6 for line in lines)
    assert driver.read_bed(calls.path) == [("chrA", 35_000, 75_000), ("chrA", 475_000, 523_000)]
    assert driver.domains_misfit(plan, 5000, 5000, 10, [calls.path]) is None
    # the table the preflight counts: the widths clamped to the band, at the resolution of the calls
    assert driver.domain_calls_table_bytes(plan, 5000, calls) == 8 * 40 * 100
    assert driver.domain_calls_table_bytes(plan, 5000, calls._replace(max_width=50_000)) == 8 * 10 * 100
    assert driver.domain_calls_table_bytes(plan, 5000, calls._replace(resolution=10_000)) == 8 * 21 * 51  # (chrA starts in the middle of a coarse bin)
    assert driver.domain_calls_table_bytes(plan[1:2], 5000, calls) == 0
    cli.check_band_memory(plan, 10**9, 10**8)
    with pytest.raises(SystemExit) as e:
        cli.check_band_memory(plan, 10**8, 10**8)
    assert "the triangle table of --call-domains (100000000 bytes)" in str(e.value)
    cli.check_band_memory(plan, 10**8)


# ---- the options and what is refused before anything is simulated -----------------------------------------------------

@pytest.fixture
def prefix(tmp_path, monkeypatch):
    for name in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(name, raising=False)
    return str(tmp_path / "out" / "p")


def parse(prefix, *extra):
    return cli.build_parser().parse_args(["simulate", "-c", "g.chrom.sizes", "-b", "b.bed", "-o", prefix,
                                          "-r", "5kb", "--no-track-1d-lef-position", *extra])


def run_preflight(prefix, *extra):
    a = parse(prefix, *extra)
    return cli.preflight(a, cli.config_from_args(a))


def test_the_plan_of_before_is_as_it_was():
    assert len(cli.Preflight._fields) == 13
    outputs = cli.Outputs(None, None, None, None)
    pre = cli.Preflight(None, outputs, 0, 1, 0)
    assert pre.domain_calls is None and pre.stripe_calls is None and len(pre) == 13
    calls = cli.DomainCalls("p", 5000, 2_000_000, 15_000, 1.0, 2)
    pre = cli.Preflight(None, outputs, 0, 1, 0, domain_calls=calls)
    assert pre.domain_calls is calls and pre.stripe_calls is None and tuple(pre) == tuple(cli.Preflight(None, outputs, 0, 1, 0))
    moved = pre._replace(rank=1)
    assert moved.rank == 1 and moved.domain_calls is calls and isinstance(moved, cli.Preflight)
    assert pre._replace(domain_calls=None).domain_calls is None and pre.domain_calls is calls
    assert cli.Preflight._make(tuple(pre)).domain_calls is None


def test_the_options_parse_and_preflight_plans_the_file(prefix):
    a = parse(prefix)
    assert [getattr(a, "call_domains" + s) for s in ("", "_max_width", "_min_width", "_gamma", "_ignore_diags",
                                                     "_resolution")] == [None] * 6
    assert run_preflight(prefix).domain_calls is None
    pre = run_preflight(prefix, "--call-domains")
    assert pre.domain_calls == cli.DomainCalls(prefix + "_domain_calls.bed", 5000, 2_000_000, 15_000, 1.0, 2)
    assert cli.domain_calls_path(prefix) == prefix + "_domain_calls.bed" and not os.path.exists(prefix + "_domain_calls.bed")
    pre = run_preflight(prefix, "--call-domains", "--call-domains-max-width", "500kb", "--call-domains-min-width", "20kb",
                        "--call-domains-gamma", "0.5", "--call-domains-ignore-diags", "0", "--call-domains-resolution", "10kb")
    assert pre.domain_calls == cli.DomainCalls(prefix + "_domain_calls.bed", 10_000, 500_000, 20_000, 0.5, 0)
    # 2 Mb in whole bins of 15 kb
    assert run_preflight(prefix, "--call-domains", "--call-domains-resolution", "15kb").domain_calls.max_width == 1_995_000
    assert run_preflight(prefix, "--call-domains", "--skip-output").domain_calls.path is None
    # analyze takes the same options
    a = cli.build_parser().parse_args(["analyze", "in.cool", "-o", prefix, "--call-domains", "--call-domains-gamma", "2"])
    assert a.call_domains is True and a.call_domains_gamma == 2.0
    # the file is refused to be overwritten like the others
    os.makedirs(os.path.dirname(prefix), exist_ok=True)
    with open(prefix + "_domain_calls.bed", "w") as fh:
        fh.write("precious")
    with pytest.raises(SystemExit) as e:
        run_preflight(prefix, "--call-domains")
    assert str(e.value) == f"refusing to overwrite {prefix}_domain_calls.bed: pass --force to overwrite"
    assert run_preflight(prefix, "--call-domains", "--force").domain_calls.path == prefix + "_domain_calls.bed"
    assert run_preflight(prefix).domain_calls is None and open(prefix + "_domain_calls.bed").read() == "precious"


def test_preflight_refuses_before_anything_is_made(prefix):
    on = ["--call-domains"]
    refused = [
        (["--call-domains-max-width", "1mb"], "--call-domains-max-width needs --call-domains"),
        (["--call-domains-min-width", "10kb"], "--call-domains-min-width needs --call-domains"),
        (["--call-domains-gamma", "2"], "--call-domains-gamma needs --call-domains"),
        (["--call-domains-ignore-diags", "2"], "--call-domains-ignore-diags needs --call-domains"),
        (["--call-domains-resolution", "10kb"], "--call-domains-resolution needs --call-domains"),
        (on + ["--call-domains-resolution", "7500"], "--call-domains-resolution: 7500 is not a multiple of the resolution (5000)"),
        (on + ["--call-domains-max-width", "52kb"], "--call-domains-max-width: 52000 is not a positive multiple"),
        (on + ["--call-domains-min-width", "0"], "--call-domains-min-width: 0 is not a positive multiple"),
        (on + ["--call-domains-min-width", "50kb", "--call-domains-max-width", "45kb"],
         "--call-domains-max-width: 45000 is below the smallest width (50000)"),
        (on + ["--call-domains-max-width", "400mb"], "--call-domains-max-width: 400000000 is 80000 bins of 5000: at most 65535"),
        (on + ["--call-domains-gamma", "-1"], "--call-domains-gamma: -1.0 is not"),
        (on + ["--call-domains-gamma", "nan"], "--call-domains-gamma: nan is not"),
        (on + ["--call-domains-gamma", "inf"], "--call-domains-gamma: inf is not"),
        (on + ["--call-domains-ignore-diags", "-1"], "--call-domains-ignore-diags: -1 is negative"),
    ]
    for options, message in refused:
        with pytest.raises(SystemExit) as e:
            run_preflight(prefix, *options)
        assert str(e.value).startswith(message), (options, str(e.value))
        assert not os.path.exists(os.path.dirname(prefix))


def test_called_is_the_domains_just_called_only_with_call_domains(prefix, tmp_path, monkeypatch):
    plan = [entry("chrA", 0, 2_000_000, 80, 400)]
    chroms = [("chrA", 2_000_000)]
    monkeypatch.chdir(tmp_path)
    # without --call-domains `called` is a path: a file of that name that is missing is refused as one
    a = parse(prefix, "--domains-at", "called")
    cfg = cli.config_from_args(a)
    pre = cli.preflight(a, cfg)
    assert pre.domains.sources == ["called"] and pre.domain_calls is None
    with pytest.raises(SystemExit) as e:
        cli.check_plan(a, cfg, pre, plan, chroms)
    assert str(e.value).startswith("--domains-at called: the file cannot be read as BED")
    # ... and one that exists is read
    with open("called", "w") as fh:
        fh.write("chrA\t100000\t300000\n")
    assert cli.check_plan(a, cfg, pre, plan, chroms) == []
    os.remove("called")
    # with --call-domains no file of that name is looked for; another source still is
    a = parse(prefix, "--call-domains", "--domains-at", "called")
    pre = cli.preflight(a, cfg)
    assert pre.domains.sources == ["called"] and pre.domain_calls is not None
    assert cli.check_plan(a, cfg, pre, plan, chroms) == []
    a = parse(prefix, "--call-domains", "--domains-at", "called", "--domains-at", "other.bed")
    with pytest.raises(SystemExit) as e:
        cli.check_plan(a, cfg, cli.preflight(a, cfg), plan, chroms)
    assert str(e.value).startswith("--domains-at other.bed: the file cannot be read as BED")
    assert driver.CALLED_DOMAINS == "called"


def test_the_help_of_simulate_is_unchanged():
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "golden", "simulate_help.txt")) as fh:
        golden = fh.read()
    ap = cli.build_parser()
    sub = next(a for a in ap._actions if hasattr(a, "choices") and a.choices and "simulate" in a.choices)
    text = sub.choices["simulate"].format_help()
    assert text == golden
    assert "call-domains" not in text and "call-domains" not in sub.choices["analyze"].format_help()
    assert "--call-domains" in cli.__doc__ and "domain_calls.bed" in cli.__doc__
