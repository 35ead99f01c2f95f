"""Pixels scattered into a band on the MI355X (include/modle_pixels.h: modle_pixels_band_check, _band_fill,
_band_from_host; modle_amd/pixels.py; api.LoadedBands): the band, the statistics and the row starts equal, word
for word, the Python-int restatement of tests/test_band_outputs.py.  The pixel arrays, the row starts and the
output lie between poisoned guard words -- the output at an address that is 4-byte aligned only, and poisoned
before the call: the library, not the caller, defines every word.  Nothing here has a tolerance."""
import ctypes as C

import numpy as np
import pytest

from test_band_outputs import ERR_ORDER, ERR_RANGE, reference_band, reference_classes, reference_order
from test_gpu_insulation import FRONT8, GuardedOut
from test_gpu_marginals import FRONT, POISON, Guarded, make_band

pytestmark = pytest.mark.gpu

INT32_MAX = 2**31 - 1
COLS, DIAGS = 64, 128  # pixels.BAND_TILE_COLS, BAND_TILE_DIAGS (asserted below): the tile of a workgroup
# the issue's shapes; then one below, at and one above the tile's columns (two tiles of diagonals would need
# more columns: the band is no deeper than wide) and its diagonals
SHAPES = [(1, 1), (3, 3), (7, 30), (40, 65), (65, 65), (200, 700),
          (20, COLS - 1), (20, COLS), (20, COLS + 1), (DIAGS - 1, 200), (DIAGS, 200), (DIAGS + 1, 200)]
FILLS = ["empty", "tenth", "full", "constant"]
OFFSETS = [-7, 0, 2**40]


@pytest.fixture(scope="module")
def ex():
    from modle_amd import pixels

    assert (pixels.BAND_TILE_COLS, pixels.BAND_TILE_DIAGS) == (COLS, DIAGS)
    with pixels.Extractor(0) as e:
        yield e


class Dev64(GuardedOut):
    """int64 `values` in device memory, 8-byte aligned, between guard words"""

    def __init__(self, values):
        import torch

        values = np.ascontiguousarray(values, dtype=np.int64)
        super().__init__(len(values))
        self.host[FRONT8:FRONT8 + self.n] = values.view(np.uint32)
        self.tensor = torch.from_numpy(self.host.view(np.int32)).to("cuda:0")
        torch.cuda.synchronize()
        assert self.data_ptr() % 8 == 0

    def values(self):
        return self.read()[FRONT8:FRONT8 + self.n].copy().view(np.int64)


def counts_dev(count):
    return Guarded(np.ascontiguousarray(count, dtype=np.int32).view(np.uint32))


def poisoned_band(nrows, ncols):
    return Guarded(np.full(nrows * ncols + 1, POISON, dtype=np.uint32))


def band_words(out):
    return out.read()[FRONT:FRONT + out.n].copy()


def host_band(nrows, ncols, fill, seed=0):
    """a seeded band whose counts fit the int32 pixel type; the words that are no pixels hold POISON"""
    if fill == "constant":
        band = make_band(nrows, ncols, "empty", seed=seed)
        keep = band == POISON
        band[:] = 5
        band[keep] = POISON
        return band
    return make_band(nrows, ncols, fill, limit=2**31, seed=seed)


def band_pixels(band, nrows, ncols, bin_offset=0):
    """the non-zero pixels of a host band in cooler order (numpy; the GPU extraction is the other source)"""
    i = np.repeat(np.arange(ncols, dtype=np.int64), nrows)
    d = np.tile(np.arange(nrows, dtype=np.int64), ncols)
    ok = i + d < ncols
    i, d = i[ok], d[ok]
    v = band[(i + d) * nrows + d]
    nz = v != 0
    return i[nz] + bin_offset, (i + d)[nz] + bin_offset, v[nz].astype(np.int32)


def weave(b1, b2, cn, nrows, ncols, bin_offset, seed):
    """the list with pixels of the other classes woven in, in order: trans (bin2 beyond the matrix), lower
    triangle, ids below the offset, beyond the band; and some counts of 0"""
    rng = np.random.default_rng([seed, nrows, ncols])
    have = {(a, b): c for a, b, c in zip(b1.tolist(), b2.tolist(), cn.tolist())}
    extra = []
    for i in rng.integers(0, ncols, size=12).tolist():
        extra += [(i, ncols + int(rng.integers(0, 50))), (i, ncols + 1000), (i, i - 1 - int(rng.integers(0, 3))),
                  (i, min(i + nrows + int(rng.integers(0, 4)), ncols + 3))]
    extra += [(-1, 0), (-3, -3), (-2, ncols), (0, -1), (ncols, ncols), (ncols + 2, ncols + 5)]
    for i, j in extra:
        have.setdefault((i + bin_offset, j + bin_offset), int(rng.integers(0, 1000)))
    keys = sorted(have)
    return (np.array([k[0] for k in keys], dtype=np.int64), np.array([k[1] for k in keys], dtype=np.int64),
            np.array([have[k] for k in keys], dtype=np.int32))


def check_list(ex, nrows, ncols, b1, b2, cn, bin_offset, stream=None):
    """check + fill and the one-call form on one list against the restatement; returns the band"""
    n = len(b1)
    want, st = reference_band(nrows, ncols, b1, b2, cn, bin_offset)
    assert st["first_bad"] == -1
    d1, d2, dc = Dev64(b1), Dev64(b2), counts_dev(cn)
    rows, out = Dev64(np.full(ncols + 1, -1, dtype=np.int64)), poisoned_band(nrows, ncols)
    assert out.data_ptr() % 8 == 4
    ptrs = (d1.data_ptr(), d2.data_ptr(), dc.data_ptr()) if n else (None, None, None)
    got = ex.band_check(*ptrs, n, nrows, ncols, bin_offset, rows.data_ptr(), stream)
    assert got._asdict() == st
    only = ex.band_check(*ptrs, n, nrows, ncols, bin_offset, None, stream)  # statistics only
    assert only == got
    targets = [bin_offset + i for i in range(ncols + 1)]  # (Python ints: 2^40 and -7 alike)
    assert rows.values().tolist() == [int(np.searchsorted(b1, t, side="left")) for t in targets]
    assert out.unchanged()
    ex.band_fill_into(ptrs[1], ptrs[2], n, nrows, ncols, bin_offset, rows.data_ptr(), out.data_ptr(), out.n, stream)
    band = band_words(out)
    assert np.array_equal(band, want)
    for g in (d1, d2, dc):
        assert g.unchanged()
    assert out.guards_intact() and rows.guards_intact()
    seen = ex.count(out.data_ptr(), nrows, ncols)
    assert (seen.nnz, seen.sum, seen.max_count) == (st["nnz_in"], st["sum_in"], st["max_count"])
    once = poisoned_band(nrows, ncols)
    assert ex.band_from_host(b1, b2, cn, nrows, ncols, bin_offset, once.data_ptr(), once.n, stream) == got
    assert np.array_equal(band_words(once), want) and once.guards_intact()
    return band


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("nrows,ncols", SHAPES)
def test_fill_of_extract_is_the_band(ex, nrows, ncols, fill):
    """the round-trip law, with the list from the GPU extraction: every pixel word comes back, every other word
    is 0 -- and the same for the list with the other classes woven in"""
    band = host_band(nrows, ncols, fill)
    src = Guarded(band)
    px = ex.extract(src.data_ptr(), nrows, ncols, 0)
    b1, b2, cn = band_pixels(band, nrows, ncols)
    assert np.array_equal(px.bin1, b1) and np.array_equal(px.bin2, b2) and np.array_equal(px.count, cn)
    got = check_list(ex, nrows, ncols, px.bin1, px.bin2, px.count, 0)
    clean = np.where(band == POISON, 0, band)  # (a count is below 2^31: POISON marks the words that are no pixels)
    assert np.array_equal(got, clean)
    assert np.array_equal(check_list(ex, nrows, ncols, *weave(b1, b2, cn, nrows, ncols, 0, 1), 0), clean)


@pytest.mark.parametrize("bin_offset", OFFSETS)
@pytest.mark.parametrize("nrows,ncols", [(3, 3), (7, 30), (40, 65), (DIAGS + 1, 200)])
def test_offsets_of_both_signs(ex, nrows, ncols, bin_offset):
    b1, b2, cn = band_pixels(host_band(nrows, ncols, "tenth", seed=3), nrows, ncols, bin_offset)
    check_list(ex, nrows, ncols, *weave(b1, b2, cn, nrows, ncols, bin_offset, 2), bin_offset)


@pytest.mark.parametrize("nrows,ncols", SHAPES)
def test_small_and_special_lists(ex, nrows, ncols):
    i64, i32 = (lambda *v: np.array(v, dtype=np.int64)), (lambda *v: np.array(v, dtype=np.int32))
    check_list(ex, nrows, ncols, i64(), i64(), i32(), 0)  # n = 0: a band of zeros
    last = ncols - 1
    for a, b, c in [(0, 0, 9), (last, last, INT32_MAX), (last - (nrows - 1), last, 1), (0, 0, 0), (last, last + 1, 4)]:
        check_list(ex, nrows, ncols, i64(a), i64(b), i32(c), 0)  # n = 1: corners, the largest count, a zero, trans
    # one row that holds every pixel of the band's width, between empty neighbours
    i = ncols // 2
    width = min(nrows, ncols - i)
    b2 = np.arange(i, i + width, dtype=np.int64)
    cn = np.arange(1, width + 1, dtype=np.int32)
    cn[width // 2] = INT32_MAX
    cn[::3] = 0  # explicit zeros: stored as 0, counted in n_in and not in nnz_in
    band = check_list(ex, nrows, ncols, np.full(width, i, dtype=np.int64), b2, cn, 0)
    assert int((band != 0).sum()) == int((cn != 0).sum())


def test_the_result_does_not_depend_on_the_stream(ex):
    import torch

    nrows, ncols = 200, 700
    b1, b2, cn = band_pixels(host_band(nrows, ncols, "tenth", seed=5), nrows, ncols, 11)
    a = check_list(ex, nrows, ncols, b1, b2, cn, 11)
    s = torch.cuda.Stream()
    b = check_list(ex, nrows, ncols, b1, b2, cn, 11, stream=s)
    s.synchronize()
    assert np.array_equal(a, b)


def spoilt_lists():
    nrows, ncols = 40, 65
    b1, b2, cn = band_pixels(host_band(nrows, ncols, "tenth", seed=7), nrows, ncols, 3)
    n = len(b1)
    assert n > 50
    out = []
    for k in (0, n // 2, n - 2):  # a swap of the entries k and k + 1: the first, a middle and the last pair
        s1, s2 = b1.copy(), b2.copy()
        s1[[k, k + 1]], s2[[k, k + 1]] = s1[[k + 1, k]], s2[[k + 1, k]]
        out.append((f"swap@{k}", s1, s2, cn))
    for k in (0, n // 2, n - 1):  # entry k twice
        out.append((f"duplicate@{k}", np.insert(b1, k, b1[k]), np.insert(b2, k, b2[k]), np.insert(cn, k, cn[k])))
    for k in (0, n // 2, n - 1):
        c = cn.copy()
        c[k] = -1 if k else -INT32_MAX - 1
        out.append((f"negative@{k}", b1, b2, c))
    both = cn.copy()  # a negative count before and at a swap
    both[n // 2 + 1] = -5
    out.append(("both", out[1][1], out[1][2], both))
    return nrows, ncols, out


@pytest.mark.parametrize("case", range(10))
def test_lists_that_are_refused(ex, case):
    from modle_amd import pixels

    nrows, ncols, lists = spoilt_lists()
    what, b1, b2, cn = lists[case]
    code, first_bad = reference_order(b1, b2, cn)
    assert code == (ERR_RANGE if what.startswith("negative") else ERR_ORDER) and first_bad >= 0
    _, st = reference_band(nrows, ncols, b1, b2, cn, 3)
    d1, d2, dc = Dev64(b1), Dev64(b2), counts_dev(cn)
    with pytest.raises(pixels.BandListError) as e:
        ex.band_check(d1.data_ptr(), d2.data_ptr(), dc.data_ptr(), len(b1), nrows, ncols, 3)
    assert e.value.code == code and e.value.stats._asdict() == st and str(first_bad) in str(e.value), what
    out = poisoned_band(nrows, ncols)
    with pytest.raises(pixels.BandListError) as e:
        ex.band_from_host(b1, b2, cn, nrows, ncols, 3, out.data_ptr(), out.n)
    assert e.value.code == code and e.value.stats.first_bad == first_bad
    assert out.unchanged()  # nothing is written


def test_invalid_arguments_leave_everything_untouched(ex):
    from modle_amd import pixels

    L = pixels.lib()
    nrows, ncols = 7, 30
    b1, b2, cn = band_pixels(host_band(nrows, ncols, "tenth"), nrows, ncols)
    n = len(b1)
    d1, d2, dc = Dev64(b1), Dev64(b2), counts_dev(cn)
    rows, out = Dev64(np.full(ncols + 1, -1, dtype=np.int64)), poisoned_band(nrows, ncols)
    st = pixels._CBandStats()
    p1, p2, pc, pr, po, words = d1.data_ptr(), d2.data_ptr(), dc.data_ptr(), rows.data_ptr(), out.data_ptr(), out.n
    h = ex._h
    check = lambda *a: pixels._call(L.modle_pixels_band_check, *a)
    fill = lambda *a: pixels._call(L.modle_pixels_band_fill, *a)
    host = lambda *a: pixels._call(L.modle_pixels_band_from_host, *a)
    hb1, hb2, hcn = b1.ctypes.data, b2.ctypes.data, cn.ctypes.data
    S = C.byref(st)
    cases = [
        ("check: null handle", check, (None, p1, p2, pc, n, nrows, ncols, 0, pr, S, None)),
        ("check: null stats", check, (h, p1, p2, pc, n, nrows, ncols, 0, pr, None, None)),
        ("check: null bin1", check, (h, None, p2, pc, n, nrows, ncols, 0, pr, S, None)),
        ("check: null count", check, (h, p1, p2, None, n, nrows, ncols, 0, pr, S, None)),
        ("check: n = 2^31", check, (h, p1, p2, pc, 2**31, nrows, ncols, 0, pr, S, None)),
        ("check: nrows > ncols", check, (h, p1, p2, pc, n, ncols + 1, ncols, 0, pr, S, None)),
        ("check: nrows == 0", check, (h, p1, p2, pc, n, 0, ncols, 0, pr, S, None)),
        ("check: misaligned bin1", check, (h, p1 + 4, p2, pc, n - 1, nrows, ncols, 0, pr, S, None)),
        ("check: misaligned row starts", check, (h, p1, p2, pc, n, nrows, ncols, 0, pr + 4, S, None)),
        ("check: row starts on bin2", check, (h, p1, p2, pc, n, nrows, ncols, 0, p2, S, None)),
        ("fill: null handle", fill, (None, p2, pc, n, nrows, ncols, 0, pr, po, words, None)),
        ("fill: null output", fill, (h, p2, pc, n, nrows, ncols, 0, pr, None, words, None)),
        ("fill: null row starts", fill, (h, p2, pc, n, nrows, ncols, 0, None, po, words, None)),
        ("fill: null bin2", fill, (h, None, pc, n, nrows, ncols, 0, pr, po, words, None)),
        ("fill: n = 2^31", fill, (h, p2, pc, 2**31, nrows, ncols, 0, pr, po, words, None)),
        ("fill: nrows > ncols", fill, (h, p2, pc, n, ncols + 1, ncols, 0, pr, po, 10**6, None)),
        ("fill: ncols == 0", fill, (h, p2, pc, n, nrows, 0, 0, pr, po, words, None)),
        ("fill: a word short", fill, (h, p2, pc, n, nrows, ncols, 0, pr, po, words - 1, None)),
        ("fill: misaligned bin2", fill, (h, p2 + 4, pc, n - 1, nrows, ncols, 0, pr, po, words, None)),
        ("fill: misaligned row starts", fill, (h, p2, pc, n, nrows, ncols, 0, pr + 4, po, words, None)),
        ("fill: output on the counts", fill, (h, p2, pc, n, nrows, ncols, 0, pr, pc, words, None)),
        ("fill: output on bin2", fill, (h, p2, pc, n, nrows, ncols, 0, pr, p2 + 8, words, None)),
        ("fill: output on the row starts", fill, (h, p2, pc, n, nrows, ncols, 0, pr, pr + 8 * ncols, words, None)),
        ("host: null handle", host, (None, hb1, hb2, hcn, n, nrows, ncols, 0, po, words, S, None)),
        ("host: null stats", host, (h, hb1, hb2, hcn, n, nrows, ncols, 0, po, words, None, None)),
        ("host: null output", host, (h, hb1, hb2, hcn, n, nrows, ncols, 0, None, words, S, None)),
        ("host: null bin2", host, (h, hb1, None, hcn, n, nrows, ncols, 0, po, words, S, None)),
        ("host: n = 2^31", host, (h, hb1, hb2, hcn, 2**31, nrows, ncols, 0, po, words, S, None)),
        ("host: nrows > ncols", host, (h, hb1, hb2, hcn, n, ncols + 1, ncols, 0, po, 10**6, S, None)),
        ("host: a word short", host, (h, hb1, hb2, hcn, n, nrows, ncols, 0, po, words - 1, S, None)),
    ]
    for what, call, args in cases:
        with pytest.raises(pixels.PixelsError) as e:
            call(*args)
        assert e.value.code == pixels.ERR_ARG, what
    for g in (d1, d2, dc, rows, out):
        assert g.unchanged()
    # d_out needs 4-byte alignment only, and the calls still work after the refusals
    assert po % 8 == 4
    ex.band_check(p1, p2, pc, n, nrows, ncols, 0, pr)
    ex.band_fill_into(p2, pc, n, nrows, ncols, 0, pr, po, words)
    assert np.array_equal(band_words(out), reference_band(nrows, ncols, b1, b2, cn)[0])


def test_fill_stays_inside_whatever_the_arrays_hold(ex):
    """row starts of garbage and a list that breaks the order: the kernel clamps what it reads and derives every
    (i, j) anew, so only the guards and the absence of an error are asserted; the band is unspecified"""
    import torch

    rng = np.random.default_rng(13)
    for nrows, ncols in [(7, 30), (65, 65), (DIAGS + 1, 200)]:
        b1, b2, cn = band_pixels(host_band(nrows, ncols, "full", seed=9), nrows, ncols)
        n = len(b1)
        order = rng.permutation(n)
        d2, dc = Dev64(b2[order]), counts_dev(cn[order])
        for garbage in (np.full(ncols + 1, -1, dtype=np.int64),  # POISON in every word
                        rng.integers(-2**63, 2**63 - 1, size=ncols + 1, dtype=np.int64),
                        rng.integers(-5, n + 5, size=ncols + 1, dtype=np.int64),
                        np.full(ncols + 1, 2**62, dtype=np.int64)):
            rows, out = Dev64(garbage), poisoned_band(nrows, ncols)
            ex.band_fill_into(d2.data_ptr(), dc.data_ptr(), n, nrows, ncols, 0, rows.data_ptr(), out.data_ptr(), out.n)
            torch.cuda.synchronize()
            assert out.guards_intact() and rows.unchanged() and d2.unchanged() and dc.unchanged()
            assert not (band_words(out)[np.where(host_band(nrows, ncols, "full") == POISON)] != 0).any()


def test_loaded_bands(ex):
    """api.LoadedBands: a band from pixels, cross-checked by the count kernel, and every analysis on it"""
    import torch

    from modle_amd import api

    nrows, ncols, off = 40, 65, 1000
    b1, b2, cn = band_pixels(host_band(nrows, ncols, "tenth", seed=21), nrows, ncols, off)
    w1, w2, wc = weave(b1, b2, cn, nrows, ncols, off, 4)
    want, st = reference_band(nrows, ncols, w1, w2, wc, off)
    with api.LoadedBands(0) as lb:
        bid, stats = lb.load_pixels(w1, w2, wc, nrows, ncols, off)
        assert stats._asdict() == st and stats.n_beyond > 0 and stats.n_outside > 0
        t = lb.band(bid)
        assert t.dtype == torch.int32 and t.numel() == nrows * ncols + 1
        assert np.array_equal(t.cpu().numpy().view(np.uint32), want)
        assert lb.outputs(bid) == (t.data_ptr(), None, nrows, ncols) and lb.copy_outputs(bid) == (None, 0, None)
        px = lb.pixels(bid, off)
        keep = wc[reference_classes(nrows, ncols, w1, w2, off) == 0] != 0
        assert px.stats.nnz == st["nnz_in"] == int(keep.sum()) and px.stats.sum == st["sum_in"]
        diag_sum, coverage = lb.marginals(bid)
        assert int(diag_sum.sum()) == st["sum_in"]
        again = lb.add_band(t.clone(), nrows, ncols)
        assert again == bid + 1 and lb.pixels(again, off).stats == px.stats
        with pytest.raises(ValueError):
            lb.add_band(t[:-1], nrows, ncols)
