"""Child process of tests/test_gpu_pixels_smallgrid.py: the pixel library is chosen when modle_amd.pixels is
imported (MODLE_PIXELS_LIB), so a run with the build of `make -C modle_amd/pixels smallgrid` lives in its own
interpreter.  That build caps the grids of the stripes kernels at 3 workgroups, the grid's y of band_fill at
2 and band_check at 2 workgroups, and scans bin1_offset 64 columns at a time: on the small shapes of the
other GPU modules every capped loop takes many trips, and the results must be the same words -- nothing may
depend on the launch geometry.  Each comparison is against the same restatement the default build is held to.
Prints one line per group of cases and exits non-zero with the first difference."""
import os
import sys
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LOWERED = (3, 2, 2, 64)  # the Makefile's smallgrid target: stripes grid, fill grid y, check groups, scan threads


def extraction(ex):
    """test_gpu_pixels.py's shapes and fills: 130, 193 and 700 columns are 3, 4 and 11 trips of the scan"""
    import test_gpu_pixels as tp

    assert max(nc for _, nc in tp.SHAPES) > 10 * LOWERED[3]
    n = 0
    for nrows, ncols in tp.SHAPES:
        for fill in tp.FILLS:
            band = tp.make_band(nrows, ncols, fill)
            ref = tp.reference_pixels(band, nrows, ncols)
            t = tp.upload(band, nrows)
            tp.assert_equal_to_reference(ex.extract(t.data_ptr(), nrows, ncols), ref)
            tp.assert_equal_to_reference(ex.extract(t.data_ptr(), nrows, ncols, bin_offset=3_000_000_000), ref,
                                         3_000_000_000)
            assert t.unchanged(), (nrows, ncols, fill)
            n += 1
    return n


def band_loading(ex):
    """test_gpu_band.py's shapes and fills -- a list of more than 2 * 256 pixels strides band_check -- and bands
    of more than 2 * 128 diagonals, whose tiles along d a workgroup of band_fill takes in turn"""
    import test_gpu_band as tb
    from modle_amd import pixels
    from test_band_outputs import reference_band, reference_order

    assert (pixels.BAND_TILE_COLS, pixels.BAND_TILE_DIAGS) == (tb.COLS, tb.DIAGS)
    deep = [(2 * tb.DIAGS + 1, 300), (600, 640)]  # 3 and 5 tiles of diagonals on a grid y of 2
    assert all(nr > LOWERED[1] * tb.DIAGS for nr, _ in deep)
    n = 0
    for nrows, ncols in tb.SHAPES + deep:
        for fill in tb.FILLS:
            band = tb.host_band(nrows, ncols, fill)
            b1, b2, cn = tb.band_pixels(band, nrows, ncols)
            clean = np.where(band == tb.POISON, 0, band)
            assert np.array_equal(tb.check_list(ex, nrows, ncols, b1, b2, cn, 0), clean), (nrows, ncols, fill)
            woven = tb.weave(b1, b2, cn, nrows, ncols, 0, 1)
            assert np.array_equal(tb.check_list(ex, nrows, ncols, *woven, 0), clean), (nrows, ncols, fill)
            n += 2
    # the smallest bad index, found in a late trip of the two workgroups
    nrows, ncols = 200, 700
    b1, b2, cn = tb.band_pixels(tb.host_band(nrows, ncols, "tenth", seed=5), nrows, ncols, 3)
    trip = LOWERED[2] * 256
    assert len(b1) > 20 * trip
    for swaps, negatives in (((3 * trip, 9 * trip + 5), ()), ((), (5 * trip + 1, 6 * trip)),
                             ((7 * trip + 100,), (2 * trip,)), ((trip, 4 * trip + 7), (trip + 1,))):
        s1, s2, c = b1.copy(), b2.copy(), cn.copy()
        for k in swaps:
            s1[[k - 1, k]], s2[[k - 1, k]] = s1[[k, k - 1]], s2[[k, k - 1]]
        for k in negatives:
            c[k] = -3
        code, first_bad = reference_order(s1, s2, c)
        assert first_bad == min(swaps + negatives)
        _, st = reference_band(nrows, ncols, s1, s2, c, 3)
        d1, d2, dc = tb.Dev64(s1), tb.Dev64(s2), tb.counts_dev(c)
        try:
            ex.band_check(d1.data_ptr(), d2.data_ptr(), dc.data_ptr(), len(s1), nrows, ncols, 3)
        except pixels.BandListError as e:
            assert e.code == code and e.stats._asdict() == st, (swaps, negatives, e.stats, st)
        else:
            raise AssertionError(f"the list with swaps at {swaps} and negative counts at {negatives} was accepted")
        n += 1
    return n


def stripes(ex):
    """test_gpu_stripes.py's shapes up to 600 diagonals and its fills, and bands of more than 3 * 64 * 4
    columns: 3 workgroups take 12 vertical stripes, 192 horizontal stripes and 3 rank stripes per trip"""
    import test_gpu_stripes as ts
    from test_stripes_outputs import ROWS, restate

    long = [(3, 1000), (70, 800)]
    assert all(nc > LOWERED[0] * 64 * 4 for _, nc in long)
    n = 0
    for nrows, ncols in [s for s in ts.SHAPES if s[0] <= 600] + long:
        for fill in ts.FILLS:
            a, b = ts.make_pair(nrows, ncols, fill)
            want = restate(a, b, nrows, ncols, 7)
            ref, tgt = ts.Guarded(a), ts.Guarded(b)
            for what in ROWS:  # every mask: each of the three kernels alone and together
                words = 2 * ROWS[what] * ncols
                d_out = ts.GuardedOut(words)
                ex.stripes_into(ref.data_ptr(), tgt.data_ptr(), nrows, ncols, what, d_out.data_ptr(), words)
                got = d_out.sums(2 * ROWS[what]).reshape(2, ROWS[what], ncols)
                assert np.array_equal(got, ts.rows_of(want, what)), (nrows, ncols, fill, what)
                assert d_out.guards_intact()
            assert np.array_equal(ex.stripes(ref.data_ptr(), tgt.data_ptr(), nrows, ncols, 7), want)
            assert ref.unchanged() and tgt.unchanged()
            n += 1
    return n


def main():
    assert os.environ.get("MODLE_PIXELS_LIB") == "libmodle_pixels_smallgrid.so"
    from modle_amd import pixels

    caps = tuple(pixels.build_caps())
    # a variable the library ignored would leave the default caps, and every comparison below would pass on them
    assert caps == LOWERED, f"the loaded library has the caps {caps}, not the lowered {LOWERED}"
    print(f"caps {caps}", flush=True)
    with pixels.Extractor(0) as ex:
        for group in (extraction, band_loading, stripes):
            print(f"{group.__name__}: {group(ex)} cases equal their restatements", flush=True)


if __name__ == "__main__":
    try:
        main()
    except BaseException:
        traceback.print_exc()
        sys.exit(1)
