"""Child process of tests/test_gpu_rescale_smallgrid.py: the pixel library is chosen when modle_amd.pixels is
imported (MODLE_PIXELS_LIB), so a run with the build of `make -C modle_amd/pixels smallgrid` lives in its own
interpreter.  That build lets at most 2 workgroups take the windows of a rescaled pileup
(MODLE_RESCALE_MAX_GROUPS; the default is 256, which leaves a workgroup one to three windows of the lists of
tests/test_gpu_rescale.py): every workgroup then walks more than a hundred windows in turn, accepted and
rejected, and pixels_rescale_sum adds the partial sums of the two -- the results must be the same words.  Each
comparison is against the restatement the default build is held to.  Prints one line and exits non-zero with the
first difference."""
import os
import sys
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

GROUPS = 2  # the Makefile's smallgrid target
FILLS = ["tenth", "full"]
NAMES = ["mix", "n = 1", "n = 257", "all rejected", "exact multiples"]


def main():
    assert os.environ.get("MODLE_PIXELS_LIB") == "libmodle_pixels_smallgrid.so"
    import test_gpu_rescale as tr
    from modle_amd import pixels

    # a variable the library ignored would leave the default cap, and every comparison below would pass on it
    assert pixels.rescale_groups() == GROUPS, f"the loaded library spreads the windows over {pixels.rescale_groups()} workgroups"
    print(f"rescale groups {pixels.rescale_groups()}", flush=True)
    n = 0
    with pixels.Extractor(0) as ex:
        for nrows, ncols, r in tr.SHAPES:
            for fill in FILLS:
                src = tr.Guarded(tr.band_of(nrows, ncols, fill))
                for name in NAMES + (["long"] if (nrows, ncols, r) == tr.LONG else []):
                    s, e = tr.window_lists(nrows, ncols, r)[name]
                    want, want_area, used = tr.wanted(nrows, ncols, r, fill, name)
                    pile, area, n_used = tr.run(ex, src, nrows, ncols, r, s, e)
                    assert n_used == used and np.array_equal(pile, want) and np.array_equal(area, want_area), \
                        (nrows, ncols, r, fill, name)
                    n += 1
                s, e = tr.window_lists(nrows, ncols, r)["mix"]
                want, want_area, used = tr.wanted(nrows, ncols, r, fill, "mix")
                got = ex.rescale(src.data_ptr(), nrows, ncols, r, s, e)
                assert got[2] == used and np.array_equal(got[0], want) and np.array_equal(got[1], want_area)
                assert src.unchanged()
    print(f"rescale: {n} cases equal their restatements", flush=True)


if __name__ == "__main__":
    try:
        main()
    except BaseException:
        traceback.print_exc()
        sys.exit(1)
