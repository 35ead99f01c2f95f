"""Child process of tests/test_gpu_scc_smallgrid.py: the pixel library is chosen when modle_amd.pixels is imported
(MODLE_PIXELS_LIB), so a run with the build of `make -C modle_amd/pixels smallgrid` lives in its own interpreter.
That build lets at most 2 workgroups walk a strip of 64 strata (MODLE_SCC_MAX_GROUPS; the default is 128, which
spreads the tiles of the shapes below one to a workgroup): every workgroup then takes several tiles in turn and
carries its sums across them, and scc_fold adds the partial sums of both -- the results must be the same words.
Each comparison is against the restatement the default build is held to.  Prints one line and exits non-zero
with the first difference."""
import os
import sys
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

GROUPS = 2  # the Makefile's smallgrid target
# (nrows, ncols, h): 7 tiles of 32 rows and 11 tiles of 64 columns in the first strip, on 2 workgroups
SHAPES = [(129, 200, 5), (600, 700, 0)]


def main():
    assert os.environ.get("MODLE_PIXELS_LIB") == "libmodle_pixels_smallgrid.so"
    import test_gpu_scc as ts
    from modle_amd import pixels
    from test_scc_outputs import restate

    # a variable the library ignored would leave the default cap, and every comparison below would pass on it
    assert pixels.scc_groups() == GROUPS, f"the loaded library lets {pixels.scc_groups()} workgroups walk a strip"
    print(f"scc groups {pixels.scc_groups()}", flush=True)
    n = 0
    with pixels.Extractor(0) as ex:
        for nrows, ncols, h in SHAPES:
            assert -(-(ncols - 1) // (32 if h else 64)) >= 3 * GROUPS  # three trips and more in the first strip
            for fill in ts.FILLS:
                a, b = ts.make_pair(nrows, ncols, fill)
                ref, tgt = ts.Guarded(a), ts.Guarded(b)
                for lo, hi in (ts.default_strata(nrows, h), (0, nrows - 1 - 2 * h), (70, 100)):
                    want = restate(a, b, nrows, ncols, h, lo, hi)
                    got = ts.scc_into(ex, ref, tgt, nrows, ncols, h, lo, hi)
                    assert np.array_equal(got, want), (nrows, ncols, h, fill, lo, hi)
                    assert np.array_equal(ex.scc(ref.data_ptr(), tgt.data_ptr(), nrows, ncols, h, lo, hi), want)
                    n += 1
                assert ref.unchanged() and tgt.unchanged()
    print(f"scc: {n} cases equal their restatements", flush=True)


if __name__ == "__main__":
    try:
        main()
    except BaseException:
        traceback.print_exc()
        sys.exit(1)
