"""The pixel library with its launch caps lowered (`make -C modle_amd/pixels smallgrid`:
modle_amd/libmodle_pixels_smallgrid.so; include/modle_pixels.h: modle_pixels_build_caps).  The headers of
pixels_scan, band_check, band_fill and the three stripes kernels promise that no result depends on the launch
geometry; the default caps (2^20 workgroups, a grid y of 65535, 1024 workgroups, 1024 threads) are out of the
reach of a band a test can afford -- stripes_horizontal would need 67 million columns, band_fill 8.4 million
diagonals.  In the lowered build the loops behind the caps take many trips on the small shapes of the other
modules.  The library is chosen at import, so the comparisons run in tests/pixels_smallgrid_child.py, once,
under a time limit; this module reports what the child printed."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 300  # seconds: the child takes well under a minute


def test_the_default_library_has_the_documented_caps():
    """(no device is needed) the values include/modle_pixels.h documents, and the ones the shapes of
    tests/test_gpu_long_bands.py are chosen around"""
    from modle_amd import pixels

    if "MODLE_PIXELS_LIB" in os.environ:
        pytest.fail("MODLE_PIXELS_LIB is set: this suite tests the default build")
    assert pixels.build_caps() == pixels.DEFAULT_BUILD_CAPS == (2**20, 65535, 1024, 1024)
    assert os.path.basename(pixels.SO_PATH) == "libmodle_pixels.so"


@pytest.fixture(scope="module")
def child():
    """the child's (return code, output), run once; a fault, an abort or the time limit ends it and fails every
    test that asks for it, and nothing more is started"""
    so = os.path.join(ROOT, "modle_amd", "libmodle_pixels_smallgrid.so")
    assert os.path.exists(so), f"{so} is missing: run `make -C modle_amd/pixels smallgrid`"
    env = dict(os.environ, MODLE_PIXELS_LIB="libmodle_pixels_smallgrid.so")
    p = subprocess.run(["timeout", "-k", "10", str(LIMIT), sys.executable,
                        os.path.join(ROOT, "tests", "pixels_smallgrid_child.py")], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    return p.returncode, p.stdout


@pytest.mark.gpu
def test_the_lowered_build_computes_the_same_words(child):
    code, out = child
    print(out)
    assert code not in (124, 137), f"the child did not finish within {LIMIT} s:\n{out[-3000:]}"
    assert code == 0, f"the child ended with {code}:\n{out[-3000:]}"
    assert "caps (3, 2, 2, 64)" in out
    for group in ("extraction", "band_loading", "stripes"):
        assert f"{group}: " in out and "cases equal their restatements" in out, group
