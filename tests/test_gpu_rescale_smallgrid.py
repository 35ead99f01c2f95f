"""modle_pixels_rescale with its launch cap lowered (`make -C modle_amd/pixels smallgrid`:
modle_amd/libmodle_pixels_smallgrid.so; include/modle_pixels.h: modle_pixels_rescale_groups).  The header promises
that no result depends on the launch geometry; with the default cap of 256 workgroups a workgroup takes one to
three windows of the lists a test can afford.  In the lowered build two workgroups share every list, hundreds of
windows each, and their partial sums are added.  The library is chosen at import, so the comparisons run in
tests/rescale_smallgrid_child.py, once, under a time limit; this module reports what the child printed."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 300  # seconds: the child takes well under a minute
CASES = 2 * (9 * 5 + 1)  # two fills, nine shapes of five lists, and the long list of one shape


def test_the_default_library_has_the_documented_cap():
    """(no device is needed)"""
    from modle_amd import pixels

    if "MODLE_PIXELS_LIB" in os.environ:
        pytest.fail("MODLE_PIXELS_LIB is set: this suite tests the default build")
    assert pixels.rescale_groups() == 256
    assert pixels.build_caps() == pixels.DEFAULT_BUILD_CAPS  # (its four words are what they were)


@pytest.fixture(scope="module")
def child():
    """the child's (return code, output), run once; a fault, an abort or the time limit ends it and fails the
    test that asks for it, and nothing more is started"""
    so = os.path.join(ROOT, "modle_amd", "libmodle_pixels_smallgrid.so")
    assert os.path.exists(so), f"{so} is missing: run `make -C modle_amd/pixels smallgrid`"
    env = dict(os.environ, MODLE_PIXELS_LIB="libmodle_pixels_smallgrid.so")
    p = subprocess.run(["timeout", "-k", "10", str(LIMIT), sys.executable,
                        os.path.join(ROOT, "tests", "rescale_smallgrid_child.py")], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    return p.returncode, p.stdout


@pytest.mark.gpu
def test_the_lowered_build_computes_the_same_words(child):
    code, out = child
    print(out)
    assert code not in (124, 137), f"the child did not finish within {LIMIT} s:\n{out[-3000:]}"
    assert code == 0, f"the child ended with {code}:\n{out[-3000:]}"
    assert "rescale groups 2" in out
    assert f"rescale: {CASES} cases equal their restatements" in out
