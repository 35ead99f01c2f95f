"""The jump table's plane layout in the GPU's LDS (modle_amd/csrc/jump_planes.h).

The host permutes the canonical table of `build_jump_table` before the upload, and the GPU's
`wave::lds_load_row` reads a row as two 16-byte halves at `jump_planes::half_row16`.  tests/jump_planes
holds a stand-alone host program (AddressSanitizer + UBSan) that applies that one index mapping and
checks that it is a bijection, and that the hop read through the plane addressing and through the
canonical addressing both equal 512 sequential generator steps -- on the 256 single-bit states, the
all-ones state and 10 000 seeded random states.
"""
import os
import subprocess

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jump_planes")


def test_plane_layout_is_a_bijection_and_hops_like_the_canonical_table():
    proc = subprocess.run(["make", "-C", HERE], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    proc = subprocess.run([os.path.join(HERE, "planes_check")], capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0, proc.stdout + proc.stderr[:4000]
    assert "Sanitizer" not in proc.stderr and "runtime error" not in proc.stderr, proc.stderr[:4000]
    assert "10257 states: plane hop == canonical hop == 512 steps" in proc.stdout
