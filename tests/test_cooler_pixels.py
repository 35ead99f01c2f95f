"""modle_cool_append_pixels (include/modle_cooler_pixels.h): a cooler written from sorted sparse
pixels is identical, dataset for dataset and attribute for attribute (the creation date apart),
to the one modle_cool_append_matrix writes from the dense band; invalid pixels are rejected and
leave the file as it was.  The pixels come from a numpy reference in this module (the row-by-row
visit modle_cool_append_matrix documents), never from the code under test."""
import json
import os
import subprocess

import numpy as np
import pytest

from modle_amd import cooler

H5PY_PYTHON = "/opt/conda/bin/python3.9"  # an interpreter with h5py (tests/h5py_cooler_reader.py)
BIN_SIZE = 5000


def read_cooler(path):
    assert os.path.exists(H5PY_PYTHON), f"{H5PY_PYTHON} (h5py) is missing"
    env = {k: v for k, v in os.environ.items() if not k.startswith("PYTHON")}
    out = subprocess.run([H5PY_PYTHON, os.path.join(os.path.dirname(__file__), "h5py_cooler_reader.py"),
                          path], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stderr
    return json.loads(out.stdout)


def assert_same_cooler(path_a, path_b):
    a, b = read_cooler(path_a), read_cooler(path_b)
    assert a.keys() == b.keys()
    a["attrs"].pop("creation-date")
    b["attrs"].pop("creation-date")
    for key in a:
        assert a[key] == b[key], key
    return a


def reference_pixels(band, nrows, ncols, bin_offset=0):
    """for i: for d < min(nrows, ncols - i): v = band[(i + d) * nrows + d]; keep if v != 0"""
    b1, b2, cn, off = [], [], [], [0]
    for i in range(ncols):
        for d in range(min(nrows, ncols - i)):
            v = int(band[(i + d) * nrows + d])
            if v != 0:
                b1.append(bin_offset + i)
                b2.append(bin_offset + i + d)
                cn.append(v)
        off.append(len(b1))
    return (np.array(b1, dtype=np.int64), np.array(b2, dtype=np.int64), np.array(cn, dtype=np.int32),
            np.array(off, dtype=np.int64))


def random_band(rng, nrows, ncols, density):
    """seeded band in the library's layout; the words that are no pixels (left-edge triangle,
    trailing word) hold garbage that neither writer may look at"""
    band = np.zeros(nrows * ncols + 1, dtype=np.uint32)
    mask = rng.random(nrows * ncols) < density
    band[:nrows * ncols][mask] = rng.integers(1, 1000, size=int(mask.sum()))
    for j in range(min(nrows, ncols)):
        band[j * nrows + j + 1:(j + 1) * nrows] = 0xFFFFFFFF
    band[nrows * ncols] = 0xFFFFFFFF
    return band


CHROMS = [("chrA", 1_003_000), ("chrQuiet", 42_000), ("chrB", 600_000), ("chrTail", 77_777)]
# (chromosome, offset_bp, nrows, ncols, density): two intervals of chrA with offsets, chrQuiet
# without contacts in between, an interval of chrB without a single pixel, a whole chromosome
INTERVALS = [("chrA", 100_000, 12, 30, 0.4), ("chrA", 500_000, 40, 90, 0.3),
             ("chrB", 50_000, 16, 40, 0.0), ("chrB", 300_000, 20, 20, 0.6),
             ("chrTail", 0, 7, 16, 1.0)]


def write_both(tmp_path, with_index):
    rng = np.random.default_rng(20)
    dense, sparse = str(tmp_path / "dense.cool"), str(tmp_path / "sparse.cool")
    n_pixels = 0
    with cooler.CoolerWriter(dense, CHROMS, BIN_SIZE, assembly="asm", generated_by="gen",
                             metadata_json='{"k": 1}') as wd, \
            cooler.CoolerWriter(sparse, CHROMS, BIN_SIZE, assembly="asm", generated_by="gen",
                                metadata_json='{"k": 1}') as ws:
        for name, off_bp, nrows, ncols, density in INTERVALS:
            band = random_band(rng, nrows, ncols, density)
            wd.append(name, band, nrows, ncols, offset_bp=off_bp)
            bin_offset = ws.bin_offset(name, off_bp)
            b1, b2, cn, off = reference_pixels(band, nrows, ncols, bin_offset)
            assert (len(b1) == 0) == (density == 0.0)
            ws.append_pixels(name, ncols, b1, b2, cn, bin1_offset=off if with_index else None,
                             offset_bp=off_bp)
            n_pixels += len(b1)
    return dense, sparse, n_pixels


@pytest.mark.parametrize("with_index", [True, False])
def test_file_from_pixels_equals_file_from_the_dense_band(tmp_path, with_index):
    dense, sparse, n_pixels = write_both(tmp_path, with_index)
    got = assert_same_cooler(dense, sparse)
    assert got["n_pixels"] == n_pixels > 1000 and got["attrs"]["nnz"] == n_pixels
    assert got["pixels_by_chrom"]["chrQuiet"] == [] and len(got["pixels_by_chrom"]["chrA"]) > 500
    assert got["attrs"]["sum"] == got["attrs"]["cis"] == sum(
        p[2] for rows in got["pixels_by_chrom"].values() for p in rows)


def test_bin_offset_is_the_chromosome_s_first_bin_plus_the_interval_s(tmp_path):
    with cooler.CoolerWriter(str(tmp_path / "o.cool"), CHROMS, BIN_SIZE) as w:
        nb = [-(-s // BIN_SIZE) for _, s in CHROMS]
        assert w.bin_offset("chrA") == 0 and w.bin_offset("chrA", 100_000) == 20
        assert w.bin_offset("chrB", 50_000) == nb[0] + nb[1] + 10
        assert w.bin_offset(3) == nb[0] + nb[1] + nb[2]


def test_rejected_pixels_leave_the_file_unharmed(tmp_path):
    """every bad call fails with its code and changes nothing: the file that is finished after
    them equals one that never saw them"""
    rng = np.random.default_rng(5)
    chroms = [("c1", 200_000), ("c2", 100_000)]  # 40 and 20 bins
    band1, band2 = random_band(rng, 6, 20, 0.5), random_band(rng, 5, 12, 0.5)
    clean, path = str(tmp_path / "clean.cool"), str(tmp_path / "bad.cool")
    with cooler.CoolerWriter(clean, chroms, BIN_SIZE) as w:
        w.append_pixels("c1", 20, *reference_pixels(band1, 6, 20, 10)[:3], offset_bp=50_000)
        w.append_pixels("c2", 12, *reference_pixels(band2, 5, 12, 40)[:3])

    def i64(*x):
        return np.array(x, dtype=np.int64)

    def i32(*x):
        return np.array(x, dtype=np.int32)

    w = cooler.CoolerWriter(path, chroms, BIN_SIZE)
    b1, b2, cn, off = reference_pixels(band1, 6, 20, 10)
    bad = [
        ("unsorted bin1", -1, (i64(12, 11), i64(12, 11), i32(1, 1), None)),
        ("unsorted bin2", -1, (i64(11, 11), i64(13, 12), i32(1, 1), None)),
        ("duplicate", -1, (i64(11, 11), i64(12, 12), i32(1, 1), None)),
        ("bin2 < bin1", -1, (i64(12), i64(11), i32(1), None)),
        ("count 0", -1, (i64(11, 12), i64(11, 12), i32(3, 0), None)),
        ("negative count", -3, (i64(11), i64(11), i32(-2), None)),
        ("bin1 before the interval", -3, (i64(9), i64(12), i32(1), None)),
        ("bin2 beyond the interval", -3, (i64(29), i64(30), i32(1), None)),
        ("id beyond the chromosome", -3, (i64(29), i64(45), i32(1), None)),
        ("index does not match", -1, (b1, b2, cn, np.roll(off, 1))),
    ]
    for what, code, (x1, x2, xc, xo) in bad:
        with pytest.raises(cooler.CoolerError) as e:
            w.append_pixels("c1", 20, x1, x2, xc, bin1_offset=xo, offset_bp=50_000)
        assert e.value.code == code, what
    with pytest.raises(cooler.CoolerError) as e:  # 20 bins from bin 30 of a chromosome of 40
        w.append_pixels("c1", 20, i64(), i64(), i32(), offset_bp=150_000)
    assert e.value.code == -3
    w.append_pixels("c1", 20, b1, b2, cn, bin1_offset=off, offset_bp=50_000)
    for what, off_bp in (("overlaps the interval before", 100_000), ("starts before it", 0)):
        with pytest.raises(cooler.CoolerError) as e:  # out-of-order intervals
            w.append_pixels("c1", 5, i64(), i64(), i32(), offset_bp=off_bp)
        assert e.value.code == -1, what
    w.append_pixels("c2", 12, *reference_pixels(band2, 5, 12, 40)[:3])
    with pytest.raises(cooler.CoolerError) as e:  # a chromosome before the last one
        w.append_pixels("c1", 2, i64(), i64(), i32(), offset_bp=190_000)
    assert e.value.code == -1
    w.close()
    got = assert_same_cooler(clean, path)
    assert got["n_pixels"] == len(b1) + len(reference_pixels(band2, 5, 12, 40)[0])


def test_pixels_and_matrices_mix_in_one_file(tmp_path):
    """both entry points keep the same indexes: a file may take one interval from each"""
    rng = np.random.default_rng(9)
    chroms = [("c1", 200_000), ("c2", 100_000)]
    band1, band2 = random_band(rng, 6, 20, 0.5), random_band(rng, 5, 20, 0.5)
    a, b = str(tmp_path / "a.cool"), str(tmp_path / "b.cool")
    with cooler.CoolerWriter(a, chroms, BIN_SIZE) as w:
        w.append("c1", band1, 6, 20, offset_bp=25_000)
        w.append("c2", band2, 5, 20)
    with cooler.CoolerWriter(b, chroms, BIN_SIZE) as w:
        w.append("c1", band1, 6, 20, offset_bp=25_000)
        w.append_pixels("c2", 20, *reference_pixels(band2, 5, 20, w.bin_offset("c2")))
    assert_same_cooler(a, b)


def test_the_header_s_symbols_are_exported():
    import re

    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "modle_cooler_pixels.h")).read()
    names = set(re.findall(r"\b(modle_cool_[a-z_0-9]+)\s*\(", header))
    assert names == {"modle_cool_bin_offset", "modle_cool_append_pixels"}
    for n in names:
        assert hasattr(cooler.lib(), n)
