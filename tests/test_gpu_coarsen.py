"""Band matrices coarsened on the MI355X (include/modle_pixels.h: modle_pixels_coarsen,
modle_pixels_coarse_to_host; modle_amd/pixels.py): the whole output buffer -- sums, and zeros in
the words that are no pixels -- equals, word for word, a numpy restatement of the definition in
this module, for bands built on the host with a seeded generator and uploaded between poisoned guard
words.  In every input band the words that are no pixels hold 0xFFFFFFFF: they must not be summed."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (nrows, ncols, factor, first_bin): one pixel; a band one word wide with a phase; everything into
# one pixel; a factor beyond the matrix, straddling two coarse bins; a factor beyond nrows; the
# largest factor on one full 64 x 64 band; one past 64 in both directions with an odd phase, factors
# 2 and 3; odd sizes with phase k - 1; several blocks with factors 2, 4 and 25 (nrows' = 25)
SHAPES = [(1, 1, 2, 0), (1, 7, 2, 1), (5, 5, 5, 0), (5, 5, 7, 3), (3, 64, 8, 5), (64, 64, 64, 0),
          (65, 130, 2, 1), (65, 130, 3, 2), (70, 193, 5, 4), (600, 700, 2, 1), (600, 700, 4, 3),
          (600, 700, 25, 7)]
# beyond that set: 64 outputs x factor 17 is a span of 1088 words, more than the kernel stages at a
# time, and the boundary of the staged chunk cuts through one output's words
SHAPES += [(1100, 1150, 17, 5)]
FILLS = ["empty", "tenth", "full"]
POISON = 0xFFFFFFFF
FRONT, BACK = 67, 96 * 601  # guard words (the front one leaves the band 4-byte aligned only)


def coarse_shape(nrows, ncols, k, first_bin):
    p = first_bin % k
    nc = (p + ncols + k - 1) // k
    return min(nc, (nrows - 1 + k - 1) // k + 1), nc


def reference_coarsen(band, nrows, ncols, k, first_bin):
    """for every fine pixel (i, j), d = j - i < nrows: coarse (I, J) = ((i + p) / k, (j + p) / k) gets
    band[j * nrows + d]; sums above 32 bits saturate; every other word of the result is 0"""
    p = first_bin % k
    nr, nc = coarse_shape(nrows, ncols, k, first_bin)
    out = np.zeros(nr * nc + 1, dtype=np.uint64)
    for d in range(nrows):
        j = np.arange(d, ncols, dtype=np.int64)
        J, I = (j + p) // k, (j - d + p) // k
        assert (J < nc).all() and (J - I < nr).all()
        np.add.at(out, J * nr + (J - I), band[j * nrows + d].astype(np.uint64))
    return np.minimum(out, POISON).astype(np.uint32), nr, nc


def reference_pixels(band, nrows, ncols, bin_offset=0):
    """for i: for d < min(nrows, ncols - i): v = band[(i + d) * nrows + d]; keep if v != 0"""
    b1, b2, cn, off = [], [], [], [0]
    total, largest = 0, 0
    for i in range(ncols):
        n = min(nrows, ncols - i)
        row = band[i * nrows:i * nrows + (n - 1) * (nrows + 1) + 1:nrows + 1]  # d = 0 .. n - 1
        assert len(row) == n
        d = np.flatnonzero(row)
        b1.append(np.full(len(d), bin_offset + i, dtype=np.int64))
        b2.append(bin_offset + i + d.astype(np.int64))
        cn.append(row[d])
        off.append(off[-1] + len(d))
        total += int(row.astype(np.uint64).sum())
        largest = max(largest, int(row.max()))
    return {"bin1": np.concatenate(b1), "bin2": np.concatenate(b2), "count": np.concatenate(cn),
            "bin1_offset": np.array(off, dtype=np.int64), "nnz": off[-1], "sum": total, "max_count": largest}


def make_band(nrows, ncols, fill, limit, seed=0):
    rng = np.random.default_rng([seed, nrows, ncols])
    band = np.zeros(nrows * ncols + 1, dtype=np.uint32)
    if fill == "full":
        band[:-1] = rng.integers(1, limit, size=nrows * ncols, dtype=np.int64)
    elif fill == "tenth":
        mask = rng.random(nrows * ncols) < 0.1
        band[:-1][mask] = rng.integers(1, limit, size=int(mask.sum()))
    for j in range(min(nrows, ncols)):
        band[j * nrows + j + 1:(j + 1) * nrows] = POISON
    band[nrows * ncols] = POISON
    return band


class Guarded:
    """`words` in device memory between guard words that hold POISON, at an address that is 4-byte
    aligned only: a read or a write beyond either end shows up"""

    def __init__(self, words):
        import torch

        self.n = len(words)
        self.host = np.full(FRONT + self.n + BACK, POISON, dtype=np.uint32)
        self.host[FRONT:FRONT + self.n] = words
        self.tensor = torch.from_numpy(self.host.view(np.int32)).to("cuda:0")
        torch.cuda.synchronize()

    def data_ptr(self):
        return self.tensor.data_ptr() + 4 * FRONT

    def read(self):
        import torch

        torch.cuda.synchronize()
        return self.tensor.cpu().numpy().view(np.uint32)

    def unchanged(self):
        return np.array_equal(self.read(), self.host)

    def guards_intact(self):
        got = self.read()
        return (got[:FRONT] == POISON).all() and (got[FRONT + self.n:] == POISON).all()

    def words(self):
        return self.read()[FRONT:FRONT + self.n]


def output_buffer(n_words):
    return Guarded(np.full(n_words, POISON, dtype=np.uint32))  # the caller does not pre-zero


def assert_pixels(got, ref, bin_offset=0):
    b1, b2, cn, off, stats = got
    assert (b1.dtype, b2.dtype, cn.dtype, off.dtype) == (np.int64, np.int64, np.int32, np.int64)
    assert (stats.nnz, stats.sum, stats.max_count) == (ref["nnz"], ref["sum"], ref["max_count"])
    assert np.array_equal(off, ref["bin1_offset"])
    assert np.array_equal(b1, ref["bin1"] + bin_offset)
    assert np.array_equal(b2, ref["bin2"] + bin_offset)
    assert np.array_equal(cn.view(np.uint32), ref["count"])


@pytest.fixture(scope="module")
def ex():
    from modle_amd import pixels

    with pixels.Extractor(0) as e:
        yield e


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("nrows,ncols,k,first_bin", SHAPES)
def test_coarse_band_equals_the_definition(ex, nrows, ncols, k, first_bin, fill):
    from modle_amd import pixels

    band = make_band(nrows, ncols, fill, 2**18 if k == 64 else 2**20)
    ref, nr, nc = reference_coarsen(band, nrows, ncols, k, first_bin)
    assert int(ref.max()) < 2**31  # no sum saturates
    if fill == "full":
        assert np.count_nonzero(ref) == sum(min(nr, J + 1) for J in range(nc))
    assert pixels.coarse_shape(nrows, ncols, k, first_bin) == (nr, nc)
    src, dst = Guarded(band), output_buffer(nr * nc + 1)
    assert ex.coarsen_into(src.data_ptr(), nrows, ncols, k, first_bin, dst.data_ptr(), nr * nc + 1) == (nr, nc)
    # the whole buffer: sums, and zeros in the triangle and the trailing word
    assert np.array_equal(dst.words(), ref)
    assert dst.guards_intact() and src.unchanged()
    # the one-call form: the pixels of the coarse band, also with ids beyond 32 bits
    want = reference_pixels(ref, nr, nc)
    assert_pixels(ex.coarse_extract(src.data_ptr(), nrows, ncols, k, first_bin), want)
    offset = 3_000_000_000
    assert_pixels(ex.coarse_extract(src.data_ptr(), nrows, ncols, k, first_bin, bin_offset=offset), want, offset)
    assert src.unchanged()


def test_a_sum_beyond_32_bits_saturates_and_is_a_range_error(ex):
    from modle_amd import pixels

    nrows, ncols, k = 5, 10, 5
    band = make_band(nrows, ncols, "tenth", 1000, seed=3)
    band[1 * nrows + 0], band[3 * nrows + 2] = 0x80000000, 0x80000000  # pixels (1, 1) and (1, 3): block (0, 0)
    ref, nr, nc = reference_coarsen(band, nrows, ncols, k, 0)
    assert (nr, nc) == (2, 2) and ref[0] == POISON
    src, dst = Guarded(band), output_buffer(nr * nc + 1)
    ex.coarsen_into(src.data_ptr(), nrows, ncols, k, 0, dst.data_ptr(), nr * nc + 1)
    assert np.array_equal(dst.words(), ref) and dst.words()[0] == POISON
    with pytest.raises(pixels.PixelsError) as e:
        ex.coarse_extract(src.data_ptr(), nrows, ncols, k, 0)
    assert e.value.code == pixels.ERR_RANGE
    # the largest sum that fits passes exactly, and the context serves the next call
    band[1 * nrows + 0], band[3 * nrows + 2] = 0x40000000, 0x3FFFFFFF
    rest = int(reference_coarsen(band, nrows, ncols, k, 0)[0][0]) - 0x7FFFFFFF
    band[3 * nrows + 2] -= rest  # (the other pixels of the block)
    ref, _, _ = reference_coarsen(band, nrows, ncols, k, 0)
    assert ref[0] == 0x7FFFFFFF
    src = Guarded(band)
    got = ex.coarse_extract(src.data_ptr(), nrows, ncols, k, 0)
    assert_pixels(got, reference_pixels(ref, nr, nc))
    assert got[4].max_count == 0x7FFFFFFF


def test_by_two_then_by_three_equals_by_six(ex):
    nrows, ncols, first_bin = 70, 193, 4
    band = make_band(nrows, ncols, "tenth", 2**20, seed=6)
    src = Guarded(band)
    r2, nr2, nc2 = reference_coarsen(band, nrows, ncols, 2, first_bin)
    r6, nr6, nc6 = reference_coarsen(band, nrows, ncols, 6, first_bin)
    mid, end, direct = output_buffer(nr2 * nc2 + 1), output_buffer(nr6 * nc6 + 1), output_buffer(nr6 * nc6 + 1)
    ex.coarsen_into(src.data_ptr(), nrows, ncols, 2, first_bin, mid.data_ptr(), nr2 * nc2 + 1)
    assert ex.coarsen_into(mid.data_ptr(), nr2, nc2, 3, first_bin // 2, end.data_ptr(), nr6 * nc6 + 1) == (nr6, nc6)
    ex.coarsen_into(src.data_ptr(), nrows, ncols, 6, first_bin, direct.data_ptr(), nr6 * nc6 + 1)
    assert np.array_equal(mid.words(), r2)
    assert np.array_equal(direct.words(), r6) and np.array_equal(end.words(), r6)
    assert mid.guards_intact() and end.guards_intact() and direct.guards_intact() and src.unchanged()


def test_a_stream_of_the_caller_and_a_scratch_that_grows():
    import torch

    from modle_amd import pixels

    stream = torch.cuda.Stream(device="cuda:0")
    assert stream.cuda_stream != 0
    small, large = make_band(5, 9, "full", 1000, seed=7), make_band(70, 193, "tenth", 2**20, seed=7)
    want_small = reference_pixels(*reference_coarsen(small, 5, 9, 2, 1))
    want_large = reference_pixels(*reference_coarsen(large, 70, 193, 3, 2))
    s, l = Guarded(small), Guarded(large)
    with pixels.Extractor(0) as e:
        first = e.coarse_extract(s.data_ptr(), 5, 9, 2, 1, 5, stream=stream)
        assert_pixels(first, want_small, 5)
        assert_pixels(e.coarse_extract(l.data_ptr(), 70, 193, 3, 2, stream=stream), want_large)  # grows
        assert_pixels(e.coarse_extract(s.data_ptr(), 5, 9, 2, 1, 5, stream=stream), want_small, 5)  # reused
        assert_pixels(e.extract(s.data_ptr(), 5, 9), reference_pixels(small, 5, 9))  # the fine path still serves
        assert_pixels(first, want_small, 5)  # the arrays handed out are the caller's
    # the module-level form (the process-wide context of the device)
    assert_pixels(pixels.coarse_extract(l.data_ptr(), 70, 193, 3, 2, bin_offset=11), want_large, 11)
    assert s.unchanged() and l.unchanged()


def test_invalid_calls_are_argument_errors_and_write_nothing(ex):
    from modle_amd import pixels

    nrows, ncols = 5, 9
    src = Guarded(make_band(nrows, ncols, "full", 1000, seed=8))
    nr, nc = coarse_shape(nrows, ncols, 2, 1)
    dst = output_buffer(nr * nc + 1)
    for what, args in [("out_words too small", (nrows, ncols, 2, 1, dst.data_ptr(), nr * nc)),
                       ("factor 1", (nrows, ncols, 1, 0, dst.data_ptr(), nr * nc + 1)),
                       ("factor 0", (nrows, ncols, 0, 0, dst.data_ptr(), nr * nc + 1)),
                       ("nrows > ncols", (ncols + 1, ncols, 2, 0, dst.data_ptr(), nr * nc + 1)),
                       ("nrows 0", (0, ncols, 2, 0, dst.data_ptr(), nr * nc + 1))]:
        with pytest.raises(pixels.PixelsError) as e:
            ex.coarsen_into(src.data_ptr(), *args)
        assert e.value.code == pixels.ERR_ARG, what
    with pytest.raises(pixels.PixelsError) as e:
        ex.coarse_extract(src.data_ptr(), nrows, ncols, 1, 0)
    assert e.value.code == pixels.ERR_ARG
    assert dst.unchanged() and src.unchanged()


def test_simulate_writes_an_mcool_whose_levels_are_the_coarsened_base(tmp_path):
    """two chromosomes, 4 cells, an interval of chrA that starts at fine bin 5 (a multiple of neither
    factor) and all of chrB: the base group of the .mcool holds the datasets of the .cool the same
    command line writes without the option, and every coarse group holds the numpy coarsening of the
    base group's pixel table"""
    from test_mcool_writer import read_group

    from modle_amd import cli

    rng = np.random.default_rng(4)
    (tmp_path / "g.chrom.sizes").write_text("chrA\t1200000\nchrB\t400000\n")
    (tmp_path / "iv.bed").write_text("chrA\t25000\t1025000\nchrB\t0\t400000\n")
    lines = [f"{c}\t{p}\t{p + 19}\t.\t{rng.uniform(0.6, 1.0):.3f}\t{'+' if rng.random() < 0.5 else '-'}"
             for c, size, n in (("chrA", 1_200_000, 16), ("chrB", 400_000, 6))
             for p in sorted(rng.choice(size - 100, size=n, replace=False))]
    (tmp_path / "b.bed").write_text("\n".join(lines) + "\n")
    base = 5000
    common = ["simulate", "-c", str(tmp_path / "g.chrom.sizes"), "-b", str(tmp_path / "b.bed"), "-g",
              str(tmp_path / "iv.bed"), "-r", "5kb", "--ncells", "4", "--target-contact-density", "0.5",
              "--seed", "5", "-q"]
    assert cli.main(common + ["-o", str(tmp_path / "plain" / "run")]) == 0
    assert cli.main(common + ["-o", str(tmp_path / "multi" / "run"), "--mcool-resolutions", "15kb,10kb"]) == 0
    assert not (tmp_path / "multi" / "run.cool").exists() and not (tmp_path / "plain" / "run.mcool").exists()
    plain = read_group(str(tmp_path / "plain" / "run.cool"))
    mcool = str(tmp_path / "multi" / "run.mcool")
    fine = read_group(mcool, f"/resolutions/{base}")
    assert fine["resolutions"] == ["5000", "10000", "15000"] and fine["root_attrs"]["format"] == "HDF5::MCOOL"
    for key in ("chroms", "bins", "pixels_by_chrom", "bin1_offset", "chrom_offset", "n_pixels", "dtypes",
                "filters", "name_dtype", "members"):
        assert fine[key] == plain[key], key
    assert fine["n_pixels"] > 1000 and len(fine["pixels_by_chrom"]["chrB"]) > 100
    assert min(p[0] for p in fine["pixels_by_chrom"]["chrA"]) >= 5
    for b in (10000, 15000):
        k = b // base
        got = read_group(mcool, f"/resolutions/{b}")
        assert got["attrs"]["bin-size"] == b and got["attrs"]["sum"] == fine["attrs"]["sum"]
        assert got["bins"][1][:2] == [0, b]
        for c, name in enumerate(["chrA", "chrB"]):
            f0, c0 = fine["chrom_offset"][c], got["chrom_offset"][c]
            acc = {}
            for b1, b2, n in fine["pixels_by_chrom"][name]:
                key = ((b1 - f0) // k + c0, (b2 - f0) // k + c0)
                acc[key] = acc.get(key, 0) + n
            assert got["pixels_by_chrom"][name] == [[x, y, acc[(x, y)]] for x, y in sorted(acc)], (b, name)
