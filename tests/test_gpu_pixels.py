"""Sparse cooler pixels extracted on the MI355X (include/modle_pixels.h, modle_amd/pixels.py):
bin1, bin2, count, bin1_offset and the statistics equal, exactly, a numpy reference in this module
(the row-by-row visit modle_cool_append_matrix documents), for bands built on the host with a seeded
generator and uploaded as torch tensors.  In every band the words that are no pixels (left-edge
triangle, trailing word) hold 0xFFFFFFFF: they must neither appear nor trip the range check."""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# the smallest shapes at which the kernels can go wrong: one pixel; a band of one word per
# column; nrows == ncols below a wave; one wave of rows; a full 64 x 64 tile; one more than a
# tile in both directions; odd sizes over several blocks; several count tiles along d and rows
# of more than 64 pixels over many blocks
SHAPES = [(1, 1), (1, 7), (5, 5), (3, 64), (64, 64), (65, 130), (70, 193), (600, 700)]
FILLS = ["empty", "full", "tenth"]
POISON = 0xFFFFFFFF


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


def make_band(nrows, ncols, fill, seed=0):
    rng = np.random.default_rng([seed, nrows, ncols])
    band = np.zeros(nrows * ncols + 1, dtype=np.uint32)
    if fill == "full":
        band[:-1] = rng.integers(1, 2**31, size=nrows * ncols, dtype=np.int64)
    elif fill == "tenth":
        mask = rng.random(nrows * ncols) < 0.1
        band[:-1][mask] = rng.integers(1, 5000, size=int(mask.sum()))
    for j in range(min(nrows, ncols)):
        band[j * nrows + j + 1:(j + 1) * nrows] = POISON
    band[nrows * ncols] = POISON
    return band


class Uploaded:
    """the band in device memory between guard words that hold POISON (and at an address that is
    4-byte aligned only): a read beyond either end of the band shows up as a pixel"""
    FRONT = 67

    def __init__(self, band, nrows):
        import torch

        self.host = np.full(self.FRONT + len(band) + 96 * (nrows + 1), POISON, dtype=np.uint32)
        self.host[self.FRONT:self.FRONT + len(band)] = band
        self.tensor = torch.from_numpy(self.host.view(np.int32)).to("cuda:0")
        torch.cuda.synchronize()

    def data_ptr(self):
        return self.tensor.data_ptr() + 4 * self.FRONT

    def unchanged(self):
        return np.array_equal(self.tensor.cpu().numpy().view(np.uint32), self.host)


def upload(band, nrows=600):
    return Uploaded(band, nrows)


def assert_equal_to_reference(got, ref, bin_offset=0):
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


@pytest.fixture(scope="module")
def sample():
    """one band, its device copy and its reference, shared by the entry-point tests"""
    nrows, ncols = 70, 193
    band = make_band(nrows, ncols, "tenth", seed=1)
    return nrows, ncols, upload(band), reference_pixels(band, nrows, ncols)


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("nrows,ncols", SHAPES)
def test_pixels_equal_the_row_by_row_visit(ex, nrows, ncols, fill):
    band = make_band(nrows, ncols, fill)
    ref = reference_pixels(band, nrows, ncols)
    if fill == "empty":
        assert ref["nnz"] == 0
    if fill == "full":  # also: rows of more than 64 pixels, their order across chunks
        assert ref["nnz"] == sum(min(nrows, ncols - i) for i in range(ncols))
    t = upload(band, nrows)
    assert_equal_to_reference(ex.extract(t.data_ptr(), nrows, ncols), ref)
    offset = 3_000_000_000  # (ids beyond 32 bits stay exact)
    assert_equal_to_reference(ex.extract(t.data_ptr(), nrows, ncols, bin_offset=offset), ref, offset)
    # the band is read, never written
    assert t.unchanged()


def test_the_largest_int32_passes_and_one_more_is_a_range_error(ex):
    from modle_amd import pixels

    nrows, ncols = 5, 9
    band = make_band(nrows, ncols, "tenth", seed=2)
    band[4 * nrows + 2] = 2**31 - 1
    ref = reference_pixels(band, nrows, ncols)
    assert ref["max_count"] == 2**31 - 1
    t = upload(band)
    assert_equal_to_reference(ex.extract(t.data_ptr(), nrows, ncols), ref)
    band[7 * nrows + 1] = 2**31
    t = upload(band)
    with pytest.raises(pixels.PixelsError) as e:
        ex.extract(t.data_ptr(), nrows, ncols)
    assert e.value.code == pixels.ERR_RANGE
    with pytest.raises(pixels.PixelsError) as e:  # the statistics-only count says the same
        ex.count(t.data_ptr(), nrows, ncols)
    assert e.value.code == pixels.ERR_RANGE
    # the context serves the next call
    band[7 * nrows + 1] = 17
    t = upload(band)
    assert_equal_to_reference(ex.extract(t.data_ptr(), nrows, ncols), reference_pixels(band, nrows, ncols))


def test_two_step_form_agrees_with_the_one_call_form(ex, sample):
    import torch

    nrows, ncols, t, ref = sample
    d_off = torch.full((ncols + 1,), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    stats = ex.count(t.data_ptr(), nrows, ncols, d_off.data_ptr())
    assert (stats.nnz, stats.sum, stats.max_count) == (ref["nnz"], ref["sum"], ref["max_count"])
    assert np.array_equal(d_off.cpu().numpy(), ref["bin1_offset"])
    guard = 8  # entries behind the result: they must stay untouched
    d1 = torch.full((stats.nnz + guard,), -7, dtype=torch.int64, device="cuda:0")
    d2 = torch.full((stats.nnz + guard,), -7, dtype=torch.int64, device="cuda:0")
    dc = torch.full((stats.nnz + guard,), -7, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    ex.extract_into(t.data_ptr(), nrows, ncols, 11, d_off.data_ptr(), d1.data_ptr(), d2.data_ptr(),
                    dc.data_ptr(), stats.nnz)
    torch.cuda.synchronize()
    got = (d1.cpu().numpy(), d2.cpu().numpy(), dc.cpu().numpy())
    for a in got:
        assert (a[stats.nnz:] == -7).all()
    assert_equal_to_reference((got[0][:stats.nnz], got[1][:stats.nnz], got[2][:stats.nnz],
                               d_off.cpu().numpy(), stats), ref, 11)
    assert_equal_to_reference(ex.extract(t.data_ptr(), nrows, ncols, 11), ref, 11)
    # statistics only: no index array is needed
    assert ex.count(t.data_ptr(), nrows, ncols) == stats


def test_a_stream_of_the_caller_and_a_second_call(ex, sample):
    import torch

    from modle_amd import pixels

    nrows, ncols, t, ref = sample
    stream = torch.cuda.Stream(device="cuda:0")
    assert stream.cuda_stream != 0
    first = ex.extract(t.data_ptr(), nrows, ncols, 5, stream=stream)
    assert_equal_to_reference(first, ref, 5)
    second = ex.extract(t.data_ptr(), nrows, ncols, 5, stream=stream)  # the same buffers again
    assert_equal_to_reference(second, ref, 5)
    # the module-level form (the process-wide context of the device)
    assert_equal_to_reference(pixels.extract(t.data_ptr(), nrows, ncols, bin_offset=5), ref, 5)
    # the arrays handed out are the caller's: the later calls did not change the first result
    assert_equal_to_reference(first, ref, 5)


def test_invalid_shapes_are_argument_errors(ex, sample):
    from modle_amd import pixels

    _, _, t, _ = sample
    for nrows, ncols in ((8, 7), (0, 5), (5, 0)):
        with pytest.raises(pixels.PixelsError) as e:
            ex.extract(t.data_ptr(), nrows, ncols)
        assert e.value.code == pixels.ERR_ARG
    b1, b2, cn, off, stats = ex.extract(None, 0, 0)  # an interval of no bins has no pixels
    assert len(b1) == len(b2) == len(cn) == 0 and off.tolist() == [0] and stats.nnz == 0


def test_simulated_interval_to_cooler_through_pixels(tmp_path):
    """a 2 Mb chromosome with barriers (and one without, which is skipped), 8 cells:
    Simulator.pixels equals the reference applied to the dense matrix, write_pixels writes
    the file write_cooler writes, and the front end's file is the same file"""
    from test_cooler_pixels import assert_same_cooler

    from modle_amd import api, cli, driver, genome

    rng = np.random.default_rng(4)
    (tmp_path / "g.chrom.sizes").write_text("chrA\t2000000\nchrB\t500000\n")
    lines = [f"chrA\t{p}\t{p + 19}\t.\t{rng.uniform(0.6, 1.0):.3f}\t{'+' if rng.random() < 0.5 else '-'}"
             for p in sorted(rng.choice(2_000_000 - 100, size=24, replace=False))]
    (tmp_path / "b.bed").write_text("\n".join(lines) + "\n")
    prefix = str(tmp_path / "out" / "run")
    argv = ["simulate", "-c", str(tmp_path / "g.chrom.sizes"), "-b", str(tmp_path / "b.bed"), "-o", prefix,
            "--ncells", "8", "--target-contact-density", "0.2", "--seed", "5", "-q"]
    assert cli.main(argv) == 0
    args = cli.build_parser().parse_args(argv)
    cfg = cli.config_from_args(args)
    chroms, ivs, _ = genome.import_genome(cfg, str(tmp_path / "g.chrom.sizes"), str(tmp_path / "b.bed"))
    plan = driver.plan_genome(cfg, ivs)
    assert [e["skipped"] for e in plan] == [False, True]
    assert (plan[0]["nrows"], plan[0]["ncols"]) == (400, 400)
    meta = json.dumps({k: v for k, v in vars(args).items() if v is not None and k != "command"},
                      sort_keys=True)
    kw = dict(assembly="unknown", generated_by="modle_amd (MI355X)", metadata_json=meta, chroms=chroms)
    dense_path, sparse_path = str(tmp_path / "dense.cool"), str(tmp_path / "sparse.cool")
    sim = api.Simulator(cfg, 0)
    try:
        ids = driver.enqueue_plan(sim, cfg, plan)
        sim.launch()
        sim.wait()
        dense, _, _ = sim.copy_outputs(ids[0])
        ref = reference_pixels(dense, 400, 400)
        assert ref["nnz"] > 1000
        assert_equal_to_reference(sim.pixels(ids[0]), ref)
        assert_equal_to_reference(sim.pixels(ids[0], bin_offset=77), ref, 77)
        driver.write_pixels(sparse_path, cfg, plan,
                            lambda k, factor, first_bin, off: None if ids[k] is None else sim.pixels(ids[k], off),
                            **kw)
    finally:
        sim.close()
    driver.write_cooler(dense_path, cfg, plan, [dense, None], **kw)
    got = assert_same_cooler(dense_path, sparse_path)
    assert got["attrs"]["nnz"] == ref["nnz"] and got["attrs"]["sum"] == ref["sum"]
    assert_same_cooler(dense_path, prefix + ".cool")
