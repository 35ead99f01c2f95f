"""Band matrices unpacked into square tiles on the MI355X (include/modle_pixels.h:
modle_pixels_dense_tiles, modle_pixels_dense_to_host; modle_amd/pixels.py, api.Simulator.dense /
dense_tiles, `simulate --dense-region`): every output word equals, exactly, a numpy restatement of
the definition in this module, for bands built on the host with a seeded generator and uploaded
between poisoned guard words.  In every input band the words that are no pixels hold 0xFFFFFFFF, and
the output buffer is filled with the same poison before the call: a word that is not written, or an
indexing slip into the left-edge triangle, shows up as a wrong value."""
import os

import numpy as np
import pytest

from test_gpu_coarsen import POISON, Guarded, make_band, output_buffer

pytestmark = pytest.mark.gpu

# (nrows, ncols, first, size, step, count): one pixel; a band one word wide with overlapping tiles;
# nrows == ncols; the band's edge through one full block; exactly one block; one past 64 both ways
# (a diagonal, an upper and a mirrored block); an odd offset with overlapping tiles, the last ending
# at ncols; a region at the right end; whole blocks outside the band; step > size at production nrows
SHAPES = [(1, 1, 0, 1, 1, 1), (1, 7, 2, 3, 1, 3), (5, 5, 0, 5, 1, 1), (3, 64, 0, 64, 1, 1), (64, 64, 0, 64, 1, 1),
          (65, 130, 0, 130, 1, 1), (65, 130, 1, 65, 32, 3), (70, 193, 128, 65, 1, 1), (40, 700, 0, 300, 1, 1),
          (600, 700, 37, 200, 230, 3)]
FILLS = ["empty", "tenth", "full"]


def reference_dense(band, nrows, first, size, step, count):
    """out[t][r][c] = d < nrows ? band[j * nrows + d] : 0 with a = lo_t + r, b = lo_t + c, d = |a - b|,
    j = max(a, b), lo_t = first + t * step"""
    out = np.zeros((count, size, size), dtype=np.uint32)
    for t in range(count):
        a = (first + t * step + np.arange(size, dtype=np.int64))[:, None]
        b = a.T
        d, j = np.abs(a - b), np.maximum(a, b)
        inside = d < nrows
        out[t][inside] = band[(j * nrows + d)[inside]]
    return out


def expand_pixels(b1, b2, cn, lo, hi):
    """the symmetric matrix of the bins [lo, hi) from a pixel table (bin1 <= bin2, ids as in the table)"""
    m = np.zeros((hi - lo, hi - lo), dtype=np.int64)
    b1, b2, cn = np.asarray(b1, dtype=np.int64), np.asarray(b2, dtype=np.int64), np.asarray(cn, dtype=np.int64)
    keep = (b1 >= lo) & (b2 < hi)
    m[b1[keep] - lo, b2[keep] - lo] = cn[keep]
    m[b2[keep] - lo, b1[keep] - lo] = cn[keep]
    return m


@pytest.fixture(scope="module")
def ex():
    from modle_amd import pixels

    with pixels.Extractor(0) as e:
        yield e


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("nrows,ncols,first,size,step,count", SHAPES)
def test_tiles_equal_the_definition(ex, nrows, ncols, first, size, step, count, fill):
    from modle_amd import pixels

    band = make_band(nrows, ncols, fill, 2**31)
    ref = reference_dense(band, nrows, first, size, step, count)
    assert not (ref == POISON).any()  # (no word of the definition is a word that is no pixel)
    assert pixels.tiles_fit(ncols, first, size, step) >= count
    words = count * size * size
    src, dst = Guarded(band), output_buffer(words)
    ex.dense_tiles_into(src.data_ptr(), nrows, ncols, first, size, step, count, dst.data_ptr(), words)
    got = dst.words().reshape(count, size, size)
    assert np.array_equal(got, ref)
    assert np.array_equal(got, got.transpose(0, 2, 1))
    if fill == "full":
        r = np.arange(size)
        assert np.count_nonzero(got) == count * int((np.abs(r[:, None] - r[None, :]) < nrows).sum())
    elif fill == "empty":
        assert not got.any()
    assert dst.guards_intact() and src.guards_intact() and src.unchanged()
    # the one-call form: tile 0 as a numpy array of the caller's
    one = ex.dense(src.data_ptr(), nrows, ncols, first, first + size)
    assert one.dtype == np.uint32 and one.shape == (size, size) and one.flags.owndata
    assert np.array_equal(one, ref[0])
    assert src.unchanged()


def test_a_stream_of_the_caller_and_a_scratch_that_grows():
    import torch

    from modle_amd import pixels

    stream = torch.cuda.Stream(device="cuda:0")
    assert stream.cuda_stream != 0
    small, large = make_band(5, 9, "full", 1000, seed=7), make_band(70, 193, "tenth", 2**20, seed=7)
    want_small = reference_dense(small, 5, 2, 6, 1, 1)[0]
    want_large = reference_dense(large, 70, 3, 190, 1, 1)[0]
    s, l = Guarded(small), Guarded(large)
    with pixels.Extractor(0) as e:
        first = e.dense(s.data_ptr(), 5, 9, 2, 8, stream=stream)
        assert np.array_equal(first, want_small)
        grown = e.dense(l.data_ptr(), 70, 193, 3, 193, stream=stream)  # grows
        assert np.array_equal(grown, want_large)
        assert np.array_equal(e.dense(s.data_ptr(), 5, 9, 2, 8, stream=stream), want_small)  # reused
        assert np.array_equal(e.dense(l.data_ptr(), 70, 193, 3, 193), want_large)  # the default stream
        # the tiles form on the caller's stream, into a torch tensor
        out = torch.full((2, 100, 100), -1, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        e.dense_tiles_into(l.data_ptr(), 70, 193, 1, 100, 92, 2, out.data_ptr(), out.numel(), stream=stream)
        stream.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), reference_dense(large, 70, 1, 100, 92, 2))
        # the arrays handed out earlier are the caller's
        assert np.array_equal(first, want_small) and np.array_equal(grown, want_large)
    # the module-level forms (the process-wide context of the device)
    assert np.array_equal(pixels.dense(l.data_ptr(), 70, 193, 3, 193, device=0), want_large)
    dst = output_buffer(36)
    pixels.dense_tiles_into(s.data_ptr(), 5, 9, 2, 6, 1, 1, dst.data_ptr(), 36, device=0)
    assert np.array_equal(dst.words().reshape(6, 6), want_small) and dst.guards_intact()
    assert s.unchanged() and l.unchanged()


def test_invalid_calls_are_argument_errors_and_write_nothing(ex):
    from modle_amd import pixels

    nrows, ncols = 5, 9
    host = make_band(nrows, ncols, "full", 1000, seed=8)
    src, dst = Guarded(host), output_buffer(2 * 4 * 4)
    band, out, n = src.data_ptr(), dst.data_ptr(), 32
    # (d_band, nrows, ncols, first, size, step, count, d_out, out_words); the valid call is
    # (band, 5, 9, 1, 4, 4, 2, out, 32): tiles at 1 and 5, and no third
    assert pixels.tiles_fit(ncols, 1, 4, 4) == 2
    for what, args in [("null band", (None, nrows, ncols, 1, 4, 4, 2, out, n)),
                       ("null output", (band, nrows, ncols, 1, 4, 4, 2, None, n)),
                       ("nrows 0", (band, 0, ncols, 1, 4, 4, 2, out, n)),
                       ("nrows > ncols", (band, ncols + 1, ncols, 1, 4, 4, 2, out, n)),
                       ("count 0", (band, nrows, ncols, 1, 4, 4, 0, out, n)),
                       ("count > max_count", (band, nrows, ncols, 1, 4, 4, 3, out, n)),
                       ("size 0", (band, nrows, ncols, 1, 0, 4, 1, out, n)),
                       ("step 0", (band, nrows, ncols, 1, 4, 0, 1, out, n)),
                       ("first + size > ncols", (band, nrows, ncols, 6, 4, 4, 1, out, n)),
                       ("out_words too small", (band, nrows, ncols, 1, 4, 4, 2, out, n - 1)),
                       ("count * size * size overflows", (band, 1, 2**40, 0, 2**32, 1, 1, out, 2**64 - 1)),
                       ("the output overlaps the band", (band, nrows, ncols, 1, 4, 4, 2, band + 16, n))]:
        with pytest.raises(pixels.PixelsError) as e:
            ex.dense_tiles_into(*args)
        assert e.value.code == pixels.ERR_ARG, what
    for what, args in [("lo == hi", (band, nrows, ncols, 3, 3)), ("lo > hi", (band, nrows, ncols, 4, 3)),
                       ("hi > ncols", (band, nrows, ncols, 3, ncols + 1)), ("nrows 0", (band, 0, ncols, 0, 3)),
                       ("null band", (None, nrows, ncols, 0, 3))]:
        with pytest.raises(pixels.PixelsError) as e:
            ex.dense(*args)
        assert e.value.code == pixels.ERR_ARG, what
    assert dst.unchanged() and src.unchanged()
    # the context serves the next call
    ex.dense_tiles_into(band, nrows, ncols, 1, 4, 4, 2, out, n)
    assert np.array_equal(dst.words().reshape(2, 4, 4), reference_dense(host, nrows, 1, 4, 4, 2))


def test_simulator_dense_equals_the_expansion_of_its_pixels():
    """an interval that starts at fine bin 5, 4 cells, a band narrower than the matrix"""
    import torch

    from modle_amd import api, driver, genome, pixels

    rng = np.random.default_rng(4)
    barriers = "".join(f"chrA\t{p}\t{p + 19}\t.\t{rng.uniform(0.6, 1.0):.3f}\t{'+' if rng.random() < 0.5 else '-'}\n"
                       for p in sorted(rng.choice(1_200_000 - 100, size=16, replace=False)))
    cfg = api.make_config(bin_size=5000, diagonal_width=400_000, num_cells=4, target_contact_density=0.5, seed=5)
    _, ivs, _ = genome.import_genome_text(cfg, "chrA\t1200000\n", barriers, "chrA\t25000\t1025000\n")
    plan = driver.plan_genome(cfg, ivs)
    assert (plan[0]["nrows"], plan[0]["ncols"]) == (80, 200)
    sim = api.Simulator(cfg, 0)
    try:
        iid = driver.enqueue_plan(sim, cfg, plan)[0]
        sim.launch()
        sim.wait()
        band_before, _, _ = sim.copy_outputs(iid)
        b1, b2, cn, _, stats = sim.pixels(iid)
        assert stats.nnz > 1000
        for lo, hi in [(0, 200), (0, 1), (31, 164), (199, 200)]:
            got = sim.dense(iid, lo, hi)
            assert got.dtype == np.uint32 and got.shape == (hi - lo, hi - lo)
            assert np.array_equal(got, expand_pixels(b1, b2, cn, lo, hi)), (lo, hi)
        # at three times the bin size, anchored at the chromosome's start: lo, hi are coarse columns
        c1, c2, ccn, _, cstats = sim.coarse_pixels(iid, 3, 5)
        nr, nc = pixels.coarse_shape(80, 200, 3, 5)
        assert cstats.sum == stats.sum and (nr, nc) == (28, 68)
        for lo, hi in [(0, nc), (2, 67)]:
            assert np.array_equal(sim.dense(iid, lo, hi, factor=3, first_bin=5), expand_pixels(c1, c2, ccn, lo, hi))
        # windows for a model: a device tensor, nothing on the host
        tiles = sim.dense_tiles(iid, 3, 64, 50)
        assert tiles.dtype == torch.int32 and tiles.device == torch.device("cuda", 0)
        assert tuple(tiles.shape) == (3, 64, 64)  # 3, 53, 103; 153 + 64 > 200
        torch.cuda.synchronize()
        for t in range(3):
            assert np.array_equal(tiles[t].cpu().numpy().view(np.uint32), sim.dense(iid, 3 + 50 * t, 67 + 50 * t))
        assert tuple(sim.dense_tiles(iid, 3, 64, 50, count=2).shape) == (2, 64, 64)
        with pytest.raises(pixels.PixelsError):
            sim.dense_tiles(iid, 3, 64, 50, count=4)
        assert np.array_equal(sim.copy_outputs(iid)[0], band_before)
    finally:
        sim.close()


def test_simulate_writes_the_dense_regions_of_its_cooler(tmp_path):
    """two chromosomes, 4 cells, an interval of chrA that starts at fine bin 5 and all of chrB: every
    array of <prefix>_dense.npz is the symmetric expansion of the pixel table of the .cool the same run
    wrote, that .cool is the one written without the option, and a region outside the interval of -g
    ends the run before any output file exists"""
    from test_mcool_writer import read_group

    from modle_amd import cli

    rng = np.random.default_rng(4)
    (tmp_path / "g.chrom.sizes").write_text("chrA\t1200000\nchrB\t400000\n")
    (tmp_path / "iv.bed").write_text("chrA\t25000\t1025000\nchrB\t0\t400000\n")
    lines = [f"{c}\t{p}\t{p + 19}\t.\t{rng.uniform(0.6, 1.0):.3f}\t{'+' if rng.random() < 0.5 else '-'}"
             for c, size, n in (("chrA", 1_200_000, 16), ("chrB", 400_000, 6))
             for p in sorted(rng.choice(size - 100, size=n, replace=False))]
    (tmp_path / "b.bed").write_text("\n".join(lines) + "\n")
    common = ["simulate", "-c", str(tmp_path / "g.chrom.sizes"), "-b", str(tmp_path / "b.bed"), "-g",
              str(tmp_path / "iv.bed"), "-r", "5kb", "--ncells", "4", "--target-contact-density", "0.5",
              "--seed", "5", "-q"]
    regions = ["--dense-region", "chrB", "--dense-region", "chrA:100kb-600kb"]
    with pytest.raises(SystemExit) as e:  # bins 0..4 of chrA are not simulated
        cli.main(common + ["-o", str(tmp_path / "bad" / "run"), "--dense-region", "chrA:0-600kb"])
    assert "--dense-region" in str(e.value)
    assert not os.path.isdir(tmp_path / "bad") or os.listdir(tmp_path / "bad") == []
    assert cli.main(common + ["-o", str(tmp_path / "plain" / "run")]) == 0
    assert cli.main(common + ["-o", str(tmp_path / "dense" / "run")] + regions) == 0
    assert not (tmp_path / "plain" / "run_dense.npz").exists()
    plain, cool = read_group(str(tmp_path / "plain" / "run.cool")), read_group(str(tmp_path / "dense" / "run.cool"))
    for key in ("chroms", "bins", "pixels_by_chrom", "bin1_offset", "chrom_offset", "n_pixels", "dtypes",
                "filters", "name_dtype", "members"):
        assert cool[key] == plain[key], key
    assert cool["n_pixels"] > 1000
    with np.load(str(tmp_path / "dense" / "run_dense.npz")) as z:
        assert sorted(z.files) == ["chrA:100000-600000", "chrB:0-400000"]
        for key, name, lo, hi in [("chrA:100000-600000", "chrA", 20, 120), ("chrB:0-400000", "chrB", 0, 80)]:
            got = z[key]
            assert got.dtype == np.int32 and got.shape == (hi - lo, hi - lo)
            off = cool["chrom_offset"][["chrA", "chrB"].index(name)]
            px = np.array(cool["pixels_by_chrom"][name], dtype=np.int64).reshape(-1, 3)
            want = expand_pixels(px[:, 0], px[:, 1], px[:, 2], off + lo, off + hi)
            assert np.count_nonzero(want) > 100
            assert np.array_equal(got, want), key
    # the outputs are covered by the refuse-to-overwrite rule, and --skip-output writes none
    with pytest.raises(SystemExit):
        cli.main(common + ["-o", str(tmp_path / "dense" / "run")] + regions)
    for other in ("run.cool", "run_lef_1d_occupancy.bw"):  # (checked before the .npz)
        os.remove(tmp_path / "dense" / other)
    assert os.listdir(tmp_path / "dense") == ["run_dense.npz"]
    with pytest.raises(SystemExit) as e:
        cli.main(common + ["-o", str(tmp_path / "dense" / "run")] + regions)
    assert "run_dense.npz" in str(e.value)
    assert cli.main(common + ["-o", str(tmp_path / "none" / "run"), "--skip-output"] + regions) == 0
    assert not (tmp_path / "none" / "run_dense.npz").exists()
