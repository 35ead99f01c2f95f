"""The marginals of a band summed on the MI355X (include/modle_pixels.h: modle_pixels_marginals,
_marginals_to_host, _coarse_marginals_to_host; modle_amd/pixels.py; api.Simulator.marginals_tensors):
the sums per diagonal and the coverage per bin equal, word for word, a numpy restatement of the
definition in this module, for bands built on the host with a seeded generator.  The input and both
outputs lie between poisoned guard words at an address that is 4-byte aligned only; the outputs are
poisoned before the call (the library, not the caller, defines every word), and in every input band
the words that are no pixels hold 0xFFFFFFFF: they must not be summed.  Nothing here has a tolerance."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (nrows, ncols) around the kernel's tile of 64 columns x 256 band words and its waves of 64: a band
# one word wide; all triangle; exactly one column tile; one past a wave and a column tile; odd sizes;
# one past the 256-deep tile and five column tiles plus one column; several tiles both ways -- and one
# below a wave with one past a column tile, and exactly one depth tile on exactly five column tiles
SHAPES = [(1, 1), (1, 7), (5, 5), (3, 64), (64, 64), (65, 130), (70, 193), (257, 321), (600, 700),
          (63, 65), (256, 320)]
FILLS = ["empty", "tenth", "full"]
COARSE = [(65, 130, 3, 2), (600, 700, 25, 7)]  # (nrows, ncols, factor, first_bin)
POISON = 0xFFFFFFFF
FRONT, BACK = 67, 96 * 601  # guard words (the front one leaves the words 4-byte aligned only)
LIMIT = 0xFFFFFFFF          # counts up to 0xFFFFFFFE: the sums of a full band pass 2^32


def min_diags(nrows):
    return [0, 1, 2, nrows, nrows + 5]  # the last two: no diagonal is kept, the coverage is all zero


def reference_marginals(band, nrows, ncols, min_diag):
    """diag_sum[d] = sum over j >= d of band[j * nrows + d]; pixel (j - d, j) counts for bin j when
    d >= max(min_diag, 0) (the column part) and for bin j - d when d >= max(min_diag, 1) (the row part)"""
    diag_sum, coverage = np.zeros(nrows, dtype=np.uint64), np.zeros(ncols, dtype=np.uint64)
    for d in range(nrows):
        j = np.arange(d, ncols, dtype=np.int64)
        v = band[j * nrows + d].astype(np.uint64)
        diag_sum[d] = v.sum(dtype=np.uint64)
        if d >= max(min_diag, 0):
            coverage[j] += v
        if d >= max(min_diag, 1):
            coverage[j - d] += v
    return diag_sum, coverage


def coarse_shape(nrows, ncols, k, first_bin):
    p = first_bin % k
    nc = (p + ncols + k - 1) // k
    return min(nc, (nrows - 1 + k - 1) // k + 1), nc


def reference_coarsen(band, nrows, ncols, k, first_bin):
    """for every fine pixel (i, j), d = j - i < nrows: coarse (I, J) = ((i + p) / k, (j + p) / k) gets
    band[j * nrows + d]; every other word of the result is 0"""
    p = first_bin % k
    nr, nc = coarse_shape(nrows, ncols, k, first_bin)
    out = np.zeros(nr * nc + 1, dtype=np.uint64)
    for d in range(nrows):
        j = np.arange(d, ncols, dtype=np.int64)
        J, I = (j + p) // k, (j - d + p) // k
        np.add.at(out, J * nr + (J - I), band[j * nrows + d].astype(np.uint64))
    assert int(out.max()) < 2**31  # no sum saturates
    return out.astype(np.uint32), nr, nc


def make_band(nrows, ncols, fill, limit=LIMIT, seed=0):
    rng = np.random.default_rng([seed, nrows, ncols])
    band = np.zeros(nrows * ncols + 1, dtype=np.uint32)
    if fill == "full":
        band[:-1] = rng.integers(1, limit, size=nrows * ncols, dtype=np.int64)
    elif fill == "tenth":
        mask = rng.random(nrows * ncols) < 0.1
        band[:-1][mask] = rng.integers(1, limit, size=int(mask.sum()), dtype=np.int64)
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

    def sums(self):
        return self.read()[FRONT:FRONT + self.n].copy().view(np.uint64)


def output_buffer(n_sums):
    out = Guarded(np.full(2 * n_sums, POISON, dtype=np.uint32))  # the caller does not pre-zero
    assert out.data_ptr() % 8 == 4
    return out


@pytest.fixture(scope="module")
def ex():
    from modle_amd import pixels

    with pixels.Extractor(0) as e:
        yield e


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("nrows,ncols", SHAPES)
def test_marginals_equal_the_definition(ex, nrows, ncols, fill):
    band = make_band(nrows, ncols, fill)
    src = Guarded(band)
    for m in min_diags(nrows):
        want_diag, want_cov = reference_marginals(band, nrows, ncols, m)
        if fill == "full":
            assert int(want_diag[0]) > 2**32 or ncols == 1
        if m >= nrows:
            assert not want_cov.any()
        # the device form, into poisoned arrays
        d_diag, d_cov = output_buffer(nrows), output_buffer(ncols)
        ex.marginals_into(src.data_ptr(), nrows, ncols, m, d_diag.data_ptr(), d_cov.data_ptr())
        assert np.array_equal(d_diag.sums(), want_diag), m
        assert np.array_equal(d_cov.sums(), want_cov), m
        assert d_diag.guards_intact() and d_cov.guards_intact()
        # the host form, twice: the same again
        for _ in range(2):
            diag, cov = ex.marginals(src.data_ptr(), nrows, ncols, m)
            assert (diag.dtype, cov.dtype, diag.shape, cov.shape) == (np.uint64, np.uint64, (nrows,), (ncols,))
            assert np.array_equal(diag, want_diag) and np.array_equal(cov, want_cov), m
    assert src.unchanged()


@pytest.mark.parametrize("nrows,ncols", SHAPES)
def test_each_output_alone(ex, nrows, ncols):
    band = make_band(nrows, ncols, "tenth", seed=1)
    src = Guarded(band)
    want_diag, want_cov = reference_marginals(band, nrows, ncols, 1)
    d_diag, d_cov = output_buffer(nrows), output_buffer(ncols)
    ex.marginals_into(src.data_ptr(), nrows, ncols, 1, d_diag.data_ptr(), None)
    assert np.array_equal(d_diag.sums(), want_diag) and d_diag.guards_intact()
    assert d_cov.unchanged()  # (still poison)
    d_diag = output_buffer(nrows)
    ex.marginals_into(src.data_ptr(), nrows, ncols, 1, None, d_cov.data_ptr())
    assert np.array_equal(d_cov.sums(), want_cov) and d_cov.guards_intact()
    assert d_diag.unchanged() and src.unchanged()


@pytest.mark.parametrize("fill", ["tenth", "full"])
@pytest.mark.parametrize("nrows,ncols", SHAPES)
def test_the_sums_of_the_marginals_are_those_of_the_count(ex, nrows, ncols, fill):
    """counts up to INT32_MAX, which modle_pixels_count accepts: the sums of a full band still pass 2^32"""
    band = make_band(nrows, ncols, fill, limit=2**31, seed=2)
    src = Guarded(band)
    stats = ex.count(src.data_ptr(), nrows, ncols)
    diag, cov = ex.marginals(src.data_ptr(), nrows, ncols)
    assert sum(int(x) for x in diag) == stats.sum
    assert sum(int(x) for x in cov) == 2 * stats.sum - int(diag[0])
    assert fill == "tenth" or ncols == 1 or stats.sum > 2**32
    assert src.unchanged()


@pytest.mark.parametrize("nrows,ncols,k,first_bin", COARSE)
def test_coarse_marginals_are_those_of_the_coarse_band(ex, nrows, ncols, k, first_bin):
    from modle_amd import pixels

    band = make_band(nrows, ncols, "tenth", limit=2**20, seed=3)
    coarse, nr, nc = reference_coarsen(band, nrows, ncols, k, first_bin)
    assert pixels.coarse_shape(nrows, ncols, k, first_bin) == (nr, nc)
    src = Guarded(band)
    for m in min_diags(nr):
        want_diag, want_cov = reference_marginals(coarse, nr, nc, m)
        diag, cov = ex.coarse_marginals(src.data_ptr(), nrows, ncols, k, first_bin, m)
        assert (diag.dtype, cov.dtype) == (np.uint64, np.uint64)
        assert np.array_equal(diag, want_diag) and np.array_equal(cov, want_cov), m
    assert int(want_diag.sum()) == int(band[band != POISON].sum(dtype=np.uint64))  # every contact is there
    # the fine path still serves, and the module-level forms (the process-wide context of the device)
    fine = reference_marginals(band, nrows, ncols, 0)
    for got in (ex.marginals(src.data_ptr(), nrows, ncols), pixels.marginals(src.data_ptr(), nrows, ncols)):
        assert np.array_equal(got[0], fine[0]) and np.array_equal(got[1], fine[1])
    got = pixels.coarse_marginals(src.data_ptr(), nrows, ncols, k, first_bin)
    want = reference_marginals(coarse, nr, nc, 0)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert src.unchanged()


def test_a_stream_of_the_caller_and_buffers_that_grow():
    import torch

    from modle_amd import pixels

    stream = torch.cuda.Stream(device="cuda:0")
    assert stream.cuda_stream != 0
    small, large = make_band(5, 9, "full", seed=7), make_band(70, 193, "tenth", seed=7)
    want_small, want_large = reference_marginals(small, 5, 9, 0), reference_marginals(large, 70, 193, 2)
    s, l = Guarded(small), Guarded(large)
    with pixels.Extractor(0) as e:
        first = e.marginals(s.data_ptr(), 5, 9, stream=stream)
        again = e.marginals(l.data_ptr(), 70, 193, 2, stream=stream)  # grows
        assert np.array_equal(again[0], want_large[0]) and np.array_equal(again[1], want_large[1])
        d_diag, d_cov = output_buffer(5), output_buffer(9)
        e.marginals_into(s.data_ptr(), 5, 9, 0, d_diag.data_ptr(), d_cov.data_ptr(), stream=stream)  # reused
        stream.synchronize()
        assert np.array_equal(d_diag.sums(), want_small[0]) and np.array_equal(d_cov.sums(), want_small[1])
        assert np.array_equal(first[0], want_small[0]) and np.array_equal(first[1], want_small[1])  # the caller's
    assert s.unchanged() and l.unchanged()


def test_invalid_calls_are_argument_errors_and_write_nothing(ex):
    from modle_amd import pixels

    nrows, ncols = 5, 9
    src = Guarded(make_band(nrows, ncols, "full", seed=8))
    d_diag, d_cov = output_buffer(ncols + 1), output_buffer(ncols + 1)
    inside = src.data_ptr() + 4 * (nrows * ncols)  # the band's trailing word: the last that is the band's
    for what, args in [("nrows > ncols", (ncols + 1, ncols, 0, d_diag.data_ptr(), d_cov.data_ptr())),
                       ("nrows 0", (0, ncols, 0, d_diag.data_ptr(), d_cov.data_ptr())),
                       ("both outputs NULL", (nrows, ncols, 0, None, None)),
                       ("diag_sum overlaps the band", (nrows, ncols, 0, inside, d_cov.data_ptr())),
                       ("coverage overlaps the band", (nrows, ncols, 0, d_diag.data_ptr(), src.data_ptr() - 8 * ncols + 4)),
                       ("coverage overlaps the band, alone", (nrows, ncols, 0, None, inside))]:
        with pytest.raises(pixels.PixelsError) as e:
            ex.marginals_into(src.data_ptr(), *args)
        assert e.value.code == pixels.ERR_ARG, what
    for args in [(ncols + 1, ncols), (0, ncols)]:
        with pytest.raises(pixels.PixelsError) as e:
            ex.marginals(src.data_ptr(), *args)
        assert e.value.code == pixels.ERR_ARG
        with pytest.raises(pixels.PixelsError) as e:
            ex.coarse_marginals(src.data_ptr(), *args, 2, 0)
        assert e.value.code == pixels.ERR_ARG
    with pytest.raises(pixels.PixelsError) as e:
        ex.coarse_marginals(src.data_ptr(), nrows, ncols, 1, 0)
    assert e.value.code == pixels.ERR_ARG
    assert d_diag.unchanged() and d_cov.unchanged() and src.unchanged()  # (still poison)
    # an output that ends where the band begins, or begins where it ends, does not overlap it
    whole = Guarded(np.concatenate([np.full(2 * nrows, POISON, dtype=np.uint32), src.host[FRONT:FRONT + src.n],
                                    np.full(2 * ncols, POISON, dtype=np.uint32)]))
    band_ptr = whole.data_ptr() + 8 * nrows
    ex.marginals_into(band_ptr, nrows, ncols, 0, whole.data_ptr(), band_ptr + 4 * (nrows * ncols + 1))
    want = reference_marginals(src.host[FRONT:FRONT + src.n], nrows, ncols, 0)
    got = whole.read()[FRONT:FRONT + whole.n]
    assert np.array_equal(got[:2 * nrows].copy().view(np.uint64), want[0])
    assert np.array_equal(got[2 * nrows + src.n:].copy().view(np.uint64), want[1])
    assert np.array_equal(got[2 * nrows:2 * nrows + src.n], src.host[FRONT:FRONT + src.n]) and whole.guards_intact()


def test_simulator_forms_agree():
    """an interval that starts at fine bin 5, 4 cells, a band narrower than the matrix: the torch form,
    the host form and the device form give the restatement on the band copied to the host"""
    import torch

    from modle_amd import api, driver, genome, pixels

    rng = np.random.default_rng(4)
    barriers = "".join(f"chrA\t{p}\t{p + 19}\t.\t{rng.uniform(0.6, 1.0):.3f}\t{'+' if rng.random() < 0.5 else '-'}\n"
                       for p in sorted(rng.choice(1_200_000 - 100, size=16, replace=False)))
    cfg = api.make_config(bin_size=5000, diagonal_width=400_000, num_cells=4, target_contact_density=0.5, seed=5)
    _, ivs, _ = genome.import_genome_text(cfg, "chrA\t1200000\n", barriers, "chrA\t25000\t1025000\n")
    plan = driver.plan_genome(cfg, ivs)
    nrows, ncols = plan[0]["nrows"], plan[0]["ncols"]
    assert (nrows, ncols) == (80, 200)
    sim = api.Simulator(cfg, 0)
    try:
        iid = driver.enqueue_plan(sim, cfg, plan)[0]
        sim.launch()
        sim.wait()
        band, _, _ = sim.copy_outputs(iid)
        stats = sim.pixels(iid).stats
        assert stats.nnz > 1000
        for m in (0, 2):
            want_diag, want_cov = reference_marginals(band, nrows, ncols, m)
            t_diag, t_cov = sim.marginals_tensors(iid, m)
            assert t_diag.dtype == t_cov.dtype == torch.int64 and t_diag.device == t_cov.device == torch.device("cuda", 0)
            assert (tuple(t_diag.shape), tuple(t_cov.shape)) == ((nrows,), (ncols,))
            torch.cuda.synchronize()
            assert np.array_equal(t_diag.cpu().numpy().view(np.uint64), want_diag)
            assert np.array_equal(t_cov.cpu().numpy().view(np.uint64), want_cov)
            diag, cov = sim.marginals(iid, m)
            assert np.array_equal(diag, want_diag) and np.array_equal(cov, want_cov)
            assert np.array_equal(sim.coverage(iid, m), want_cov)
            d_diag, d_cov = output_buffer(nrows), output_buffer(ncols)
            pixels.marginals_into(sim.outputs(iid)[0], nrows, ncols, m, d_diag.data_ptr(), d_cov.data_ptr())
            assert np.array_equal(d_diag.sums(), want_diag) and np.array_equal(d_cov.sums(), want_cov)
        diag, n_valid = sim.expected(iid)
        assert np.array_equal(diag, reference_marginals(band, nrows, ncols, 0)[0])
        assert n_valid.dtype == np.uint64 and n_valid.tolist() == [ncols - d for d in range(nrows)]
        assert int(diag.sum()) == stats.sum and int(sim.coverage(iid).sum()) == 2 * stats.sum - int(diag[0])
        # at three times the bin size, anchored at the chromosome's start
        coarse, nr, nc = reference_coarsen(band, nrows, ncols, 3, 5)
        diag3, n_valid3 = sim.expected(iid, factor=3, first_bin=5)
        assert np.array_equal(diag3, reference_marginals(coarse, nr, nc, 0)[0])
        assert n_valid3.tolist() == [nc - d for d in range(nr)] and int(diag3.sum()) == stats.sum
        assert np.array_equal(sim.coverage(iid, 1, factor=3, first_bin=5), reference_marginals(coarse, nr, nc, 1)[1])
        assert np.array_equal(sim.copy_outputs(iid)[0], band)
    finally:
        sim.close()
