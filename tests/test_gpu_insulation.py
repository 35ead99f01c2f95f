"""The insulation sums of a band formed on the MI355X (include/modle_pixels.h: modle_pixels_insulation,
_insulation_to_host, _coarse_insulation_to_host; modle_amd/pixels.py; api.Simulator.insulation and
insulation_tensor): for every window and bin the sum over the sliding diamond equals, word for word, the
numpy restatement of tests/test_insulation_outputs.py, for bands built on the host with a seeded generator.
The input lies between poisoned guard words at an address that is 4-byte aligned only, the output at an
8-byte aligned address between guard words, poisoned before the call (the library, not the caller, defines
every word), and in every input band the words that are no pixels hold 0xFFFFFFFF: they must not be
summed.  Nothing here has a tolerance."""
import numpy as np
import pytest

from test_gpu_marginals import BACK, FRONT, POISON, Guarded, make_band, reference_coarsen, reference_marginals
from test_insulation_outputs import identity_rhs, prefix_insulation

pytestmark = pytest.mark.gpu

# (nrows, ncols, windows) around the 64 bins a workgroup owns, the 64-word chunk of the scan and the cap
# of 1024 bins: the smallest band; all triangle; exactly one group of bins; spans 2w - 1 of 127 / 129 around
# two chunks with a column halo that crosses two groups; windows unsorted in the call; eight windows on the
# reference's default band depth; the cap (16 MB; `tenth` fill only)
SHAPES = [(1, 1, [1]), (1, 7, [1]), (5, 5, [1, 3]), (5, 9, [2, 3]), (63, 65, [32]), (64, 64, [32]),
          (129, 130, [1, 33, 64, 65]), (199, 321, [100, 7]), (257, 321, [64, 128, 129]),
          (600, 700, [300, 8, 64, 65, 1, 2, 3, 150]), (2047, 2100, [1024])]
CASES = [(nr, nc, ws, fill) for nr, nc, ws in SHAPES for fill in ("empty", "tenth", "full")
         if fill == "tenth" or max(ws) < 1024]
COARSE = [(130, 260, 3, 2, [5, 20]), (600, 700, 25, 7, [3, 12])]  # (nrows, ncols, factor, first_bin, windows)
FRONT8 = 66  # guard words in front of an output: the words behind them are 8-byte aligned


def min_diags(windows):
    wmax = max(windows)
    return [0, 1, 2, 2 * wmax - 1, 2 * wmax + 4]  # the last two: zeros for every window


class GuardedOut:
    """`n_sums` poisoned 64-bit words in device memory, 8-byte aligned, between guard words that hold
    POISON: the caller does not pre-zero, and a write beyond either end shows up"""

    def __init__(self, n_sums):
        import torch

        self.n = 2 * n_sums
        self.host = np.full(FRONT8 + self.n + BACK, POISON, dtype=np.uint32)
        self.tensor = torch.from_numpy(self.host.view(np.int32)).to("cuda:0")
        torch.cuda.synchronize()
        assert self.data_ptr() % 8 == 0

    def data_ptr(self):
        return self.tensor.data_ptr() + 4 * FRONT8

    def read(self):
        import torch

        torch.cuda.synchronize()
        return self.tensor.cpu().numpy().view(np.uint32)

    def unchanged(self):
        return np.array_equal(self.read(), self.host)

    def guards_intact(self):
        got = self.read()
        return (got[:FRONT8] == POISON).all() and (got[FRONT8 + self.n:] == POISON).all()

    def sums(self, n_windows):
        return self.read()[FRONT8:FRONT8 + self.n].copy().view(np.uint64).reshape(n_windows, -1)


@pytest.fixture(scope="module")
def ex():
    from modle_amd import pixels

    with pixels.Extractor(0) as e:
        yield e


@pytest.mark.parametrize("nrows,ncols,windows,fill", CASES)
def test_insulation_equals_the_definition(ex, nrows, ncols, windows, fill):
    band = make_band(nrows, ncols, fill)
    src = Guarded(band)
    for m in min_diags(windows):
        want = prefix_insulation(band, nrows, ncols, windows, m)
        if fill == "full" and m == 0:
            for k, w in enumerate(windows):
                assert w == 1 or ncols == 1 or int(want[k].max()) > 2**32
        if fill == "empty" or m >= 2 * max(windows) - 1:
            assert not want.any()
        # the device form, into a poisoned array
        d_out = GuardedOut(len(windows) * ncols)
        ex.insulation_into(src.data_ptr(), nrows, ncols, windows, m, d_out.data_ptr(), len(windows) * ncols)
        assert np.array_equal(d_out.sums(len(windows)), want), m
        assert d_out.guards_intact()
        # the host form, twice: the same again
        for _ in range(2):
            got = ex.insulation(src.data_ptr(), nrows, ncols, windows, m)
            assert got.dtype == np.uint64 and got.shape == (len(windows), ncols)
            assert np.array_equal(got, want), m
    assert src.unchanged()


@pytest.mark.parametrize("nrows,ncols,windows", [s for s in SHAPES if len(s[2]) > 1 and s[0] <= 600])
def test_a_window_alone_is_its_row_of_the_call_with_all(ex, nrows, ncols, windows):
    src = Guarded(make_band(nrows, ncols, "tenth", seed=1))
    together = ex.insulation(src.data_ptr(), nrows, ncols, windows, 1)
    for k, w in enumerate(windows):
        assert np.array_equal(ex.insulation(src.data_ptr(), nrows, ncols, [w], 1)[0], together[k]), w
    assert src.unchanged()


@pytest.mark.parametrize("nrows,ncols,windows", SHAPES[:-1])
def test_the_sums_add_up_to_the_weighted_diagonal_sums_of_the_marginals(ex, nrows, ncols, windows):
    src = Guarded(make_band(nrows, ncols, "full", seed=2))
    diag_sum, _ = ex.marginals(src.data_ptr(), nrows, ncols)
    for m in (0, 2):
        got = ex.insulation(src.data_ptr(), nrows, ncols, windows, m)
        for k, w in enumerate(windows):
            assert sum(int(x) for x in got[k]) == identity_rhs(diag_sum, w, m), (w, m)
    assert src.unchanged()


@pytest.mark.parametrize("nrows,ncols,k,first_bin,windows", COARSE)
def test_coarse_insulation_is_that_of_the_coarse_band(ex, nrows, ncols, k, first_bin, windows):
    from modle_amd import pixels

    band = make_band(nrows, ncols, "tenth", limit=2**20, seed=3)
    coarse, nr, nc = reference_coarsen(band, nrows, ncols, k, first_bin)
    assert pixels.coarse_shape(nrows, ncols, k, first_bin) == (nr, nc) and 2 * max(windows) - 1 <= nr
    src = Guarded(band)
    for m in min_diags(windows):
        want = prefix_insulation(coarse, nr, nc, windows, m)
        got = ex.coarse_insulation(src.data_ptr(), nrows, ncols, k, first_bin, windows, m)
        assert got.dtype == np.uint64 and got.shape == (len(windows), nc)
        assert np.array_equal(got, want), m
    # the fine path still serves, and the module-level forms (the process-wide context of the device)
    fine = prefix_insulation(band, nrows, ncols, windows, 2)
    for got in (ex.insulation(src.data_ptr(), nrows, ncols, windows), pixels.insulation(src.data_ptr(), nrows, ncols, windows)):
        assert np.array_equal(got, fine)
    assert np.array_equal(pixels.coarse_insulation(src.data_ptr(), nrows, ncols, k, first_bin, windows),
                          prefix_insulation(coarse, nr, nc, windows, 2))
    # a window that fits the fine band only is refused against the coarse shape
    with pytest.raises(pixels.PixelsError) as e:
        ex.coarse_insulation(src.data_ptr(), nrows, ncols, k, first_bin, [nr // 2 + 1 + nr % 2])
    assert e.value.code == pixels.ERR_ARG
    assert src.unchanged()


def test_a_stream_of_the_caller_and_buffers_that_grow():
    import torch

    from modle_amd import pixels

    stream = torch.cuda.Stream(device="cuda:0")
    assert stream.cuda_stream != 0
    small, large = make_band(5, 9, "full", seed=7), make_band(70, 193, "tenth", seed=7)
    want_small, want_large = prefix_insulation(small, 5, 9, [2, 3], 0), prefix_insulation(large, 70, 193, [35, 4, 9], 2)
    s, l = Guarded(small), Guarded(large)
    with pixels.Extractor(0) as e:
        first = e.insulation(s.data_ptr(), 5, 9, [2, 3], 0, stream=stream)
        again = e.insulation(l.data_ptr(), 70, 193, [35, 4, 9], 2, stream=stream)  # grows
        assert np.array_equal(again, want_large)
        d_out = GuardedOut(2 * 9)
        e.insulation_into(s.data_ptr(), 5, 9, [2, 3], 0, d_out.data_ptr(), 2 * 9, stream=stream)
        shrunk = e.insulation(s.data_ptr(), 5, 9, [2, 3], 0, stream=stream)  # reused
        stream.synchronize()
        assert np.array_equal(d_out.sums(2), want_small) and d_out.guards_intact()
        assert np.array_equal(shrunk, want_small)
        assert np.array_equal(first, want_small)  # the caller's
    assert s.unchanged() and l.unchanged()


def test_invalid_calls_are_argument_errors_and_write_nothing(ex):
    from modle_amd import pixels

    nrows, ncols = 5, 9
    src = Guarded(make_band(nrows, ncols, "full", seed=8))
    d_out = GuardedOut(9 * (ncols + 1))
    out, words = d_out.data_ptr(), 9 * (ncols + 1)
    inside = src.data_ptr() + 4 * (nrows * ncols)  # the band's trailing word: the last that is the band's
    inside -= inside % 8
    band = src.data_ptr()
    for what, args in [("w == 0", (band, nrows, ncols, [2, 0], 0, out, words)),
                       ("2w - 1 > nrows", (band, nrows, ncols, [4], 0, out, words)),
                       ("2w - 1 > nrows, among others", (band, nrows, ncols, [1, 3, 4], 0, out, words)),
                       ("w > 1024", (band, nrows, ncols, [1025], 0, out, words)),
                       ("no window", (band, nrows, ncols, [], 0, out, words)),
                       ("nine windows", (band, nrows, ncols, [1] * 9, 0, out, words)),
                       ("no band", (None, nrows, ncols, [2], 0, out, words)),
                       ("no output", (band, nrows, ncols, [2], 0, None, words)),
                       ("out_words too small", (band, nrows, ncols, [2, 3], 0, out, 2 * ncols - 1)),
                       ("a misaligned output", (band, nrows, ncols, [2], 0, out + 4, words)),
                       ("the output overlaps the band", (band, nrows, ncols, [2], 0, inside, words)),
                       ("the output ends inside the band", (band, nrows, ncols, [2], 0, band - band % 8 - 8 * ncols + 8, words)),
                       ("nrows > ncols", (band, ncols + 1, ncols, [2], 0, out, words)),
                       ("nrows 0", (band, 0, ncols, [1], 0, out, words))]:
        with pytest.raises(pixels.PixelsError) as e:
            ex.insulation_into(*args)
        assert e.value.code == pixels.ERR_ARG, what
    for windows in ([2, 0], [4], [1025], [], [1] * 9):
        with pytest.raises(pixels.PixelsError) as e:
            ex.insulation(band, nrows, ncols, windows)
        assert e.value.code == pixels.ERR_ARG
        with pytest.raises(pixels.PixelsError) as e:
            ex.coarse_insulation(band, nrows, ncols, 2, 0, windows if windows != [4] else [3])  # nrows' is 3
        assert e.value.code == pixels.ERR_ARG
    with pytest.raises(pixels.PixelsError) as e:
        ex.coarse_insulation(band, nrows, ncols, 1, 0, [2])
    assert e.value.code == pixels.ERR_ARG
    with pytest.raises(pixels.PixelsError) as e:
        ex.insulation(band, ncols + 1, ncols, [2])
    assert e.value.code == pixels.ERR_ARG
    with pytest.raises(pixels.PixelsError) as e:
        pixels.Extractor.insulation(ex, None, nrows, ncols, [2])
    assert e.value.code == pixels.ERR_ARG
    assert d_out.unchanged() and src.unchanged()  # (still poison)
    # an output that ends exactly where the band begins does not overlap it
    n_out = 2 * ncols  # two windows
    whole = GuardedOut(n_out + (nrows * ncols + 1 + 1) // 2)
    words32 = whole.host.copy()
    words32[FRONT8 + 2 * n_out:FRONT8 + 2 * n_out + nrows * ncols + 1] = src.host[FRONT:FRONT + src.n]
    import torch

    whole.host = words32
    whole.tensor = torch.from_numpy(words32.view(np.int32)).to("cuda:0")
    torch.cuda.synchronize()
    band_ptr = whole.data_ptr() + 8 * n_out
    ex.insulation_into(band_ptr, nrows, ncols, [3, 1], 1, whole.data_ptr(), n_out)
    got = whole.read()
    want = prefix_insulation(src.host[FRONT:FRONT + src.n], nrows, ncols, [3, 1], 1)
    assert np.array_equal(got[FRONT8:FRONT8 + 2 * n_out].copy().view(np.uint64).reshape(2, ncols), want)
    assert np.array_equal(got[FRONT8 + 2 * n_out:], words32[FRONT8 + 2 * n_out:]) and whole.guards_intact()


def test_simulator_forms_agree():
    """the interval of tests/test_gpu_marginals.py's test of the same name (80 x 200, from fine bin 5, 4
    cells): the host form, the torch form and the device form give the restatement on the band copied to
    the host, at the bin size and at three times it"""
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
        assert sim.pixels(iid).stats.nnz > 1000
        windows = [5, 40]
        for m in (2, 0):
            want = prefix_insulation(band, nrows, ncols, windows, m)
            assert want.any()
            t = sim.insulation_tensor(iid, windows, m)
            assert t.dtype == torch.int64 and t.device == torch.device("cuda", 0) and tuple(t.shape) == (2, ncols)
            torch.cuda.synchronize()
            assert np.array_equal(t.cpu().numpy().view(np.uint64), want)
            ins_sum, n_valid = sim.insulation(iid, windows, m)
            assert ins_sum.dtype == n_valid.dtype == np.uint64 and ins_sum.shape == n_valid.shape == (2, ncols)
            assert np.array_equal(ins_sum, want)
            assert all(np.array_equal(n_valid[k], pixels.insulation_n_valid(ncols, w, m)) for k, w in enumerate(windows))
            d_out = GuardedOut(2 * ncols)
            pixels.insulation_into(sim.outputs(iid)[0], nrows, ncols, windows, m, d_out.data_ptr(), 2 * ncols)
            assert np.array_equal(d_out.sums(2), want) and d_out.guards_intact()
            driver.check_insulation("chrA:25000-1025000", windows, m, ins_sum, reference_marginals(band, nrows, ncols, 0)[0])
        assert np.array_equal(sim.insulation(iid, windows)[0], prefix_insulation(band, nrows, ncols, windows, 2))  # the default
        score = api.insulation_score(*sim.insulation(iid, windows))
        assert score.shape == (2, ncols) and np.isfinite(score[1]).sum() > ncols // 2
        # at three times the bin size, anchored at the chromosome's start
        coarse, nr, nc = reference_coarsen(band, nrows, ncols, 3, 5)
        ins3, n_valid3 = sim.insulation(iid, [3, 10], 2, factor=3, first_bin=5)
        assert ins3.shape == n_valid3.shape == (2, nc)
        assert np.array_equal(ins3, prefix_insulation(coarse, nr, nc, [3, 10], 2))
        assert np.array_equal(n_valid3[1], pixels.insulation_n_valid(nc, 10, 2))
        assert np.array_equal(sim.copy_outputs(iid)[0], band)
    finally:
        sim.close()
