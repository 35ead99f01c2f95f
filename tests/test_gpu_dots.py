"""Dot calling on the MI355X (include/modle_pixels.h: modle_pixels_dots, _dots_to_host, _coarse_dots_to_host;
modle_amd/pixels.py; api.Simulator.dots, dots_tensors and dot_sums_tensor): the four neighbourhood sums of
every valid pixel and the candidate band equal, word for word, the numpy restatement of
tests/test_dots_outputs.py, for bands built on the host with a seeded generator.  The input lies between
poisoned guard words at an address that is 4-byte aligned only and holds 0xFFFFFFFF in every word that is
no pixel; both outputs are poisoned between guard words before the call (the library, not the caller,
defines every word).  The decision is one double product and one comparison on both sides: nothing here
has a tolerance."""
import functools

import numpy as np
import pytest

from test_dots_outputs import candidate_pixels, reference_candidates, sat_dot_sums, valid_mask
from test_gpu_insulation import GuardedOut
from test_gpu_marginals import FRONT, POISON, Guarded, make_band, reference_coarsen, reference_marginals

pytestmark = pytest.mark.gpu

T = 64  # the kernel's block of pixels (modle_dots.hip)
# (nrows, ncols, w, p, min_diag): exactly one valid pixel; a 5 x 5 window with a peak; one valid
# diagonal; T - 1, T, T + 1 and 2 T + 2 w + 1 columns with the band's upper edge inside a block, p = 0 and
# p = w - 1 among them; the cap w = 20 with one and three valid diagonals; one larger band
# A band without a valid pixel would need ncols <= 4 w + min_diag < nrows, which no call of the library
# accepts (nrows <= ncols is the band layout): (5, 4, 1, 0, 0) is held to that in the test of the refusals.
SHAPES = [(5, 5, 1, 0, 0), (9, 9, 2, 1, 0), (7, 30, 1, 0, 2),
          (40, T - 1, 3, 0, 0), (40, T, 3, 2, 2), (40, T + 1, 3, 1, 1), (100, 2 * T + 2 * 3 + 1, 3, 1, 2),
          (81, 200, 20, 19, 0), (83, 199, 20, 0, 2), (83, 201, 20, 7, 0), (200, 700, 5, 2, 2)]
FILLS = ["empty", "tenth", "full", "constant"]


@functools.lru_cache(maxsize=None)
def case(nrows, ncols, w, p, min_diag, fill, limit=0xFFFFFFFF, seed=0):
    """(band, sums) of a shape and a fill, made once; neither is written to"""
    if fill == "constant":
        band = make_band(nrows, ncols, "empty")
        band[band == 0] = 3
    else:
        band = make_band(nrows, ncols, fill, limit=limit, seed=seed)
    sums = sat_dot_sums(band, nrows, ncols, w, p, min_diag)
    band.setflags(write=False)
    sums.setflags(write=False)
    return band, sums


def tables(nrows, w, p, seed):
    """all zeros (every valid pixel with obs >= min_count is a candidate), all +inf (none unless the sum is
    0: 0 * inf is NaN, also none), and two seeded tables around 1 / area with zeros and infinities mixed in"""
    from modle_amd import pixels

    rng = np.random.default_rng([seed, nrows, w, p])
    out = [np.zeros((4, nrows)), np.full((4, nrows), np.inf)]
    for spread in (2.0, 0.5):
        t = rng.random((4, nrows)) * spread / np.array(pixels.dot_areas(w, p), dtype=np.float64)[:, None]
        t[rng.random((4, nrows)) < 0.05] = 0.0
        t[rng.random((4, nrows)) < 0.02] = np.inf
        out.append(t)
    return out


def cand_buffer(nrows, ncols):
    return Guarded(np.full(nrows * ncols + 1, POISON, dtype=np.uint32))  # the caller does not pre-zero


def cand_words(buf):
    return buf.read()[FRONT:FRONT + buf.n]


@pytest.fixture(scope="module")
def ex():
    from modle_amd import pixels

    with pixels.Extractor(0) as e:
        yield e


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("nrows,ncols,w,p,min_diag", SHAPES)
def test_sums_and_candidates_equal_the_definition(ex, nrows, ncols, w, p, min_diag, fill):
    band, sums = case(nrows, ncols, w, p, min_diag, fill)
    n_valid = int(valid_mask(nrows, ncols, w, min_diag).sum())
    if fill == "full" and n_valid:
        assert int(sums.max()) > 2**32
    if fill == "empty" or n_valid == 0:
        assert not sums.any()
    src = Guarded(band)
    for n, table in enumerate(tables(nrows, w, p, 1)):
        min_count = (1, 1, 2, 2**31)[n]
        want = reference_candidates(band, nrows, ncols, sums, table, w, min_diag, min_count)
        if n == 0 and fill in ("full", "constant"):
            assert np.count_nonzero(want) == n_valid
        d_cand, d_sums = cand_buffer(nrows, ncols), GuardedOut(4 * nrows * ncols)
        ex.dots_into(src.data_ptr(), nrows, ncols, w, p, min_diag, min_count, table, d_cand.data_ptr(),
                     d_sums.data_ptr())
        assert np.array_equal(d_sums.sums(4).reshape(4, ncols, nrows), sums), n
        assert np.array_equal(cand_words(d_cand), want), n
        assert d_cand.guards_intact() and d_sums.guards_intact()
    assert src.unchanged()


@pytest.mark.parametrize("nrows,ncols,w,p,min_diag", [SHAPES[0], SHAPES[1], SHAPES[5], SHAPES[8]])
def test_each_output_alone(ex, nrows, ncols, w, p, min_diag):
    band, sums = case(nrows, ncols, w, p, min_diag, "tenth")
    table = tables(nrows, w, p, 2)[2]
    src = Guarded(band)
    d_cand = cand_buffer(nrows, ncols)
    ex.dots_into(src.data_ptr(), nrows, ncols, w, p, min_diag, 1, table, d_cand.data_ptr(), None)
    assert np.array_equal(cand_words(d_cand), reference_candidates(band, nrows, ncols, sums, table, w, min_diag, 1))
    d_sums = GuardedOut(4 * nrows * ncols)
    ex.dots_into(src.data_ptr(), nrows, ncols, w, p, min_diag, 1, None, None, d_sums.data_ptr())  # no table needed
    assert np.array_equal(d_sums.sums(4).reshape(4, ncols, nrows), sums)
    assert d_cand.guards_intact() and d_sums.guards_intact() and src.unchanged()


def test_a_threshold_that_equals_the_count_exactly_and_one_ulp_more(ex):
    """a constant band, w = 1, p = 0: the areas are 4 and 1, so with the table (0.25, 1, 0, 0) both
    products equal obs and the pixel is a candidate; with one ulp more, whatever numpy says"""
    nrows, ncols = 7, 70
    band, sums = case(nrows, ncols, 1, 0, 0, "constant")
    src = Guarded(band)
    for first in (0.25, np.nextafter(0.25, 1.0), np.nextafter(0.25, 0.0)):
        table = np.zeros((4, nrows))
        table[0], table[1] = first, 1.0
        want = reference_candidates(band, nrows, ncols, sums, table, 1, 0, 1)
        assert np.count_nonzero(want) == (0 if first > 0.25 else valid_mask(nrows, ncols, 1, 0).sum())
        d_cand = cand_buffer(nrows, ncols)
        ex.dots_into(src.data_ptr(), nrows, ncols, 1, 0, 0, 1, table, d_cand.data_ptr(), None)
        assert np.array_equal(cand_words(d_cand), want), first
    assert src.unchanged()


@pytest.mark.parametrize("nrows,ncols,w,p,min_diag", [SHAPES[0], SHAPES[1], SHAPES[6], SHAPES[9], SHAPES[10]])
def test_the_host_form_is_the_extraction_of_the_candidate_band(ex, nrows, ncols, w, p, min_diag):
    """counts below 2^31, which the extraction accepts; twice in a row: the same again"""
    band, sums = case(nrows, ncols, w, p, min_diag, "full", limit=2**31, seed=4)
    src = Guarded(band)
    for table, min_count in zip(tables(nrows, w, p, 3), (1, 1, 2**29, 1)):
        want = reference_candidates(band, nrows, ncols, sums, table, w, min_diag, min_count)
        b1, b2, cnt = candidate_pixels(want, nrows, ncols)
        for _ in range(2):
            got = ex.dots(src.data_ptr(), nrows, ncols, w, p, min_diag, min_count, table, bin_offset=11)
            assert got.bin1.dtype == got.bin2.dtype == np.int64 and got.count.dtype == np.int32
            assert np.array_equal(got.bin1, b1 + 11) and np.array_equal(got.bin2, b2 + 11)
            assert np.array_equal(got.count, cnt)
            assert got.stats.nnz == len(b1) and got.stats.sum == int(cnt.astype(np.int64).sum())
            assert len(got.bin1_offset) == ncols + 1 and got.bin1_offset[-1] == len(b1)
        # the same pixels as extract() finds in the restated candidate band
        held = Guarded(want)
        px = ex.extract(held.data_ptr(), nrows, ncols, 11)
        assert np.array_equal(px.bin1, got.bin1) and np.array_equal(px.bin2, got.bin2)
        assert np.array_equal(px.count, got.count) and np.array_equal(px.bin1_offset, got.bin1_offset)
    assert src.unchanged()


@pytest.mark.parametrize("nrows,ncols,k,first_bin,w,p", [(65, 130, 3, 2, 2, 1), (200, 700, 4, 7, 5, 0)])
def test_coarse_dots_are_those_of_the_coarse_band(ex, nrows, ncols, k, first_bin, w, p):
    from modle_amd import pixels

    band = make_band(nrows, ncols, "tenth", limit=2**20, seed=3)
    coarse, nr, nc = reference_coarsen(band, nrows, ncols, k, first_bin)
    assert pixels.coarse_shape(nrows, ncols, k, first_bin) == (nr, nc) and 4 * w + 1 + 2 <= nr
    src = Guarded(band)
    sums = sat_dot_sums(coarse, nr, nc, w, p, 2)
    for table in tables(nr, w, p, 5):
        b1, b2, cnt = candidate_pixels(reference_candidates(coarse, nr, nc, sums, table, w, 2, 1), nr, nc)
        for got in (ex.coarse_dots(src.data_ptr(), nrows, ncols, k, first_bin, w, p, 2, 1, table),
                    pixels.coarse_dots(src.data_ptr(), nrows, ncols, k, first_bin, w, p, 2, 1, table)):
            assert np.array_equal(got.bin1, b1) and np.array_equal(got.bin2, b2) and np.array_equal(got.count, cnt)
            assert len(got.bin1_offset) == nc + 1
    # the fine path still serves, and a window that fits the fine band only is refused against the coarse shape
    fine = sat_dot_sums(band, nrows, ncols, w, p, 2)
    table = tables(nrows, w, p, 5)[3]
    b1, b2, cnt = candidate_pixels(reference_candidates(band, nrows, ncols, fine, table, w, 2, 1), nrows, ncols)
    got = pixels.dots(src.data_ptr(), nrows, ncols, w, p, 2, 1, table)
    assert np.array_equal(got.bin1, b1) and np.array_equal(got.bin2, b2) and np.array_equal(got.count, cnt)
    wide = (nr - 3) // 4 + 1
    assert wide <= 20 and 4 * wide + 3 <= nrows
    with pytest.raises(pixels.PixelsError) as e:
        ex.coarse_dots(src.data_ptr(), nrows, ncols, k, first_bin, wide, 0, 2, 1, np.zeros((4, nr)))
    assert e.value.code == pixels.ERR_ARG
    assert src.unchanged()


def test_a_stream_of_the_caller_and_buffers_that_grow():
    import torch

    from modle_amd import pixels

    stream = torch.cuda.Stream(device="cuda:0")
    assert stream.cuda_stream != 0
    (small, s_sums), (large, l_sums) = case(9, 9, 2, 1, 0, "full", 2**31, 7), case(100, 135, 3, 1, 2, "tenth", 2**31, 7)
    t_small, t_large = tables(9, 2, 1, 7)[0], tables(100, 3, 1, 7)[2]
    want_small = reference_candidates(small, 9, 9, s_sums, t_small, 2, 0, 1)
    want_large = reference_candidates(large, 100, 135, l_sums, t_large, 3, 2, 1)
    assert want_small.any() and want_large.any()
    s, l = Guarded(small), Guarded(large)
    with pixels.Extractor(0) as e:
        first = e.dots(s.data_ptr(), 9, 9, 2, 1, 0, 1, t_small, stream=stream)
        again = e.dots(l.data_ptr(), 100, 135, 3, 1, 2, 1, t_large, stream=stream)  # grows
        d_cand, d_sums = cand_buffer(100, 135), GuardedOut(4 * 9 * 9)
        e.dots_into(l.data_ptr(), 100, 135, 3, 1, 2, 1, t_large, d_cand.data_ptr(), None, stream=stream)
        e.dots_into(s.data_ptr(), 9, 9, 2, 1, 0, 1, t_small, None, d_sums.data_ptr(), stream=stream)  # the table shrinks
        shrunk = e.dots(s.data_ptr(), 9, 9, 2, 1, 0, 1, t_small, stream=stream)  # reused
        stream.synchronize()
        assert np.array_equal(cand_words(d_cand), want_large) and d_cand.guards_intact()
        assert np.array_equal(d_sums.sums(4).reshape(4, 9, 9), s_sums) and d_sums.guards_intact()
        for got, want, shape in ((first, want_small, (9, 9)), (again, want_large, (100, 135)), (shrunk, want_small, (9, 9))):
            b1, b2, cnt = candidate_pixels(want, *shape)
            assert np.array_equal(got.bin1, b1) and np.array_equal(got.bin2, b2) and np.array_equal(got.count, cnt)
    assert s.unchanged() and l.unchanged()


def test_invalid_calls_are_argument_errors_and_write_nothing(ex):
    from modle_amd import pixels

    nrows, ncols = 9, 12
    src = Guarded(make_band(nrows, ncols, "full", seed=8))
    d_cand, d_sums = cand_buffer(nrows, ncols), GuardedOut(4 * nrows * ncols)
    band, cand, sums = src.data_ptr(), d_cand.data_ptr(), d_sums.data_ptr()
    ok = np.zeros((4, nrows))
    nan, neg, outside = ok.copy(), ok.copy(), ok.copy()
    nan[2, 4], neg[0, 5] = np.nan, -1e-300
    outside[:, :4], outside[:, 7:] = np.nan, -1.0  # w = 2, min_diag = 0: only d = 4 .. 4 is read; w = 1: 2 .. 6
    inside = band + 4 * (nrows * ncols)  # the band's trailing word
    for what, args in [("no band", (None, nrows, ncols, 2, 1, 0, 1, ok, cand, sums)),
                       ("no output", (band, nrows, ncols, 2, 1, 0, 1, ok, None, None)),
                       ("nrows 0", (band, 0, ncols, 2, 1, 0, 1, ok, cand, sums)),
                       ("no valid pixel: nrows 5 > ncols 4", (band, 5, 4, 1, 0, 0, 1, np.zeros((4, 5)), cand, sums)),
                       ("nrows > ncols", (band, ncols + 1, ncols, 2, 1, 0, 1, np.zeros((4, ncols + 1)), cand, sums)),
                       ("p == w", (band, nrows, ncols, 2, 2, 0, 1, ok, cand, sums)),
                       ("p > w", (band, nrows, ncols, 1, 2, 0, 1, ok, cand, sums)),
                       ("w == 0", (band, nrows, ncols, 0, 0, 0, 1, ok, cand, sums)),
                       ("w > 20", (band, nrows, ncols, 21, 0, 0, 1, ok, cand, sums)),
                       ("4w + 1 > nrows", (band, nrows, ncols, 3, 0, 0, 1, ok, cand, sums)),
                       ("4w + 1 + min_diag > nrows", (band, nrows, ncols, 2, 0, 1, 1, ok, cand, sums)),
                       ("a huge min_diag", (band, nrows, ncols, 2, 0, 2**64 - 8, 1, ok, cand, sums)),
                       ("min_count 0", (band, nrows, ncols, 2, 1, 0, 0, ok, cand, sums)),
                       ("a NaN at a valid d", (band, nrows, ncols, 2, 1, 0, 1, nan, cand, sums)),
                       ("a NaN at a valid d, sums only", (band, nrows, ncols, 2, 1, 0, 1, nan, None, sums)),
                       ("a negative entry at a valid d", (band, nrows, ncols, 1, 0, 0, 1, neg, cand, sums)),
                       ("no table with candidates", (band, nrows, ncols, 2, 1, 0, 1, None, cand, None)),
                       ("a misaligned d_sums", (band, nrows, ncols, 2, 1, 0, 1, ok, cand, sums + 4)),
                       ("d_cand overlaps the band", (band, nrows, ncols, 2, 1, 0, 1, ok, inside, sums)),
                       ("d_cand ends inside the band", (band, nrows, ncols, 2, 1, 0, 1, ok, band - 4 * nrows * ncols, sums)),
                       ("d_sums overlaps the band", (band, nrows, ncols, 2, 1, 0, 1, ok, cand, inside - inside % 8)),
                       ("the outputs overlap", (band, nrows, ncols, 2, 1, 0, 1, ok, sums + 32 * nrows * ncols - 4, sums)),
                       ("d_cand inside d_sums", (band, nrows, ncols, 2, 1, 0, 1, ok, sums + 8, sums))]:
        with pytest.raises(pixels.PixelsError) as e:
            ex.dots_into(*args)
        assert e.value.code == pixels.ERR_ARG, what
    with pytest.raises(pixels.PixelsError) as e:
        ex.dots_into(band, nrows, ncols, 2, 1, 0, 1, np.zeros((4, nrows + 1)), cand, sums)  # refused by pixels.py
    assert e.value.code == pixels.ERR_ARG
    for args in [(2, 2, 0, 1, ok), (0, 0, 0, 1, ok), (21, 0, 0, 1, ok), (3, 0, 0, 1, ok), (2, 0, 1, 1, ok), (2, 1, 0, 0, ok),
                 (2, 1, 0, 1, nan), (2, 1, 0, 1, None)]:
        with pytest.raises(pixels.PixelsError) as e:
            ex.dots(band, nrows, ncols, *args)
        assert e.value.code == pixels.ERR_ARG, args
    with pytest.raises(pixels.PixelsError) as e:
        ex.dots(band, nrows, ncols, 2, 1, 0, 1, ok, bin_offset=-1)
    assert e.value.code == pixels.ERR_ARG
    with pytest.raises(pixels.PixelsError) as e:
        ex.dots(None, nrows, ncols, 2, 1, 0, 1, ok)
    assert e.value.code == pixels.ERR_ARG
    with pytest.raises(pixels.PixelsError) as e:
        ex.coarse_dots(band, nrows, ncols, 1, 0, 1, 0, 0, 1, ok)  # factor 1
    assert e.value.code == pixels.ERR_ARG
    with pytest.raises(pixels.PixelsError) as e:
        ex.coarse_dots(band, nrows, ncols, 2, 0, 2, 1, 0, 1, np.zeros((4, 5)))  # nrows' is 5: 4 w + 1 = 9
    assert e.value.code == pixels.ERR_ARG
    assert d_cand.unchanged() and d_sums.unchanged() and src.unchanged()  # (still poison)
    # entries outside the valid diagonals are not looked at
    want_sums = sat_dot_sums(src.host[FRONT:FRONT + src.n], nrows, ncols, 2, 1, 0)
    ex.dots_into(band, nrows, ncols, 2, 1, 0, 1, outside, cand, sums)
    assert np.array_equal(cand_words(d_cand),
                          reference_candidates(src.host[FRONT:FRONT + src.n], nrows, ncols, want_sums, ok, 2, 0, 1))
    assert np.array_equal(d_sums.sums(4).reshape(4, ncols, nrows), want_sums)
    assert d_cand.guards_intact() and d_sums.guards_intact()


def test_simulator_forms_agree():
    """the interval of tests/test_gpu_marginals.py's test of the same name (80 x 200, from fine bin 5, 4
    cells): dots, dots_tensors and dot_sums_tensor give the restatement on the band copied to the host, at
    the bin size and at three times it"""
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
        folds = (1.1, 1.1, 1.05, 1.05)
        for factor, first_bin, w, p in ((1, 0, 5, 2), (3, 5, 3, 1)):
            if factor == 1:
                b, nr, nc = band, nrows, ncols
            else:
                b, nr, nc = reference_coarsen(band, nrows, ncols, factor, first_bin)
            for min_diag, min_count in ((2, 1), (0, 2)):
                sums = sat_dot_sums(b, nr, nc, w, p, min_diag)
                diag_sum = reference_marginals(b, nr, nc, 0)[0]
                table = pixels.dot_scales(diag_sum, nc, w, p, folds, min_diag)
                b1, b2, cnt = candidate_pixels(reference_candidates(b, nr, nc, sums, table, w, min_diag, min_count), nr, nc)
                assert 0 < len(b1) < valid_mask(nr, nc, w, min_diag).sum()
                kw = dict(w=w, p=p, min_count=min_count, folds=folds, min_diag=min_diag, factor=factor, first_bin=first_bin)
                g1, g2, gc, ge = sim.dots(iid, **kw)
                assert np.array_equal(g1, b1) and np.array_equal(g2, b2) and np.array_equal(gc, cnt)
                assert ge.dtype == np.float64
                assert np.array_equal(ge, (diag_sum.astype(np.float64) / (nc - np.arange(nr)))[b2 - b1])
                driver.check_dots("chrA:25000-1025000", nr, nc, w, min_diag, min_count, g1, g2, gc)
                t1, t2, tc = sim.dots_tensors(iid, **kw)
                assert t1.dtype == t2.dtype == torch.int64 and tc.dtype == torch.int32
                assert t1.device == torch.device("cuda", 0)
                assert np.array_equal(t1.cpu().numpy(), b1) and np.array_equal(t2.cpu().numpy(), b2)
                assert np.array_equal(tc.cpu().numpy(), cnt)
                t = sim.dot_sums_tensor(iid, w, p, min_diag, factor=factor, first_bin=first_bin)
                assert t.dtype == torch.int64 and tuple(t.shape) == (4, nc, nr) and t.device == torch.device("cuda", 0)
                torch.cuda.synchronize()
                assert np.array_equal(t.cpu().numpy().view(np.uint64), sums)
        assert np.array_equal(sim.copy_outputs(iid)[0], band)
    finally:
        sim.close()
