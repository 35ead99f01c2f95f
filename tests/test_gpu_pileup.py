"""Pileups on the MI355X (include/modle_pixels.h: modle_pixels_pileup, _pileup_to_host, _coarse_pileup_to_host;
modle_amd/pixels.py; api.Simulator.pileup and pileup_tensors): the summed windows and the count of accepted
anchors equal, word for word, the restatement of tests/test_pileup_outputs.py, for bands built on the host
with a seeded generator.  The band lies between poisoned guard words at an address that is 4-byte aligned
only and holds 0xFFFFFFFF in every word that is no pixel, so a window that left the band or the matrix
would show in the sum; both outputs are poisoned between guard words before the call (the library, not the
caller, defines every word).  The sums are integers: nothing here has a tolerance."""
import functools

import numpy as np
import pytest

from test_gpu_insulation import GuardedOut
from test_gpu_marginals import FRONT, POISON, Guarded, make_band, reference_coarsen
from test_pileup_outputs import I64_MAX, I64_MIN, reference_accepts, reference_pileup

pytestmark = pytest.mark.gpu

# (nrows, ncols, f): one word; exactly one acceptable anchor, on the diagonal; a thin band; 225 and 289 cells,
# either side of the step from one accumulator per lane to four; 961 cells, the last of the four; the cap
# f = 32 (17 accumulators) on a band that is all triangle and on one with five free diagonals; a larger band
SHAPES = [(1, 1, 0), (3, 3, 1), (7, 30, 1), (40, 65, 7), (40, 65, 8), (40, 200, 15), (65, 65, 32), (70, 300, 32),
          (200, 700, 10)]
FILLS = ["empty", "tenth", "full", "constant"]
BATCH = 256  # anchors of a batch = lanes of a workgroup (modle_pileup.hip)


@functools.lru_cache(maxsize=None)
def band_of(nrows, ncols, fill, limit=0xFFFFFFFF, seed=0):
    if fill == "constant":
        band = make_band(nrows, ncols, "empty")
        band[band == 0] = 3
    else:
        band = make_band(nrows, ncols, fill, limit=limit, seed=seed)
    band.setflags(write=False)
    return band


def long_n():
    """an anchor count that uses every workgroup of the capped grid: workgroup g of G takes the anchors
    [g n / G, (g + 1) n / G), here 273 or 274 of them -- a whole batch and a ragged one, of two lengths"""
    from modle_amd import pixels

    g = pixels.PILEUP_GROUPS
    n = g * (BATCH + 17) + 112
    assert n <= 70_000 and n >= 8 * g  # (a workgroup per 8 anchors until the cap binds)
    sizes = {(k + 1) * n // g - k * n // g for k in range(g)}
    assert len(sizes) == 2 and BATCH < min(sizes) and max(sizes) < 2 * BATCH
    return n


@functools.lru_cache(maxsize=None)
def anchor_lists(nrows, ncols, f):
    """name -> (a, b), int64 arrays relative to the band"""
    rng = np.random.default_rng([7, nrows, ncols, f])
    dmax = nrows - 1 - 2 * f

    def valid(m):
        d = rng.integers(0, dmax + 1, size=m)
        a = f + (rng.random(m) * (ncols - 2 * f - d)).astype(np.int64)
        return a, a + d

    def rejected(m):
        kind = rng.integers(0, 4, size=m)
        a, b = valid(m)
        a2 = np.where(kind == 0, rng.integers(-5, f, size=m) if f else -1 - rng.integers(0, 5, size=m), a)  # a < f
        b2 = np.where(kind == 0, np.maximum(a2, b), b)
        b2 = np.where(kind == 1, ncols - f + rng.integers(0, 4, size=m), b2)  # b + f > ncols - 1
        a2 = np.where(kind == 2, b2 + 1 + rng.integers(0, 3, size=m), a2)     # a > b
        b2 = np.where(kind == 3, a2 + dmax + 1 + rng.integers(0, 3, size=m), b2)  # the window leaves the band
        return a2, b2

    va, vb = valid(320)
    ra, rb = rejected(320)
    extremes = np.array([[I64_MIN, I64_MIN], [I64_MAX, I64_MAX], [I64_MIN, I64_MAX], [I64_MAX, I64_MIN], [f, I64_MAX],
                         [I64_MIN, f]], dtype=np.int64)
    ma, mb = np.concatenate([va, ra, extremes[:, 0]]), np.concatenate([vb, rb, extremes[:, 1]])
    order = rng.permutation(len(ma))
    ma, mb = ma[order], mb[order]
    lists = {"mix": (ma, mb), "mix shuffled": (ma[::-1].copy(), mb[::-1].copy())}
    for n in (0, 1, 255, 256, 257):
        lists[f"n = {n}"] = (ma[:n], mb[:n])
    lists["all rejected"] = rejected(300)
    da = f + (rng.random(300) * (ncols - 2 * f)).astype(np.int64)
    lists["all on the diagonal"] = (da, da.copy())
    lists["all the same"] = (np.full(300, va[0]), np.full(300, vb[0]))
    lists["the four extreme positions"] = (np.array([f, f, ncols - 1 - f - dmax, ncols - 1 - f], dtype=np.int64),
                                           np.array([f, f + dmax, ncols - 1 - f, ncols - 1 - f], dtype=np.int64))
    la, lb = valid(long_n())
    holes = rng.random(len(la)) < 0.1
    lists["long"] = (np.where(holes, -1, la), lb)
    for a, b in lists.values():
        a.setflags(write=False), b.setflags(write=False)
    return lists


@functools.lru_cache(maxsize=None)
def wanted(nrows, ncols, f, fill, name):
    a, b = anchor_lists(nrows, ncols, f)[name]
    return reference_pileup(band_of(nrows, ncols, fill), nrows, ncols, f, a, b)


def on_device(values):
    import torch

    return torch.from_numpy(np.array(values, dtype=np.int64)).to("cuda:0")  # (a copy: the lists are read-only)


def run(ex, src, nrows, ncols, f, a, b, bin_offset=0, with_n_used=True):
    """the device form into poisoned outputs: (pile, n_used or None)"""
    s = 2 * f + 1
    d_a, d_b = on_device(np.asarray(a) + bin_offset), on_device(np.asarray(b) + bin_offset)
    d_pile, d_used = GuardedOut(s * s), GuardedOut(1)
    n = len(a)
    ex.pileup_into(src.data_ptr(), nrows, ncols, f, d_a.data_ptr() if n else None, d_b.data_ptr() if n else None, n,
                   d_pile.data_ptr(), d_used.data_ptr() if with_n_used else None, bin_offset)
    pile = d_pile.sums(1).reshape(s, s)
    assert d_pile.guards_intact() and d_used.guards_intact()
    if not with_n_used:
        assert d_used.unchanged()
        return pile, None
    return pile, int(d_used.sums(1)[0, 0])


@pytest.fixture(scope="module")
def ex():
    from modle_amd import pixels

    with pixels.Extractor(0) as e:
        yield e


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("nrows,ncols,f", SHAPES)
def test_piles_equal_the_definition(ex, nrows, ncols, f, fill):
    band = band_of(nrows, ncols, fill)
    src = Guarded(band)
    lists = anchor_lists(nrows, ncols, f)
    got = {}
    for name, (a, b) in lists.items():
        want, used = wanted(nrows, ncols, f, fill, name)
        assert used == int(reference_accepts(nrows, ncols, f, a, b).sum())
        if name == "all rejected" or name == "n = 0":
            assert used == 0 and not want.any()
        elif name in ("all on the diagonal", "all the same", "the four extreme positions"):
            assert used == len(a)
        elif name.startswith("mix") or name == "long":
            assert 0.35 * len(a) < used < len(a)
        if fill == "empty":
            assert not want.any()
        if fill == "constant":
            assert (want == 3 * used).all()
        if fill == "full" and used > 1:
            assert int(want.max()) > 2**32, name
        pile, n_used = got[name] = run(ex, src, nrows, ncols, f, a, b)
        assert n_used == used, name
        assert np.array_equal(pile, want), name
    assert np.array_equal(got["mix"][0], got["mix shuffled"][0]) and got["mix"][1] == got["mix shuffled"][1]
    if f:  # a window on the diagonal is symmetric
        assert np.array_equal(got["all on the diagonal"][0], got["all on the diagonal"][0].T)
    assert src.unchanged()


@pytest.mark.parametrize("nrows,ncols,f", [SHAPES[1], SHAPES[4], SHAPES[7]])
def test_without_n_used_and_with_a_bin_offset(ex, nrows, ncols, f):
    src = Guarded(band_of(nrows, ncols, "tenth"))
    a, b = anchor_lists(nrows, ncols, f)["mix"]
    want, used = wanted(nrows, ncols, f, "tenth", "mix")
    pile, none = run(ex, src, nrows, ncols, f, a, b, with_n_used=False)
    assert none is None and np.array_equal(pile, want)
    keep = (np.abs(a.astype(np.float64)) < 2**62) & (np.abs(b.astype(np.float64)) < 2**62)  # the shift stays an int64
    want, used = reference_pileup(band_of(nrows, ncols, "tenth"), nrows, ncols, f, a[keep], b[keep])
    for off in (11, -9, 2**61, -2**61):
        pile, n_used = run(ex, src, nrows, ncols, f, a[keep], b[keep], bin_offset=off)
        assert n_used == used and np.array_equal(pile, want), off
    # unshifted anchors against an offset: the extremes must not wrap into the band
    for off in (I64_MIN, I64_MAX, -1, 1):
        d_a, d_b = on_device(a), on_device(b)
        d_pile, d_used = GuardedOut((2 * f + 1) ** 2), GuardedOut(1)
        ex.pileup_into(src.data_ptr(), nrows, ncols, f, d_a.data_ptr(), d_b.data_ptr(), len(a), d_pile.data_ptr(),
                       d_used.data_ptr(), off)
        ok = reference_accepts(nrows, ncols, f, a, b, off)
        shifted = [(int(x) - off, int(y) - off) for x, y in zip(a[ok], b[ok])]
        want, used = reference_pileup(band_of(nrows, ncols, "tenth"), nrows, ncols, f, [p[0] for p in shifted],
                                      [p[1] for p in shifted])
        assert used == int(ok.sum()) == int(d_used.sums(1)[0, 0])
        assert np.array_equal(d_pile.sums(1).reshape(want.shape), want), off
    assert src.unchanged()


@pytest.mark.parametrize("nrows,ncols,f", [SHAPES[0], SHAPES[3], SHAPES[5], SHAPES[7]])
def test_the_host_form_twice_in_a_row(ex, nrows, ncols, f):
    from modle_amd import pixels

    src = Guarded(band_of(nrows, ncols, "full"))
    for name in ("mix", "n = 0", "long", "n = 1"):
        a, b = anchor_lists(nrows, ncols, f)[name]
        want, used = wanted(nrows, ncols, f, "full", name)
        for form in (ex.pileup, ex.pileup, pixels.pileup):
            pile, n_used = form(src.data_ptr(), nrows, ncols, f, a + 3, b + 3, bin_offset=3)
            assert pile.dtype == np.uint64 and pile.shape == (2 * f + 1, 2 * f + 1) and type(n_used) is int
            assert n_used == used and np.array_equal(pile, want), name
    assert src.unchanged()


@pytest.mark.parametrize("nrows,ncols,k,first_bin,f", [(65, 130, 2, 3, 5), (200, 700, 5, 7, 10)])
def test_coarse_piles_are_those_of_the_coarse_band(ex, nrows, ncols, k, first_bin, f):
    from modle_amd import pixels

    assert first_bin % k != 0
    band = make_band(nrows, ncols, "tenth", limit=2**20, seed=3)
    coarse, nr, nc = reference_coarsen(band, nrows, ncols, k, first_bin)
    assert pixels.coarse_shape(nrows, ncols, k, first_bin) == (nr, nc) and 2 * f + 1 <= nr
    src = Guarded(band)
    for name in ("mix", "all on the diagonal", "n = 257"):
        a, b = anchor_lists(nr, nc, f)[name]
        want, used = reference_pileup(coarse, nr, nc, f, a, b)
        assert used > 0 and want.any()
        for got in (ex.coarse_pileup(src.data_ptr(), nrows, ncols, k, first_bin, f, a, b),
                    pixels.coarse_pileup(src.data_ptr(), nrows, ncols, k, first_bin, f, a + 4, b + 4, bin_offset=4)):
            assert got[1] == used and np.array_equal(got[0], want), name
    # the fine path still serves, and a flank that fits the fine band only is refused against the coarse shape
    a, b = anchor_lists(nrows, ncols, f)["mix"]
    want, used = reference_pileup(band, nrows, ncols, f, a, b)
    got = ex.pileup(src.data_ptr(), nrows, ncols, f, a, b)
    assert got[1] == used and np.array_equal(got[0], want)
    wide = nr // 2 + 1
    assert wide <= 32 and 2 * wide + 1 <= nrows and 2 * wide + 1 > nr
    with pytest.raises(pixels.PixelsError) as e:
        ex.coarse_pileup(src.data_ptr(), nrows, ncols, k, first_bin, wide, [wide], [wide])
    assert e.value.code == pixels.ERR_ARG
    assert src.unchanged()


def test_invalid_calls_are_argument_errors_and_write_nothing(ex):
    import ctypes as C

    from modle_amd import pixels

    nrows, ncols, f = 70, 80, 2
    src = Guarded(make_band(nrows, ncols, "full", seed=8))
    d_a, d_b = on_device([5, 6, 7]), on_device([9, 9, 9])
    d_pile, d_used = GuardedOut(25), GuardedOut(1)
    band, pa, pb, pile, used = src.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), d_pile.data_ptr(), d_used.data_ptr()
    inside = band + 4 * (nrows * ncols)  # the band's trailing word
    inside -= inside % 8
    for what, args in [("no band", (None, nrows, ncols, f, pa, pb, 3, pile, used)),
                       ("no first anchors", (band, nrows, ncols, f, None, pb, 3, pile, used)),
                       ("no second anchors", (band, nrows, ncols, f, pa, None, 3, pile, used)),
                       ("no pile", (band, nrows, ncols, f, pa, pb, 3, None, used)),
                       ("f > 32", (band, nrows, ncols, 33, pa, pb, 3, pile, used)),
                       ("2 f + 1 > nrows", (band, 4, ncols, f, pa, pb, 3, pile, used)),
                       ("nrows == 0", (band, 0, ncols, 0, pa, pb, 3, pile, used)),
                       ("nrows > ncols", (band, ncols + 1, ncols, f, pa, pb, 3, pile, used)),
                       ("n == 2^31", (band, nrows, ncols, f, pa, pb, 2**31, pile, used)),
                       ("a misaligned pile", (band, nrows, ncols, f, pa, pb, 3, pile + 4, used)),
                       ("a misaligned n_used", (band, nrows, ncols, f, pa, pb, 3, pile, used + 4)),
                       ("the pile overlaps the band", (band, nrows, ncols, f, pa, pb, 3, inside, used)),
                       ("the pile ends inside the band", (band, nrows, ncols, f, pa, pb, 3, band - band % 8 - 8 * 24, used)),
                       ("n_used overlaps the band", (band, nrows, ncols, f, pa, pb, 3, pile, inside)),
                       ("the pile overlaps the first anchors", (band, nrows, ncols, f, pa, pb, 3, pa + 16, used)),
                       ("the pile overlaps the second anchors", (band, nrows, ncols, f, pa, pb, 3, pb - 8 * 24, used)),
                       ("n_used overlaps the anchors", (band, nrows, ncols, f, pa, pb, 3, pile, pb + 8)),
                       ("n_used inside the pile", (band, nrows, ncols, f, pa, pb, 3, pile, pile + 8 * 24))]:
        with pytest.raises(pixels.PixelsError) as e:
            ex.pileup_into(*args)
        assert e.value.code == pixels.ERR_ARG, what
    with pytest.raises(pixels.PixelsError) as e:
        ex.pileup_into(band, nrows, ncols, -1, pa, pb, 3, pile, used)  # refused by pixels.py
    assert e.value.code == pixels.ERR_ARG
    err = C.create_string_buffer(64)
    assert pixels.lib().modle_pixels_pileup(None, band, nrows, ncols, f, 0, pa, pb, 3, pile, used, None, err, 64) == pixels.ERR_ARG
    p1, p2 = C.c_void_p(), C.c_void_p()
    one = (C.c_int64 * 1)(9)
    assert pixels.lib().modle_pixels_pileup_to_host(None, band, nrows, ncols, f, 0, one, one, 1, C.byref(p1), C.byref(p2),
                                                    None, err, 64) == pixels.ERR_ARG
    for args in [(None, nrows, ncols, f, [5], [9]), (band, nrows, ncols, 33, [5], [9]), (band, 4, ncols, f, [5], [9]),
                 (band, 0, ncols, 0, [5], [9]), (band, ncols + 1, ncols, f, [5], [9])]:
        with pytest.raises(pixels.PixelsError) as e:
            ex.pileup(*args)
        assert e.value.code == pixels.ERR_ARG, args
    with pytest.raises(pixels.PixelsError) as e:
        ex.pileup(band, nrows, ncols, f, [5, 6], [9])  # refused by pixels.py
    assert e.value.code == pixels.ERR_ARG
    with pytest.raises(pixels.PixelsError) as e:
        ex.coarse_pileup(band, nrows, ncols, 1, 0, f, [5], [9])  # factor 1
    assert e.value.code == pixels.ERR_ARG
    assert d_pile.unchanged() and d_used.unchanged() and src.unchanged()  # (still poison)
    assert np.array_equal(d_a.cpu().numpy(), [5, 6, 7]) and np.array_equal(d_b.cpu().numpy(), [9, 9, 9])
    # outputs next to each other and next to the anchors are accepted
    both = GuardedOut(26)
    ex.pileup_into(band, nrows, ncols, f, pa, pb, 3, both.data_ptr(), both.data_ptr() + 8 * 25)
    want, n_used = reference_pileup(src.host[FRONT:FRONT + src.n], nrows, ncols, f, [5, 6, 7], [9, 9, 9])
    got = both.sums(1)[0]
    assert n_used == 3 == int(got[25]) and np.array_equal(got[:25].reshape(5, 5), want) and both.guards_intact()


def test_a_stream_of_the_caller_and_scratch_that_grows():
    import torch

    from modle_amd import pixels

    stream = torch.cuda.Stream(device="cuda:0")
    assert stream.cuda_stream != 0
    small, large = (7, 30, 1), (70, 300, 32)
    s, l = Guarded(band_of(*small[:2], "full")), Guarded(band_of(*large[:2], "full"))
    with pixels.Extractor(0) as e:
        first = e.pileup(s.data_ptr(), *small, *anchor_lists(*small)["n = 257"], stream=stream)
        again = e.pileup(l.data_ptr(), *large, *anchor_lists(*large)["long"], stream=stream)  # grows
        a, b = anchor_lists(*large)["mix"]
        d_a, d_b = on_device(a), on_device(b)
        torch.cuda.synchronize()
        d_pile, d_used = GuardedOut(65 * 65), GuardedOut(1)
        e.pileup_into(l.data_ptr(), *large, d_a.data_ptr(), d_b.data_ptr(), len(a), d_pile.data_ptr(), d_used.data_ptr(),
                      stream=stream)
        shrunk = e.pileup(s.data_ptr(), *small, *anchor_lists(*small)["n = 257"], stream=stream)  # reused
        stream.synchronize()
        want, used = wanted(*large, "full", "mix")
        assert np.array_equal(d_pile.sums(1).reshape(65, 65), want) and int(d_used.sums(1)[0, 0]) == used
        for got, key in ((first, (*small, "full", "n = 257")), (again, (*large, "full", "long")),
                         (shrunk, (*small, "full", "n = 257"))):
            want, used = wanted(*key)
            assert got[1] == used and np.array_equal(got[0], want)
    assert s.unchanged() and l.unchanged()


def test_simulator_forms_agree():
    """the interval of tests/test_gpu_dots.py's test of the same name (80 x 200, from fine bin 5, 4 cells):
    pileup_tensors fed with dots_tensors' tensors equals pileup fed with dots' arrays, and both the
    restatement on the band copied to the host; pileup at three times the bin size; barriers on the diagonal"""
    import torch

    from modle_amd import api, driver, genome

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
        kw = dict(w=5, p=2, min_count=1, folds=(1.1, 1.1, 1.05, 1.05), min_diag=2)
        b1, b2, _, _ = sim.dots(iid, **kw)
        t1, t2, _ = sim.dots_tensors(iid, **kw)
        assert len(b1) > 10 and np.array_equal(t1.cpu().numpy(), b1)
        for f in (4, 10, 32):
            want, used = reference_pileup(band, nrows, ncols, f, b1, b2)
            assert used == len(b1) or f > 4  # w = 5 > 4: every dot's window of 9 x 9 lies in the band
            pile, n_used, hist = sim.pileup(iid, b1, b2, f)
            assert n_used == used and np.array_equal(pile, want)
            ok = reference_accepts(nrows, ncols, f, b1, b2)
            assert hist.dtype == np.uint64 and len(hist) == nrows and int(hist.sum()) == used
            assert np.array_equal(hist, np.bincount((b2 - b1)[ok], minlength=nrows))
            tp, tn = sim.pileup_tensors(iid, t1, t2, f)
            assert tp.dtype == tn.dtype == torch.int64 and tuple(tp.shape) == (2 * f + 1, 2 * f + 1) and tuple(tn.shape) == (1,)
            assert tp.device == tn.device == torch.device("cuda", 0)
            torch.cuda.synchronize()
            assert np.array_equal(tp.cpu().numpy().view(np.uint64), want) and int(tn.cpu()[0]) == used
        # a bin_offset, and the coarse form
        pile, n_used, _ = sim.pileup(iid, b1 + 100, b2 + 100, 4, bin_offset=100)
        want, used = reference_pileup(band, nrows, ncols, 4, b1, b2)
        assert n_used == used and np.array_equal(pile, want)
        coarse, nr, nc = reference_coarsen(band, nrows, ncols, 3, 5)
        where = np.arange(nc, dtype=np.int64)
        want, used = reference_pileup(coarse, nr, nc, 3, where, where)
        pile, n_used, hist = sim.pileup(iid, where, where, 3, factor=3, first_bin=5)
        assert n_used == used == nc - 6 and np.array_equal(pile, want) and np.array_equal(pile, pile.T)
        assert len(hist) == nr and hist[0] == used and not hist[1:].any()
        empty = torch.empty(0, dtype=torch.int64, device="cuda:0")
        tp, tn = sim.pileup_tensors(iid, empty, empty, 2)
        assert not tp.cpu().numpy().any() and int(tn.cpu()[0]) == 0
        assert np.array_equal(sim.copy_outputs(iid)[0], band)
    finally:
        sim.close()
