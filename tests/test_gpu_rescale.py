"""Rescaled pileups on the MI355X (include/modle_pixels.h: modle_pixels_rescale, _rescale_to_host,
_coarse_rescale_to_host; modle_amd/pixels.py; api.Simulator.rescaled_pileup and rescaled_pileup_tensors): the
pile, the area and the count of accepted windows equal, word for word, the restatement of
tests/test_rescale_outputs.py (rescale_blocks, which that module holds to the triple loop), for bands built on
the host with a seeded generator.  The band lies between poisoned guard words at an address that is 4-byte
aligned only and holds 0xFFFFFFFF in every word that is no pixel, so a window that left the band or the matrix
would show in the sum; the outputs are poisoned between guard words before the call (the library, not the
caller, defines every word).  The sums are integers: nothing here has a tolerance."""
import functools

import numpy as np
import pytest

from test_gpu_insulation import GuardedOut
from test_gpu_marginals import FRONT, Guarded, make_band, reference_coarsen
from test_pileup_outputs import I64_MAX, I64_MIN, reference_pileup
from test_rescale_outputs import reference_rescale_accepts, rescale_blocks

pytestmark = pytest.mark.gpu

# (nrows, ncols, R): one word; R = 1, the window's total; a thin band; widths 9 .. 40; the window that is the whole
# matrix, all triangle, on a grid one below and at its width; the cap R = 128 with widths 128 .. 130; second trips
# of the loops over a cell's rows and columns, cells up to 5 x 5 and 7 x 7
SHAPES = [(1, 1, 1), (3, 3, 1), (7, 30, 3), (40, 65, 9), (65, 65, 64), (65, 65, 65), (130, 300, 128), (257, 321, 60),
          (200, 700, 30)]
LONG = (40, 65, 9)  # the shape of the long list
FILLS = ["empty", "tenth", "full", "constant"]
POOL = 40  # distinct valid windows of a shape at most, outside the long list: the restatement forms each once


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
    """a window count that gives every workgroup of the capped grid a second and a third trip: workgroup g of G
    takes the windows g, g + G, ..., here 3 of them below g = G / 3 and 2 from there on"""
    from modle_amd import pixels

    g = pixels.rescale_groups()
    n = 2 * g + g // 3
    assert {len(range(k, n, g)) for k in range(g)} == {2, 3} or g < 3
    return n


@functools.lru_cache(maxsize=None)
def window_lists(nrows, ncols, r):
    """name -> (start, end), int64 arrays relative to the band"""
    rng = np.random.default_rng([11, nrows, ncols, r])

    def draw(m):
        w = rng.integers(r, nrows + 1, size=m)
        s = (rng.random(m) * (ncols - w + 1)).astype(np.int64)
        return s, s + w

    pool = draw(POOL)

    def valid(m):
        pick = rng.integers(0, POOL, size=m)
        return pool[0][pick], pool[1][pick]

    def rejected(m):
        kind = rng.integers(0, 5, size=m)
        s, e = valid(m)
        w = e - s
        s2 = np.where(kind == 0, -1 - rng.integers(0, 5, size=m), s)                       # s < 0
        e2 = np.where(kind == 0, s2 + w, e)
        e2 = np.where(kind == 1, ncols + 1 + rng.integers(0, 4, size=m), e2)               # e > ncols
        s2 = np.where(kind == 1, e2 - w, s2)
        e2 = np.where(kind == 2, s2 + r - 1 - rng.integers(0, 3, size=m), e2)              # W < R: also W <= 0
        e2 = np.where(kind == 3, s2 + nrows + 1 + rng.integers(0, 3, size=m), e2)          # W > nrows
        s2, e2 = np.where(kind == 4, e, s2), np.where(kind == 4, s, e2)                     # the ends swapped
        return s2, e2

    vs, ve = valid(320)
    rs, re = rejected(320)
    extremes = np.array([[I64_MIN, I64_MIN], [I64_MAX, I64_MAX], [I64_MIN, I64_MAX], [I64_MAX, I64_MIN], [0, I64_MAX],
                         [I64_MIN, r], [I64_MIN, 0], [r, I64_MIN], [I64_MAX - r, I64_MAX]], dtype=np.int64)
    ms, me = np.concatenate([vs, rs, extremes[:, 0]]), np.concatenate([ve, re, extremes[:, 1]])
    order = rng.permutation(len(ms))
    ms, me = ms[order], me[order]
    lists = {"mix": (ms, me), "mix shuffled": (ms[::-1].copy(), me[::-1].copy())}
    for n in (0, 1, 255, 256, 257):
        lists[f"n = {n}"] = (ms[:n], me[:n])
    lists["all rejected"] = rejected(300)
    lists["all the same"] = (np.full(300, vs[0]), np.full(300, ve[0]))
    at = rng.integers(0, ncols - r + 1, size=30)[rng.integers(0, 30, size=300)]
    lists["all of the grid's width"] = (at, at + r)
    ks = np.arange(1, nrows // r + 1, dtype=np.int64)
    lists["exact multiples"] = (np.concatenate([np.zeros(len(ks), dtype=np.int64), ncols - ks * r]),
                                np.concatenate([ks * r, np.full(len(ks), ncols, dtype=np.int64)]))
    lists["the extreme positions"] = (np.array([0, 0, ncols - r, ncols - nrows], dtype=np.int64),
                                      np.array([r, nrows, ncols, ncols], dtype=np.int64))
    if (nrows, ncols, r) == LONG:
        ls, le = draw(long_n())
        holes = rng.random(len(ls)) < 0.1
        lists["long"] = (np.where(holes, -1, ls), le)
    for s, e in lists.values():
        s.setflags(write=False), e.setflags(write=False)
    return lists


_BLOCKS = {}  # (nrows, ncols, r, fill) -> {(s, e): the window's blocks}


@functools.lru_cache(maxsize=None)
def wanted(nrows, ncols, r, fill, name):
    s, e = window_lists(nrows, ncols, r)[name]
    cache = _BLOCKS.setdefault((nrows, ncols, r, fill), {})
    pile, area, used = rescale_blocks(band_of(nrows, ncols, fill), nrows, ncols, r, s, e, cache)
    pile.setflags(write=False), area.setflags(write=False)
    return pile, area, used


def on_device(values):
    import torch

    return torch.from_numpy(np.array(values, dtype=np.int64)).to("cuda:0")  # (a copy: the lists are read-only)


def run(ex, src, nrows, ncols, r, s, e, bin_offset=0, with_area=True, with_n_used=True):
    """the device form into poisoned outputs: (pile, area or None, n_used or None)"""
    d_s, d_e = on_device(np.asarray(s) + bin_offset), on_device(np.asarray(e) + bin_offset)
    d_pile, d_area, d_used = GuardedOut(r * r), GuardedOut(r * r), GuardedOut(1)
    n = len(s)
    ex.rescale_into(src.data_ptr(), nrows, ncols, r, d_s.data_ptr() if n else None, d_e.data_ptr() if n else None, n,
                    d_pile.data_ptr(), d_area.data_ptr() if with_area else None,
                    d_used.data_ptr() if with_n_used else None, bin_offset)
    pile = d_pile.sums(1).reshape(r, r)
    assert d_pile.guards_intact() and d_area.guards_intact() and d_used.guards_intact()
    if not with_area:
        assert d_area.unchanged()
    if not with_n_used:
        assert d_used.unchanged()
    return (pile, d_area.sums(1).reshape(r, r) if with_area else None,
            int(d_used.sums(1)[0, 0]) if with_n_used else None)


@pytest.fixture(scope="module")
def ex():
    from modle_amd import pixels

    with pixels.Extractor(0) as e:
        yield e


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("nrows,ncols,r", SHAPES)
def test_piles_equal_the_definition(ex, nrows, ncols, r, fill):
    from modle_amd import api

    band = band_of(nrows, ncols, fill)
    src = Guarded(band)
    lists = window_lists(nrows, ncols, r)
    assert ("long" in lists) == ((nrows, ncols, r) == LONG)
    got = {}
    for name, (s, e) in lists.items():
        want, want_area, used = wanted(nrows, ncols, r, fill, name)
        ok = reference_rescale_accepts(nrows, ncols, r, s, e)
        assert used == int(ok.sum())
        if name == "all rejected" or name == "n = 0":
            assert used == 0 and not want.any() and not want_area.any()
        elif name in ("all the same", "all of the grid's width", "exact multiples", "the extreme positions"):
            assert used == len(s)
        elif name.startswith("mix") or name == "long":
            assert 0.35 * len(s) < used < len(s)
        if fill == "empty":
            assert not want.any()
        if fill == "constant":
            assert np.array_equal(want, 3 * want_area)
        if fill == "full" and used >= 100:
            assert int(want.max()) > 2**32, name  # carries into the high word
        if name == "all of the grid's width":
            assert (want_area == used).all()
            if r % 2 == 1:
                piled, n = reference_pileup(band, nrows, ncols, r // 2, s + r // 2, s + r // 2)
                assert n == used and np.array_equal(piled, want)
        if name == "exact multiples":
            assert np.array_equal(want_area, np.full((r, r), 2 * sum(k * k for k in range(1, nrows // r + 1))))
        pile, area, n_used = got[name] = run(ex, src, nrows, ncols, r, s, e)
        assert n_used == used, name
        assert np.array_equal(pile, want), name
        assert np.array_equal(area, want_area), name
        assert np.array_equal(pile, pile.T) and np.array_equal(area, area.T), name
        assert np.array_equal(area, api.rescaled_area(np.bincount((e - s)[ok], minlength=nrows + 1), r)), name
        assert used == 0 or (area > 0).all(), name
    assert all(np.array_equal(x, y) for x, y in zip(got["mix"][:2], got["mix shuffled"][:2]))
    assert got["mix"][2] == got["mix shuffled"][2]
    assert src.unchanged()


@pytest.mark.parametrize("nrows,ncols,r", [SHAPES[1], SHAPES[3], SHAPES[6]])
def test_without_area_and_n_used_and_with_a_bin_offset(ex, nrows, ncols, r):
    band = band_of(nrows, ncols, "tenth")
    src = Guarded(band)
    s, e = window_lists(nrows, ncols, r)["mix"]
    want, want_area, used = wanted(nrows, ncols, r, "tenth", "mix")
    for with_area, with_n_used in ((False, False), (True, False), (False, True)):
        pile, area, n_used = run(ex, src, nrows, ncols, r, s, e, with_area=with_area, with_n_used=with_n_used)
        assert np.array_equal(pile, want)
        assert (area is None) != with_area and (n_used is None) != with_n_used
        assert area is None or np.array_equal(area, want_area)
        assert n_used is None or n_used == used
    keep = (np.abs(s.astype(np.float64)) < 2**62) & (np.abs(e.astype(np.float64)) < 2**62)  # the shift stays an int64
    cache = _BLOCKS[(nrows, ncols, r, "tenth")]
    want, want_area, used = rescale_blocks(band, nrows, ncols, r, s[keep], e[keep], cache)
    for off in (11, -9, 2**61, -2**61):
        pile, area, n_used = run(ex, src, nrows, ncols, r, s[keep], e[keep], bin_offset=off)
        assert n_used == used and np.array_equal(pile, want) and np.array_equal(area, want_area), off
    # unshifted windows against an offset: the extremes must not wrap into the band
    for off in (I64_MIN, I64_MAX, -1, 1):
        d_s, d_e = on_device(s), on_device(e)
        d_pile, d_area, d_used = GuardedOut(r * r), GuardedOut(r * r), GuardedOut(1)
        ex.rescale_into(src.data_ptr(), nrows, ncols, r, d_s.data_ptr(), d_e.data_ptr(), len(s), d_pile.data_ptr(),
                        d_area.data_ptr(), d_used.data_ptr(), off)
        ok = reference_rescale_accepts(nrows, ncols, r, s, e, off)
        shifted = [(int(x) - off, int(y) - off) for x, y in zip(s[ok], e[ok])]
        want, want_area, used = rescale_blocks(band, nrows, ncols, r, [p[0] for p in shifted], [p[1] for p in shifted])
        assert used == int(ok.sum()) == int(d_used.sums(1)[0, 0])
        assert np.array_equal(d_pile.sums(1).reshape(r, r), want) and np.array_equal(d_area.sums(1).reshape(r, r), want_area), off
    assert src.unchanged()


@pytest.mark.parametrize("nrows,ncols,r", [SHAPES[0], SHAPES[3], SHAPES[5], SHAPES[7]])
def test_the_host_form_twice_in_a_row(ex, nrows, ncols, r):
    from modle_amd import pixels

    src = Guarded(band_of(nrows, ncols, "full"))
    names = ["mix", "n = 0", "n = 1"] + (["long"] if (nrows, ncols, r) == LONG else [])
    for name in names:
        s, e = window_lists(nrows, ncols, r)[name]
        want, want_area, used = wanted(nrows, ncols, r, "full", name)
        for form in (ex.rescale, ex.rescale, pixels.rescale):
            pile, area, n_used = form(src.data_ptr(), nrows, ncols, r, s + 3, e + 3, bin_offset=3)
            assert pile.dtype == area.dtype == np.uint64 and pile.shape == area.shape == (r, r) and type(n_used) is int
            assert n_used == used and np.array_equal(pile, want) and np.array_equal(area, want_area), name
    assert src.unchanged()


@pytest.mark.parametrize("nrows,ncols,k,first_bin,r", [(65, 130, 2, 3, 9), (200, 700, 3, 7, 30)])
def test_coarse_piles_are_those_of_the_coarse_band(ex, nrows, ncols, k, first_bin, r):
    from modle_amd import pixels

    assert first_bin % k != 0
    band = make_band(nrows, ncols, "tenth", limit=2**20, seed=3)
    coarse, nr, nc = reference_coarsen(band, nrows, ncols, k, first_bin)
    assert pixels.coarse_shape(nrows, ncols, k, first_bin) == (nr, nc) and r < nr
    src = Guarded(band)
    for name in ("mix", "exact multiples", "n = 257"):
        s, e = window_lists(nr, nc, r)[name]
        want, want_area, used = rescale_blocks(coarse, nr, nc, r, s, e)
        assert used > 0 and want.any()
        for got in (ex.coarse_rescale(src.data_ptr(), nrows, ncols, k, first_bin, r, s, e),
                    pixels.coarse_rescale(src.data_ptr(), nrows, ncols, k, first_bin, r, s + 4, e + 4, bin_offset=4)):
            assert got[2] == used and np.array_equal(got[0], want) and np.array_equal(got[1], want_area), name
    # the fine path still serves, and the rule holds against the coarse shape: a window of the fine band's depth is
    # not used
    s, e = window_lists(nrows, ncols, r)["mix"]
    want, want_area, used = rescale_blocks(band, nrows, ncols, r, s, e)
    got = ex.rescale(src.data_ptr(), nrows, ncols, r, s, e)
    assert got[2] == used and np.array_equal(got[0], want) and np.array_equal(got[1], want_area)
    assert nr < nrows <= nc
    got = ex.coarse_rescale(src.data_ptr(), nrows, ncols, k, first_bin, r, [0, 0], [nrows, nr])
    assert got[2] == 1 and np.array_equal(got[0], rescale_blocks(coarse, nr, nc, r, [0], [nr])[0])
    assert src.unchanged()


def test_invalid_calls_are_argument_errors_and_write_nothing(ex):
    import ctypes as C

    from modle_amd import pixels

    nrows, ncols, r = 70, 80, 5
    src = Guarded(make_band(nrows, ncols, "full", seed=8))
    d_s, d_e = on_device([5, 6, 7]), on_device([19, 29, 39])
    d_pile, d_area, d_used = GuardedOut(25), GuardedOut(25), GuardedOut(1)
    band, ps, pe = src.data_ptr(), d_s.data_ptr(), d_e.data_ptr()
    pile, area, used = d_pile.data_ptr(), d_area.data_ptr(), d_used.data_ptr()
    inside = band + 4 * (nrows * ncols)  # the band's trailing word
    inside -= inside % 8
    for what, args in [("no band", (None, nrows, ncols, r, ps, pe, 3, pile, area, used)),
                       ("no starts", (band, nrows, ncols, r, None, pe, 3, pile, area, used)),
                       ("no ends", (band, nrows, ncols, r, ps, None, 3, pile, area, used)),
                       ("no pile", (band, nrows, ncols, r, ps, pe, 3, None, area, used)),
                       ("size == 0", (band, nrows, ncols, 0, ps, pe, 3, pile, area, used)),
                       ("size > 128", (band, nrows, ncols, 129, ps, pe, 3, pile, area, used)),
                       ("nrows == 0", (band, 0, ncols, r, ps, pe, 3, pile, area, used)),
                       ("nrows > ncols", (band, ncols + 1, ncols, r, ps, pe, 3, pile, area, used)),
                       ("n == 2^31", (band, nrows, ncols, r, ps, pe, 2**31, pile, area, used)),
                       ("n * ceil(70 / 5)^2 == 2^32 and more", (band, nrows, ncols, r, ps, pe, 2**32 // 196 + 1, pile, area, used)),
                       ("a misaligned pile", (band, nrows, ncols, r, ps, pe, 3, pile + 4, area, used)),
                       ("a misaligned area", (band, nrows, ncols, r, ps, pe, 3, pile, area + 4, used)),
                       ("a misaligned n_used", (band, nrows, ncols, r, ps, pe, 3, pile, area, used + 4)),
                       ("the pile overlaps the band", (band, nrows, ncols, r, ps, pe, 3, inside, area, used)),
                       ("the pile ends inside the band", (band, nrows, ncols, r, ps, pe, 3, band - band % 8 - 8 * 24, area, used)),
                       ("the area overlaps the band", (band, nrows, ncols, r, ps, pe, 3, pile, inside, used)),
                       ("n_used overlaps the band", (band, nrows, ncols, r, ps, pe, 3, pile, area, inside)),
                       ("the pile overlaps the starts", (band, nrows, ncols, r, ps, pe, 3, ps + 16, area, used)),
                       ("the area overlaps the ends", (band, nrows, ncols, r, ps, pe, 3, pile, pe - 8 * 24, used)),
                       ("n_used overlaps the ends", (band, nrows, ncols, r, ps, pe, 3, pile, area, pe + 8)),
                       ("the area overlaps the pile", (band, nrows, ncols, r, ps, pe, 3, pile, pile + 8 * 24, used)),
                       ("n_used inside the area", (band, nrows, ncols, r, ps, pe, 3, pile, area, area + 8 * 24))]:
        with pytest.raises(pixels.PixelsError) as e:
            ex.rescale_into(*args)
        assert e.value.code == pixels.ERR_ARG, what
    with pytest.raises(pixels.PixelsError) as e:
        ex.rescale_into(band, nrows, ncols, -1, ps, pe, 3, pile, area, used)  # refused by pixels.py
    assert e.value.code == pixels.ERR_ARG
    err = C.create_string_buffer(64)
    assert pixels.lib().modle_pixels_rescale(None, band, nrows, ncols, r, 0, ps, pe, 3, pile, area, used, None, err, 64) == pixels.ERR_ARG
    p1, p2, p3 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    one = (C.c_int64 * 1)(9)
    assert pixels.lib().modle_pixels_rescale_to_host(None, band, nrows, ncols, r, 0, one, one, 1, C.byref(p1), C.byref(p2),
                                                     C.byref(p3), None, err, 64) == pixels.ERR_ARG
    for args in [(None, nrows, ncols, r, [5], [19]), (band, nrows, ncols, 129, [5], [19]), (band, nrows, ncols, 0, [5], [19]),
                 (band, 0, ncols, r, [5], [19]), (band, ncols + 1, ncols, r, [5], [19])]:
        with pytest.raises(pixels.PixelsError) as e:
            ex.rescale(*args)
        assert e.value.code == pixels.ERR_ARG, args
    with pytest.raises(pixels.PixelsError) as e:
        ex.rescale(band, nrows, ncols, r, [5, 6], [19])  # refused by pixels.py
    assert e.value.code == pixels.ERR_ARG
    with pytest.raises(pixels.PixelsError) as e:
        ex.coarse_rescale(band, nrows, ncols, 1, 0, r, [5], [19])  # factor 1
    assert e.value.code == pixels.ERR_ARG
    assert d_pile.unchanged() and d_area.unchanged() and d_used.unchanged() and src.unchanged()  # (still poison)
    assert np.array_equal(d_s.cpu().numpy(), [5, 6, 7]) and np.array_equal(d_e.cpu().numpy(), [19, 29, 39])
    # outputs next to each other are accepted
    all3 = GuardedOut(51)
    ex.rescale_into(band, nrows, ncols, r, ps, pe, 3, all3.data_ptr(), all3.data_ptr() + 8 * 25, all3.data_ptr() + 8 * 50)
    want, want_area, n_used = rescale_blocks(src.host[FRONT:FRONT + src.n], nrows, ncols, r, [5, 6, 7], [19, 29, 39])
    got = all3.sums(1)[0]
    assert n_used == 3 == int(got[50]) and np.array_equal(got[:25].reshape(5, 5), want) and all3.guards_intact()
    assert np.array_equal(got[25:50].reshape(5, 5), want_area)


def test_a_stream_of_the_caller_and_scratch_that_grows():
    import torch

    from modle_amd import pixels

    stream = torch.cuda.Stream(device="cuda:0")
    assert stream.cuda_stream != 0
    small, large = (7, 30, 3), (130, 300, 128)
    s, l = Guarded(band_of(*small[:2], "full")), Guarded(band_of(*large[:2], "full"))
    with pixels.Extractor(0) as e:
        first = e.rescale(s.data_ptr(), *small, *window_lists(*small)["n = 1"], stream=stream)
        again = e.rescale(l.data_ptr(), *large, *window_lists(*large)["mix"], stream=stream)  # grows
        ws, we = window_lists(*large)["n = 257"]
        d_s, d_e = on_device(ws), on_device(we)
        torch.cuda.synchronize()
        d_pile, d_area, d_used = GuardedOut(128 * 128), GuardedOut(128 * 128), GuardedOut(1)
        e.rescale_into(l.data_ptr(), *large, d_s.data_ptr(), d_e.data_ptr(), len(ws), d_pile.data_ptr(), d_area.data_ptr(),
                       d_used.data_ptr(), stream=stream)
        shrunk = e.rescale(s.data_ptr(), *small, *window_lists(*small)["n = 257"], stream=stream)  # reused
        stream.synchronize()
        want, want_area, used = wanted(*large, "full", "n = 257")
        assert np.array_equal(d_pile.sums(1).reshape(128, 128), want) and int(d_used.sums(1)[0, 0]) == used
        assert np.array_equal(d_area.sums(1).reshape(128, 128), want_area)
        for got, key in ((first, (*small, "full", "n = 1")), (again, (*large, "full", "mix")),
                         (shrunk, (*small, "full", "n = 257"))):
            want, want_area, used = wanted(*key)
            assert got[2] == used and np.array_equal(got[0], want) and np.array_equal(got[1], want_area)
    assert s.unchanged() and l.unchanged()


def test_simulator_forms_agree():
    """the interval of tests/test_gpu_pileup.py's test of the same name (80 x 200, from fine bin 5, 4 cells):
    rescaled_pileup_tensors fed from device tensors equals rescaled_pileup fed with arrays, and both the
    restatement on the band copied to the host; the form at three times the bin size; a loaded band"""
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
        assert band.any()
        for r in (1, 13, 60, 80):
            s, e = window_lists(nrows, ncols, r)["mix"]
            want, want_area, used = rescale_blocks(band, nrows, ncols, r, s, e)
            ok = reference_rescale_accepts(nrows, ncols, r, s, e)
            pile, area, n_used, hist = sim.rescaled_pileup(iid, s, e, r)
            assert n_used == used > 100 and np.array_equal(pile, want) and np.array_equal(area, want_area)
            assert hist.dtype == np.uint64 and len(hist) == nrows + 1 and int(hist.sum()) == used
            assert np.array_equal(hist, np.bincount((e - s)[ok], minlength=nrows + 1))
            tp, ta, tn = sim.rescaled_pileup_tensors(iid, on_device(s), on_device(e), r)
            assert tp.dtype == ta.dtype == tn.dtype == torch.int64 and tuple(tp.shape) == tuple(ta.shape) == (r, r)
            assert tuple(tn.shape) == (1,) and tp.device == ta.device == tn.device == torch.device("cuda", 0)
            torch.cuda.synchronize()
            assert np.array_equal(tp.cpu().numpy().view(np.uint64), want) and int(tn.cpu()[0]) == used
            assert np.array_equal(ta.cpu().numpy().view(np.uint64), want_area)
        # a bin_offset, and the coarse form
        s, e = window_lists(nrows, ncols, 13)["mix"]
        keep = (np.abs(s.astype(np.float64)) < 2**62) & (np.abs(e.astype(np.float64)) < 2**62)
        pile, area, n_used, _ = sim.rescaled_pileup(iid, s[keep] + 100, e[keep] + 100, 13, bin_offset=100)
        want, want_area, used = rescale_blocks(band, nrows, ncols, 13, s[keep], e[keep])
        assert n_used == used and np.array_equal(pile, want) and np.array_equal(area, want_area)
        coarse, nr, nc = reference_coarsen(band, nrows, ncols, 3, 5)
        s, e = window_lists(nr, nc, 7)["mix"]
        want, want_area, used = rescale_blocks(coarse, nr, nc, 7, s, e)
        pile, area, n_used, hist = sim.rescaled_pileup(iid, s, e, 7, factor=3, first_bin=5)
        assert n_used == used > 100 and np.array_equal(pile, want) and np.array_equal(area, want_area)
        assert len(hist) == nr + 1 and int(hist.sum()) == used
        empty = torch.empty(0, dtype=torch.int64, device="cuda:0")
        tp, ta, tn = sim.rescaled_pileup_tensors(iid, empty, empty, 2)
        assert not tp.cpu().numpy().any() and not ta.cpu().numpy().any() and int(tn.cpu()[0]) == 0
        with pytest.raises(ValueError):
            sim.rescaled_pileup_tensors(iid, empty, empty.cpu(), 2)
        assert np.array_equal(sim.copy_outputs(iid)[0], band)
        # the same band, loaded: LoadedBands has the same analyses
        with api.LoadedBands(0) as loaded:
            words = np.zeros(nrows * ncols + 1, dtype=np.uint32)
            words[:nrows * ncols] = band[:nrows * ncols]
            bid = loaded.add_band(torch.from_numpy(words.view(np.int32)).to("cuda:0"), nrows, ncols)
            s, e = window_lists(nrows, ncols, 13)["mix"]
            pile, area, n_used, _ = loaded.rescaled_pileup(bid, s, e, 13)
            want, want_area, used = rescale_blocks(band, nrows, ncols, 13, s, e)
            assert n_used == used and np.array_equal(pile, want) and np.array_equal(area, want_area)
    finally:
        sim.close()
