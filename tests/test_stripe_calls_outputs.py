"""Stripe profiles and stripe calling, without a GPU: the numpy restatement of the sums of include/modle_pixels.h
(modle_pixels_stripe_profiles) that the GPU tests compare against, written from the two formulas of the
definition and cross-checked against a triple loop over a dense symmetric matrix; pixels.stripe_profile_n_valid
against counting; the two identities that tie the profiles to the sums per diagonal (driver.check_stripe_profiles);
pixels.stripe_calls on planted stripes; api.directionality_index and api.stripe_profile_expected; the argument
refusals of the C entry points and of pixels.stripe_profile_misfit, which need no device; and what
cli.stripe_calls_options plans and refuses of --call-stripes.

Everything here is an integer and is compared exactly, except the directionality index and the expected centre,
which are float64 statements of a few operations and are compared with what the same operations give."""
import ctypes as C
import math
import os
from fractions import Fraction

import numpy as np
import pytest

from modle_amd import api, cli, driver, pixels

M64 = (1 << 64) - 1
POISON = 0xFFFFFFFF


# ---- the restatement ---------------------------------------------------------------------------------------

def restate(band, nrows, ncols, m, lengths, d0):
    """uint64 [2, K, 2 m + 1, ncols]: what modle_pixels_stripe_profiles writes for `band`.  Term by term from
        V[k][o][c] = sum over d0 <= d < L_k of M(c - d, c + o) = band[(c + o) * nrows + (d + o)]
        H[k][o][c] = sum over d0 <= d < L_k of M(c + o, c + d) = band[(c + d) * nrows + (d - o)]
    one distance d at a time for all anchors c whose cell lies inside the chromosome; a sum has fewer than nrows
    terms below 2^32, so uint64 is exact"""
    assert pixels.stripe_profile_misfit(nrows, ncols, m, lengths, d0) is None
    b = np.asarray(band[:nrows * ncols]).reshape(ncols, nrows).astype(np.uint64)
    out = np.zeros((2, len(lengths), 2 * m + 1, ncols), dtype=np.uint64)
    c = np.arange(ncols, dtype=np.int64)
    for o in range(-m, m + 1):
        side = (c + o >= 0) & (c + o < ncols)
        v, h = np.zeros(ncols, dtype=np.uint64), np.zeros(ncols, dtype=np.uint64)
        for d in range(d0, lengths[-1]):
            at = c[side & (c - d >= 0)]
            v[at] += b[at + o, d + o]
            at = c[side & (c + d < ncols)]
            h[at] += b[at + d, d - o]
            for k, length in enumerate(lengths):
                if d == length - 1:
                    out[0, k, o + m], out[1, k, o + m] = v, h
    return out


def make_band(nrows, ncols, fill, seed=0):
    """a band whose words that are no pixels (the left-edge triangle, the trailing word) hold 0xFFFFFFFF.
    `sparse`: a tenth of the pixels, counts below 2^32; `max`: every pixel 2^32 - 1; `corners`: one pixel at
    each corner of the band, each a power of 256 of its own; `ones`: every pixel 1"""
    rng = np.random.default_rng([seed, nrows, ncols])
    n = nrows * ncols
    band = np.zeros(n + 1, dtype=np.uint32)
    if fill == "sparse":
        mask = rng.random(n) < 0.1
        band[:-1][mask] = rng.integers(1, 2**32, size=int(mask.sum()), dtype=np.int64)
    elif fill == "max":
        band[:-1] = 0xFFFFFFFF
    elif fill == "ones":
        band[:-1] = 1
    elif fill == "corners":
        for value, (j, d) in zip((1, 1 << 8, 1 << 16, 1 << 24),
                                 ((0, 0), (nrows - 1, nrows - 1), (ncols - 1, 0), (ncols - 1, nrows - 1))):
            band[j * nrows + d] += value
    else:
        raise ValueError(fill)
    for j in range(min(nrows, ncols)):
        band[j * nrows + j + 1:(j + 1) * nrows] = POISON
    band[n] = POISON
    return band


def dense(band, nrows, ncols):
    m = [[0] * ncols for _ in range(ncols)]
    for j in range(ncols):
        for d in range(min(nrows, j + 1)):
            m[j - d][j] = m[j][j - d] = int(band[j * nrows + d])
    return m


def cell(m, x, y):
    return m[x][y] if 0 <= x < len(m) and 0 <= y < len(m) else 0


@pytest.mark.parametrize("m,lengths,d0", [(0, [1], 0), (0, [9], 0), (2, [3, 5, 7], 2), (3, [4, 6], 3), (1, [2, 3, 5, 8], 1),
                                          (4, [5], 4)])
@pytest.mark.parametrize("fill", ["sparse", "max", "corners", "ones"])
def test_the_restatement_is_the_definition_written_as_loops(m, lengths, d0, fill):
    nrows, ncols = 9, 12
    band = make_band(nrows, ncols, fill)
    mat = dense(band, nrows, ncols)
    got = restate(band, nrows, ncols, m, lengths, d0)
    assert got.shape == (2, len(lengths), 2 * m + 1, ncols) and got.dtype == np.uint64
    for k, length in enumerate(lengths):
        for o in range(-m, m + 1):
            for c in range(ncols):
                assert int(got[0, k, o + m, c]) == sum(cell(mat, c - d, c + o) for d in range(d0, length)), (k, o, c)
                assert int(got[1, k, o + m, c]) == sum(cell(mat, c + o, c + d) for d in range(d0, length)), (k, o, c)
    if fill == "ones":
        assert np.array_equal(got, pixels.stripe_profile_n_valid(ncols, m, lengths, d0))


@pytest.mark.parametrize("ncols,m,lengths,d0", [(1, 0, [1], 0), (12, 2, [3, 5, 7], 2), (7, 3, [4, 9], 3), (30, 8, [9, 20], 8)])
def test_the_valid_cells_are_those_counted(ncols, m, lengths, d0):
    got = pixels.stripe_profile_n_valid(ncols, m, lengths, d0)
    assert got.shape == (2, len(lengths), 2 * m + 1, ncols) and got.dtype == np.uint64
    for k, length in enumerate(lengths):
        for o in range(-m, m + 1):
            for c in range(ncols):
                inside = 0 <= c + o < ncols
                assert got[0, k, o + m, c] == sum(1 for d in range(d0, length) if inside and c - d >= 0)
                assert got[1, k, o + m, c] == sum(1 for d in range(d0, length) if inside and c + d < ncols)
    for bad in ((-1, 0, [1], 0), (5, -1, [1], 0), (5, 0, [], 0), (5, 0, [1], -1)):
        with pytest.raises(pixels.PixelsError):
            pixels.stripe_profile_n_valid(*bad)


def diag_sums(band, nrows, ncols):
    b = np.asarray(band[:nrows * ncols], dtype=np.uint64).reshape(ncols, nrows)
    return np.array([int(b[d:, d].sum()) for d in range(nrows)], dtype=np.uint64)


@pytest.mark.parametrize("nrows,ncols,m,lengths,d0", [(9, 12, 2, [3, 5, 7], 2), (17, 17, 8, [9], 8), (20, 65, 3, [5, 9, 17], 3),
                                                      (40, 41, 0, [1, 40], 0)])
def test_the_profiles_add_up_to_the_sums_per_diagonal(nrows, ncols, m, lengths, d0):
    """for o >= 0 the sum over c of V, for o <= 0 that of H, is the sum of the diagonals d0 + |o| .. L_k + |o| - 1"""
    band = make_band(nrows, ncols, "sparse", seed=3)
    prof, diag = restate(band, nrows, ncols, m, lengths, d0), diag_sums(band, nrows, ncols)
    driver.check_stripe_profiles("chrA:0-60000", prof, m, lengths, d0, diag)
    for k, length in enumerate(lengths):
        for o in range(m + 1):
            want = sum(int(diag[d + o]) for d in range(d0, length))
            assert sum(int(x) for x in prof[0, k, m + o]) == want == sum(int(x) for x in prof[1, k, m - o])
    # the other signs lose the pixels whose anchor would lie outside the chromosome
    if m > 0:
        ones = restate(make_band(nrows, ncols, "ones"), nrows, ncols, m, lengths, d0)
        for direction, o in ((0, -m), (1, m)):
            got = sum(int(x) for x in ones[direction, 0, o + m])
            # (diagonal d - m has ncols - (d - m) pixels; those of m columns, or rows, have no anchor)
            assert got == sum(ncols - d for d in range(d0, lengths[0])) < sum(ncols - (d - m) for d in range(d0, lengths[0]))
    for direction, o in ((0, m), (1, 0)):
        bad = prof.copy()
        bad[direction, -1, o, ncols // 2] += np.uint64(1)
        with pytest.raises(RuntimeError) as e:
            driver.check_stripe_profiles("chrA:0-60000", bad, m, lengths, d0, diag)
        assert str(e.value).startswith("chrA:0-60000: the " + ("upstream", "downstream")[direction] + " profiles")


# ---- the decision ------------------------------------------------------------------------------------------

def planted(nrows, ncols, background, stripes):
    """a band of constant `background` with stripes (direction, anchor, length, value): the cells at the distances
    1 .. length - 1 upstream (0) or downstream (1) of the anchor hold `value`"""
    band = np.zeros(nrows * ncols + 1, dtype=np.uint32)
    band[:-1] = background
    for direction, c, length, value in stripes:
        for d in range(1, length):
            if direction == 0 and d <= c:
                band[c * nrows + d] = value  # M(c - d, c)
            elif direction == 1 and c + d < ncols:
                band[(c + d) * nrows + d] = value  # M(c, c + d)
    return band


def calls_of(band, nrows, ncols, m, lengths, d0, **options):
    prof = restate(band, nrows, ncols, m, lengths, d0)
    return pixels.stripe_calls(prof, pixels.stripe_profile_n_valid(ncols, m, lengths, d0), m, lengths, d0, **options)


def test_planted_stripes_are_called_where_they_are_and_as_long_as_they_are():
    nrows, ncols, m, lengths, d0 = 40, 120, 3, [8, 16, 32], 3
    band = planted(nrows, ncols, 10, [(0, 70, 16, 40), (1, 30, 32, 40)])
    got = calls_of(band, nrows, ncols, m, lengths, d0, fold=3)
    assert [(s.direction, s.bin, s.k) for s in got] == [(0, 70, 1), (1, 30, 2)]
    up, down = got
    assert (up.centre, up.n_centre, up.left, up.n_left, up.right, up.n_right) == (40 * 13, 13, 3 * 130, 39, 3 * 130, 39)
    assert (down.centre, down.n_centre, down.left, down.n_left) == (40 * 29, 29, 3 * 290, 87)
    # at the longest class the vertical stripe is diluted below the fold: (13 * 40 + 16 * 10) / 29 < 3 * 10
    assert Fraction(13 * 40 + 16 * 10, 29) < 30
    # a centre of three bins holds the stripe and two columns of background: a mean of 20, and so do the centres
    # of the two bins beside it, unless the stripe ends inside them; the thinning keeps the best, ties the smaller
    assert calls_of(band, nrows, ncols, m, lengths, d0, half_width=1, fold=3) == []
    wide = calls_of(band, nrows, ncols, m, lengths, d0, half_width=1, fold="3/2")
    assert [(s.direction, s.bin, s.k) for s in wide] == [(0, 69, 1), (0, 70, 1), (0, 71, 1), (1, 29, 2), (1, 30, 2), (1, 31, 2)]
    assert [Fraction(s.centre, s.n_centre) for s in wide] == [Fraction(750, 39), 20, 20, 20, 20, Fraction(1710, 87)]
    wide = calls_of(band, nrows, ncols, m, lengths, d0, half_width=1, fold=Fraction(3, 2), radius=1)
    assert [(s.direction, s.bin) for s in wide] == [(0, 70), (1, 29)]
    # a flat band calls nothing above a fold of 1, everything that is valid at it
    flat = planted(nrows, ncols, 10, [])
    assert calls_of(flat, nrows, ncols, m, lengths, d0, fold=1.01) == []
    every = calls_of(flat, nrows, ncols, m, lengths, d0, fold=1)
    assert [s.bin for s in every if s.direction == 0] == list(range(7, ncols - m))  # L_1 - 1 cells upstream, m beside
    assert all(s.k == (2 if s.bin >= 31 else 1 if s.bin >= 15 else 0) for s in every if s.direction == 0)
    assert calls_of(flat, nrows, ncols, m, lengths, d0, fold=1, min_count=10 * 29 + 1) == []


def test_an_anchor_near_an_end_is_never_called():
    nrows, ncols, m, lengths, d0 = 20, 60, 3, [6], 3
    stripes = [(1, c, 6, 90) for c in (0, 2, 3, 55, 57)] + [(0, c, 6, 90) for c in (4, 30, 56, 57, 59)]
    got = calls_of(planted(nrows, ncols, 1, stripes), nrows, ncols, m, lengths, d0, fold=2)
    # downstream: 0 and 2 are nearer than m to the start, 55 and 57 run off the chromosome at this length;
    # upstream: 4 lacks cells at this length, 57 and 59 are nearer than m to the end
    assert [(s.direction, s.bin) for s in got] == [(0, 30), (0, 56), (1, 3)]


def test_calls_are_thinned_to_the_best_within_the_radius_and_ties_go_to_the_smaller_bin():
    nrows, ncols, m, lengths, d0 = 20, 80, 2, [6], 2
    stripes = [(0, 20, 6, 50), (0, 24, 6, 50), (0, 40, 6, 50), (0, 43, 6, 60), (0, 46, 6, 50), (0, 60, 6, 50)]
    band = planted(nrows, ncols, 1, stripes)
    assert [s.bin for s in calls_of(band, nrows, ncols, m, lengths, d0, fold=2)] == [20, 24, 40, 43, 46, 60]
    assert [s.bin for s in calls_of(band, nrows, ncols, m, lengths, d0, fold=2, radius=3)] == [20, 24, 43, 60]
    assert [s.bin for s in calls_of(band, nrows, ncols, m, lengths, d0, fold=2, radius=4)] == [20, 43, 60]
    # a local-maximum filter: 24 and 40 tie with 20 and lose to the smaller bin, 60 loses to 40 although 40 is gone
    assert [s.bin for s in calls_of(band, nrows, ncols, m, lengths, d0, fold=2, radius=20)] == [20, 43]


def test_what_the_decision_refuses():
    prof = np.zeros((2, 1, 5, 9), dtype=np.uint64)
    nv = pixels.stripe_profile_n_valid(9, 2, [4], 2)
    assert pixels.stripe_calls(prof, nv, 2, [4], 2) == []  # no contact: below min_count
    for kwargs in ({"half_width": 2}, {"half_width": -1}, {"fold": -1}, {"radius": -1}):
        with pytest.raises(ValueError):
            pixels.stripe_calls(prof, nv, 2, [4], 2, **kwargs)
    for bad in (prof[0], prof.astype(np.int64), prof[:, :, :3]):
        with pytest.raises(ValueError):
            pixels.stripe_calls(bad, nv, 2, [4], 2)
    with pytest.raises(ValueError):
        pixels.stripe_calls(prof, nv[:, :, :, :8], 2, [4], 2)
    assert (pixels.STRIPE_FOLD, pixels.STRIPE_MIN_COUNT, pixels.STRIPE_RADIUS) == (1.5, 1, 0)


# ---- the directionality index and the expected centre -----------------------------------------------------

def test_the_directionality_index_changes_sign_across_a_boundary():
    nrows, ncols, m, lengths, d0 = 12, 40, 0, [10], 1
    band = np.zeros(nrows * ncols + 1, dtype=np.uint32)
    for j in range(ncols):  # two domains, [0, 20) and [20, 40): contacts inside a domain only
        for d in range(min(nrows, j + 1)):
            band[j * nrows + d] = 5 if (j < 20) == (j - d < 20) else 0
    prof = restate(band, nrows, ncols, m, lengths, d0)
    nv = pixels.stripe_profile_n_valid(ncols, m, lengths, d0)
    di = api.directionality_index(prof, nv, 0)
    assert di.dtype == np.float64 and di.shape == (ncols,)
    assert di[19] < 0 < di[20]  # the last bin of a domain looks upstream, the first one downstream
    assert (di[10:19] <= 0).all() and (di[21:30] >= 0).all() and di[10] == 0
    a, b = int(prof[0, 0, 0, 19]), int(prof[1, 0, 0, 19])
    e = (a + b) / 2
    assert di[19] == math.copysign(((a - e) ** 2 + (b - e) ** 2) / e, b - a)
    empty = api.directionality_index(np.zeros_like(prof), nv, 0)
    assert np.isnan(empty).all()
    with pytest.raises(ValueError):
        api.directionality_index(prof, nv, 1)


def test_the_expected_centre_follows_the_distance_decay():
    ncols, m, lengths, d0 = 50, 2, [4, 7], 2
    diag = np.array([500, 300, 200, 100, 50, 30, 20, 10, 5, 1], dtype=np.uint64)
    got = api.stripe_profile_expected(diag, ncols, lengths, d0)
    e = [float(diag[d]) / float(ncols - d) for d in range(len(diag))]
    assert got == [math.fsum(e[2:4]), math.fsum(e[2:7])]
    assert api.stripe_profile_expected(diag, ncols, lengths, d0, half_width=1) == \
        [math.fsum(e[d + o] for d in range(d0, length) for o in (-1, 0, 1)) for length in lengths]
    with pytest.raises(ValueError):
        api.stripe_profile_expected(diag, ncols, [10], 2, half_width=1)  # diagonal 10 is not held


# ---- what is refused without a device ---------------------------------------------------------------------

def test_what_the_entry_points_refuse_without_a_device():
    """every refusal comes before the handle or the band is touched: the handle here is host memory that names a
    device no machine has, and the band and the output are addresses nobody owns"""
    lb = pixels.lib()
    handle = (C.c_uint64 * 512)()
    C.cast(handle, C.POINTER(C.c_int))[0] = 1 << 20  # modle_pixels_handle.device
    h = C.addressof(handle)
    band, out = 0x10000000, 0x30000000
    nrows, ncols = 50, 90
    band_bytes = (nrows * ncols + 1) * 4

    def arr(*ls):
        return (C.c_uint64 * len(ls))(*ls)

    def words(m, k, nc=ncols):
        return 2 * k * (2 * m + 1) * nc

    err = C.create_string_buffer(512)
    # handle, band, nrows, ncols, m, lengths, K, d0, out, out_words
    accepted = {
        "d0 == m": (h, band, nrows, ncols, 8, arr(9, 42), 2, 8, out, words(8, 2)),
        "L_K + m == nrows": (h, band, nrows, ncols, 8, arr(42), 1, 8, out, words(8, 1)),
        "m == 0 and the whole band": (h, band, nrows, ncols, 0, arr(50), 1, 0, out, words(0, 1)),
        "four lengths": (h, band, nrows, ncols, 2, arr(3, 4, 5, 48), 4, 2, out, words(2, 4)),
        "the output ends where the band begins": (h, band, nrows, ncols, 0, arr(5), 1, 0, band - 8 * words(0, 1), words(0, 1)),
    }
    refused = {
        "no handle": (None, band, nrows, ncols, 2, arr(5), 1, 2, out, words(2, 1)),
        "no band": (h, None, nrows, ncols, 2, arr(5), 1, 2, out, words(2, 1)),
        "no lengths": (h, band, nrows, ncols, 2, None, 1, 2, out, words(2, 1)),
        "no output": (h, band, nrows, ncols, 2, arr(5), 1, 2, None, words(2, 1)),
        "nrows 0": (h, band, 0, ncols, 0, arr(1), 1, 0, out, words(0, 1)),
        "an empty band": (h, band, 0, 0, 0, arr(1), 1, 0, out, 0),
        "nrows > ncols": (h, band, ncols + 1, ncols, 2, arr(5), 1, 2, out, words(2, 1)),
        "m above 8": (h, band, nrows, ncols, 9, arr(20), 1, 9, out, words(9, 1)),
        "an m that wraps": (h, band, nrows, ncols, M64, arr(20), 1, M64, out, 0),
        "K == 0": (h, band, nrows, ncols, 2, arr(5), 0, 2, out, 0),
        "K == 5": (h, band, nrows, ncols, 2, arr(3, 4, 5, 6, 7), 5, 2, out, words(2, 5)),
        "d0 == m - 1": (h, band, nrows, ncols, 8, arr(9, 42), 2, 7, out, words(8, 2)),
        "d0 == L_1": (h, band, nrows, ncols, 2, arr(5, 9), 2, 5, out, words(2, 2)),
        "lengths that repeat": (h, band, nrows, ncols, 2, arr(5, 5), 2, 2, out, words(2, 2)),
        "lengths that fall": (h, band, nrows, ncols, 2, arr(9, 5), 2, 2, out, words(2, 2)),
        "L_K + m == nrows + 1": (h, band, nrows, ncols, 8, arr(43), 1, 8, out, words(8, 1)),
        "a length beyond the band": (h, band, nrows, ncols, 0, arr(51), 1, 0, out, words(0, 1)),
        "a length that wraps": (h, band, nrows, ncols, 2, arr(5, M64), 2, 2, out, words(2, 2)),
        "out_words too small": (h, band, nrows, ncols, 2, arr(5), 1, 2, out, words(2, 1) - 1),
        "out_words too large": (h, band, nrows, ncols, 2, arr(5), 1, 2, out, words(2, 1) + 1),
        "a misaligned output": (h, band, nrows, ncols, 2, arr(5), 1, 2, out + 4, words(2, 1)),
        "the output overlaps the band": (h, band, nrows, ncols, 2, arr(5), 1, 2, band + band_bytes - 8, words(2, 1)),
        "the output ends in the band": (h, band, nrows, ncols, 2, arr(5), 1, 2, band - 8 * words(2, 1) + 8, words(2, 1)),
        "the output is the band": (h, band, nrows, ncols, 2, arr(5), 1, 2, band, words(2, 1)),
    }
    for name, args in refused.items():
        err.value = b""
        assert lb.modle_pixels_stripe_profiles(*args, None, err, len(err)) == pixels.ERR_ARG, name
        assert err.value.startswith(b"modle_pixels_stripe_profiles: "), name
    for name, args in accepted.items():  # past the argument checks: the device of the handle does not exist
        err.value = b""
        assert lb.modle_pixels_stripe_profiles(*args, None, err, len(err)) == pixels.ERR_DEVICE, name
    ptr = C.c_void_p(1)
    for name, args in refused.items():
        if "out" in name:
            continue
        for fn, extra in ((lb.modle_pixels_stripe_profiles_to_host, ()), (lb.modle_pixels_coarse_stripe_profiles_to_host, (1, 0))):
            # (the coarse form at a factor of 1, which it refuses whatever the rest)
            ptr.value = 1
            assert fn(*args[:4], *extra, *args[4:8], C.byref(ptr), None, err, len(err)) == pixels.ERR_ARG, name
            assert ptr.value is None, name
    # the rule holds against the coarse shape: 50 diagonals by 5 are 11, and 10 + 2 > 11
    assert pixels.coarse_shape(nrows, ncols, 5, 0) == (11, 18)
    ptr.value = 1
    assert lb.modle_pixels_coarse_stripe_profiles_to_host(h, band, nrows, ncols, 5, 0, 2, arr(10), 1, 2, C.byref(ptr), None,
                                                          err, len(err)) == pixels.ERR_ARG
    assert ptr.value is None and b"of the coarse band" in err.value
    assert lb.modle_pixels_stripe_profiles_to_host(h, band, nrows, ncols, 2, arr(5), 1, 2, None, None, err, len(err)) == pixels.ERR_ARG
    # the statement of the rule on the host agrees, and the python forms refuse what ctypes would wrap
    for name, a in list(accepted.items()) + list(refused.items()):
        if a[0] is None or a[1] is None or a[5] is None or "out" in name or "wraps" in name:
            continue
        misfit = pixels.stripe_profile_misfit(a[2], a[3], a[4], list(a[5])[:a[6]], a[7])
        assert (misfit is None) == (name in accepted), (name, misfit)
    for args in ((-1, [5], 2), (2, [5], -1), (2, [-5], 2), (2, [1 << 64], 2)):
        with pytest.raises(pixels.PixelsError) as e:
            pixels._profile_args(*args)
        assert e.value.code == pixels.ERR_ARG
    assert (pixels.MAX_PROFILE_OFFSET, pixels.MAX_PROFILE_LENGTHS) == (8, 4)


# ---- <prefix>_stripe_calls.bedpe ---------------------------------------------------------------------------

def entry(name, start, end, nrows, ncols, skipped=False):
    return {"interval": {"name": name, "size": end, "start": start, "end": end}, "nrows": nrows, "ncols": ncols,
            "tasks": None, "skipped": skipped}


def test_the_lines_of_the_file(tmp_path):
    calls = cli.StripeCalls(str(tmp_path / "p_stripe_calls.bedpe"), 5000, [40_000, 80_000], 15_000, 5000, 1.5, 1, 3, 15_000)
    assert driver.stripe_calls_bins(calls) == (3, 0, [8, 16], 3, 3)
    assert driver.stripe_calls_bins(calls._replace(width=15_000, radius=0)) == (3, 1, [8, 16], 3, 0)
    header = driver.stripe_calls_header(calls)
    assert header == ("# resolution=5000 lengths=40000,80000 flank=15000 width=5000 fold=1.5 min_count=1 ignore_diags=3 "
                      "radius=15000\n#chrom1\tstart1\tend1\tchrom2\tstart2\tend2\tdirection\tlength\tcentre_sum\t"
                      "centre_cells\tleft_mean\tright_mean\tenrichment\tobserved_over_expected\n")
    iv = {"name": "chrA", "start": 25_000, "end": 525_000}
    rows = [api.StripeRow(1, 30, 1, 16, 520, 13, 10.0, 0.0, 4.0, math.nan), api.StripeRow(0, 30, 0, 8, 50, 5, 2.5, 1 / 3, 4.0, 2.0),
            api.StripeRow(0, 20, 0, 8, 7, 5, 0.0, 0.0, math.inf, 0.5)]
    lines = driver.stripe_calls_lines(iv, 5000, 1, 0, 3, rows)
    assert lines == [
        "chrA\t125000\t130000\tchrA\t90000\t115000\tup\t40000\t7\t5\t0\t0\tinf\t0.5\n",
        "chrA\t175000\t180000\tchrA\t140000\t165000\tup\t40000\t50\t5\t2.5\t0.33333333333333331\t4\t2\n",
        "chrA\t175000\t180000\tchrA\t190000\t255000\tdown\t80000\t520\t13\t10\t0\t4\tnan\n"]
    # a centre of three bins at twice the bin size: the anchor is the three coarse bins, the ends are bin_span's
    wide = driver.stripe_calls_lines(iv, 5000, 2, 1, 3, [api.StripeRow(0, 30, 0, 8, 50, 15, 1.0, 1.0, 1.0, 1.0)])
    assert wide == ["chrA\t310000\t340000\tchrA\t250000\t300000\tup\t80000\t50\t15\t1\t1\t1\t1\n"]
    plan = [entry("chrA", 25_000, 525_000, 40, 100), entry("chrB", 0, 9_000, 2, 2, skipped=True), entry("chrC", 0, 500_000, 40, 100)]
    asked = []

    def each(k, factor, first_bin):
        asked.append((k, factor, first_bin))
        return None if k == 2 else rows

    driver.write_stripe_calls(calls.path, plan, 5000, calls, each)
    assert asked == [(0, 1, 5), (2, 1, 0)]  # an entry that is skipped is not asked for, one without a matrix writes nothing
    assert open(calls.path).read() == header + "".join(lines)
    assert driver.stripe_calls_misfit(plan, 5000, 5000, [40_000, 185_000], 15_000) is None  # 37 + 3 == 40
    assert driver.stripe_calls_misfit(plan, 5000, 5000, [40_000, 190_000], 15_000) == \
        "the length of 190000 with the flank of 15000 needs 41 diagonals of 5000, the band of chrA:25000-525000 has 40"
    assert driver.stripe_calls_misfit(plan, 5000, 10_000, [100_000], 10_000) is None  # 21 diagonals at 10 kb: 10 + 1
    assert driver.stripe_calls_misfit(plan, 5000, 10_000, [200_000], 20_000).startswith("the length of 200000")


# ---- the options and what is refused before anything is simulated -------------------------------------------

@pytest.fixture
def prefix(tmp_path, monkeypatch):
    for name in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(name, raising=False)
    return str(tmp_path / "out" / "p")


def parse(prefix, *extra):
    return cli.build_parser().parse_args(["simulate", "-c", "g.chrom.sizes", "-b", "b.bed", "-o", prefix,
                                          "-r", "5kb", "--no-track-1d-lef-position", *extra])


def run_preflight(prefix, *extra):
    a = parse(prefix, *extra)
    return cli.preflight(a, cli.config_from_args(a))


def test_the_plan_of_before_is_as_it_was():
    fields = ("bin_sizes", "outputs", "rank", "world", "device", "insulation", "dots", "pileup", "subsample", "stripes",
              "coverage_min_diag", "domains", "scc")
    assert cli.Preflight._fields == fields and len(fields) == 13 and cli.Outputs._fields == (
        "cooler", "bigwig", "dense", "state_log", "expected", "coverage")
    outputs = cli.Outputs(None, None, None, None)
    for n_fields in (5, 11, 13):  # the positional five, and every field of before
        pre = cli.Preflight(*([None, outputs, 0, 1, 0] + [None] * (n_fields - 5)))
        assert pre.scc is None and pre.outputs is outputs and pre.stripe_calls is None and len(pre) == 13
    with pytest.raises(TypeError):
        cli.Preflight(*([None] * 14))  # no fourteenth field
    calls = cli.StripeCalls("p", 5000, [40_000], 15_000, 5000, 1.5, 1, 3, 15_000)
    pre = cli.Preflight(None, outputs, 0, 1, 0, stripe_calls=calls)
    assert pre.stripe_calls is calls and tuple(pre) == tuple(cli.Preflight(None, outputs, 0, 1, 0))
    moved = pre._replace(rank=1)
    assert moved.rank == 1 and moved.stripe_calls is calls and isinstance(moved, cli.Preflight)
    assert pre._replace(stripe_calls=None).stripe_calls is None and pre.stripe_calls is calls
    assert cli.Preflight._make(tuple(pre)).stripe_calls is None
    assert cli.StripeCalls._fields == ("path", "resolution", "lengths", "flank", "width", "fold", "min_count", "min_diag",
                                       "radius")


def test_the_options_parse_and_preflight_plans_the_file(prefix):
    a = parse(prefix)
    assert [getattr(a, "call_stripes" + s) for s in ("", "_lengths", "_flank", "_width", "_fold", "_min_count",
                                                     "_ignore_diags", "_radius", "_resolution")] == [None] * 9
    assert run_preflight(prefix).stripe_calls is None
    pre = run_preflight(prefix, "--call-stripes")
    assert pre.stripe_calls == cli.StripeCalls(prefix + "_stripe_calls.bedpe", 5000, [200_000, 400_000, 800_000], 40_000, 5000,
                                               1.5, 1, 8, 40_000)  # 50 kb are 10 bins: the 8 the library takes
    assert cli.stripe_calls_path(prefix) == prefix + "_stripe_calls.bedpe" and not os.path.exists(prefix + "_stripe_calls.bedpe")
    pre = run_preflight(prefix, "--call-stripes", "--call-stripes-lengths", "100kb,150kb",
                        "--call-stripes-resolution", "10kb", "--call-stripes-flank", "30kb", "--call-stripes-width", "30kb",
                        "--call-stripes-fold", "2", "--call-stripes-min-count", "0", "--call-stripes-ignore-diags", "4",
                        "--call-stripes-radius", "0")
    assert pre.stripe_calls == cli.StripeCalls(prefix + "_stripe_calls.bedpe", 10_000, [100_000, 150_000], 30_000, 30_000, 2.0, 0,
                                               4, 0)
    assert run_preflight(prefix, "--call-stripes", "--call-stripes-resolution", "25kb").stripe_calls.flank == 50_000
    assert run_preflight(prefix, "--call-stripes", "--skip-output").stripe_calls.path is None
    # analyze takes the same options
    a = cli.build_parser().parse_args(["analyze", "in.cool", "-o", prefix, "--call-stripes", "--call-stripes-flank", "10kb"])
    assert a.call_stripes is True and a.call_stripes_flank == 10_000
    # the file is refused to be overwritten like the others
    os.makedirs(os.path.dirname(prefix), exist_ok=True)
    with open(prefix + "_stripe_calls.bedpe", "w") as fh:
        fh.write("precious")
    with pytest.raises(SystemExit) as e:
        run_preflight(prefix, "--call-stripes")
    assert str(e.value) == f"refusing to overwrite {prefix}_stripe_calls.bedpe: pass --force to overwrite"
    assert run_preflight(prefix, "--call-stripes", "--force").stripe_calls.path == prefix + "_stripe_calls.bedpe"
    assert run_preflight(prefix).stripe_calls is None and open(prefix + "_stripe_calls.bedpe").read() == "precious"


def test_preflight_refuses_before_anything_is_made(prefix):
    on = ["--call-stripes"]
    refused = [
        (["--call-stripes-lengths", "100kb"], "--call-stripes-lengths needs --call-stripes"),
        (["--call-stripes-flank", "10kb"], "--call-stripes-flank needs --call-stripes"),
        (["--call-stripes-width", "5kb"], "--call-stripes-width needs --call-stripes"),
        (["--call-stripes-fold", "2"], "--call-stripes-fold needs --call-stripes"),
        (["--call-stripes-min-count", "2"], "--call-stripes-min-count needs --call-stripes"),
        (["--call-stripes-ignore-diags", "2"], "--call-stripes-ignore-diags needs --call-stripes"),
        (["--call-stripes-radius", "10kb"], "--call-stripes-radius needs --call-stripes"),
        (["--call-stripes-resolution", "10kb"], "--call-stripes-resolution needs --call-stripes"),
        (on + ["--call-stripes-resolution", "7500"], "--call-stripes-resolution: 7500 is not a multiple of the resolution (5000)"),
        (on + ["--call-stripes-lengths", "50kb,60kb,70kb,80kb,90kb"], "--call-stripes-lengths: 5 lengths: 1 to 4"),
        (on + ["--call-stripes-lengths", "52kb"], "--call-stripes-lengths: 52000 is not a multiple of the resolution of the calls (5000)"),
        (on + ["--call-stripes-width", "10kb"], "--call-stripes-width: 10000 is not an odd number of bins"),
        (on + ["--call-stripes-width", "7kb"], "--call-stripes-width: 7000 is not an odd number of bins"),
        (on + ["--call-stripes-width", "15kb", "--call-stripes-flank", "10kb"],
         "--call-stripes-flank: 10000 is below the width of the centre (15000)"),
        (on + ["--call-stripes-flank", "45kb"], "--call-stripes-flank: 45000 is 9 bins of 5000: at most 8"),
        (on + ["--call-stripes-flank", "12kb"], "--call-stripes-flank: 12000 is not a multiple"),
        (on + ["--call-stripes-radius", "12kb"], "--call-stripes-radius: 12000 is not a multiple"),
        (on + ["--call-stripes-flank", "15kb", "--call-stripes-ignore-diags", "2"],
         "--call-stripes-ignore-diags: 2 is below the 3 bins of the flank"),
        (on + ["--call-stripes-flank", "15kb", "--call-stripes-lengths", "15kb,50kb"],
         "--call-stripes-lengths: 15000 is not above the 3 ignored diagonals (15000)"),
        (on + ["--call-stripes-lengths", "100kb,100kb"], "--call-stripes-lengths: 100000 is not above 100000"),
        (on + ["--call-stripes-fold", "0"], "--call-stripes-fold: 0.0 is not a positive number"),
        (on + ["--call-stripes-fold", "nan"], "--call-stripes-fold: nan is not a positive number"),
        (on + ["--call-stripes-min-count", "-1"], "--call-stripes-min-count: -1 is negative"),
    ]
    for options, message in refused:
        with pytest.raises(SystemExit) as e:
            run_preflight(prefix, *options)
        assert str(e.value).startswith(message), (options, str(e.value))
        assert not os.path.exists(os.path.dirname(prefix))


def test_what_the_plan_refuses(prefix):
    plan = [entry("chrA", 0, 2_000_000, 40, 400), entry("chrB", 0, 40_000, 4, 8, skipped=True)]
    chroms = [("chrA", 2_000_000), ("chrB", 40_000)]
    a = parse(prefix, "--call-stripes", "--call-stripes-lengths", "50kb,190kb", "--call-stripes-flank", "15kb")
    cfg = cli.config_from_args(a)
    with pytest.raises(SystemExit) as e:
        cli.check_plan(a, cfg, cli.preflight(a, cfg), plan, chroms)
    assert str(e.value) == ("--call-stripes-lengths: the length of 190000 with the flank of 15000 needs 41 diagonals of 5000, "
                            "the band of chrA:0-2000000 has 40: widen the band with -w")
    a = parse(prefix, "--call-stripes", "--call-stripes-lengths", "50kb,185kb", "--call-stripes-flank", "15kb")
    assert cli.check_plan(a, cfg, cli.preflight(a, cfg), plan, chroms) == []


def test_the_help_of_simulate_is_unchanged():
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "golden", "simulate_help.txt")) as fh:
        golden = fh.read()
    ap = cli.build_parser()
    sub = next(a for a in ap._actions if hasattr(a, "choices") and a.choices and "simulate" in a.choices)
    text = sub.choices["simulate"].format_help()
    assert "call-stripes" not in text and "call-stripes" not in sub.choices["analyze"].format_help()
    assert "call-stripes" not in golden
