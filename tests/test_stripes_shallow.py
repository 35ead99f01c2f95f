"""A restatement of the stripe sums for bands of at most three diagonals that has no loop over the columns:
tests/test_stripes_outputs.py's restate() walks the columns in Python (lists of Python ints for the 128-bit
sums, a searchsorted per stripe for the ranks), which a band of a million columns turns into half a minute.
For nrows <= 3 everything has a closed form in whole-array numpy:

    ranks    R2(x_i) = 1 + sum over k of (2 * [x_k < x_i] + [x_k == x_i]), nine comparisons per stripe;
    moments  a product of two uint32 fits uint64 exactly; the low and the high 32 bits of the at most three
             products are summed apart (below 3 * 2^32 each) and joined into the two words with one carry.

restate_shallow is pinned here, without a device, to restate() word for word; tests/test_gpu_long_bands.py
holds the rank kernel at its real grid cap against it."""
import numpy as np
import pytest

from test_stripes_outputs import MASKED, MOMENTS, RANKS, band_stripes, random_pair, restate

M32 = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def shallow_moments(a, b, masked):
    """the nine rows of restate_moments for stripes uint64 [ncols, nrows <= 3]"""
    if masked:
        w = ((a != 0) & (b != 0)).astype(np.uint64)
        a, b, n = a * w, b * w, w.sum(axis=1, dtype=np.uint64)
    else:
        n = np.full(a.shape[0], a.shape[1], dtype=np.uint64)
    rows = [n, a.sum(axis=1, dtype=np.uint64), b.sum(axis=1, dtype=np.uint64)]
    for x, y in ((a, a), (b, b), (a, b)):
        p = x * y  # below 2^64: exact
        lo, hi = (p & M32).sum(axis=1, dtype=np.uint64), (p >> S32).sum(axis=1, dtype=np.uint64)
        # the sum is lo + hi * 2^32 with lo, hi < 3 * 2^32: the low word wraps at most once
        shifted = (hi & M32) << S32
        low = lo + shifted
        rows += [low, (hi >> S32) + (low < lo).astype(np.uint64)]
    return np.stack(rows)


def shallow_ranks(a, b):
    """the three rows of restate_ranks for stripes uint64 [ncols, nrows <= 3]"""
    def r2(x):
        mine, other = x[:, :, None], x[:, None, :]
        return (2 * (other < mine).sum(axis=2, dtype=np.uint64) + (other == mine).sum(axis=2, dtype=np.uint64)
                + np.uint64(1))

    ra, rb = r2(a), r2(b)
    return np.stack([(ra * ra).sum(axis=1, dtype=np.uint64), (rb * rb).sum(axis=1, dtype=np.uint64),
                     (ra * rb).sum(axis=1, dtype=np.uint64)])


def restate_shallow(band_a, band_b, nrows, ncols, what):
    """uint64 [2, rows(what), ncols]: what restate() returns, for nrows <= 3"""
    assert 1 <= nrows <= 3
    out = []
    for d in (0, 1):
        a, b = band_stripes(band_a, nrows, ncols, d), band_stripes(band_b, nrows, ncols, d)
        blocks = []
        if what & MOMENTS:
            blocks.append(shallow_moments(a, b, False))
        if what & MASKED:
            blocks.append(shallow_moments(a, b, True))
        if what & RANKS:
            blocks.append(shallow_ranks(a, b))
        out.append(np.concatenate(blocks))
    return np.stack(out)


# counts below 3 tie in nearly every stripe; counts up to 2^32 - 1 carry into the high words
@pytest.mark.parametrize("below", [3, 2**32])
@pytest.mark.parametrize("nrows,ncols", [(3, 300), (2, 65), (1, 7), (3, 3)])
def test_the_closed_form_equals_the_restatement(nrows, ncols, below):
    a, b = random_pair(nrows, ncols, below)
    want = restate(a, b, nrows, ncols, 7)
    if below == 2**32 and nrows * ncols > 100:
        assert want[:, [4, 6, 8]].any(axis=(0, 2)).all()  # every second moment passes 2^64 somewhere
    if below == 3 and ncols > 100:
        ranks = want[:, 18:20]
        assert len(np.unique(ranks)) > 2  # stripes with and without ties
    for what in range(1, 8):
        got = restate_shallow(a, b, nrows, ncols, what)
        assert got.dtype == np.uint64 and np.array_equal(got, restate(a, b, nrows, ncols, what)), what
    full = np.full(nrows * ncols + 1, 0xFFFFFFFF, dtype=np.uint32)  # three products of (2^32 - 1)^2
    assert np.array_equal(restate_shallow(full, full, nrows, ncols, 7), restate(full, full, nrows, ncols, 7))
