"""The regimes of the random draws that the law tests (tests/test_oracle_draw_laws.py) and the device
tests (tests/test_emu_draws.py, tests/test_gpu_draws.py) share: one table, so that every regime whose
law is held on the oracle is also a regime where the device code is held against the oracle.

The regimes sit where the algorithms of sim_rng.h / modle_oracle.c switch, not where the simulation
happens to draw: Poisson mean 10 (inversion | PTRD), m = (t + 1) p = 10 | 11 (inversion | BTRD),
k < 10 (table | Stirling series in the acceptance tests), km <= 15, the DBL_EPS break of the binomial
inversion, the bucket rule of uniform_int for ranges that divide 2^64, r == 1.0 in canonical.

Kinds, parameter words and forms are those of MODLE_HIP_UNIT_DRAWS / MODLE_HIP_UNIT_DRAW_FORMS
(include/modle_hip.h)."""
import struct
from collections import namedtuple

import numpy as np

UNIT_DRAWS, UNIT_DRAW_FORMS = 7, 8
CANONICAL, BERNOULLI, UNIFORM_INT, NORMAL, POISSON, BINOMIAL, GENEXTREME = 1, 2, 3, 4, 5, 6, 7
FORM_CANONICAL, FORM_BERNOULLI, FORM_BUCKET_UDIV, FORM_GENEXTREME, FORM_BINOM_FC, FORM_UDIV = 1, 2, 3, 4, 5, 6
HEAD_PAIRS = 3  # pairs of a DRAWS call that carry kind, seed, parameters and count

M64 = (1 << 64) - 1


def f64_bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def bits_f64(b):
    return struct.unpack("<d", struct.pack("<Q", int(b)))[0]


# `params`: the values as the caller thinks of them (floats, or integers for uniform_int and binomial's t);
# `words`: the three parameter words of the call
Regime = namedtuple("Regime", "name kind params words")


def _r(name, kind, *params):
    if kind == UNIFORM_INT:
        words = [int(params[0]), int(params[1]), 0]
    elif kind == BINOMIAL:
        words = [int(params[0]) & M64, f64_bits(params[1]), 0]
    else:
        words = [f64_bits(p) for p in params] + [0] * (3 - len(params))
    return Regime(name, kind, params, words)


REGIMES = [
    # ---- Poisson: inversion below mean 10, PTRD from 10 on
    _r("poisson_0", POISSON, 0.0),
    _r("poisson_1e-3", POISSON, 1e-3),
    _r("poisson_0.43", POISSON, 0.43),
    _r("poisson_below_10", POISSON, 9.999999999),  # the last mean of the inversion ...
    _r("poisson_10", POISSON, 10.0),               # ... and the first of PTRD
    _r("poisson_10.5", POISSON, 10.5),             # k < 10 (the log-factorial table) is frequent in the acceptance test
    _r("poisson_12", POISSON, 12.0),
    _r("poisson_26.6", POISSON, 26.6),             # chr1 defaults
    _r("poisson_300", POISSON, 300.0),
    _r("poisson_2250", POISSON, 2250.0),           # the binding rate of 45 000 LEFs over 20 epochs
    # ---- binomial: inversion while m = (t + 1) min(p, 1 - p) < 11, BTRD from 11 on
    _r("binomial_t0", BINOMIAL, 0, 1 / 6),
    _r("binomial_p0", BINOMIAL, 100, 0.0),
    _r("binomial_p1", BINOMIAL, 100, 1.0),
    _r("binomial_20_half", BINOMIAL, 20, 0.5),     # p = 0.5 exactly: not mirrored; inversion ...
    _r("binomial_797_half", BINOMIAL, 797, 0.5),   # ... and BTRD
    _r("binomial_13_sixth", BINOMIAL, 13, 1 / 6),
    _r("binomial_59_sixth", BINOMIAL, 59, 1 / 6),  # m = 10: the last of the inversion
    _r("binomial_65_sixth", BINOMIAL, 65, 1 / 6),  # 66 * fl(1/6) rounds to 11.0: m = 11, the first of BTRD
    _r("binomial_66_sixth", BINOMIAL, 66, 1 / 6),
    _r("binomial_797_sixth", BINOMIAL, 797, 1 / 6),
    _r("binomial_5000_0.8", BINOMIAL, 5000, 0.8),  # mirrored: t - k
    _r("binomial_1e6_sixth", BINOMIAL, 10 ** 6, 1 / 6),
    _r("binomial_40_1e-9", BINOMIAL, 40, 1e-9),    # reaches the r1 < DBL_EPS break of the inversion
    # ---- normal
    _r("normal_0_1", NORMAL, 0.0, 1.0),
    _r("normal_4000_200", NORMAL, 4000.0, 200.0),
    _r("normal_65000_120", NORMAL, 65000.0, 120.0),  # the top of the NARROW speeds
    # ---- uniform_int {lo, hi}
    _r("uniform_int_lo_eq_hi", UNIFORM_INT, 42, 42),  # makes no draw
    _r("uniform_int_range_1", UNIFORM_INT, 0, 1),     # ranges r with r + 1 | 2^64 take the ++bucket branch
    _r("uniform_int_range_2", UNIFORM_INT, 0, 2),
    _r("uniform_int_range_9", UNIFORM_INT, 0, 9),
    _r("uniform_int_range_255", UNIFORM_INT, 0, 255),
    _r("uniform_int_range_2p32m1", UNIFORM_INT, 0, (1 << 32) - 1),
    _r("uniform_int_range_2p63m1", UNIFORM_INT, 0, (1 << 63) - 1),  # ++bucket makes it 2: no output is rejected
    _r("uniform_int_range_2p63", UNIFORM_INT, 0, 1 << 63),  # bucket 1: every other raw output is rejected
    _r("uniform_int_range_2p64m2", UNIFORM_INT, 0, (1 << 64) - 2),
    _r("uniform_int_window", UNIFORM_INT, (1 << 40) + 3, (1 << 40) + 102),  # does not start at 0
    # ---- bernoulli
    _r("bernoulli_0", BERNOULLI, 0.0),  # draws nothing
    _r("bernoulli_1", BERNOULLI, 1.0),
    _r("bernoulli_0.75", BERNOULLI, 0.75),
    _r("bernoulli_2p-60", BERNOULLI, 2.0 ** -60),
    # ---- genextreme {mu, sigma, xi}; xi = 0 is the reference's own (mu - sigma) * log(-log u)
    # (genextreme_value_distribution.hpp:91-94), which is NOT the Gumbel law of (mu, sigma)
    _r("genextreme_xi_0", GENEXTREME, 1000.0, 5000.0, 0.0),
    _r("genextreme_xi_0.001", GENEXTREME, 0.0, 5000.0, 0.001),
    _r("genextreme_xi_0.2", GENEXTREME, 0.0, 5000.0, 0.2),
    _r("genextreme_xi_-0.2", GENEXTREME, 0.0, 5000.0, -0.2),
    # ---- canonical
    _r("canonical", CANONICAL),
]
REGIME_IDS = [r.name for r in REGIMES]


def draws_call(regime, seed, m, pairs):
    """the `in` words of a DRAWS call of `pairs` pairs that makes m draws (m + 1 <= 2 pairs)"""
    assert pairs >= HEAD_PAIRS and m + 1 <= 2 * pairs
    words = np.zeros(2 * pairs, dtype=np.uint64)
    words[:6] = np.array([regime.kind, seed] + list(regime.words) + [m], dtype=np.uint64)
    return words


# ---------------------------------------------------------------------------------------------
# Forms: (form, name, elements of four words).  Every input keeps the conversions of the forms
# defined (no double beyond 2^64 is converted to an integer), so that the oracle, the emulator and
# the GPU must agree on every one of them.
# ---------------------------------------------------------------------------------------------
RAWS = [0, 1, 1 << 53, (1 << 64) - (1 << 10) - 1, (1 << 64) - (1 << 10), (1 << 64) - 1,
        # around the tie (2^64 - 2^10 is where double(raw) starts to round to 2^64, i.e. r == 1.0 in canonical)
        (1 << 64) - (1 << 11), (1 << 64) - (1 << 10) + 1, (1 << 63), (1 << 63) + (1 << 10), 0x9E3779B97F4A7C15]

# p where p * 2^64 is not exact does not exist for a double p (a power-of-two scaling); what rounds is
# double(raw): raws around p * 2^64 that are not representable are the edge of `double(raw) <= p * 2^64`
_P = [0.75, 2.0 ** -60, 1 / 3, 0.1, 1.0 - 2.0 ** -53, 2.0 ** -64, 1.0, 5e-324]


def _bernoulli_elements():
    out = []
    for p in _P:
        t = int(p * 2.0 ** 64)  # exact: p * 2^64 is a double, and an integer for p >= 2^-11 or so
        for raw in RAWS + [max(t - 1, 0), min(t, M64), min(t + 1, M64), min(t + 1024, M64), min(t + 1025, M64),
                           max(t - 1025, 0)]:
            out.append([raw, f64_bits(p), 0, 0])
    return out


# ranges r: r + 1 divides 2^64 (the ++bucket branch) or not; the side of udiv_by_uniform's stated bound
# ("d <= 2^62, quotient < 2^40") each bucket d is on is told by `udiv_within_bound`
RANGES = [1, 2, 3, 4, 9, 255, 256, (1 << 20) - 1, 1 << 20, (1 << 24) - 1, (1 << 32) - 1, 1 << 32, 10 ** 9, 5_000_000 - 1,
          (1 << 40) - 1, (1 << 44) - 1, (1 << 44) + 12345]


def bucket_of(r):
    """uniform_int's bucket in Python integers: the largest b with (r + 1) b <= 2^64.  (The code's rule,
    (2^64 - 1) / (r + 1) and one more where the remainder is r, is this number: the remainder is r exactly
    where r + 1 divides 2^64.)"""
    return (1 << 64) // (r + 1)


def udiv_within_bound(raw, d):
    """the bound sim_rng.h states for udiv_by_uniform: d <= 2^62 and quotient < 2^40"""
    return d <= (1 << 62) and raw // d < (1 << 40)


def _raws_for_divisor(d):
    # multiples of d and their neighbours are where a quotient that is off by one shows
    raws = set(RAWS)
    for q in (1, 2, 3, 1000, (1 << 32) - 1, (1 << 39), (1 << 40) - 1):
        for delta in (-1, 0, 1, d - 1):
            raws.add(q * d + delta)
    top = (M64 // d) * d
    raws.update([top - 1, top, min(top + d - 1, M64)])
    # keep double(raw) / d below 2^63: beyond, the conversion back to an integer is not defined
    return sorted(r for r in raws if 0 <= r <= M64 and r // d < (1 << 62))


def _bucket_elements():
    return [[r, raw, 0, 0] for r in RANGES for raw in _raws_for_divisor(bucket_of(r))]


# divisors at 2^32, at 2^62 and just beyond it, and small ones whose quotients pass 2^40
DIVISORS = [1 << 32, (1 << 32) + 1, (1 << 62) - 1, 1 << 62, (1 << 62) + 1, (1 << 62) + (1 << 20), 0x5555555555555555,
            1 << 63, (1 << 24), (1 << 24) - 1, (1 << 20) + 7, 3_689_348_814_741]


def _udiv_elements():
    return [[raw, d, 0, 0] for d in DIVISORS for raw in _raws_for_divisor(d)]


_US = [2.0 ** -1074, 2.0 ** -53, 0.5, 1.0 - 2.0 ** -53, 2.0 ** -1022, 0.25, 0.999, 1e-300, 0.36787944117144233]
_GEV = [(0.0, 5000.0, 0.0), (1000.0, 5000.0, 0.0), (0.0, 5000.0, 0.001), (0.0, 5000.0, 0.2), (0.0, 5000.0, -0.2),
        (12.5, 3.0, 1.0)]

FORMS = [
    (FORM_CANONICAL, "canonical_raw", [[raw, 0, 0, 0] for raw in RAWS]),
    (FORM_BERNOULLI, "bernoulli_raw", _bernoulli_elements()),
    (FORM_BUCKET_UDIV, "bucket_and_udiv", _bucket_elements()),
    (FORM_GENEXTREME, "genextreme_from_canonical",
     [[f64_bits(u), f64_bits(mu), f64_bits(s), f64_bits(xi)] for (mu, s, xi) in _GEV for u in _US]),
    (FORM_BINOM_FC, "binom_fc", [[k, 0, 0, 0] for k in list(range(21)) + [10 ** 6]]),
    (FORM_UDIV, "udiv_by_uniform", _udiv_elements()),
]
FORM_IDS = [f[1] for f in FORMS]


def forms_call(form, elements):
    """the `in` words of a DRAW_FORMS call: the head pair, then two pairs per element"""
    el = np.array(elements, dtype=np.uint64).reshape(-1, 4)
    return np.concatenate([np.array([form, 0], dtype=np.uint64), el.reshape(-1)])


# ---------------------------------------------------------------------------------------------
# running a backend of the device code (the lane emulator or the GPU) against the oracle.
# `units(what, words, out)` fills `out` (2 n words for n pairs of `words`).
# ---------------------------------------------------------------------------------------------
POISON = 0xDEADBEEFCAFEF00D
GUARD = 8


def run_guarded(units, what, words):
    """runs one call with its output between poisoned guard words and checks that they survive"""
    buf = np.full(len(words) + 2 * GUARD, POISON, dtype=np.uint64)
    out = buf[GUARD:-GUARD]
    out[:] = 0
    units(what, words, out)
    assert np.all(buf[:GUARD] == POISON) and np.all(buf[-GUARD:] == POISON), "guard words overwritten"
    return out


def check_draws(units, oracle, regime, seed, m, pairs):
    """m draws of the regime from `seed`: the device code's draws and its count of engine outputs equal the
    oracle's, word for word.  The oracle draws first: a call that ends there ends on the device"""
    want, consumed = oracle.draw_many(regime.kind, regime.words, seed, m)
    out = run_guarded(units, UNIT_DRAWS, draws_call(regime, seed, m, pairs))
    assert int(out[0]) == consumed, f"{regime.name} seed {seed}: engine outputs consumed"
    bad = np.flatnonzero(out[1:m + 1] != want)
    assert len(bad) == 0, (f"{regime.name} seed {seed}: draw {bad[0]} differs: device {int(out[1 + bad[0]]):#x}, "
                           f"oracle {int(want[bad[0]]):#x}")
    assert not out[m + 1:].any(), "words beyond the draws were written"


def exact_form(form, e):
    """what Python integers give for the forms that have such an answer: (word 0, word 1), None = not held"""
    if form == FORM_BUCKET_UDIV:
        d = bucket_of(e[0])
        return d, (e[1] // d if udiv_within_bound(e[1], d) else None)
    if form == FORM_UDIV:
        return (e[0] // e[1] if udiv_within_bound(e[0], e[1]) else None), 0
    if form == FORM_CANONICAL:  # the nearest double of raw / 2^64, and the largest double below 1 where that is 1
        r = float(e[0]) / 2.0 ** 64  # (int -> float rounds to nearest even; the division by 2^64 is exact)
        return f64_bits(r if r != 1.0 else 1.0 - 2.0 ** -53), 0
    if form == FORM_BERNOULLI:
        return int(float(e[0]) <= bits_f64(e[1]) * 2.0 ** 64), 0
    return None, None


def check_forms(units, oracle, form, elements):
    """every element: device == oracle on all four words, and both == Python's integers where those answer"""
    want = oracle.draw_forms(form, elements)
    out = run_guarded(units, UNIT_DRAW_FORMS, forms_call(form, elements))
    assert out[0] == 0 and out[1] == 0
    got = out[2:].reshape(-1, 4)
    for i in np.flatnonzero((got != want).any(axis=1))[:1]:
        raise AssertionError(f"form {form} on {[hex(x) for x in elements[i]]}: device {list(got[i])}, "
                             f"oracle {list(want[i])}")
    seen = set()
    for e, w in zip(elements, want):
        if tuple(e) in seen:
            continue
        seen.add(tuple(e))
        for word, exact in enumerate(exact_form(form, e)):
            if exact is not None:
                assert int(w[word]) == exact, f"form {form} on {[hex(x) for x in e]}: word {word}"
