"""Statistics that hold a sample of draws against the exact law of its regime (tests/draw_cases.py).
Shared by tests/test_oracle_draw_laws.py and tools/draw_law_mutations.py; not a test module.

What this instrument resolves: at 4 000 000 draws it catches gross errors and whole wrong branches,
not fifth digits.  A constant whose change moves the law by less than the sample resolves, or only
the sampler's efficiency, passes here (profiles/draw_laws/mutations.txt lists such mutants)."""
import math
import os
import re

import numpy as np
from scipy import special, stats

import draw_cases as dc

N_DRAWS = 4_000_000
SEED = 7
P_LINE = 1e-6  # a statistic fails below this p: a condition, not a measurement
MIN_EXPECTED = 20.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def read_zig_tables(path=None):
    """the generated ziggurat tables (oracle/zig_tables.h): name -> array of doubles"""
    text = open(path or os.path.join(ROOT, "oracle", "zig_tables.h")).read()
    out = {}
    for m in re.finditer(r"static const double (ZIG_\w+)\[(\d+)\] = \{(.*?)\};", text, re.S):
        vals = [float.fromhex(t) for t in re.findall(r"-?0x[0-9a-fA-F.]+p[+-]?\d+", m.group(3))]
        assert len(vals) == int(m.group(2)), m.group(1)
        out[m.group(1)] = np.array(vals)
    return out


def pooled_chi2(observed, prob, n):
    """chi-square p-value of ordered bins; from either end towards the largest bin, neighbours are pooled until
    every expectation reaches MIN_EXPECTED (what is left over joins the largest bin).  None when fewer than
    two bins remain (a law with one atom at this n)"""
    observed = np.asarray(observed, dtype=float)
    expected = np.asarray(prob, dtype=float) * n
    peak = int(np.argmax(expected))
    obs, exp = [], []
    rest_o = rest_e = 0.0
    for idx in (range(0, peak), range(len(expected) - 1, peak, -1)):
        acc_o = acc_e = 0.0
        side_o, side_e = [], []
        for i in idx:
            acc_o, acc_e = acc_o + observed[i], acc_e + expected[i]
            if acc_e >= MIN_EXPECTED:
                side_o.append(acc_o)
                side_e.append(acc_e)
                acc_o = acc_e = 0.0
        rest_o, rest_e = rest_o + acc_o, rest_e + acc_e
        obs.append(side_o)
        exp.append(side_e)
    obs = np.array(obs[0] + [observed[peak] + rest_o] + obs[1][::-1])
    exp = np.array(exp[0] + [expected[peak] + rest_e] + exp[1][::-1])
    if len(exp) < 2 or exp.min() < MIN_EXPECTED:
        return None
    return float(stats.chi2.sf(((obs - exp) ** 2 / exp).sum(), len(exp) - 1))


def z_p(value, expected, se):
    return float(2 * stats.norm.sf(abs(value - expected) / se))


def exact_two_sided(dist, s):
    """two-sided p of an integer statistic under its exact discrete law"""
    return float(min(1.0, 2 * min(dist.cdf(s), dist.sf(s - 1))))


def _discrete(draws, law, total_law):
    """chi-square over the values within 6 sigma (tails pooled), the sum under its exact law (the sum of n
    Poisson / binomial draws is Poisson / binomial again), and a z-test of the variance with its exact
    standard error sqrt((mu4 - sigma^4) / n) where the sum of squared deviations is a sum of many terms"""
    n = len(draws)
    mean, var = (float(x) for x in law.stats(moments="mv"))
    out = {}
    if var == 0.0:
        out["all_equal"] = 1.0 if np.all(draws == np.uint64(int(round(mean)))) else 0.0
        return out
    sd = math.sqrt(var)
    lo, hi = max(int(law.support()[0]), int(math.floor(mean - 6 * sd))), int(math.ceil(mean + 6 * sd))
    hi = min(hi, int(law.support()[1])) if math.isfinite(law.support()[1]) else hi
    v = draws.astype(np.int64)
    counts = np.bincount(np.clip(v, lo - 1, hi + 1) - (lo - 1), minlength=hi - lo + 3)
    k = np.arange(lo, hi + 1)
    prob = np.concatenate([[law.cdf(lo - 1)], law.pmf(k), [law.sf(hi)]])
    p = pooled_chi2(counts, prob, n)
    if p is not None:
        out["chi2"] = p
    out["sum_exact"] = exact_two_sided(total_law, int(v.sum()))
    if n * var >= 1000:
        mu4 = (float(law.stats(moments="k")) + 3.0) * var * var
        s2 = float(((v - mean) ** 2).mean())
        out["variance_z"] = z_p(s2, var, math.sqrt((mu4 - var * var) / n))
    return out


def normal_bins(zig):
    """edges at the ziggurat's own abscissae -x_1 .. -x_127, 0, x_127 .. x_1: each layer's strip is a bin of
    its own on either side, and so is either tail beyond x_1"""
    x = zig["ZIG_NORM_X"]
    assert len(x) == 129 and x[128] == 0.0
    pos = x[1:129][::-1]  # 0, x_127, ..., x_1
    return np.concatenate([-pos[::-1][:-1], pos])


def _normal(draws, mean, sigma, zig):
    n = len(draws)
    z = (draws.view(np.float64) - mean) / sigma
    edges = normal_bins(zig)
    counts = np.bincount(np.searchsorted(edges, z, side="right"), minlength=len(edges) + 1)
    cdf = np.concatenate([[0.0], special.ndtr(edges), [1.0]])
    # the upper half through the survival function: differences of values near 1 lose the tail's digits
    sf = np.concatenate([[1.0], special.ndtr(-edges), [0.0]])
    prob = np.where(np.arange(len(cdf) - 1) < len(edges) // 2 + 1, np.diff(cdf), -np.diff(sf))
    assert abs(prob.sum() - 1.0) < 1e-12
    return {"chi2_layers": pooled_chi2(counts, prob, n),
            "mean_z": z_p(float(z.mean()), 0.0, 1.0 / math.sqrt(n)),
            "variance_z": z_p(float((z * z).mean()), 1.0, math.sqrt(2.0 / n))}


def exponential_outputs_per_draw(zig):
    """engine outputs one unit_exponential draw consumes on average, from the table's own areas.  Per
    attempt (attempts are independent: Wald's identity gives outputs = cost per attempt / P(return)):
    one output, one more for the wedge test where x >= x_{i+1} in a layer i >= 1 (layer 0 shifts and
    tries again without one).  The wedge accepts the part of its rectangle under exp(-x), whose integral
    over [x_{i+1}, x_i] is y_{i+1} - y_i.  (uniform_01's own redraw, p = 2^-53, is left out.)"""
    x, y = zig["ZIG_EXP_X"], zig["ZIG_EXP_Y"]
    i = np.arange(1, 256)
    fast = x[i + 1] / x[i]
    dx, dy = x[i] - x[i + 1], y[i + 1] - y[i]
    wedge = np.where(dx > 0, (dy - y[i] * dx) / np.where(dx > 0, dx * dy, 1.0), 0.0)
    cost = 1.0 + (1.0 - fast).sum() / 256
    ret = (x[1] / x[0] + (fast + (1.0 - fast) * wedge).sum()) / 256
    return cost / ret


def normal_outputs_per_draw(zig):
    """the same for unit_normal: layer 0 beyond x_1 runs the tail loop, two exponentials per round, accepted
    with P(2 E2 > (E1 / x_1)^2) = x_1 sqrt(2 pi) exp(x_1^2 / 2) (1 - Phi(x_1))"""
    x, y = zig["ZIG_NORM_X"], zig["ZIG_NORM_Y"]
    i = np.arange(1, 128)
    fast = x[i + 1] / x[i]
    dx, dy = x[i] - x[i + 1], y[i + 1] - y[i]
    area = math.sqrt(2 * math.pi) * (special.ndtr(x[i]) - special.ndtr(x[i + 1]))  # of exp(-x^2 / 2) over the strip
    wedge = (area - y[i] * dx) / (dx * dy)
    a = x[1]
    p_tail = a * math.sqrt(2 * math.pi) * special.erfcx(a / math.sqrt(2)) / 2
    tail = 2 * exponential_outputs_per_draw(zig) / p_tail
    cost = 1.0 + ((1.0 - fast).sum() + (1.0 - x[1] / x[0]) * tail) / 128
    ret = (1.0 + (fast + (1.0 - fast) * wedge).sum()) / 128
    return cost / ret


def normal_outputs_ratio_p(ratios, zig):
    """z-test of the mean of per-sample ratios (engine outputs / draws, one sample per seed) against the value
    the table gives; the standard error is the samples' own"""
    r = np.asarray(ratios, dtype=float)
    return z_p(float(r.mean()), normal_outputs_per_draw(zig), float(r.std(ddof=1)) / math.sqrt(len(r)))


def _uniform_int(draws, consumed, lo, hi):
    n = len(draws)
    rng = hi - lo
    if rng == 0:
        return {"all_equal": 1.0 if np.all(draws == np.uint64(lo)) else 0.0,
                "outputs_exact": 1.0 if consumed == 0 else 0.0}
    v = draws - np.uint64(lo)
    if int(v.max()) > rng:
        return {"in_range": 0.0}
    shift = max(0, rng.bit_length() - 8)  # every value for the small ranges, the top 8 bits for the large ones
    nb = (rng >> shift) + 1
    counts = np.bincount((v >> np.uint64(shift)).astype(np.int64), minlength=nb)
    sizes = np.array([min(rng, ((b + 1) << shift) - 1) - (b << shift) + 1 for b in range(nb)], dtype=float)
    out = {"chi2": pooled_chi2(counts, sizes / (rng + 1.0), n),
           "mean_z": z_p(float(v.astype(np.float64).mean()), rng / 2.0,
                         math.sqrt(((rng + 1.0) ** 2 - 1.0) / 12.0 / n))}
    # outputs: every attempt is accepted with a = (range + 1) bucket / 2^64; the attempts n draws take are
    # n plus a negative-binomial count of rejections
    a = (rng + 1) * dc.bucket_of(rng) / 2.0 ** 64
    rejected = n * (1 - a) / a
    if (rng + 1) * dc.bucket_of(rng) == 1 << 64:
        out["outputs_exact"] = 1.0 if consumed == n else 0.0
    elif rejected >= 1000:
        out["outputs_z"] = z_p(consumed - n, rejected, math.sqrt(n * (1 - a)) / a)
    return out


def _uniform01_chi2(u, n):
    if not (np.all(u >= 0.0) and np.all(u < 1.0)):
        return 0.0
    counts = np.bincount((u * 256).astype(np.int64), minlength=256)
    return pooled_chi2(counts, np.full(256, 1 / 256), n)


def genextreme_cdf(x, mu, sigma, xi):
    """P(X <= x) of the reference's genextreme_value_distribution: X = g(u) grows with the canonical u, so the
    law's CDF is g's inverse.  xi == 0 is (mu - sigma) log(-log u), NOT the Gumbel law of (mu, sigma)"""
    if xi == 0.0:
        return np.exp(-np.exp(x / (mu - sigma))) if mu - sigma < 0 else 1.0 - np.exp(-np.exp(x / (mu - sigma)))
    return np.exp(-np.exp(np.log1p(-xi * (x - mu) / sigma) / xi))


def statistics(regime, draws, consumed, zig=None):
    """name -> p-value of every statistic of the regime (1.0 / 0.0 for conditions that hold or do not)"""
    n = len(draws)
    k, p = regime.kind, regime.params
    if k == dc.POISSON:
        out = _discrete(draws, stats.poisson(p[0]), stats.poisson(n * p[0]))
    elif k == dc.BINOMIAL:
        out = _discrete(draws, stats.binom(p[0], p[1]), stats.binom(n * p[0], p[1]))
    elif k == dc.NORMAL:
        out = _normal(draws, p[0], p[1], zig or read_zig_tables())
    elif k == dc.UNIFORM_INT:
        out = _uniform_int(draws, consumed, p[0], p[1])
    elif k == dc.BERNOULLI:
        if not np.all(draws <= 1):
            return {"is_0_or_1": 0.0}
        # P(double(raw) <= p 2^64) = (floor(p 2^64) + 1) / 2^64 up to the rounding of double(raw), 2^-53 relative
        q = min(1.0, p[0] + 2.0 ** -64) if p[0] > 0 else 0.0
        out = {"ones_exact": exact_two_sided(stats.binom(n, q), int(draws.sum())),
               "outputs_exact": 1.0 if consumed == (0 if p[0] == 0 else n) else 0.0}
    elif k == dc.GENEXTREME:
        x = draws.view(np.float64)
        out = {"chi2_cdf": _uniform01_chi2(genextreme_cdf(x, *p), n) if np.all(np.isfinite(x)) else 0.0,
               "outputs_exact": 1.0 if consumed == n else 0.0}
    else:
        u = draws.view(np.float64)
        out = {"chi2": _uniform01_chi2(u, n), "mean_z": z_p(float(u.mean()), 0.5, math.sqrt(1 / 12 / n)),
               "variance_z": z_p(float(((u - 0.5) ** 2).mean()), 1 / 12, math.sqrt((1 / 80 - 1 / 144) / n)),
               "outputs_exact": 1.0 if consumed == n else 0.0}
    return {name: val for name, val in out.items() if val is not None}


# ---------------------------------------------------------------------------------------------
# table literals, held deterministically
# ---------------------------------------------------------------------------------------------
def stirling_remainder(k):
    """lgamma(k + 1) - ((k + 1/2) ln(k + 1) - (k + 1) + ln(2 pi) / 2) at 50 digits: what binom_fc tabulates
    for k < 10 and expands in 1 / (k + 1) from 10 on"""
    import mpmath

    with mpmath.workdps(50):
        k = mpmath.mpf(k)
        return mpmath.loggamma(k + 1) - ((k + 0.5) * mpmath.log(k + 1) - (k + 1) + mpmath.log(2 * mpmath.pi) / 2)


FC_KS = list(range(21)) + [10 ** 6]


def binom_fc_deviation(binom_fc):
    """largest |binom_fc(k) - Stirling remainder| over k = 0 .. 20 and 10^6, as a float"""
    import mpmath

    with mpmath.workdps(50):
        return float(max(abs(mpmath.mpf(binom_fc(k)) - stirling_remainder(k)) for k in FC_KS))


# The unmutated oracle reaches 3.02e-11 (profiles/draw_laws/oracle_p_values.txt), at k = 10: the first term
# the three-term series leaves out there, 1 / (1680 (k + 1)^7) = 3.05e-11.  The ten table literals are good to
# 1e-17.  The limit sits a small margin above what is reached.
FC_LIMIT = 5e-11
