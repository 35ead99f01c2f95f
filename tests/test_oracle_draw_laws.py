"""The oracle's random draws against the exact laws (CPU, no device).

Every GPU test compares the device with oracle/modle_oracle.c word for word, and both restate
Boost.Random by the same hand: a wrong PTRD / BTRD constant, ziggurat layer or uniform_int bucket
rule in both is invisible to parity.  Here 4 000 000 draws per regime of tests/draw_cases.py, made
in C (mo_draw_many), are held against scipy's laws: chi-square with pooled tails, the sum under its
exact law, z-tests with exact standard errors, the normal binned at the ziggurat's own abscissae, and
the engine outputs consumed against what the table's areas give.

What this catches: gross errors and whole wrong branches, not fifth digits
(profiles/draw_laws/mutations.txt: the mutants it catches, and the ones beyond its reach).  The table
literals of binom_fc, which the sample cannot resolve, are held deterministically below.

A statistic fails below p = 1e-6.  Seeds are fixed, so the tests are deterministic; the unmutated
oracle's smallest p per regime is recorded in profiles/draw_laws/oracle_p_values.txt."""
import numpy as np
import pytest

import draw_cases as dc
import draw_laws as dl


@pytest.fixture(scope="module")
def zig():
    return dl.read_zig_tables()


@pytest.mark.parametrize("regime", dc.REGIMES, ids=dc.REGIME_IDS)
def test_draws_follow_the_law(oracle, zig, regime):
    draws, consumed = oracle.draw_many(regime.kind, regime.words, dl.SEED, dl.N_DRAWS)
    got = dl.statistics(regime, draws, consumed, zig)
    assert got, "no statistic for this regime"
    print({k: f"{v:.3g}" for k, v in got.items()})
    assert all(p >= dl.P_LINE for p in got.values()), got


def test_normal_engine_outputs_per_draw_follow_the_table(oracle, zig):
    """engine outputs per normal draw against the value computed from the table's areas (about 1.04: ~1.2 % of
    the attempts need a wedge test, ~0.9 % are rejected, and the tail costs a loop of exponentials), not
    against a range: 400 seeds of 10 000 draws, the mean of their ratios under a z-test"""
    regime = next(r for r in dc.REGIMES if r.name == "normal_0_1")
    ratios = [oracle.draw_many(regime.kind, regime.words, 1000 + s, 10_000)[1] / 10_000 for s in range(400)]
    expected = dl.normal_outputs_per_draw(zig)
    p = dl.normal_outputs_ratio_p(ratios, zig)
    print(f"outputs per draw: table {expected:.6f}, sample {np.mean(ratios):.6f}, p = {p:.3g}")
    assert 1.0 < expected < 1.1
    assert p >= dl.P_LINE


def test_binom_fc_against_the_stirling_remainder(oracle):
    """binom_fc(0..9) (table literals) and the series from k = 10 on against the Stirling remainder at 50
    digits.  FC_LIMIT is a small margin above what the unmutated oracle reaches (draw_laws.py); a table entry
    off by 9e-5, which no sample of this size resolves, is far beyond it"""
    L = oracle.lib()
    dev = dl.binom_fc_deviation(L.mo_binom_fc)
    print(f"largest deviation of binom_fc from the Stirling remainder: {dev:.3g} (limit {dl.FC_LIMIT:.3g})")
    assert dev <= dl.FC_LIMIT
    assert dl.binom_fc_deviation(lambda k: L.mo_binom_fc(k) + (9e-5 if k == 2 else 0.0)) > dl.FC_LIMIT


def test_bucket_rule_against_python_integers(oracle):
    """uniform_int's bucket: the largest b with (range + 1) b <= 2^64, in Python integers -- one more than
    (2^64 - 1) // (range + 1) exactly where range + 1 divides 2^64"""
    L = oracle.lib()
    ranges = dc.RANGES + [r.params[1] - r.params[0] for r in dc.REGIMES
                          if r.kind == dc.UNIFORM_INT and 0 < r.params[1] - r.params[0] < dc.M64]
    for r in ranges:
        b = L.mo_uniform_int_bucket(r)
        assert b == dc.bucket_of(r) == (1 << 64) // (r + 1), r
        assert (r + 1) * b <= 1 << 64 < (r + 1) * (b + 1), r
