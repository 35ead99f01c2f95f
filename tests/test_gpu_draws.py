"""The device code's random draws (sim_rng.h) on the REAL GPU against the oracle, word for word, in every
regime of tests/draw_cases.py: 2^18 draws per regime as four calls with four seeds, each through the NARROW
unit kernel and through the WIDE one (a call of 65 536 pairs), and the pure forms on their edge inputs.

Parity of whole cells only reaches the regimes the simulation happens to draw in; the switches between the
algorithms (Poisson mean 10, m = 10 | 11, k < 10, the DBL_EPS break, the ziggurat's tail, the ++bucket
branch) sit elsewhere, and the GPU evaluates them with its own floating-point library and compiler.

Every call launches one wave and makes a number of draws fixed by the call; the oracle makes the same
draws first, so a call that ends there ends on the device (the two are bit-identical or the test fails)."""
import pytest

import draw_cases as dc
from unit_vector_runner import base_config

pytestmark = pytest.mark.gpu

N_PER_CALL = 1 << 16
SEEDS = [7, 752741483, 10556020843759504871, 0]
NARROW_PAIRS = N_PER_CALL // 2 + 1  # 32 769 pairs: just room for the count and the draws
WIDE_PAIRS = 1 << 16                # 65 536 pairs or more run the WIDE unit kernel


@pytest.fixture(scope="module")
def gpu_units():
    from modle_amd import api

    sim = api.Simulator(base_config(), 0)

    def units(what, words, out):
        sim.test_units(what, words, out=out)

    yield units
    sim.close()


@pytest.mark.parametrize("regime", dc.REGIMES, ids=dc.REGIME_IDS)
def test_gpu_draws_equal_the_oracle(oracle, gpu_units, regime):
    for seed in SEEDS:
        for pairs in (NARROW_PAIRS, WIDE_PAIRS):
            dc.check_draws(gpu_units, oracle, regime, seed, N_PER_CALL, pairs)


@pytest.mark.parametrize("form,name,elements", dc.FORMS, ids=dc.FORM_IDS)
def test_gpu_forms_equal_the_oracle(oracle, gpu_units, form, name, elements):
    dc.check_forms(gpu_units, oracle, form, elements)
    # the same elements repeated up to a call of the WIDE size class (1 + 2 * 32 768 pairs)
    reps = -(-(1 << 15) // len(elements))
    dc.check_forms(gpu_units, oracle, form, list(elements) * reps)
