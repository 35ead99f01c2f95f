"""Randomised multi-batch phase-level parity on the real GPU (modle_hip_test_phases) vs oracle."""
import pytest

from phase_backend import _advance
from phase_random import NEAR_LIMIT_SEQUENCES, run_sequences

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed,n,nb,kw,dense", [
    (1, 300, 60, {}, False),
    (2, 1500, 400, {}, False),
    (3, 1000, 300, {"bypass": 0.0}, False),
    (4, 1200, 500, {"minor": 0.3, "major": 0.9, "bypass": 0.3}, True),
    (5, 5000, 3000, {}, False),
    # few units over long lists: a block of 256 ranks whose unit windows span more list entries than the LDS
    # window holds takes the LEF-BAR sweep's fall-back (per-unit searches in the list in device memory)
    (6, 40, 3000, {"minor": 1.0}, False),   # one block spans both lists (about 2 400 entries each)
    (7, 300, 6000, {"minor": 1.0}, False),  # a block that falls back, then 44 ranks that restage the window
    (8, 40, 3000, {}, False),               # default probabilities: the two lists differ
] + NEAR_LIMIT_SEQUENCES)
def test_random_phases_gpu(oracle, seed, n, nb, kw, dense):
    from modle_amd import api

    sims = {}

    def phases(cfg, mask, st, state, skip):
        key = (cfg.probability_of_extrusion_unit_bypass, cfg.lef_bar_major_collision_pblock,
               cfg.lef_bar_minor_collision_pblock, cfg.rev_extrusion_speed, cfg.fwd_extrusion_speed)
        if key not in sims:
            sims[key] = api.Simulator(cfg.copy(), 0)
        return sims[key].test_phases(mask, st, _advance(state, skip))

    try:
        run_sequences(oracle, phases, seed, n, nb, kw, dense)
    finally:
        for s in sims.values():
            s.close()
