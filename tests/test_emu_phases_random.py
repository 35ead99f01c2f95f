"""Randomised multi-batch phase-level parity: emulated device code vs oracle (CPU), with the geometry of
the 8-wave kernels and with that of the 12-wave ones (phase_backend.emu_phases)."""
import functools

import pytest

from phase_backend import emu_phases
from phase_random import NEAR_LIMIT_SEQUENCES, run_sequences

SEQUENCES = [
    (1, 300, 60, {}, False),
    (2, 1500, 400, {}, False),
    (3, 1000, 300, {"bypass": 0.0}, False),
    (4, 1200, 500, {"minor": 0.3, "major": 0.9, "bypass": 0.3}, True),
    # few units over long lists: a block of 256 ranks whose unit windows span more list entries than the LDS
    # window holds takes the LEF-BAR sweep's fall-back (per-unit searches in the list in device memory)
    (6, 40, 3000, {"minor": 1.0}, False),   # one block spans both lists (about 2 400 entries each)
    (7, 300, 6000, {"minor": 1.0}, False),  # a block that falls back, then 44 ranks that restage the window
    (8, 40, 3000, {}, False),               # default probabilities: the two lists differ
]
SEQUENCES += NEAR_LIMIT_SEQUENCES


@pytest.mark.parametrize("seed,n,nb,kw,dense", SEQUENCES)
def test_random_phases_emulated(oracle, seed, n, nb, kw, dense):
    run_sequences(oracle, emu_phases, seed, n, nb, kw, dense)


@pytest.mark.parametrize("seed,n,nb,kw,dense", SEQUENCES)
def test_random_phases_emulated_12_wave_geometry(oracle, seed, n, nb, kw, dense):
    run_sequences(oracle, functools.partial(emu_phases, geometry="w12"), seed, n, nb, kw, dense)
