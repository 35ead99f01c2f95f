"""Pass 1 of primary LEF-LEF detection on the GPU (modle_hip_test_phases) against the oracle at the smallest
shapes at which its blocks of 256 rev ranks, its short search and its two fall-backs can go wrong
(tests/primary_block_cases.py)."""
import pytest

import primary_block_cases as pc
from phase_backend import _advance

pytestmark = pytest.mark.gpu
NEAR, BACK = 16, 128  # modle_amd/csrc/sim_collisions.h: MODLE_PRIMARY_NEAR, MODLE_PRIMARY_BACK


@pytest.fixture(scope="module")
def gpu_phases():
    from modle_amd import api

    sims = {}

    def phases(cfg, mask, st, state, skip):
        key = bytes(cfg)
        if key not in sims:
            sims[key] = api.Simulator(cfg.copy(), 0)
        return sims[key].test_phases(mask, st, _advance(state, skip))

    yield phases
    for s in sims.values():
        s.close()


def test_block_boundaries_and_boundary_counts(oracle, gpu_phases):
    hits = 0
    for n, n5, n3 in pc.boundary_cases():
        st = pc.at_boundaries(pc.plain_state(n, seed=n), n5, n3)
        hits += pc.check_primary(oracle, gpu_phases, st, expect_counts=(n5, min(n3, n - 1)))  # (the fwd unit of rank 0 is never counted)
    assert hits > 1000  # (the moves make many neighbours meet)


@pytest.mark.parametrize("n,k,depth,rest,device", pc.depth_cases(NEAR, BACK))
def test_nested_loops_take_the_three_searches(oracle, gpu_phases, n, k, depth, rest, device):
    """(which search the units of a case take is asserted on the emulator's trace: test_emu_primary_blocks.py)"""
    assert pc.check_primary(oracle, gpu_phases, pc.nested(pc.plain_state(n, seed=depth), k, depth)) > 100


@pytest.mark.parametrize("bypass", [0.0, 0.3, 1.0])
def test_draw_order_and_special_layouts(oracle, gpu_phases, bypass):
    pc.check_primary(oracle, gpu_phases, pc.plain_state(513, seed=3), bypass)
    pc.check_primary(oracle, gpu_phases, pc.all_rev_upstream(513), bypass)
    pc.check_primary(oracle, gpu_phases, pc.released_tail(pc.plain_state(513, seed=4), 20), bypass)
    pc.check_primary(oracle, gpu_phases, pc.released_tail(pc.nested(pc.plain_state(700, seed=5), 400, 40), 150), bypass)
    pc.check_primary(oracle, gpu_phases, pc.equal_positions(pc.plain_state(385, seed=6)), bypass)
