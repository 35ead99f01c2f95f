"""The same differential test as tests/test_gpu_fuzz_parity.py with the device code running under
the CPU lane emulator (one cell per set-up: the emulator is slow), in the emulator builds with the
geometry of the 8-wave kernels and with that of the 12-wave ones (a set-up of the WIDE size class
resolves to the WIDE build of the same geometry, emu_sim.simulate_interval)."""
import pytest

import emu_sim
from fuzz_cases import random_case, random_case_v2, random_case_v3, random_case_v4, random_case_v5
from modle_amd import api
from parity_cases import assert_same_outputs, assert_same_results


# (790172: round 4 -- 70 re-inserted units of 395 with displaced units listed by other lanes than the ones that
# initialise their counts: a read-modify-write of LDS across lanes without a barrier in between.  The GPU
# executes a wave's LDS operations in order and never saw it; the emulator runs the lanes one after the
# other and crashed in the release that followed the broken rank order)
SEEDS_V1 = [100, 101, 105, 108, 1148, 790172]
SEEDS_V2 = [4, 5, 6, 8]
SEEDS_V3 = [1, 2, 3, 4, 5, 6]
SEEDS_V4 = [3, 7, 11, 36, 52]
SEEDS_V5 = [57, 112, 135, 8, 19, 15, 13]


@pytest.mark.parametrize("seed", SEEDS_V1)
def test_emulated_device_code_matches_oracle_on_random_setups(oracle, seed):
    _compare(oracle, random_case(seed), f"seed {seed}")


@pytest.mark.parametrize("seed", SEEDS_V2)
def test_emulated_device_code_matches_oracle_on_random_setups_v2(oracle, seed):
    _compare(oracle, random_case_v2(seed), f"v2 seed {seed}")


@pytest.mark.parametrize("seed", SEEDS_V3)
def test_emulated_device_code_matches_oracle_on_random_setups_v3(oracle, seed):
    _compare(oracle, random_case_v3(seed), f"v3 seed {seed}")


@pytest.mark.parametrize("seed", SEEDS_V4)
def test_emulated_device_code_matches_oracle_on_random_setups_v4(oracle, seed):
    """burn-in parameters, stopping rules, zero release probabilities (fuzz_cases.random_case_v4)"""
    _compare(oracle, random_case_v4(seed), f"v4 seed {seed}")


@pytest.mark.parametrize("seed", SEEDS_V5)
def test_emulated_device_code_matches_oracle_on_random_setups_v5(oracle, seed):
    """the top of the NARROW class's move and id ranges, both sides of the size-class rule's border
    (fuzz_cases.random_case_v5).  Seeds 57, 112 and 135 (rev / fwd speeds of 5 kb / 62.8 kb with 1 500 LEFs,
    5 kb / 64.6 kb with 531, 65.1 kb / 5 kb with 40) gave other numbers than the oracle on the device code as it
    was: the rule classed them NARROW and a unit put next to a barrier-stalled one moved more than 16 bits hold.
    They are WIDE now; 8, 15 and 19 sit on the rule's border."""
    _compare(oracle, random_case_v5(seed), f"v5 seed {seed}")


# --- the same seeds with the geometry of the 12-wave kernels ------------------------------------
@pytest.mark.parametrize("seed", SEEDS_V1)
def test_emulated_12_wave_geometry_matches_oracle_on_random_setups(oracle, seed):
    _compare(oracle, random_case(seed), f"12-wave geometry, seed {seed}", variant="w12")


@pytest.mark.parametrize("seed", SEEDS_V2)
def test_emulated_12_wave_geometry_matches_oracle_on_random_setups_v2(oracle, seed):
    _compare(oracle, random_case_v2(seed), f"12-wave geometry, v2 seed {seed}", variant="w12")


@pytest.mark.parametrize("seed", SEEDS_V3)
def test_emulated_12_wave_geometry_matches_oracle_on_random_setups_v3(oracle, seed):
    _compare(oracle, random_case_v3(seed), f"12-wave geometry, v3 seed {seed}", variant="w12")


@pytest.mark.parametrize("seed", SEEDS_V4)
def test_emulated_12_wave_geometry_matches_oracle_on_random_setups_v4(oracle, seed):
    _compare(oracle, random_case_v4(seed), f"12-wave geometry, v4 seed {seed}", variant="w12")


@pytest.mark.parametrize("seed", SEEDS_V5)
def test_emulated_12_wave_geometry_matches_oracle_on_random_setups_v5(oracle, seed):
    _compare(oracle, random_case_v5(seed), f"12-wave geometry, v5 seed {seed}", variant="w12")


def test_a_rank_reported_for_an_id_that_shares_its_filter_bit_carries_no_stall_flag(oracle):
    """v5 seed 30, cell 3 (45 000 LEFs, 15 kb / 5 kb per epoch, burn-in): found on the GPU, in both size classes.
    With more LEFs than the LDS id filter has bits, the extrusion sweep reports the rank of every id that shares its
    bit with a release candidate, hard-stall flag included; only the candidates' entries had the flag taken off
    again, and a hard-stalled bystander kept `rank | 0x80000000` in the inverse permutation.  The cell drew 44
    raws more than the oracle's in epoch 28.  The burn-in is cut there and the cell ends at its first contact."""
    case = random_case_v5(30)
    cfg, chrom = case["cfg"], case["chrom"]
    assert case["tasks"][0].num_lefs == 45000
    cfg.max_burnin_epochs = 28
    tasks = api.slice_tasks(case["tasks"], 3, 4)
    tasks[0].num_target_contacts = 1
    track = bool(cfg.track_1d_lef_position)
    oc, om, oo, ores = oracle.simulate_interval(
        cfg, chrom["start"], chrom["end"], chrom["bar_pos"], chrom["bar_dir"],
        case["stp_active"], case["stp_inactive"], tasks, nthreads=1, track_occupancy=track)
    assert ores[0].burnin_epochs == 29 and ores[0].raws_consumed == 2037147
    ec, em, eo, eres = emu_sim.simulate_interval(
        cfg, chrom["start"], chrom["end"], chrom["bar_pos"], chrom["bar_dir"], case["stp_active"],
        case["stp_inactive"], tasks, case["nrows"], case["ncols"], track_occupancy=track)
    assert_same_results(ores, eres, "v5 seed 30, cell 3")
    assert_same_outputs((oc, om, oo), (ec, em, eo), "v5 seed 30, cell 3")


def _compare(oracle, case, label, variant=None):
    cfg, chrom = case["cfg"], case["chrom"]
    tasks = api.slice_tasks(case["tasks"], 0, 1)
    track = bool(cfg.track_1d_lef_position)
    oc, om, oo, ores = oracle.simulate_interval(
        cfg, chrom["start"], chrom["end"], chrom["bar_pos"], chrom["bar_dir"],
        case["stp_active"], case["stp_inactive"], tasks, nthreads=1, track_occupancy=track)
    ec, em, eo, eres = emu_sim.simulate_interval(
        cfg, chrom["start"], chrom["end"], chrom["bar_pos"], chrom["bar_dir"], case["stp_active"],
        case["stp_inactive"], tasks, case["nrows"], case["ncols"], track_occupancy=track, variant=variant)
    what = f"{label}: {case['kw']}, size {case['size']}"
    assert_same_results(ores, eres, what)
    assert_same_outputs((oc, om, oo), (ec, em, eo), what)
