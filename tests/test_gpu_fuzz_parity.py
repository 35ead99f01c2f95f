"""Differential test on the GPU over seeded random set-ups (sizes, LEF densities, bypass / block
probabilities, stall multipliers, sampling strategies, resolutions): every output word and every
per-cell counter of the HIP path must equal the oracle's."""
import pytest

from fuzz_cases import random_case, random_case_v2, random_case_v3, random_case_v4, random_case_v5
from parity_cases import assert_launch_mode, assert_same_outputs, assert_same_results, launch_modes

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", list(range(100, 116)) + [1121, 1148, 1178, 5482, 5645, 6024])
def test_gpu_matches_oracle_on_random_setups(oracle, seed):
    _compare(oracle, random_case(seed), f"seed {seed}")


@pytest.mark.parametrize("seed", list(range(1, 13)))
def test_gpu_matches_oracle_on_random_setups_v2(oracle, seed):
    """wider generator: windows that do not start at 0, barrier density, speeds, noise, ..."""
    _compare(oracle, random_case_v2(seed), f"v2 seed {seed}")


@pytest.mark.parametrize("seed", list(range(1, 17)))
def test_gpu_matches_oracle_on_random_setups_v3(oracle, seed):
    """blocking probabilities in {0, 1}: the compacted-barrier path of LEF-BAR detection"""
    _compare(oracle, random_case_v3(seed), f"v3 seed {seed}")


@pytest.mark.parametrize("seed", list(range(1, 17)))
def test_gpu_matches_oracle_on_random_setups_v4(oracle, seed):
    """burn-in parameters (minimum length, history, smoothing window, activation ramp), stopping on
    epochs with burn-in, TAD-to-loop ratio at its extremes, release probabilities of exactly zero"""
    _compare(oracle, random_case_v4(seed), f"v4 seed {seed}")


@pytest.mark.parametrize("seed", [57, 112, 135, 8, 19, 15, 13, 30, 7, 9])
def test_gpu_matches_oracle_on_random_setups_v5(oracle, seed):
    """the top of the NARROW class's 16-bit move and id ranges: unequal speeds up to 65 kb per epoch, tens of
    thousands of LEFs, both sides of the size-class rule's border, each in the class the library picks.  Seeds 57,
    112 and 135 gave other numbers than the oracle on the emulated device code as it was (see
    test_emu_fuzz_parity.py); 8, 15, 19 and 30 sit on the rule's border, 30 with 45 000 LEFs through a burn-in."""
    _compare(oracle, random_case_v5(seed), f"v5 seed {seed}")


def _compare(oracle, case, label, modes=None):
    """the oracle once, the launch in every mode of parity_cases.launch_modes (12 cells: also with the twelve of them
    side by side in one 12-wave workgroup), or in those of them that `modes` names"""
    from modle_amd import api

    cfg, chrom = case["cfg"], case["chrom"]
    tasks = api.slice_tasks(case["tasks"], 0, min(12, len(case["tasks"])))
    track = bool(cfg.track_1d_lef_position)
    oc, om, oo, ores = oracle.simulate_interval(
        cfg, chrom["start"], chrom["end"], chrom["bar_pos"], chrom["bar_dir"],
        case["stp_active"], case["stp_inactive"], tasks, nthreads=8, track_occupancy=track)
    for mode in launch_modes(len(tasks)):
        if modes is not None and mode not in modes:
            continue
        sim = api.Simulator(cfg, 0)
        try:
            sim.set_wait_timeout(300.0)
            gc, gm, go, gres = sim.simulate_interval(
                chrom["start"], chrom["end"], chrom["bar_pos"], chrom["bar_dir"], case["stp_active"],
                case["stp_inactive"], tasks)
            info = sim.launch_info()
        finally:
            sim.close()
        what = f"{label} (launch mode {mode}): {case['kw']}, size {case['size']}"
        assert_launch_mode(info, mode, len(tasks))
        assert_same_results(ores, gres, what)
        assert_same_outputs((oc, om, oo), (gc, gm, go if track else None), what)


# --- seeds nobody has seen yet ---------------------------------------------------------
# The seeds above are the committed regression set: every run of the suite repeats them.  These take up to 64
# seeds per generator from the DATE of the run (MODLE_FUZZ_DATE=YYYYMMDD reproduces a day), so that the driver's
# round-end run and every builder run in between cover set-ups no campaign has visited.  A generator's share of
# the suite is bounded in time (the oracle runs on the host): it reports how many seeds it compared.
FRESH_SEEDS_PER_GENERATOR = 64
FRESH_BUDGET_S = 60.0


def _date_base():
    import datetime
    import os

    day = os.environ.get("MODLE_FUZZ_DATE") or datetime.date.today().strftime("%Y%m%d")
    return int(day) * 1000


@pytest.mark.parametrize("name", ["v1", "v2", "v3", "v4", "v5"])
def test_gpu_matches_oracle_on_seeds_of_the_day(oracle, name):
    import time

    from modle_amd import api

    gen = {"v1": random_case, "v2": random_case_v2, "v3": random_case_v3, "v4": random_case_v4,
           "v5": random_case_v5}[name]
    base = _date_base()
    t0 = time.time()
    done = skipped = 0
    # (v5's cells have up to 45 000 LEFs and the oracle runs twelve of them per seed: a quarter of the seeds)
    for i in range(FRESH_SEEDS_PER_GENERATOR // 4 if name == "v5" else FRESH_SEEDS_PER_GENERATOR):
        if time.time() - t0 > FRESH_BUDGET_S:
            break
        seed = base + i
        case = gen(seed)
        cfg = case["cfg"]
        # (keep the oracle's share short, like tools/fuzz_campaign.py: skip set-ups whose cells need many epochs)
        per_epoch = max(1, api.compute_contacts_per_epoch(cfg, case["tasks"][0].num_lefs))
        if cfg.target_contact_density >= 0 and case["tasks"][0].num_target_contacts / per_epoch > 3000:
            skipped += 1
            continue
        # (both modes of the 8-wave kernels for every seed, the 12-wave kernels for every other one: one more
        # small launch against an oracle run per seed)
        _compare(oracle, case, f"{name} seed of the day {seed} (MODLE_FUZZ_DATE={base // 1000})",
                 modes=("0", "1", "12") if seed % 2 == 1 else ("0", "1"))
        done += 1
    print(f"{name}: {done} fresh seeds from {base} compared in both launch modes (odd seeds: with the 12-wave kernels "
          f"too), {skipped} skipped (long cells), "
          f"{time.time() - t0:.0f} s")
    assert done >= 8, f"only {done} fresh seeds fitted the time budget"
