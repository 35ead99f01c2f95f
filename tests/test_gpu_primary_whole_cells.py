"""Whole cells against the oracle, word for word, on shapes picked for pass 1 of primary LEF-LEF detection
(modle_amd/csrc/sim_collisions.h: blocks of 256 rev ranks, a short search below the unit's own rank with two
fall-backs) and for the burn-in stability test on a short history (sim_burnin.h).

One 2 Mb interval with its ~20 barriers:

  * 257 and 513 LEFs (one unit past one and two blocks of 256), 128 and 256 LEFs per Mb: dense enough for loops
    to nest as they grow during the burn-in.  (How deep they nest is not asserted here; the searches a given
    depth takes are asserted on the emulator's trace in test_emu_primary_blocks.py.);
  * 257 LEFs with burnin_history_length = 8 and burnin_smoothing_window_size = 2: the history ring wraps
    every 8 epochs of a burn-in that lasts hundreds.

`test_cases_have_the_shapes` asserts the LEF counts and the length of the burn-in on the oracle's results.
Every launch mode of parity_cases.launch_modes runs every case: matrices, occupancy, prng_final,
raws_consumed, epochs.
"""
import pytest

from parity_cases import (assert_launch_mode, assert_same_outputs, assert_same_results, describe_launch,
                          launch_modes)

NCELLS = 12
CASES = {
    "lefs257": dict(lefs=257, cfg=dict(number_of_lefs_per_mbp=128.5)),
    "lefs513": dict(lefs=513, cfg=dict(number_of_lefs_per_mbp=256.5)),
    "lefs257_history8": dict(lefs=257, cfg=dict(number_of_lefs_per_mbp=128.5, burnin_history_length=8,
                                                burnin_smoothing_window_size=2)),
}

_cache = {}


def _case(oracle, name):
    """the inputs of a case and the oracle's outputs for it (computed once, never modified)"""
    if name not in _cache:
        from modle_amd import api, synthetic

        spec = CASES[name]
        cfg = api.make_config(num_cells=NCELLS, target_contact_density=0.05, max_burnin_epochs=400, seed=5,
                              **spec["cfg"])
        chrom = synthetic.synthetic_chromosome("chrT", 2_000_000, with_barriers=True)
        stp_active, stp_inactive = api.barrier_stps(cfg, chrom["bar_occupancy"])
        tasks = api.make_tasks(cfg, chrom["name"], chrom["size"], chrom["start"], chrom["end"])
        assert len(tasks) == NCELLS
        expected = oracle.simulate_interval(cfg, chrom["start"], chrom["end"], chrom["bar_pos"], chrom["bar_dir"],
                                            stp_active, stp_inactive, tasks, nthreads=4,
                                            track_occupancy=bool(cfg.track_1d_lef_position))
        _cache[name] = dict(cfg=cfg, chrom=chrom, stp_active=stp_active, stp_inactive=stp_inactive, tasks=tasks,
                            expected=expected)
    return _cache[name]


@pytest.mark.parametrize("name", list(CASES))
def test_cases_have_the_shapes(oracle, name):
    case = _case(oracle, name)
    assert all(int(t.num_lefs) == CASES[name]["lefs"] for t in case["tasks"])
    assert 15 <= len(case["chrom"]["bar_pos"]) <= 30
    burnin = [int(r.burnin_epochs) for r in case["expected"][3]]
    print(name, "burn-in epochs:", sorted(burnin), "epochs:", sorted(int(r.epochs) for r in case["expected"][3]))
    cap = int(case["cfg"].burnin_history_length)
    # the statistics start once every LEF is active; the history then fills and its ring wraps
    assert min(burnin) > 3 * cap if cap == 8 else min(burnin) > cap


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_gpu_matches_oracle_in_every_launch_mode(oracle, name):
    from modle_amd import api

    case = _case(oracle, name)
    cfg, chrom = case["cfg"], case["chrom"]
    oc, om, oo, ores = case["expected"]
    modes = []
    for mode in launch_modes(NCELLS):
        sim = api.Simulator(cfg, 0)
        try:
            sim.set_wait_timeout(60.0)
            gc, gm, go, gres = sim.simulate_interval(
                chrom["start"], chrom["end"], chrom["bar_pos"], chrom["bar_dir"], case["stp_active"],
                case["stp_inactive"], case["tasks"])
            info = sim.launch_info()
        finally:
            sim.close()
        print(f"{name}: launch mode {mode}: {describe_launch(info)}")
        assert_launch_mode(info, mode, NCELLS)
        assert_same_results(ores, gres, f"{name}, launch mode {mode}")
        if not cfg.track_1d_lef_position:
            go = None
        assert_same_outputs((oc, om, oo), (gc, gm, go), f"{name}, launch mode {mode}")
        modes.append(mode)
    assert modes == ["0", "1", "12", "12packed"]
