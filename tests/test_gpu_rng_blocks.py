"""The block logic of the PRNG generator (modle_amd/csrc/sim_rng.h: rng_gen_block_call, rng_hop,
rng_final_state) at its smallest, on whole cells against the oracle.

One 2 Mb interval, 40 LEFs, 25 barriers, no burn-in, stopped after a fixed number of epochs: a cell
draws ~220 raw outputs per epoch, so 8 and 14 epochs consume more than three pairs of blocks (1 536
raws: both ring halves wrap, states are parked and taken back several times) and end

  * seed 198,  8 epochs: between 1 719 and 1 794 raws -- in the first block of a pair (block 6 of 256),
    in the second (block 7 after 1 792), and one cell exactly at 1 792 = 7 x 256, a block boundary inside a pair;
  * seed  61, 14 epochs: between 3 015 and 3 089 raws -- in the second block of a pair, in the first,
    and three cells exactly at 3 072 = 6 x 512, a pair boundary (and a block boundary of the 8-wave
    kernels, whose blocks hold 512).

The boundaries are the two branches of rng_final_state.  The seeds were found by running the oracle
over seeds 1-199; `test_cases_cover_the_block_positions` asserts the coverage on the oracle's
raws_consumed, so a change of the model that moves the cells off these positions fails there instead
of letting the comparison pass on less.

Every cell runs in every launch mode of parity_cases.launch_modes; with 12 cells "12packed" puts
twelve waves side by side on one jump table.  raws_consumed, prng_final, the counters and every output
word are compared.
"""
import pytest

from parity_cases import (assert_launch_mode, assert_same_outputs, assert_same_results, describe_launch,
                          launch_modes)

NCELLS = 12
BLOCK12 = 256   # RNG_BLOCK of the 12-wave kernels (two blocks per hop: a pair is 512)
BLOCK8 = 512    # RNG_BLOCK of the 8-wave kernels
CASES = {"seed198_8epochs": dict(seed=198, epochs=8), "seed61_14epochs": dict(seed=61, epochs=14)}

_cache = {}


def _case(oracle, name):
    """the inputs of a case and the oracle's outputs for it (computed once, never modified)"""
    if name not in _cache:
        from modle_amd import api, synthetic

        spec = CASES[name]
        cfg = api.make_config(num_cells=NCELLS, target_contact_density=-1.0,
                              target_simulation_epochs=spec["epochs"], skip_burnin=1,
                              number_of_lefs_per_mbp=20.0, seed=spec["seed"])
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


def test_cases_cover_the_block_positions(oracle):
    raws = [int(r.raws_consumed) for name in CASES for r in _case(oracle, name)["expected"][3]]
    print("raws_consumed:", sorted(raws))
    assert len(raws) == NCELLS * len(CASES)
    # more than three pairs of blocks: both ring halves wrap, states are parked and taken back
    assert min(raws) > 3 * 2 * BLOCK12
    inside = [x for x in raws if x % BLOCK12 != 0]
    assert any((x // BLOCK12) % 2 == 0 for x in inside), "no cell ends in the first block of a pair"
    assert any((x // BLOCK12) % 2 == 1 for x in inside), "no cell ends in the second block of a pair"
    assert any(x % (2 * BLOCK12) == BLOCK12 for x in raws), "no cell ends on a block boundary inside a pair"
    assert any(x % (2 * BLOCK12) == 0 for x in raws), "no cell ends on a pair boundary"
    # the 8-wave kernels: both ring halves, and a block boundary
    inside8 = [x for x in raws if x % BLOCK8 != 0]
    assert {(x // BLOCK8) % 2 for x in inside8} == {0, 1}, "8-wave kernels: a ring half is never the last one"
    assert any(x % BLOCK8 == 0 for x in raws), "8-wave kernels: no cell ends on a block boundary"


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
