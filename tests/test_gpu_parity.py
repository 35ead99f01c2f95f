"""Whole-cell parity on the real GPU: the HIP path (through the C ABI) must reproduce the CPU
oracle bit for bit -- every word of the band contact matrix, the 1-D occupancy track, the
missed-update counter and per-cell (epochs, burn-in epochs, contacts, PRNG outputs drawn)."""
import numpy as np
import pytest

from parity_cases import (CASES, assert_launch_mode, assert_same_outputs, assert_same_results, build_case,
                          describe_launch, launch_modes)

pytestmark = pytest.mark.gpu

# cells compared per case (the oracle runs them on the host cores of the GPU box).  A case with at least
# 12 cells also runs with all twelve waves of a 12-wave workgroup simulating a cell at once (launch mode
# "12packed" of parity_cases.launch_modes): the cases whose epochs overflow the halved LDS buffers of the
# 12-wave kernels (mass_release, the rebind cases, dense_stress) have 12 cells for that reason.
NCELLS = {"config0_5mb_nobarriers": 64, "chr20mb_barriers": 96, "chr12mb_dense_softstall": 64,
          "chr8mb_loop_only": 64, "chr6mb_skip_burnin": 64, "tiny_single_lef": 8,
          "zero_target_cells": 128, "epochs_stop_tad_only": 16, "window_near_position_limit": 64,
          "dense_barriers_trials": 8, "ultra_dense_barriers_trials": 4, "mass_release": 12,
          "many_lefs_hashed_filters": 2, "many_rebinds_per_epoch": 12,
          "rebinds_beyond_sort_buffer": 12, "rebinds_beyond_sort_buffer_burnin": 12,
          "dense_stress_rebinds_and_displaced": 12,
          "burnin_three_windows": 12}


@pytest.mark.parametrize("name", list(CASES))
def test_gpu_matches_oracle(oracle, name):
    from modle_amd import api

    # (a case defined with fewer cells than are compared here is built with more cells of the same kind)
    case = build_case(name, num_cells=max(NCELLS[name], CASES[name]["cfg"]["num_cells"]))
    cfg, chrom = case["cfg"], case["chrom"]
    n = min(NCELLS[name], len(case["tasks"]))
    assert n == NCELLS[name]
    tasks = api.slice_tasks(case["tasks"], 0, n)
    oc, om, oo, ores = oracle.simulate_interval(
        cfg, chrom["start"], chrom["end"], chrom["bar_pos"], chrom["bar_dir"],
        case["stp_active"], case["stp_inactive"], tasks, nthreads=8,
        track_occupancy=bool(cfg.track_1d_lef_position))
    for mode in launch_modes(n):
        sim = api.Simulator(cfg, 0)
        try:
            sim.set_wait_timeout(300.0)
            gc, gm, go, gres = sim.simulate_interval(
                chrom["start"], chrom["end"], chrom["bar_pos"], chrom["bar_dir"], case["stp_active"],
                case["stp_inactive"], tasks)
            info = sim.launch_info()
        finally:
            sim.close()
        print(f"{name}: launch mode {mode}: {describe_launch(info)}")
        assert_launch_mode(info, mode, n)
        assert_same_results(ores, gres, f"{name}, launch mode {mode}")
        if not cfg.track_1d_lef_position:
            go = None
        assert_same_outputs((oc, om, oo), (gc, gm, go), f"{name}, launch mode {mode}")
    assert int(oc.sum()) + om == sum(r.num_contacts for r in ores)


def test_gpu_queue_api_matches_one_call(oracle):
    """add_interval/submit/launch/wait with two intervals in one launch == per-interval runs."""
    from modle_amd import api

    a, b = build_case("config0_5mb_nobarriers"), build_case("chr8mb_loop_only")
    assert a["cfg"].contact_sampling_strategy != b["cfg"].contact_sampling_strategy
    # both intervals must share one Config: rebuild b's tasks under a's config
    cfg = a["cfg"]
    chrom_b = b["chrom"]
    stp_a, stp_i = api.barrier_stps(cfg, chrom_b["bar_occupancy"])
    tasks_b = api.make_tasks(cfg, "chrU", chrom_b["size"], 0, chrom_b["size"])
    ta = api.slice_tasks(a["tasks"], 0, 24)
    tb = api.slice_tasks(tasks_b, 0, 24)
    sim = api.Simulator(cfg, 0)
    try:
        ia = sim.add_interval(0, a["chrom"]["size"], a["chrom"]["bar_pos"], a["chrom"]["bar_dir"],
                              a["stp_active"], a["stp_inactive"])
        ib = sim.add_interval(0, chrom_b["size"], chrom_b["bar_pos"], chrom_b["bar_dir"], stp_a,
                              stp_i)
        sim.submit(ia, ta)
        sim.submit(ib, tb)
        sim.launch()
        sim.wait()
        assert sim.kernel_ms() > 0
        out_a, out_b = sim.copy_outputs(ia), sim.copy_outputs(ib)
        res_a, res_b = sim.results(ia), sim.results(ib)
    finally:
        sim.close()
    for chrom, stps, tasks, out, res in ((a["chrom"], (a["stp_active"], a["stp_inactive"]), ta,
                                          out_a, res_a),
                                         (chrom_b, (stp_a, stp_i), tb, out_b, res_b)):
        oc, om, oo, ores = oracle.simulate_interval(cfg, 0, chrom["size"], chrom["bar_pos"],
                                                    chrom["bar_dir"], stps[0], stps[1], tasks,
                                                    nthreads=8)
        assert_same_results(ores, res, "queue api")
        assert_same_outputs((oc, om, oo), out, "queue api")
