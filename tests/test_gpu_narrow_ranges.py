"""The NARROW kernels at the top of their 16-bit move and id ranges (narrow_range_cases.py) on the real GPU
against the oracle, in every launch mode, in the class the library picks -- NARROW for the NARROW cases of the
table, nothing forced -- and once more with WIDE forced.  The cases the corrected rule moved to the WIDE class
run in it (see narrow_range_cases.py; the emulator tests run the NARROW device code on them)."""
import pytest

import narrow_range_cases as nrc
from parity_cases import (assert_launch_mode, assert_same_outputs, assert_same_results, describe_launch,
                          launch_modes)

pytestmark = pytest.mark.gpu


def _ncells(name):
    # 12: the launch modes "12" with all twelve waves busy and "12packed" are included
    return {"lefs_60000_skip_burnin": 2, "lefs_60000_burnin": 2, "lefs_65500_burnin": 1}.get(name, 12)


def _launch(api, case, tasks):
    cfg, ch = case["cfg"], case["chrom"]
    sim = api.Simulator(cfg, 0)
    try:
        sim.set_wait_timeout(300.0)
        gc, gm, go, gres = sim.simulate_interval(ch["start"], ch["end"], ch["bar_pos"], ch["bar_dir"],
                                                 case["stp_active"], case["stp_inactive"], tasks)
        info = sim.launch_info()
    finally:
        sim.close()
    return (gc, gm, go if cfg.track_1d_lef_position else None), gres, info


@pytest.mark.parametrize("name", list(nrc.CASES))
def test_gpu_matches_oracle_at_the_top_of_the_narrow_ranges(oracle, monkeypatch, name):
    from modle_amd import api

    monkeypatch.delenv("MODLE_HIP_SIZE_CLASS", raising=False)
    n = _ncells(name)
    case = nrc.build(name, num_cells=n)
    cfg, ch = case["cfg"], case["chrom"]
    tasks = api.slice_tasks(case["tasks"], 0, n)
    assert len(case["tasks"]) == n
    oc, om, oo, ores = oracle.simulate_interval(cfg, ch["start"], ch["end"], ch["bar_pos"], ch["bar_dir"],
                                                case["stp_active"], case["stp_inactive"], tasks, nthreads=8,
                                                track_occupancy=bool(cfg.track_1d_lef_position))
    nrc.assert_oracle_result(case, ores, name)
    expect = 0 if case["narrow"] else 1
    for mode in launch_modes(n):
        out, gres, info = _launch(api, case, tasks)
        print(f"{name}: launch mode {mode}: {describe_launch(info)}, size_class {info['size_class']}")
        assert_launch_mode(info, mode, n)
        assert info["size_class"] == expect, info
        assert_same_results(ores, gres, f"{name}, launch mode {mode}")
        assert_same_outputs((oc, om, oo), out, f"{name}, launch mode {mode}")
    if case["narrow"]:
        monkeypatch.setenv("MODLE_HIP_SIZE_CLASS", "wide")
        out, gres, info = _launch(api, case, tasks)
        print(f"{name}: WIDE forced: {describe_launch(info)}, size_class {info['size_class']}")
        assert info["size_class"] == 1, info
        assert_same_results(ores, gres, f"{name}, WIDE forced")
        assert_same_outputs((oc, om, oo), out, f"{name}, WIDE forced")
