"""A launch is laid out as `api.plan_launch` says (modle_host::plan_launch is what modle_hip_launch calls).

Six cells of the recorded table (tests/golden/launch_plans.json, tools/launch_plans.py), one per layout: every wave
a main wave, fixed roles with and without the PRNG producer, 12 waves per workgroup by the rule and by name, the
WIDE class by name.  Each is launched again as it was recorded, and `Simulator.launch_info()` -- without the
three fields that describe the workspace's placement -- must equal the plan for this device's compute units."""
import pytest

from tools.launch_plans import CASES, geometry, layout_env, run_case

pytestmark = pytest.mark.gpu

LAYOUTS = {"tasks9": "every wave a main wave", "tasks3": "1 to 2 main waves, helper and PRNG producer",
           "tasks8": "3 to 4 main waves and their helpers", "tasks24": "12 waves by the rule",
           "tasks9_waves12": "12 waves by name", "tasks9_wide": "WIDE by name"}


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_the_launch_is_the_plan(name):
    from modle_amd import api
    from tools.launch_plans import case_config

    case = next(c for c in CASES if c["name"] == name)
    entry = run_case(case, wait_timeout_s=120.0)  # (set_wait_timeout on its simulator)
    info = entry["info"]
    with layout_env(case["env"]):
        plan = api.plan_launch(case_config(case), entry["n_tasks"], info["num_cus"], entry["max_lefs"])
    assert geometry(info) == geometry(plan), LAYOUTS[name]
    expect = {"tasks9": (8, 8, 0, 0, 1, 0), "tasks3": (8, 2, 1, 1, 0, 0), "tasks8": (8, 4, 1, 0, 0, 0),
              "tasks24": (12, 12, 0, 0, 1, 0), "tasks9_waves12": (12, 12, 0, 0, 1, 0),
              "tasks9_wide": (8, 8, 0, 0, 1, 1)}[name]
    assert (info["waves_per_workgroup"], info["main_waves_per_workgroup"], info["helper_waves"],
            info["prng_producer_waves"], info["tail_helpers"], info["size_class"]) == expect, LAYOUTS[name]
    assert info["workgroups"] == 2 and info["n_tasks"] == entry["n_tasks"]
