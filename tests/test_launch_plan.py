"""The launch rule (`modle_host::plan_launch`, modle_amd/csrc/launch_common.hpp) without a device.

`api.plan_launch` is the rule as a launch applies it: the same function, the same read of the environment, the
same build switches.  It is held to

 - `tests/golden/launch_plans.json`: what `Simulator.launch_info()` said after real launches of the library as it
   was before the rule became one function (tools/launch_plans.py recorded them), field for field;
 - the rule as the documentation states it (restated in `_rule` below) at sizes no test
   launch reaches cheaply: the thresholds of a whole device, one compute unit, fewer tasks than compute units."""
import itertools
import json

import pytest

from tools.launch_plans import GOLDEN, WORKSPACE_FIELDS, geometry, layout_env

with open(GOLDEN) as f:
    ENTRIES = json.load(f)


def _plan(config, n_tasks, num_cus, max_lefs, env):
    from modle_amd import api

    with layout_env(env):
        return api.plan_launch(api.make_config(**config), n_tasks, num_cus, max_lefs)


def test_the_table_covers_the_rule():
    """(what the recording has to hold: the thresholds, every override, both sides of the re-insertion bound)"""
    names = {e["name"] for e in ENTRIES}
    assert len(names) == len(ENTRIES)
    plain = {e["n_tasks"] for e in ENTRIES if e["env"] == {"MODLE_HIP_GRID": "2"} and not e["config"]}
    assert plain == {1, 2, 3, 4, 5, 8, 9, 23, 24, 25}
    for value in ("0", "1", ""):
        assert {e["n_tasks"] for e in ENTRIES if e["env"].get("MODLE_HIP_PAIRED") == value
                and "MODLE_HIP_WAVES" not in e["env"]} == plain
    for var, values in (("MODLE_HIP_WAVES", ("8", "12")), ("MODLE_HIP_TAIL_HELPERS", ("0",)),
                        ("MODLE_HIP_ACTIVE_WAVES", ("0", "3", "13")), ("MODLE_HIP_SIZE_CLASS", ("wide",))):
        assert {e["env"][var] for e in ENTRIES if var in e["env"]} == set(values), var
    assert any(e["env"].get("MODLE_HIP_WAVES") == "12" and e["env"].get("MODLE_HIP_PAIRED") == "1" for e in ENTRIES)
    assert any("MODLE_HIP_GRID" not in e["env"] for e in ENTRIES)
    assert {e["max_lefs"] for e in ENTRIES if e["config"]} == {212, 213}
    assert not any("MODLE_HIP_TEST_FAULT" in e["env"] for e in ENTRIES)
    for e in ENTRIES:  # (every layout a launch can have shows)
        assert e["info"]["n_tasks"] == e["n_tasks"] and e["info"]["num_cus"] == e["num_cus"]
    seen = {(e["info"]["waves_per_workgroup"], e["info"]["helper_waves"], e["info"]["prng_producer_waves"],
             e["info"]["tail_helpers"], e["info"]["size_class"]) for e in ENTRIES}
    assert {(8, 1, 1, 0, 0), (8, 1, 0, 0, 0), (8, 0, 0, 1, 0), (8, 0, 0, 0, 0), (12, 0, 0, 1, 0), (12, 0, 0, 0, 0),
            (8, 0, 0, 1, 1), (12, 0, 0, 1, 1)} <= seen


@pytest.mark.parametrize("entry", ENTRIES, ids=[e["name"] for e in ENTRIES])
def test_the_plan_equals_the_recorded_launch(entry):
    plan = _plan(entry["config"], entry["n_tasks"], entry["num_cus"], entry["max_lefs"], entry["env"])
    assert geometry(plan) == geometry(entry["info"])
    assert all(plan[k] == 0 for k in WORKSPACE_FIELDS)  # (a plan places no workspace)


def _rule(n_tasks, num_cus, max_lefs, cfg, env, needs_wide=False):
    """The rule, from its text: grid, then waves, then fixed roles, tail helpers, active waves, producer."""
    def number(name):
        try:
            return int(env.get(name, "0").split()[0])
        except (ValueError, IndexError):
            return 0

    grid = max(1, min(num_cus, n_tasks))
    if number("MODLE_HIP_GRID") >= 1:
        grid = min(grid, number("MODLE_HIP_GRID"))
    waves = 8
    if n_tasks > grid * 4 and n_tasks >= grid * 12 and \
            max_lefs * max(cfg.prob_of_lef_release, cfg.prob_of_lef_release_burnin) < 170.0:
        waves = 12
    if number("MODLE_HIP_WAVES") in (8, 12):
        waves = number("MODLE_HIP_WAVES")
    forced = env.get("MODLE_HIP_PAIRED", "")
    if forced != "" and forced[0] != "0":
        waves = 8
    paired = waves == 8 and n_tasks <= grid * 4
    if forced != "":
        paired = forced[0] != "0"
    pair_mains = min(4, -(-n_tasks // grid)) if paired and waves == 8 else 0
    tail_helpers = 1 if pair_mains == 0 else 0
    if env.get("MODLE_HIP_TAIL_HELPERS", "")[:1] == "0":
        tail_helpers = 0
    active = waves
    if 1 <= number("MODLE_HIP_ACTIVE_WAVES") <= waves:
        active = number("MODLE_HIP_ACTIVE_WAVES")
    return {"n_tasks": n_tasks, "num_cus": num_cus, "workgroups": grid, "waves_per_workgroup": waves,
            "main_waves_per_workgroup": pair_mains if pair_mains else active,
            "helper_waves": 1 if pair_mains else 0,
            "prng_producer_waves": 1 if 1 <= pair_mains <= 2 else 0,
            "tail_helpers": tail_helpers,
            "size_class": 1 if needs_wide or env.get("MODLE_HIP_SIZE_CLASS", "")[:1] == "w" else 0}


ENVS = [{}, {"MODLE_HIP_PAIRED": "0"}, {"MODLE_HIP_PAIRED": "1"}, {"MODLE_HIP_PAIRED": ""},
        {"MODLE_HIP_WAVES": "8"}, {"MODLE_HIP_WAVES": "12"}, {"MODLE_HIP_WAVES": "10"},
        {"MODLE_HIP_WAVES": "12", "MODLE_HIP_PAIRED": "1"}, {"MODLE_HIP_WAVES": "12", "MODLE_HIP_PAIRED": "0"},
        {"MODLE_HIP_TAIL_HELPERS": "0"}, {"MODLE_HIP_TAIL_HELPERS": "1"},
        {"MODLE_HIP_ACTIVE_WAVES": "0"}, {"MODLE_HIP_ACTIVE_WAVES": "3"}, {"MODLE_HIP_ACTIVE_WAVES": "9"},
        {"MODLE_HIP_ACTIVE_WAVES": "13"}, {"MODLE_HIP_SIZE_CLASS": "wide"}, {"MODLE_HIP_SIZE_CLASS": "narrow"},
        {"MODLE_HIP_GRID": "0"}, {"MODLE_HIP_GRID": "100"}, {"MODLE_HIP_GRID": "1000"}]


def test_the_rule_restated_equals_the_recorded_launches():
    """(the restatement below is the rule the table was recorded from, before it is trusted at other sizes)"""
    from modle_amd import api

    for e in ENTRIES:
        cfg = api.make_config(**e["config"])
        assert _rule(e["n_tasks"], e["num_cus"], e["max_lefs"], cfg, e["env"]) == geometry(e["info"]), e["name"]


@pytest.mark.parametrize("num_cus,n_tasks", [(256, 1024), (256, 1025), (256, 3071), (256, 3072),  # a whole device
                                             (1, 1), (1, 4), (1, 5), (1, 11), (1, 12), (1, 13),  # one compute unit
                                             (256, 1), (256, 100), (256, 255), (256, 256), (256, 257),
                                             (256, 0), (304, 3647), (304, 3648)])
def test_the_rule_at_sizes_no_test_launch_reaches(num_cus, n_tasks):
    from modle_amd import api

    default = api.make_config()
    for env in ENVS:
        assert _plan({}, n_tasks, num_cus, 4979, env) == \
            dict(_rule(n_tasks, num_cus, 4979, default, env), **{k: 0 for k in WORKSPACE_FIELDS}), env
    # the re-insertion bound decides between 8 and 12 waves on a launch that fills the device, whichever of the two
    # release probabilities is the larger; a set-up that needs 32-bit ids is WIDE by itself
    busy = dict(avg_lef_processivity=10_000)  # (release probability 0.8)
    slow_burnin = dict(avg_lef_processivity=10_000, burnin_speed_coefficient=0.5)
    fast_burnin = dict(avg_lef_processivity=20_000, burnin_speed_coefficient=2.0)
    for config, max_lefs in itertools.product((busy, slow_burnin, fast_burnin), (212, 213)):
        cfg = api.make_config(**config)
        assert max(cfg.prob_of_lef_release, cfg.prob_of_lef_release_burnin) == pytest.approx(0.8, abs=1e-12)
        plan = _plan(config, n_tasks, num_cus, max_lefs, {})
        assert geometry(plan) == _rule(n_tasks, num_cus, max_lefs, cfg, {}), (config, max_lefs)
        if n_tasks >= 12 * num_cus:
            assert plan["waves_per_workgroup"] == (12 if max_lefs == 212 else 8)
    assert geometry(_plan({}, n_tasks, num_cus, 70_000, {})) == _rule(n_tasks, num_cus, 70_000, default, {}, True)


def test_the_environment_is_read_at_every_call(monkeypatch):
    from modle_amd import api

    cfg = api.make_config()
    for name in ("MODLE_HIP_GRID", "MODLE_HIP_WAVES", "MODLE_HIP_PAIRED"):
        monkeypatch.delenv(name, raising=False)
    assert api.plan_launch(cfg, 3072, 256, 4979)["waves_per_workgroup"] == 12
    monkeypatch.setenv("MODLE_HIP_WAVES", "8")
    assert api.plan_launch(cfg, 3072, 256, 4979)["waves_per_workgroup"] == 8
    monkeypatch.delenv("MODLE_HIP_WAVES")
    assert api.plan_launch(cfg, 3072, 256, 4979)["waves_per_workgroup"] == 12
    assert sorted(api.plan_launch(cfg, 1, 1, 1)) == sorted(name for name, _ in api.LaunchInfo._fields_)
