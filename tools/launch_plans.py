#!/usr/bin/env python3
"""Records how the library lays out real launches: tests/golden/launch_plans.json.

The rule that picks a launch's workgroups, waves per workgroup, fixed roles, tail helpers and size class is
`modle_host::plan_launch` (modle_amd/csrc/launch_common.hpp).  The table written here is what the library DID on a
GPU -- `Simulator.launch_info()` after real launches -- for the task counts around the rule's thresholds and for
every override of the environment.  `tests/test_launch_plan.py` holds `api.plan_launch` to it on the CPU;
`tests/test_gpu_launch_plan.py` launches some of the same cells again and compares the launch with the plan.

    python tools/launch_plans.py                 records every case (needs a GPU), one process per case, and stops at
                                                 the first case that fails; run it under one `timeout`
    python tools/launch_plans.py --case NAME     runs one case in this process and prints its entry as one JSON line

The cells are tiny (a 1 Mbp chromosome, a few hundred epochs at most) and MODLE_HIP_GRID=2 puts the thresholds
at 8 tasks (fixed roles) and 24 tasks (12 waves per workgroup), so the whole table takes seconds of GPU time.
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_plans.json")
CHROM_SIZE = 1_000_000
# every variable a launch reads for its layout: a case sets the ones it names and clears the rest
LAYOUT_ENV = ("MODLE_HIP_GRID", "MODLE_HIP_WAVES", "MODLE_HIP_PAIRED", "MODLE_HIP_TAIL_HELPERS",
              "MODLE_HIP_ACTIVE_WAVES", "MODLE_HIP_SIZE_CLASS")
WORKSPACE_FIELDS = ("workspace_tries", "workspace_probe_us", "workspace_probe_worst_us")
EDGES = (1, 2, 3, 4, 5, 8, 9, 23, 24, 25)  # (2 workgroups: fixed roles up to 8 tasks, 12 waves from 24)


def _cases():
    grid2 = {"MODLE_HIP_GRID": "2"}
    out = []

    def add(name, n_tasks, env, **config):
        out.append({"name": name, "n_tasks": n_tasks, "env": env, "config": config})

    for n in EDGES:
        add(f"tasks{n}", n, dict(grid2))
    for value, tag in (("0", "0"), ("1", "1"), ("", "empty")):
        for n in EDGES:
            add(f"tasks{n}_paired_{tag}", n, dict(grid2, MODLE_HIP_PAIRED=value))
    for n in (5, 24):
        add(f"tasks{n}_waves8", n, dict(grid2, MODLE_HIP_WAVES="8"))
    for n in (4, 9, 24):
        add(f"tasks{n}_waves12", n, dict(grid2, MODLE_HIP_WAVES="12"))
    for n in (4, 24):
        add(f"tasks{n}_waves12_paired_1", n, dict(grid2, MODLE_HIP_WAVES="12", MODLE_HIP_PAIRED="1"))
    for n in (4, 9, 24):
        add(f"tasks{n}_no_tail_helpers", n, dict(grid2, MODLE_HIP_TAIL_HELPERS="0"))
    for n in (9, 24):  # (launches where every wave pulls tasks: a fixed-role launch needs all of its waves)
        for v in ("0", "3", "13"):
            add(f"tasks{n}_active{v}", n, dict(grid2, MODLE_HIP_ACTIVE_WAVES=v))
    for n in (4, 9, 24):
        add(f"tasks{n}_wide", n, dict(grid2, MODLE_HIP_SIZE_CLASS="wide"))
    # LEFs x release probability on either side of 170: p_release = (8000 bp per epoch) / (10 kb processivity) = 0.8
    for lefs in (212, 213):
        add(f"tasks24_lefs{lefs}_release0.8", 24, dict(grid2), number_of_lefs_per_mbp=float(lefs),
            avg_lef_processivity=10_000)
    add("tasks5_whole_device", 5, {})
    return out


CASES = _cases()


def case_config(case):
    from modle_amd import api

    settings = dict(num_cells=case["n_tasks"], seed=7, target_contact_density=0.01, max_burnin_epochs=50)
    settings.update(case["config"])
    return api.make_config(**settings)


def geometry(info):
    """a launch's record without the fields that describe the placement of its workspace"""
    return {k: v for k, v in info.items() if k not in WORKSPACE_FIELDS}


class layout_env:
    """the process environment as a case sets it (and back)"""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in LAYOUT_ENV}
        for k in LAYOUT_ENV:
            os.environ.pop(k, None)
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def run_case(case, wait_timeout_s=60.0):
    """Launches the case's cells on device 0 and returns its entry of the table."""
    from modle_amd import api, synthetic

    cfg = case_config(case)
    chrom = synthetic.synthetic_chromosome("chrP", CHROM_SIZE, seed=5)
    stp_a, stp_i = api.barrier_stps(cfg, chrom["bar_occupancy"])
    tasks = api.make_tasks(cfg, chrom["name"], chrom["size"], 0, chrom["size"])
    with layout_env(case["env"]):
        sim = api.Simulator(cfg, 0)
        try:
            sim.set_wait_timeout(wait_timeout_s)
            iid = sim.add_interval(0, chrom["size"], chrom["bar_pos"], chrom["bar_dir"], stp_a, stp_i)
            sim.submit(iid, tasks)
            sim.launch()
            sim.wait()
            info = sim.launch_info()
        finally:
            sim.close()
    assert info["n_tasks"] == case["n_tasks"], info
    return {"name": case["name"], "config": case["config"], "n_tasks": case["n_tasks"],
            "max_lefs": int(max(t.num_lefs for t in tasks)), "num_cus": info["num_cus"], "env": case["env"],
            "info": info}


def main(argv):
    by_name = {c["name"]: c for c in CASES}
    if len(argv) == 2 and argv[0] == "--case":
        print(json.dumps(run_case(by_name[argv[1]])))
        return 0
    entries = []
    for case in CASES:
        proc = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case["name"]],
                              capture_output=True, text=True)
        if proc.returncode != 0:
            print(f"{case['name']}: exit status {proc.returncode}; nothing written\n{proc.stdout}\n{proc.stderr}")
            return 1
        entries.append(json.loads(proc.stdout.strip().splitlines()[-1]))
        print(f"{case['name']}: {geometry(entries[-1]['info'])}", flush=True)
    with open(GOLDEN, "w") as f:
        f.write("[\n" + ",\n".join(" " + json.dumps(e, sort_keys=True) for e in entries) + "\n]\n")
    print(f"{len(entries)} launches -> {GOLDEN}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
