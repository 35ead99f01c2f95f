"""Set-ups at the top of the NARROW size class's 16-bit ranges (modle_amd/csrc/sim_types.h: moves up to
MOVE_LIMIT = 65533 below the two marks, LEF ids / previous ranks / carried-over counts up to 65535), shared by
test_emu_narrow_ranges.py and test_gpu_narrow_ranges.py.

The table has two kinds of cases.  NARROW cases are classed NARROW by the library's own rule
(launch_common.hpp: size_class_required) and must equal the oracle in that class.  RECLASSED cases were NARROW
under the rule as it was before the move of a unit that is put next to a barrier-stalled one was counted (it is
bounded by the SUM of a rev and a fwd move, not by the unit's own draw): the rule now classes them WIDE, where they
must equal the oracle, and the NARROW device code, made to run them all the same, must either equal the oracle or
end the cell with ERR_MOVE_RANGE -- never give other numbers.  Three of them (`fwd_64900_sd0`,
`fwd_old_limit_sd0`, `rev_old_limit_sd0`) gave other numbers before.

`build` asserts what each case is for, so that a later change of defaults cannot hollow a case out."""
from modle_amd import api, synthetic

MOVE_LIMIT = 65533
SLOW = 1000

_SMALL = dict(num_cells=2, target_contact_density=0.05, max_burnin_epochs=150)
_LIMIT_SIZE, _LIMIT_DENSITY, _LIMIT_LEFS = 17_700_000, 30.0, 531


def _speeds(rev, fwd, rev_sd=0.0, fwd_sd=0.0, **kw):
    return dict(_SMALL, rev_extrusion_speed=rev, fwd_extrusion_speed=fwd, rev_extrusion_speed_set=1,
                fwd_extrusion_speed_set=1, rev_extrusion_speed_std=rev_sd, fwd_extrusion_speed_std=fwd_sd, **kw)


def _on_limit_chromosome(rev, fwd, rev_sd=0.0, fwd_sd=0.0, kind=("fast",), narrow=True):
    return dict(size=_LIMIT_SIZE, seed=7, kind=kind, burnin=True, narrow=narrow,
                cfg=_speeds(rev, fwd, rev_sd, fwd_sd, number_of_lefs_per_mbp=_LIMIT_DENSITY))


# sd 0: slow + fast + LEFs == MOVE_LIMIT, the border of the rule
_AT_LIMIT = MOVE_LIMIT - SLOW - _LIMIT_LEFS  # 64002
_MANY = dict(num_cells=1, rev_extrusion_speed=1000, fwd_extrusion_speed=1000, rev_extrusion_speed_set=1,
             fwd_extrusion_speed_set=1, rev_extrusion_speed_std=10.0, fwd_extrusion_speed_std=10.0,
             number_of_lefs_per_mbp=600.0, target_contact_density=0.001)
_SHORT_BURNIN = dict(burnin_target_epochs_for_lef_activation=20)

CASES = {
    # ---- NARROW ---------------------------------------------------------------------------------------------
    # one direction as fast as the rule lets it be next to a slow one: the bound is exactly MOVE_LIMIT
    "fwd_at_limit_sd0": _on_limit_chromosome(SLOW, _AT_LIMIT, kind=("fast", "limit")),
    "rev_at_limit_sd0": _on_limit_chromosome(_AT_LIMIT, SLOW, kind=("fast", "limit")),
    # both directions at half of what is left: the bound is exactly MOVE_LIMIT again
    "both_half_limit_sd0": _on_limit_chromosome((MOVE_LIMIT - _LIMIT_LEFS) // 2, (MOVE_LIMIT - _LIMIT_LEFS) // 2,
                                                kind=("limit",)),
    # draws between 54 kb and 62 kb in one direction
    "fast_fwd_spread_narrow": _on_limit_chromosome(SLOW, 58000, 10.0, 100.0),
    "fast_rev_spread_narrow": _on_limit_chromosome(58000, SLOW, 100.0, 10.0),
    # ids, previous ranks and carried-over counts above 32767: 60 000 LEFs, bound all at once ...
    "lefs_60000_skip_burnin": dict(size=100_000_000, seed=42, kind=("many",), burnin=False, narrow=True,
                                   cfg=dict(_MANY, skip_burnin=1)),
    # ... and through the binds of a burn-in
    "lefs_60000_burnin": dict(size=100_000_000, seed=42, kind=("many",), burnin=True, narrow=True,
                              cfg=dict(_MANY, max_burnin_epochs=25), post=_SHORT_BURNIN),
    # ids up to 65499: the rule's bound is 20 + 10 + 65500 (the emulator needs minutes for it: GPU only)
    "lefs_65500_burnin": dict(size=100_000_000, seed=42, kind=("many", "top"), burnin=True, narrow=True,
                              cfg=dict(_MANY, number_of_lefs_per_mbp=655.0, rev_extrusion_speed=20,
                                       fwd_extrusion_speed=10, rev_extrusion_speed_std=0.0,
                                       fwd_extrusion_speed_std=0.0, max_burnin_epochs=25),
                              post=_SHORT_BURNIN),
    # ---- RECLASSED: NARROW by the rule as it was, WIDE by the rule as it is ---------------------------------
    # both directions fast, with a spread: draws between 36 kb and 60 kb, occupancy tracked
    "fast_both_spread": dict(size=20_000_000, seed=42, kind=("fast",), burnin=True, narrow=False,
                             cfg=_speeds(48000, 48000, 300.0, 300.0, track_1d_lef_position=1)),
    # where the bound of the rule as it was equalled MOVE_LIMIT (65000 + 531 LEFs + 2)
    "fwd_old_limit_sd0": _on_limit_chromosome(SLOW, 65000, narrow=False),
    "rev_old_limit_sd0": _on_limit_chromosome(65000, SLOW, narrow=False),
    "both_at_limit_sd0": _on_limit_chromosome(65000, 65000, narrow=False),
    # the pair that bracketed the divergence: a rev unit that meets a barrier-stalled fwd unit moves up to
    # 1000 + 64800 (64900) + the adjustments, and the first such move past 65535 came between the two
    "fwd_64800_sd0": _on_limit_chromosome(SLOW, 64800, narrow=False),
    "fwd_64900_sd0": _on_limit_chromosome(SLOW, 64900, narrow=False),
    "fast_fwd_spread": _on_limit_chromosome(SLOW, 60000, 10.0, 100.0, narrow=False),
    "fast_rev_spread": _on_limit_chromosome(60000, SLOW, 100.0, 10.0, narrow=False),
}
NARROW = [name for name, spec in CASES.items() if spec["narrow"]]
RECLASSED = [name for name, spec in CASES.items() if not spec["narrow"]]
EMULATED = [name for name in CASES if name != "lefs_65500_burnin"]


def rule_bound(cfg, num_lefs):
    """the bound of size_class_required, from the cfg's fields: the larger of a unit's own move (draw + adjustment)
    and of the move next to a barrier-stalled unit (rev draw + fwd draw + both adjustments)"""
    rev = max(int(cfg.rev_extrusion_speed), int(cfg.rev_extrusion_speed_burnin))
    fwd = max(int(cfg.fwd_extrusion_speed), int(cfg.fwd_extrusion_speed_burnin))
    rev_sd, fwd_sd = abs(float(cfg.rev_extrusion_speed_std)), abs(float(cfg.fwd_extrusion_speed_std))
    own = max(rev, fwd) + 40.0 * max(rev_sd, fwd_sd) + int(num_lefs) + 2
    pair = rev + fwd + 40.0 * (rev_sd + fwd_sd) + int(num_lefs)
    return max(own, pair)


def old_rule_bound(cfg, num_lefs):
    """... and of the rule as it was: a unit's own move only"""
    speed = max(int(cfg.rev_extrusion_speed), int(cfg.fwd_extrusion_speed), int(cfg.rev_extrusion_speed_burnin),
                int(cfg.fwd_extrusion_speed_burnin))
    sd = max(abs(float(cfg.rev_extrusion_speed_std)), abs(float(cfg.fwd_extrusion_speed_std)))
    return speed + 40.0 * sd + int(num_lefs) + 2


def size_class(cfg, max_lefs):
    import ctypes as C

    from modle_amd import _lib
    from modle_amd.params import Config

    L = _lib.lib()
    L.modle_hip_size_class.argtypes = [C.POINTER(Config), C.c_uint64]
    return L.modle_hip_size_class(C.byref(cfg), int(max_lefs))


def build(name, num_cells=None):
    """cfg, chromosome, stps, tasks and shape of a case; `num_cells` as in parity_cases.build_case (the cells keep
    the share of contacts they have in CASES)"""
    import os

    spec = CASES[name]
    kw = dict(spec["cfg"])
    if num_cells is not None and num_cells != kw["num_cells"]:
        kw["target_contact_density"] = kw["target_contact_density"] * num_cells / kw["num_cells"]
        kw["num_cells"] = num_cells
    cfg = api.make_config(**kw)
    for field, value in spec.get("post", {}).items():
        setattr(cfg, field, value)
    chrom = synthetic.synthetic_chromosome("chrN", spec["size"], seed=spec["seed"])
    stp_active, stp_inactive = api.barrier_stps(cfg, chrom["bar_occupancy"])
    tasks = api.make_tasks(cfg, chrom["name"], chrom["size"], chrom["start"], chrom["end"])
    nrows, ncols = api.matrix_shape(cfg, chrom["end"] - chrom["start"])
    num_lefs = max(int(t.num_lefs) for t in tasks)
    # what the case is for
    assert "MODLE_HIP_SIZE_CLASS" not in os.environ, "build() is called with no class forced"
    kind = spec["kind"]
    if spec["narrow"]:
        assert size_class(cfg, num_lefs) == 0, name
        assert rule_bound(cfg, num_lefs) <= MOVE_LIMIT, name
    else:
        assert size_class(cfg, num_lefs) == 1, name
        assert num_lefs < 65536 and old_rule_bound(cfg, num_lefs) <= MOVE_LIMIT < rule_bound(cfg, num_lefs), name
    if "limit" in kind:
        assert rule_bound(cfg, num_lefs) == MOVE_LIMIT, (name, rule_bound(cfg, num_lefs))
    if "fast" in kind:
        fastest = max((int(cfg.rev_extrusion_speed), float(cfg.rev_extrusion_speed_std)),
                      (int(cfg.fwd_extrusion_speed), float(cfg.fwd_extrusion_speed_std)))
        assert fastest[0] - 40.0 * fastest[1] > 32767, (name, fastest)
    if "many" in kind:
        assert num_lefs > 32768, (name, num_lefs)
    if "top" in kind:
        assert 65500 <= num_lefs < 65536, (name, num_lefs)
    assert bool(cfg.skip_burnin) != spec["burnin"], name
    return dict(cfg=cfg, chrom=chrom, stp_active=stp_active, stp_inactive=stp_inactive, tasks=tasks, nrows=nrows,
                ncols=ncols, burnin=spec["burnin"], num_lefs=num_lefs, narrow=spec["narrow"])


def assert_oracle_result(case, results, name):
    """the oracle's cells did what the case means them to: a burn-in where one is meant, and contacts"""
    for i, r in enumerate(results):
        if case["burnin"]:
            assert r.burnin_epochs > 0, f"{name}: cell {i} had no burn-in"
        assert r.num_contacts > 0, f"{name}: cell {i} registered no contact"
