"""The NARROW device code at the top of its 16-bit move and id ranges (narrow_range_cases.py), on the CPU lane
emulator against the oracle, with the geometry of the 8-wave and of the 12-wave kernels.

Three-way agreement: the same cells with the WIDE class forced must equal the oracle too, which shows which side is
wrong when one of the three differs.

What these cases found: a unit that meets a unit stalled by a barrier (primary LEF-LEF collision) is put next to
it, whatever it drew itself -- a move bounded by the SUM of a rev and a fwd move.  The rule classed 1 kb / 64.9 kb
per epoch NARROW, a rev unit moved 65.6 kb, and the 16-bit store kept the low half: about 85 000 contact words
and the per-cell results differed from the oracle's (`fwd_64900_sd0`, `fwd_old_limit_sd0`, `rev_old_limit_sd0`;
`fwd_64800_sd0` happened to stay below 65536).  The rule now counts that move, and the corrections check what they
store: test_reclassed_cases_in_the_narrow_build_* fail on the device code as it was with "contact matrices
differ" / a results mismatch."""
import pytest

import emu_sim
import narrow_range_cases as nrc
from modle_amd import api
from parity_cases import assert_same_outputs, assert_same_results

_EMULATED_NARROW = [n for n in nrc.EMULATED if n in nrc.NARROW]
_ORACLE = {}


def _cells(name):
    """the case, its tasks and the oracle's outputs (computed once per case, never changed)"""
    if name not in _ORACLE:
        from oracle import binding

        case = nrc.build(name)
        cfg, ch = case["cfg"], case["chrom"]
        tasks = api.slice_tasks(case["tasks"], 0, int(cfg.num_cells))
        ref = binding.simulate_interval(cfg, ch["start"], ch["end"], ch["bar_pos"], ch["bar_dir"], case["stp_active"],
                                        case["stp_inactive"], tasks, nthreads=2,
                                        track_occupancy=bool(cfg.track_1d_lef_position))
        nrc.assert_oracle_result(case, ref[3], name)
        for a in ref[:3]:
            if hasattr(a, "setflags"):
                a.setflags(write=False)
        _ORACLE[name] = (case, tasks, ref)
    return _ORACLE[name]


def _emulate(case, tasks, geometry, **kw):
    cfg, ch = case["cfg"], case["chrom"]
    return emu_sim.simulate_interval_status(cfg, ch["start"], ch["end"], ch["bar_pos"], ch["bar_dir"],
                                            case["stp_active"], case["stp_inactive"], tasks, case["nrows"],
                                            case["ncols"], track_occupancy=bool(cfg.track_1d_lef_position),
                                            variant=geometry, **kw)


def _narrow_against_oracle(oracle, monkeypatch, name, geometry):
    monkeypatch.delenv("MODLE_HIP_SIZE_CLASS", raising=False)
    case, tasks, ref = _cells(name)
    for forced in (None, "wide"):
        if forced:
            monkeypatch.setenv("MODLE_HIP_SIZE_CLASS", forced)
        rc, *got = _emulate(case, tasks, geometry)
        what = f"{name}, emulator, {12 if geometry else 8}-wave geometry, class {forced or 'NARROW as classed'}"
        assert rc == 0, f"{what}: status {rc}"
        assert_same_results(ref[3], got[3], what)
        assert_same_outputs(ref[:3], got[:3], what)


@pytest.mark.parametrize("name", _EMULATED_NARROW)
def test_narrow_cases_8_wave_geometry(oracle, monkeypatch, name):
    _narrow_against_oracle(oracle, monkeypatch, name, None)


@pytest.mark.parametrize("name", _EMULATED_NARROW)
def test_narrow_cases_12_wave_geometry(oracle, monkeypatch, name):
    _narrow_against_oracle(oracle, monkeypatch, name, "w12")


def _reclassed_against_oracle(oracle, monkeypatch, name, geometry):
    """as classed (WIDE) the cells equal the oracle; in the NARROW build they equal it too or end with an error"""
    monkeypatch.delenv("MODLE_HIP_SIZE_CLASS", raising=False)
    case, tasks, ref = _cells(name)
    label = f"{name}, emulator, {12 if geometry else 8}-wave geometry"
    rc, *got = _emulate(case, tasks, geometry)
    assert rc == 0, f"{label}, WIDE as classed: status {rc}"
    assert_same_results(ref[3], got[3], label + ", WIDE as classed")
    assert_same_outputs(ref[:3], got[:3], label + ", WIDE as classed")
    rc, *got = _emulate(case, tasks, geometry, force_narrow=True)
    print(f"{label}, NARROW build: status {rc}")
    if rc != api.ERR_STATE:  # (ERR_MOVE_RANGE: a move the class cannot hold)
        assert rc == 0, f"{label}, NARROW build: status {rc}"
        assert_same_results(ref[3], got[3], label + ", NARROW build")
        assert_same_outputs(ref[:3], got[:3], label + ", NARROW build")
    return rc


@pytest.mark.parametrize("name", nrc.RECLASSED)
def test_reclassed_cases_in_the_narrow_build_8_wave_geometry(oracle, monkeypatch, name):
    rc = _reclassed_against_oracle(oracle, monkeypatch, name, None)
    if name in ("fwd_64900_sd0", "fwd_old_limit_sd0", "rev_old_limit_sd0"):
        # a move past 65535 is known to occur in these cells: the NARROW build has to say so
        assert rc == api.ERR_STATE, name


@pytest.mark.parametrize("name", nrc.RECLASSED)
def test_reclassed_cases_in_the_narrow_build_12_wave_geometry(oracle, monkeypatch, name):
    _reclassed_against_oracle(oracle, monkeypatch, name, "w12")
