"""Pass 1 of primary LEF-LEF detection under the lane emulator, both geometries, against the oracle: the
shapes of tests/primary_block_cases.py on the product's constants, and random sequences of 700 LEFs on a
build with -DMODLE_PRIMARY_NEAR=4 -DMODLE_PRIMARY_BACK=8, where both fall-backs of the short search are
taken all the time."""
import ctypes as C
import functools
import os
import subprocess

import pytest

import primary_block_cases as pc
from phase_backend import _advance, _declare_phases, emu_phases, emu_size_class
from phase_random import run_sequences

NEAR, BACK = 16, 128  # modle_amd/csrc/sim_collisions.h: MODLE_PRIMARY_NEAR, MODLE_PRIMARY_BACK
GEOMETRIES = [None, "w12"]
HERE = os.path.dirname(os.path.abspath(__file__))


def _backend(geometry):
    return functools.partial(emu_phases, geometry=geometry)


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_block_boundaries_and_boundary_counts(oracle, geometry):
    hits = 0
    for n, n5, n3 in pc.boundary_cases():
        st = pc.at_boundaries(pc.plain_state(n, seed=n), n5, n3)
        hits += pc.check_primary(oracle, _backend(geometry), st, expect_counts=(n5, min(n3, n - 1)))  # (the fwd unit of rank 0 is never counted)
    assert hits > 1000


@pytest.mark.parametrize("geometry", GEOMETRIES)
@pytest.mark.parametrize("bypass", [0.0, 0.3, 1.0])
def test_draw_order_and_special_layouts(oracle, geometry, bypass):
    be = _backend(geometry)
    pc.check_primary(oracle, be, pc.plain_state(513, seed=3), bypass)
    pc.check_primary(oracle, be, pc.all_rev_upstream(513), bypass)
    pc.check_primary(oracle, be, pc.released_tail(pc.plain_state(513, seed=4), 20), bypass)
    pc.check_primary(oracle, be, pc.released_tail(pc.nested(pc.plain_state(700, seed=5), 400, 40), 150), bypass)
    pc.check_primary(oracle, be, pc.equal_positions(pc.plain_state(385, seed=6)), bypass)


@pytest.fixture(scope="module")
def traced_builds(tmp_path_factory):
    """the emulator with -DMODLE_EMU_TRACE_PRIMARY (every unit that leaves its short search says where it goes),
    both geometries: with the product's constants, and with a short search of 4 entries and a slice that
    reaches 8 ranks back"""
    emu = os.path.join(HERE, "wave_emu")
    csrc = os.path.join(HERE, "..", "modle_amd", "csrc")
    out = tmp_path_factory.mktemp("emu_traced")
    procs = {}
    for reach, rflags in (("product", []), ("short", ["-DMODLE_PRIMARY_NEAR=4", "-DMODLE_PRIMARY_BACK=8"])):
        for geometry, gflags in ((None, []), ("w12", ["-DMODLE_WAVES_PER_CU=12"])):
            so = str(out / f"libmodle_emu_{reach}_{geometry}.so")
            procs[reach, geometry] = (so, subprocess.Popen(
                ["g++", "-O2", "-DMODLE_STAGE_TRACE", "-DMODLE_EMU_TRACE_PRIMARY", "-std=c++17", "-fPIC",
                 "-ffp-contract=off", *rflags, *gflags, "-I" + emu, "-I" + csrc,
                 "-I" + os.path.join(HERE, "..", "include"), "-shared", "-o", so, os.path.join(emu, "wave_emu.cpp"),
                 os.path.join(emu, "emu_api.cpp"), os.path.join(csrc, "host_logic.cpp"), "-lm"],
                stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    libs = {}
    for key, (so, proc) in procs.items():
        log = proc.communicate()[0]
        assert proc.returncode == 0, log[-4000:]
        libs[key] = _declare_phases(C.CDLL(so))
    return libs


def _phases_on(L):
    def phases(cfg, mask, st, state, skip):
        assert emu_size_class(cfg, st.n, (st.rev_moves, st.fwd_moves)) == 0  # (the NARROW class, like the build)
        prng = (C.c_uint64 * 4)(*_advance(state, skip))
        consumed = C.c_uint64(0)
        rc = L.emu_test_phases(C.byref(cfg), mask, st.start, st.end, st.n, st.rev_pos, st.fwd_pos, st.epoch,
                               st.rev_rank, st.fwd_rank, st.rev_moves, st.fwd_moves, st.rev_coll, st.fwd_coll,
                               len(st.bar_pos), st.bar_pos, st.bar_dir, st.bar_active, prng, C.byref(consumed))
        assert rc == 0, f"emu_test_phases failed: {rc}"
        return consumed.value
    return phases


@pytest.mark.parametrize("geometry", GEOMETRIES)
@pytest.mark.parametrize("reach,near,back", [("product", NEAR, BACK), ("short", 4, 8)])
def test_nested_loops_take_the_three_searches(oracle, traced_builds, capfd, geometry, reach, near, back):
    """the parity of every case, and the searches its units took: counted from the build's trace"""
    be = _phases_on(traced_builds[reach, geometry])
    capfd.readouterr()
    # no loop over any unit: nobody leaves the short search (the first ranks of the array included)
    pc.check_primary(oracle, be, pc.plain_state(700, seed=1))
    assert pc.searches_taken(capfd.readouterr().err) == (0, 0)
    for n, k, depth, rest, device in pc.depth_cases(near, back):
        assert pc.check_primary(oracle, be, pc.nested(pc.plain_state(n, seed=depth), k, depth)) > 100
        assert pc.searches_taken(capfd.readouterr().err) == (rest, device), (n, k, depth)
    # every rev unit upstream of every fwd unit: the units of the blocks behind the first go to device memory
    pc.check_primary(oracle, be, pc.all_rev_upstream(513))
    assert pc.searches_taken(capfd.readouterr().err)[1] == 513 - 256


@pytest.mark.parametrize("geometry", GEOMETRIES)
@pytest.mark.parametrize("seed,kw,dense", [(11, {}, False), (12, {"bypass": 0.3}, True), (13, {"bypass": 0.0}, True)])
def test_random_sequences_with_a_short_reach(oracle, traced_builds, capfd, geometry, seed, kw, dense):
    be = _phases_on(traced_builds["short", geometry])
    capfd.readouterr()
    run_sequences(oracle, be, seed, 700, 200, kw, dense)
    rest, device = pc.searches_taken(capfd.readouterr().err)
    assert rest > 0 and device > 0, (rest, device)
