"""States for the phase-level tests of primary LEF-LEF detection's pass 1 (modle_amd/csrc/sim_collisions.h:
detect_primary): blocks of 256 rev ranks, a short search of PRIMARY_NEAR entries below the unit's own rank,
a search of the rest of the staged slice, and a look-up in device memory for an answer before the slice.  Shared by
test_emu_primary_blocks.py and test_gpu_primary_blocks.py."""
import numpy as np

from kat_runner import UNBOUND
from oracle_backend import OracleBackend
from phase_backend import (PH_BOUNDARIES, PH_CORRECT_LEF_BAR, PH_CORRECT_PRIMARY, PH_PRIMARY,
                           PH_USE_BOUNDARY_COUNTS, PhaseBackend)
from phase_random import State, assert_equal_states, clone

START, SIZE = 1000, 4_000_000
GAP = 4000  # distance between the rev units of consecutive LEFs of the plain layout
NS = (1, 2, 3, 4, 5, 255, 256, 257, 383, 384, 385, 511, 512, 513)
N5S = (0, 1, 3, 255, 256, 257)
N3S = (0, 1, 2)


def plain_state(n, seed=0):
    """n disjoint loops (depth 0: pf(k) = k); neighbours 2 000 bp apart with moves of 700 .. 1 400 bp, so that
    some pairs meet within an epoch and some do not"""
    rng = np.random.default_rng(seed)
    st = State()
    st.n = n
    st.start, st.end = START, START + SIZE
    i = np.arange(n, dtype=np.uint64)
    st.rev_pos = np.uint64(START + 10) + i * np.uint64(GAP)
    st.fwd_pos = st.rev_pos + np.uint64(GAP // 2)
    st.epoch = np.zeros(n, dtype=np.uint64)
    st.rev_moves = rng.integers(700, 1400, n).astype(np.uint64)
    st.fwd_moves = rng.integers(700, 1400, n).astype(np.uint64)
    st.rev_coll = np.zeros(n, dtype=np.uint64)
    st.fwd_coll = np.zeros(n, dtype=np.uint64)
    st.bar_pos = np.zeros(0, dtype=np.uint64)
    st.bar_dir = np.zeros(0, dtype=np.uint8)
    st.bar_active = np.zeros(0, dtype=np.uint8)
    st.rev_rank = np.arange(n, dtype=np.uint64)
    st.fwd_rank = np.arange(n, dtype=np.uint64)
    return st


def at_boundaries(st, n5, n3):
    """the first n5 LEFs have their rev unit at the interval's start (tiny loops), the last n3 their fwd
    unit at its last base pair"""
    for i in range(n5):
        st.rev_pos[i] = st.start
        st.fwd_pos[i] = st.start + i // 2  # (pairs of equal fwd positions too)
    for i in range(st.n - n3, st.n):
        st.fwd_pos[i] = st.end - 1
    return st


def nested(st, k, depth):
    """`depth` loops over the rev unit of LEF k: the LEFs before it end right behind it"""
    assert depth <= k
    for j, i in enumerate(range(k - depth, k)):
        st.fwd_pos[i] = st.rev_pos[k] + 1 + j
    return st


def all_rev_upstream(n):
    """every rev unit upstream of every fwd unit: pf = 0 for all"""
    st = plain_state(n)
    i = np.arange(n, dtype=np.uint64)
    st.rev_pos = np.uint64(START + 10) + i * np.uint64(7)
    st.fwd_pos = np.uint64(START + 2_000_000) + i * np.uint64(900)
    return st


def released_tail(st, count):
    for i in range(st.n - count, st.n):
        st.rev_pos[i] = st.fwd_pos[i] = st.epoch[i] = UNBOUND
    return st


def equal_positions(st, every=5):
    """the fwd unit of LEF i at the position of the rev unit of LEF i + 1 (not strictly upstream of it)"""
    for i in range(0, st.n - 1, every):
        st.fwd_pos[i] = st.rev_pos[i + 1]
    return st


def check_primary(oracle_binding, phases, st, bypass=0.1, seed=7, expect_counts=None):
    """boundaries + primary detection + both move corrections: oracle against the device code"""
    ob = OracleBackend(oracle_binding)
    pb = PhaseBackend(phases)
    ob.rank_lefs(st, init_buffers=True)
    cfgd = dict(bypass=bypass, major_pblock=1.0, minor_pblock=0.0, rev_speed=1000, fwd_speed=1000)
    a, b = clone(st), clone(st)
    rng_a, rng_b = ob.make_prng(seed), pb.make_prng(seed)
    cfg_a, cfg_b = ob.make_config(cfgd), pb.make_config(cfgd)
    n5, n3 = ob.detect_units_at_interval_boundaries(a)
    if expect_counts is not None:
        assert (n5, n3) == expect_counts, (n5, n3, expect_counts)
    ob.detect_primary_lef_lef_collisions(cfg_a, a, rng_a, n5, n3)
    ob.correct_moves_for_lef_bar_collisions(a)
    ob.L.mo_correct_moves_for_primary_lef_lef_collisions(
        a.n, a.rev_pos, a.fwd_pos, a.rev_rank, a.fwd_rank, a.rev_moves, a.fwd_moves, a.rev_coll, a.fwd_coll)
    pb._run(cfg_b, PH_BOUNDARIES | PH_USE_BOUNDARY_COUNTS | PH_PRIMARY | PH_CORRECT_LEF_BAR | PH_CORRECT_PRIMARY,
            b, rng_b)
    what = f"n {st.n} n5 {n5} n3 {n3} bypass {bypass}"
    assert_equal_states(a, b, what)
    assert rng_a.count == rng_b["consumed"], what + ": raws consumed differ"
    return int(np.count_nonzero(a.rev_coll))


def boundary_cases():
    """(n, n5, n3) for every n, with every pair of boundary counts that fits (the fwd unit of rank 0 is never
    counted, so n3 stays below n)"""
    return [(n, n5, n3) for n in NS for n5 in N5S for n3 in N3S if n5 + n3 <= n and n3 < n]


def depth_cases(near, back):
    """(n, k, depth, searches of the rest of the slice, look-ups in device memory): `depth` nested loops over
    the rev unit of rank k in the second and in the third block of 256.  Unit k - i, i < depth, lies under
    depth - i of them, so the deepest units leave their window of `near` entries: depth - near + 1 of them
    (none at depth near - 1).  The slice of a block starts `back` ranks before the block: a unit whose answer
    k - depth lies before that start -- k on the block's first rank, depth back + 1 -- goes to device memory."""
    out = []
    for k in (300, 600):
        for d in (near - 1, near, near + 1):
            out.append((700, k, d, max(0, d - near + 1), 0))
    for k in (256, 512):
        out.append((700, k, back + 1, back + 1 - near + 1, 1))
    return out


def searches_taken(err):
    """(units that searched the rest of the slice, units looked up in device memory) from the trace a build with
    -DMODLE_EMU_TRACE_PRIMARY writes"""
    return err.count("rest of the slice"), err.count("device memory")
