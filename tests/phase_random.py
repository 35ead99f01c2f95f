"""Randomised phase-level differential test: the product's device code (emulated or on the GPU)
against the oracle on synthetic multi-batch states (hundreds to thousands of LEFs), one hook
sequence at a time.  Complements the reference's tiny unit-test vectors, which fit in one batch."""
import numpy as np

from kat_runner import UNBOUND
from modle_amd.params import DIR_FWD, DIR_REV
from oracle_backend import OracleBackend
from phase_backend import PhaseBackend


class State:
    pass


# move distributions of the states near the top of the NARROW class's move range (sim_types.h: MOVE_LIMIT = 65533).
# One direction is fast, the other slow: a unit that meets a barrier-stalled unit of the other direction is put next
# to it, a move of up to the SUM of the two (launch_common.hpp: size_class_required), and the states must stay
# within what the NARROW build can hold.  `speeds`: nominal speeds for which the rule says NARROW for the n used.
MOVE_LIMIT = 65533


def near_limit_moves(fast, pinned=False):
    """`fast`: "rev" or "fwd".  Moves around 60000 (sd 200) against 300 (sd 20); `pinned`: a sixth of the fast
    moves at exactly 65533, 65532 and 65000 (a third each), against a slow direction that does not move"""
    slow = "fwd" if fast == "rev" else "rev"
    if pinned:
        return {fast: (60000, 200), slow: (0, 0), "pinned": (fast, (MOVE_LIMIT, MOVE_LIMIT - 1, 65000), 6),
                "speeds": {fast: 65000, slow: 0}, "loop_max": 200_000}
    return {fast: (60000, 200), slow: (300, 20), "speeds": {fast: 60000, slow: 300}, "loop_max": 200_000}

# moves at the top of the NARROW class's 16-bit range (phase_random.near_limit_moves): around 60000 in one
# direction, and a share of them at exactly 65533, 65532 and 65000; n within what the rule classes NARROW
NEAR_LIMIT_SEQUENCES = [
    (11, 700, 200, {"moves": near_limit_moves("rev")}, False),
    (12, 700, 200, {"moves": near_limit_moves("fwd")}, False),
    (13, 1200, 300, {"moves": near_limit_moves("rev"), "bypass": 0.3}, True),
    (14, 1200, 300, {"moves": near_limit_moves("fwd"), "minor": 0.3, "major": 0.9}, True),
    (15, 500, 200, {"moves": near_limit_moves("rev", pinned=True)}, False),
    (16, 500, 200, {"moves": near_limit_moves("fwd", pinned=True)}, False),
    (17, 500, 100, {"moves": near_limit_moves("rev", pinned=True), "bypass": 0.0}, True),
    (18, 500, 100, {"moves": near_limit_moves("fwd", pinned=True), "bypass": 0.0}, True),
]


def random_state(seed, n, nb, size=2_000_000, start=1000, dense=False, moves=None):
    """`moves`: None (both directions normal(4000, 200), loops up to 60 kb) or {"rev": (mean, sd), "fwd": (mean, sd),
    "loop_max": ..., "pinned": (direction, values, one move in how many)} -- see near_limit_moves"""
    moves = moves or {}
    rev_mean, rev_sd = moves.get("rev", (4000, 200))
    fwd_mean, fwd_sd = moves.get("fwd", (4000, 200))
    rng = np.random.default_rng(seed)
    st = State()
    st.n = n
    st.start, st.end = start, start + size
    span = size // 8 if dense else size
    rev = rng.integers(start, start + span - 1, n, dtype=np.uint64)
    loop = rng.integers(0, moves.get("loop_max", 60_000) if not dense else 5_000, n, dtype=np.uint64)
    # a few LEFs sit at the interval ends / share positions
    rev[: n // 50] = start
    fwd = np.minimum(rev + loop, np.uint64(st.end - 1))
    fwd[n - n // 50:] = st.end - 1
    dup = rng.integers(0, n, n // 20)
    rev[dup] = rev[(dup + 1) % n]
    fwd = np.maximum(fwd, rev)
    st.rev_pos, st.fwd_pos = rev.copy(), fwd.copy()
    st.epoch = rng.integers(0, 50, n, dtype=np.uint64)
    st.rev_rank = np.lexsort((np.arange(n), st.epoch, st.rev_pos)).astype(np.uint64)
    st.fwd_rank = np.lexsort((np.arange(n), np.uint64(1000) - st.epoch, st.fwd_pos)).astype(np.uint64)
    st.rev_moves = np.round(rng.normal(rev_mean, rev_sd, n)).astype(np.uint64)
    st.fwd_moves = np.round(rng.normal(fwd_mean, fwd_sd, n)).astype(np.uint64)
    st.rev_coll = np.zeros(n, dtype=np.uint64)
    st.fwd_coll = np.zeros(n, dtype=np.uint64)
    pos = np.sort(rng.choice(np.arange(start + 1, st.end - 1), nb, replace=False)).astype(np.uint64)
    st.bar_pos = pos
    st.bar_dir = rng.choice([DIR_FWD, DIR_REV], nb).astype(np.uint8)
    st.bar_active = (rng.random(nb) < 0.8).astype(np.uint8)
    st.n5 = st.n3 = 0
    if "pinned" in moves:
        # (a generator of its own: the draws above stay what they are)
        direction, values, one_in = moves["pinned"]
        prng = np.random.default_rng(seed + 1_000_003)
        target = st.rev_moves if direction == "rev" else st.fwd_moves
        # (not where units share a position: the adjustment would push the one in front a base pair further than
        # the unit pinned at the limit, beyond what the class holds)
        pos = st.rev_pos if direction == "rev" else st.fwd_pos
        _, first, count = np.unique(pos, return_index=True, return_counts=True)
        alone = np.zeros(n, dtype=bool)
        alone[first[count == 1]] = True
        which = np.nonzero((prng.integers(0, one_in, n) == 0) & alone)[0]
        target[which] = np.asarray(values, dtype=np.uint64)[prng.integers(0, len(values), len(which))]
    return st


def clone(st):
    c = State()
    for k, v in st.__dict__.items():
        setattr(c, k, v.copy() if isinstance(v, np.ndarray) else v)
    return c


FIELDS = ("rev_pos", "fwd_pos", "rev_rank", "fwd_rank", "rev_moves", "fwd_moves", "rev_coll",
          "fwd_coll")


def assert_equal_states(a, b, what):
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        if not np.array_equal(x, y):
            bad = np.nonzero(x != y)[0]
            raise AssertionError(f"{what}: {f} differs at {len(bad)} entries, first {bad[:5]}: "
                                 f"{x[bad[:5]]} vs {y[bad[:5]]}")


def run_sequences(oracle_binding, phases, seed, n, nb, cfg_kw, dense=False):
    """`cfg_kw["moves"]`: the move distribution and the speeds of the state (random_state; near_limit_moves)"""
    ob = OracleBackend(oracle_binding)
    pb = PhaseBackend(phases)
    moves = cfg_kw.get("moves")
    speeds = (moves or {}).get("speeds", {"rev": 4000, "fwd": 4000})
    cfgd = dict(bypass=cfg_kw.get("bypass", 0.1), major_pblock=cfg_kw.get("major", 1.0),
                minor_pblock=cfg_kw.get("minor", 0.0), rev_speed=speeds["rev"], fwd_speed=speeds["fwd"])
    base = random_state(seed, n, nb, dense=dense, moves=moves)
    # 1. ranking from scratch
    a, b = clone(base), clone(base)
    ob.rank_lefs(a, init_buffers=True)
    pb.rank_lefs(b, init_buffers=True)
    # only the ranks are meaningful across a re-ranking (moves are regenerated every epoch)
    assert np.array_equal(a.rev_rank, b.rev_rank), "rank_lefs: rev ranks differ"
    assert np.array_equal(a.fwd_rank, b.fwd_rank), "rank_lefs: fwd ranks differ"
    b = clone(a)
    # 2. adjust + clamp, then the whole collision pipeline, then fix_secondary
    drawn = clone(a)
    ob.adjust_and_clamp_moves(a)
    if moves is not None:
        assert_near_limit_state_is_what_it_is_for(moves, drawn, a)
    pb.adjust_and_clamp_moves(b)
    assert_equal_states(a, b, "adjust_and_clamp_moves")
    rng_a, rng_b = ob.make_prng(seed), pb.make_prng(seed)
    cfg_a, cfg_b = ob.make_config(cfgd), pb.make_config(cfgd)
    ob.process_collisions(cfg_a, a, rng_a)
    pb.process_collisions(cfg_b, b, rng_b)
    assert_equal_states(a, b, "process_collisions")
    assert rng_a.count == rng_b["consumed"], "process_collisions: raws consumed differ"
    ob.fix_secondary_lef_lef_collisions(a)
    pb.fix_secondary_lef_lef_collisions(b)
    assert_equal_states(a, b, "fix_secondary")
    if moves is not None:
        # the oracle's moves stayed within the NARROW class to the end: the device code ran its NARROW build
        # (phase_backend.emu_phases / modle_hip_test_phases send a state with a larger move to the WIDE one)
        assert max(int(a.rev_moves.max()), int(a.fwd_moves.max())) <= MOVE_LIMIT


def assert_near_limit_state_is_what_it_is_for(moves, drawn, adjusted):
    """on the oracle's state: the adjustment raised a move, the clamp shortened one, the fast direction is at the
    top of the 16-bit range and nothing went beyond MOVE_LIMIT"""
    fast = "rev" if moves["speeds"]["rev"] > moves["speeds"]["fwd"] else "fwd"
    before = getattr(drawn, fast + "_moves").astype(np.int64)
    after = getattr(adjusted, fast + "_moves").astype(np.int64)
    assert np.any(after > before), "no move of the fast direction was raised by the adjustment"
    assert np.any(after < before), "no move of the fast direction was clamped at the interval's end"
    top = max(int(adjusted.rev_moves.max()), int(adjusted.fwd_moves.max()))
    assert 59000 < top <= MOVE_LIMIT, top
    if "pinned" in moves:
        assert top == MOVE_LIMIT and np.any(after == MOVE_LIMIT - 1) and np.any(after == 65000)
