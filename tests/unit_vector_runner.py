"""Replays tests/golden/reference_unit_vectors.json (the reference's small unit tests that touch
the hot path: descriptive statistics, contact-matrix layout and increments, collision words, and
the Bind LEFs / Generate LEF moves property tests) on a backend: the CPU oracle, the device code
under the lane emulator, or the GPU through the C ABI.  Same runner for all three."""
import ctypes as C
import json
import os

import numpy as np

from kat_runner import UNBOUND, KatState
from modle_amd.params import Config

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "reference_unit_vectors.json")
UNIT_LOOP_STATS, UNIT_MATRIX_INCREMENT, UNIT_COLLISION_WORDS = 1, 2, 3
UNIT_DRAWS, UNIT_DRAW_FORMS = 7, 8  # (the regimes and the checks of these two: tests/draw_cases.py)
PH_BIND, PH_GEN_MOVES = 0x1000, 0x2000
EV_COLLISION = 0x10
KINDS = [0x08, 0x04, 0x02, 0x01]  # predicate bit order: CHROM_BOUNDARY, LEF_BAR, PRIMARY, SECONDARY


def load():
    with open(GOLDEN) as fh:
        return json.load(fh)


def all_vectors():
    d = load()
    return [(group, v) for group in ("stats", "matrix_internal", "matrix_dense", "collision_encoding",
                                     "property_tests") for v in d[group]]


def base_config():
    cfg = Config()
    cfg.bin_size = 1
    cfg.burnin_history_length = 100
    cfg.burnin_smoothing_window_size = 5
    cfg.lef_bar_major_collision_pblock = 1.0
    return cfg


# ---------------------------------------------------------------------------------------------
# backends
# ---------------------------------------------------------------------------------------------
class OracleUnits:
    """the CPU oracle (test infrastructure)"""
    name = "oracle"

    def __init__(self, binding):
        self.b = binding
        L = binding.lib()
        u64p = np.ctypeslib.ndpointer(dtype=np.uint64, flags="C_CONTIGUOUS")
        u32p = np.ctypeslib.ndpointer(dtype=np.uint32, flags="C_CONTIGUOUS")
        dp = C.POINTER(C.c_double)
        L.mo_loop_size_stats.argtypes = [C.c_size_t, u64p, u64p, dp, dp, dp, dp]
        L.mo_loop_size_stats.restype = None
        L.mo_matrix_increment.argtypes = [u32p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64,
                                          C.POINTER(C.c_uint64)]
        L.mo_matrix_increment.restype = None
        L.mo_collision_word.argtypes = [C.c_uint64, C.c_uint]
        L.mo_collision_word.restype = C.c_uint64
        L.mo_collision_predicates.argtypes = [C.c_uint64]
        L.mo_collision_predicates.restype = C.c_uint
        L.mo_select_and_bind_lefs.argtypes = ([C.c_uint64, C.c_uint64, C.c_size_t] + [u64p] * 5 +
                                              [C.c_uint64, C.POINTER(binding.Prng), u64p])
        L.mo_select_and_bind_lefs.restype = None
        self.L = L

    def loop_stats(self, rev, fwd):
        a, s, v, d = C.c_double(), C.c_double(), C.c_double(), C.c_double()
        self.L.mo_loop_size_stats(len(rev), rev, fwd, C.byref(a), C.byref(s), C.byref(v), C.byref(d))
        return {"mean": a.value, "ssd": s.value, "variance": v.value, "std": d.value}

    def matrix_increment(self, contacts, nrows, ncols, missed, pairs):
        m = C.c_uint64(missed)
        for r, c in pairs:
            self.L.mo_matrix_increment(contacts, nrows, ncols, r, c, C.byref(m))
        return m.value

    def collision(self, idx, ev):
        w = self.L.mo_collision_word(idx, ev)
        return w, self.L.mo_collision_predicates(w)

    def draws(self, kind, words, seed, m):
        return self.b.draw_many(kind, words, seed, m)

    def draw_forms(self, form, elements):
        return self.b.draw_forms(form, elements)

    def make_prng(self, seed):
        return self.b.prng_from_seed(seed)

    def draws_done(self, rng):
        return rng.count

    def select_and_bind(self, cfg, st, epoch_now, rng):
        scratch = np.zeros(3 * max(st.n, 1), dtype=np.uint64)
        self.L.mo_select_and_bind_lefs(st.start, st.end, st.n, st.rev_pos, st.fwd_pos, st.epoch,
                                       st.rev_rank, st.fwd_rank, epoch_now, C.byref(rng), scratch)

    def generate_moves(self, cfg, st, rng):
        self.L.mo_generate_moves(C.byref(cfg), st.start, st.end, st.n, st.rev_pos, st.fwd_pos,
                                 st.epoch, st.rev_rank, st.fwd_rank, st.rev_moves, st.fwd_moves,
                                 1, C.byref(rng), 1)


class DeviceUnits:
    """the product's device code: `units(cfg, what, pairs, nrows, ncols, contacts, missed) ->
    (out, missed)` and `phases(cfg, mask, st, state, skip) -> raws consumed` come from the lane
    emulator or from the GPU"""

    def __init__(self, name, units, phases, oracle_binding):
        self.name = name
        self._units = units
        self._phases = phases
        self.b = oracle_binding  # only for PRNG bookkeeping of the property tests' inputs

    def loop_stats(self, rev, fwd):
        pairs = np.stack([rev, fwd], axis=1).astype(np.uint64)
        out, _ = self._units(base_config(), UNIT_LOOP_STATS, pairs, 0, 0, None, 0)
        mean, std = out[:2].view(np.float64)
        # the device exposes what compute_loop_size_stats uses (mean, std); the two quantities in
        # between follow from std
        return {"mean": float(mean), "std": float(std), "variance": float(std) ** 2,
                "ssd": float(std) ** 2 * len(rev)}

    def matrix_increment(self, contacts, nrows, ncols, missed, pairs):
        _, m = self._units(base_config(), UNIT_MATRIX_INCREMENT, np.array(pairs, dtype=np.uint64),
                           nrows, ncols, contacts, missed)
        return m

    def collision(self, idx, ev):
        out, _ = self._units(base_config(), UNIT_COLLISION_WORDS,
                             np.array([[idx, ev]], dtype=np.uint64), 0, 0, None, 0)
        return int(out[0]), int(out[1])

    def draws(self, kind, words, seed, m):
        """m draws of one kind by the device's `*_exact` routines: (the draws, engine outputs consumed)"""
        call = np.zeros(2 * max(3, (m + 2) // 2), dtype=np.uint64)
        call[:6] = np.array([kind, seed] + list(words) + [m], dtype=np.uint64)
        out, _ = self._units(base_config(), UNIT_DRAWS, call, 0, 0, None, 0)
        return out[1:m + 1], int(out[0])

    def draw_forms(self, form, elements):
        """the pure forms on elements of four words: four words out per element"""
        el = np.ascontiguousarray(elements, dtype=np.uint64).reshape(-1)
        call = np.concatenate([np.array([form, 0], dtype=np.uint64), el])
        out, _ = self._units(base_config(), UNIT_DRAW_FORMS, call, 0, 0, None, 0)
        return out[2:].reshape(-1, 4)

    def make_prng(self, seed):
        from phase_backend import splitmix_seed
        return {"seed_state": splitmix_seed(seed), "consumed": 0}

    def draws_done(self, rng):
        return rng["consumed"]

    def _run(self, cfg, mask, st, rng):
        rng["consumed"] += self._phases(cfg, mask, st, list(rng["seed_state"]), rng["consumed"])

    def select_and_bind(self, cfg, st, epoch_now, rng):
        self._run(cfg, PH_BIND | (epoch_now << 16), st, rng)

    def generate_moves(self, cfg, st, rng):
        self._run(cfg, PH_GEN_MOVES, st, rng)


# ---------------------------------------------------------------------------------------------
# runner
# ---------------------------------------------------------------------------------------------
def _close(a, b, rel):
    return abs(a - b) <= rel * max(abs(a), abs(b))


def run_stats(be, v):
    vals = np.array(v["values"], dtype=np.uint64)
    rev = np.full(len(vals), 1000, dtype=np.uint64)
    got = be.loop_stats(rev, rev + vals)
    assert _close(got[v["what"]], v["expected"], v["rel_tolerance"]), (v["name"], got)
    if v["what"] == "mean":
        assert got["mean"] == v["expected"]  # integers: exact


def run_matrix_internal(be, v):
    if v["what"] == "transpose":
        nrows = ncols = 4
        for r, c, tr, tc in v["cases"]:
            a = np.zeros(nrows * ncols + 1, dtype=np.uint32)
            b = np.zeros(nrows * ncols + 1, dtype=np.uint32)
            be.matrix_increment(a, nrows, ncols, 0, [(r, c)])
            be.matrix_increment(b, nrows, ncols, 0, [(tr, tc)])
            assert a.sum() == 1 and np.array_equal(a, b), v["name"]
        return
    nrows = v["nrows"]
    ncols = 4
    for case in v["cases"]:
        if v["what"] == "encode":
            r, c, idx = case
        else:  # decode_idx(i) == (r, c)  <=>  encode_idx(r, c) == i (the layout is a bijection)
            idx, r, c = case
        a = np.zeros(nrows * ncols + 1, dtype=np.uint32)
        be.matrix_increment(a, nrows, ncols, 0, [(r, c)])
        assert np.flatnonzero(a).tolist() == [idx], (v["name"], case)


def run_matrix_dense(be, v):
    nrows, ncols = v["nrows"], v["ncols"]
    band = np.zeros(nrows * ncols + 1, dtype=np.uint32)
    missed = 0

    def cell(r, c):
        i, j = (r - c, r) if r > c else (c - r, c)
        return j * nrows + i if i < nrows else None

    for step in v["steps"]:
        if "op" in step:
            if step["op"] == "increment":
                missed = be.matrix_increment(band, nrows, ncols, missed, [(step["row"], step["col"])])
            else:
                # decrement / subtract are not on the simulation path: applied to the buffer here
                band[cell(step["row"], step["col"])] -= step["n"]
        elif step["check"] == "get":
            k = cell(*step["args"])
            assert (0 if k is None else int(band[k])) == step["expected"], (v["name"], step)
        elif step["check"] == "get_tot_contacts":
            assert int(band.sum()) == step["expected"], (v["name"], step)
        else:
            assert missed == step["expected"], (v["name"], step)


def run_collision(be, v):
    if v["what"] == "roundtrip":
        for idx in (v["index"], v["second_index"], (1 << 24) - 1):
            # (the device's word keeps 24 index bits, the reference's 55: the ABI widens it)
            for ev in v["events"]:
                w, _ = be.collision(idx, ev)
                assert w & ((1 << 56) - 1) == idx and w >> 56 == ev, (v["name"], idx, ev)
        w, f = be.collision(0, EV_COLLISION | 0x04)
        assert f & 1 and f & (4 << 1)  # set_event(COLLISION | LEF_BAR): occurred(LEF_BAR)
        w, f = be.collision(v["second_index"], 0x02)
        assert f & 2 and f & (64 << 2) and w & ((1 << 56) - 1) == v["second_index"]
        return
    k = KINDS.index(v["kind"])
    for idx in v["indices"]:
        _, f = be.collision(idx, EV_COLLISION | v["kind"])
        assert f & 1 and f & (4 << k) and not f & 2 and not f & (64 << k), v["name"]
        _, f = be.collision(idx, v["kind"])
        assert not f & 1 and not f & (4 << k) and f & 2 and f & (64 << k), v["name"]


def _blank_state(v, n):
    case = {"lefs": [[0, 0, 0]] * n, "interval": v["interval"]}
    st = KatState(case)
    st.rev_pos[:] = UNBOUND
    st.fwd_pos[:] = UNBOUND
    st.epoch[:] = UNBOUND
    return st


def _sorted_by_rank(st):
    rp = st.rev_pos[st.rev_rank.astype(np.int64)]
    fp = st.fwd_pos[st.fwd_rank.astype(np.int64)]
    return bool(np.all(np.diff(rp.astype(np.float64)) >= 0) and np.all(np.diff(fp.astype(np.float64)) >= 0))


def run_property(be, v, oracle_be=None, iters=None):
    """returns the final state so that callers can compare backends word for word"""
    cfg = base_config()
    iv = v["interval"]
    n = v["nlefs"]
    rng = be.make_prng(v["seed"])
    name = v["name"]
    if name.startswith("Bind LEFs"):
        st = _blank_state(v, n)
        if name.startswith("Bind LEFs 001"):
            # the mask: ten Bernoulli(0.5) draws from the test's engine (first ten outputs of the
            # stream, bernoulli = raw <= p * 2^64).  LEFs outside the mask are not to be touched:
            # they enter as bound LEFs (select_and_bind_lefs binds exactly the released ones)
            g = be.b.prng_from_seed(v["seed"])
            mask = [bool(be.b.lib().mo_bernoulli(C.byref(g), v["mask_probability"])) for _ in range(n)]
            if isinstance(rng, dict):
                rng["consumed"] = n
            else:
                rng = g
            for i in range(n):
                if not mask[i]:
                    st.rev_pos[i] = st.fwd_pos[i] = 100 + 37 * i
                    st.epoch[i] = 0
            before = (st.rev_pos.copy(), st.fwd_pos.copy())
        elif "002" in name:
            mask = [False] * n
            st.rev_pos[:] = np.arange(n) * 50 + 10
            st.fwd_pos[:] = st.rev_pos + 5
            st.epoch[:] = 0
            before = (st.rev_pos.copy(), st.fwd_pos.copy())
        else:
            mask = [True] * n
            before = None
        d0 = be.draws_done(rng)
        be.select_and_bind(cfg, st, 1, rng)
        assert _sorted_by_rank(st), name  # check_that_lefs_are_sorted_by_idx
        for i in range(n):
            if mask[i]:
                assert st.epoch[i] != UNBOUND and st.rev_pos[i] == st.fwd_pos[i], name
                assert iv["start"] <= st.rev_pos[i] < iv["end"], name
            else:
                assert st.rev_pos[i] == before[0][i] and st.fwd_pos[i] == before[1][i], name
        assert be.draws_done(rng) - d0 >= sum(mask)
        if not any(mask):
            assert be.draws_done(rng) == d0
        return st, be.draws_done(rng)
    # Generate LEF moves 001
    cfg.bin_size = v["bin_size"]
    cfg.rev_extrusion_speed = cfg.fwd_extrusion_speed = v["bin_size"]
    cfg.rev_extrusion_speed_std = cfg.fwd_extrusion_speed_std = v["bin_size"] * v["speed_std_fraction"]
    st = _blank_state(v, n)
    g = be.b.prng_from_seed(v["seed"])  # the engine of the test: positions, then moves, per iteration
    L = be.b.lib()
    for it in range(iters or v["iters"]):
        for i in range(n):
            st.rev_pos[i] = st.fwd_pos[i] = L.mo_uniform_int(C.byref(g), iv["start"], iv["end"] - 1)
            st.epoch[i] = it
        order = np.argsort(st.rev_pos, kind="stable").astype(np.uint64)
        st.rev_rank[:] = order
        st.fwd_rank[:] = order
        if isinstance(rng, dict):
            rng["consumed"] = g.count
            be.generate_moves(cfg, st, rng)
            for _ in range(rng["consumed"] - g.count):
                L.mo_prng_next(C.byref(g))
        else:
            be.generate_moves(cfg, st, g)
        assert np.all(st.rev_pos >= iv["start"] + st.rev_moves), name
        assert np.all(st.fwd_pos + st.fwd_moves < iv["end"]), name
        assert np.all(st.rev_pos < iv["end"]) and np.all(st.fwd_pos >= iv["start"]), name
    return st, g.count


def run_vector(be, group, v, **kw):
    return {"stats": run_stats, "matrix_internal": run_matrix_internal,
            "matrix_dense": run_matrix_dense, "collision_encoding": run_collision,
            "property_tests": run_property}[group](be, v, **kw)
