"""The device code's random draws (sim_rng.h) under the lane emulator against the oracle, word for word,
in every regime of tests/draw_cases.py: the draws and the count of engine outputs consumed
(MODLE_HIP_UNIT_DRAWS), and the pure forms on their edge inputs (MODLE_HIP_UNIT_DRAW_FORMS).  Both
geometries of the emulator builds: the 8-wave kernels' and the 12-wave kernels'."""
import ctypes as C

import numpy as np
import pytest

import draw_cases as dc
from unit_vector_runner import base_config

N_DRAWS = 1 << 14
GEOMETRIES = [None, "w12"]


def _emu_units(geometry):
    from modle_amd.params import Config
    from phase_backend import emu_lib

    L = emu_lib(geometry)
    u64p = np.ctypeslib.ndpointer(dtype=np.uint64, flags="C_CONTIGUOUS")
    L.emu_test_units.argtypes = [C.POINTER(Config), C.c_uint32, u64p, C.c_size_t, C.c_uint64, C.c_uint64,
                                 C.c_void_p, C.POINTER(C.c_uint64), u64p]
    L.emu_test_units.restype = C.c_int
    cfg = base_config()

    def units(what, words, out):
        m = C.c_uint64(0)
        assert L.emu_test_units(C.byref(cfg), what, words, len(words) // 2, 0, 0, None, C.byref(m), out) == 0

    return units


@pytest.fixture(scope="module", params=GEOMETRIES, ids=["w8", "w12"])
def emu_units(request):
    return _emu_units(request.param)


@pytest.mark.parametrize("regime", dc.REGIMES, ids=dc.REGIME_IDS)
def test_emulated_draws_equal_the_oracle(oracle, emu_units, regime):
    dc.check_draws(emu_units, oracle, regime, seed=7, m=N_DRAWS, pairs=N_DRAWS // 2 + 1)


@pytest.mark.parametrize("form,name,elements", dc.FORMS, ids=dc.FORM_IDS)
def test_emulated_forms_equal_the_oracle(oracle, emu_units, form, name, elements):
    dc.check_forms(emu_units, oracle, form, elements)


def test_oracle_forms_equal_python_integers(oracle):
    """the oracle's own forms on the same inputs (the identity backend): what check_forms holds against
    Python's integers is held on the oracle without any device code"""
    def units(what, words, out):
        out[2:] = oracle.draw_forms(int(words[0]), words[2:].reshape(-1, 4)).reshape(-1)

    for form, _, elements in dc.FORMS:
        dc.check_forms(units, oracle, form, elements)


def test_unit_vector_backends_draw_alike(oracle):
    """the same two units through the backends of tests/unit_vector_runner.py (oracle | emulated device code)"""
    from test_oracle_unit_vectors import _emu_backend
    from unit_vector_runner import OracleUnits

    be_o, be_d = OracleUnits(oracle), _emu_backend(oracle)
    for regime in (r for r in dc.REGIMES if r.name in ("poisson_10.5", "binomial_66_sixth", "normal_4000_200")):
        (a, na), (b, nb) = be_o.draws(regime.kind, regime.words, 3, 999), be_d.draws(regime.kind, regime.words, 3, 999)
        assert na == nb and np.array_equal(a, b), regime.name
    form, _, elements = dc.FORMS[2]
    assert np.array_equal(be_o.draw_forms(form, elements), be_d.draw_forms(form, elements))


def test_draws_unit_refuses_a_count_beyond_its_output(emu_units):
    """m + 1 words must fit the 2 n words of the call: the unit reports an error and writes nothing"""
    regime = dc.REGIMES[0]
    for m in (6, dc.M64):  # six draws and the count do not fit six words; nor does a count whose m + 1 wraps to 0
        words = dc.draws_call(regime, 7, 5, dc.HEAD_PAIRS)
        words[5] = m
        out = np.zeros(len(words), dtype=np.uint64)
        with pytest.raises(AssertionError):
            emu_units(dc.UNIT_DRAWS, words, out)
        assert not out.any()
