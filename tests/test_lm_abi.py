"""CPU checks of LmCMAES at the drop-in boundary: the Python signature against
tests/golden/class_surface.json, bbo_lm_params_default, the enum value, the untouched layout of
bbo_params, the statuses of the bbo_lm_* entry points that need no handle, the refusals of the class
(a DeviceObjective, a restart driver's base, the BaseCMAES methods it does not have) and the refusal
to run without a device (the statuses that need a live handle are in tests/test_lm_gpu.py)."""
import ctypes as C
import inspect
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mfev", "tol", "np", "memory", "sigma0", "bound", "rademacher", "usenew"]
SYMBOLS = ("bbo_lm_params_default", "bbo_lm_configure", "bbo_lm_phase", "bbo_lm_inject_draws")


def _golden(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as fh:
        return json.load(fh)


def test_algorithm_number_and_the_untouched_parameter_struct():
    import bboptpy_amd as bb
    from bboptpy_amd import _ffi
    assert bb.LmCMAES._algo == _ffi.ALGO_LM_CMAES == 17
    base = _ffi.Params.stol.offset
    assert base == _ffi.Params.pcauchy.offset + 8 and C.sizeof(_ffi.Params) == base + 16
    # mfev, tol, np, sigma0 and bound travel in the part of the struct every caller has: nothing
    # behind it is written
    fn = C.CDLL(_ffi.LIB_PATH).bbo_params_default
    fn.argtypes, fn.restype = [C.c_void_p, C.c_int], None
    buf = (C.c_ubyte * (base + 64))(*([0xA5] * (base + 64)))
    fn(C.addressof(buf), _ffi.ALGO_LM_CMAES)
    assert C.c_int.from_buffer(buf, 0).value == 17 and bytes(buf[base:]) == b"\xA5" * 64
    p = _ffi.default_params(_ffi.ALGO_LM_CMAES)
    assert (p.algo, p.np, p.sigma0, p.bound, p.populations, p.device, p.poll_every) == (17, 0, 2., 0, 1, 0, 8)
    text = open(os.path.join(ROOT, "include", "bbopt_hip.h")).read()
    assert "BBO_ALGO_LM_CMAES = 17" in text and "bbo_lm_params" in text
    for name in SYMBOLS:
        assert name in text


def test_lm_params_default_and_the_statuses_that_need_no_handle():
    from bboptpy_amd import _ffi
    L = _ffi.lib()
    d = _ffi.LmParams()
    C.memset(C.byref(d), 0xA5, C.sizeof(d))
    L.bbo_lm_params_default(C.byref(d))
    assert (d.memory, d.rademacher, d.usenew) == (0, 1, 1)
    assert C.sizeof(_ffi.LmParams) == 12
    L.bbo_lm_params_default(None)      # tolerated
    assert L.bbo_lm_configure(None, C.byref(d)) == _ffi.ERR_ARG
    assert L.bbo_lm_phase(None, 0) == _ffi.ERR_ARG
    assert L.bbo_lm_inject_draws(None, None, 0) == _ffi.ERR_ARG
    for name in SYMBOLS:
        assert name in _ffi.EXPORTED_SYMBOLS and hasattr(C.CDLL(_ffi.LIB_PATH), name)
    assert (_ffi.LM_PHASE_SAMPLE, _ffi.LM_PHASE_EVALUATE, _ffi.LM_PHASE_RANK, _ffi.LM_PHASE_UPDATE,
            _ffi.LM_PHASE_HISTORY_STOP) == (0, 1, 2, 3, 4)
    assert (_ffi.LM_FLAG_MAXITER, _ffi.LM_FLAG_TOLHISTFUN, _ffi.LM_FLAG_EQUALFUNVALS, _ffi.LM_FLAG_SIGMA) == (1, 2, 3, 11)


def test_class_signature_is_the_reference_signature():
    import bboptpy_amd as bb
    E = inspect.Parameter.empty
    cls = bb.LmCMAES
    ps = inspect.signature(cls.__init__).parameters
    mine = [(k, v.default) for k, v in ps.items() if k not in ("self", "ext")]
    surface = _golden("class_surface.json")["classes"]["LmCMAES"]
    assert surface["base"] == "BaseCMAES"
    want = [(a["name"], E if a["required"] else a["default"]) for a in surface["init"]["keywords"]]
    assert [k for k, _ in mine] == [k for k, _ in want] == NAMES
    for (k, got), (_, exp) in zip(mine, want):
        assert (got is E) == (exp is E), k
        if exp is not E:
            assert got == exp and type(got) is type(exp), (k, got, exp)
    assert any(v.kind is inspect.Parameter.VAR_KEYWORD for v in ps.values())
    assert bb.BaseCMAES in cls.__mro__[1:] and bb.MultivariateSearch in cls.__mro__[1:]
    assert not issubclass(cls, bb.CMAES)
    assert "LmCMAES" in bb.__all__ and cls._accepts_program is False
    for name in ("optimize", "initialize", "iterate", "solution", "run", "phase", "inject_draws"):
        assert callable(getattr(cls, name))


def test_constructor_marshals_both_structs():
    import bboptpy_amd as bb
    a = bb.LmCMAES(5000, 1e-8, 24, seed=9, populations=3, poll_every=2)
    p, s = a._params, a._lm
    assert (p.algo, p.mfev, p.tol, p.np, p.sigma0, p.bound) == (17, 5000, 1e-8, 24, 2., 0)
    assert (p.seed, p.populations, p.poll_every) == (9, 3, 2)
    assert (s.memory, s.rademacher, s.usenew) == (0, 1, 1)
    a = bb.LmCMAES(700, 0., 7, 5, 0.5, True, False, False)
    assert (a._params.sigma0, a._params.bound) == (0.5, 1)
    assert (a._lm.memory, a._lm.rademacher, a._lm.usenew) == (5, 0, 0)
    a = bb.LmCMAES(mfev=700, tol=0., np=7, memory=3, sigma0=1., bound=True, rademacher=False, usenew=False)
    assert (a._lm.memory, a._lm.rademacher, a._lm.usenew, a._params.bound) == (3, 0, 0, 1)
    with pytest.raises(TypeError):
        bb.LmCMAES(700, 1e-8)                    # np is required
    with pytest.raises(TypeError):
        bb.LmCMAES(700, 1e-8, 7, eigenrate=0.25)  # the reference's constructor has no eigenrate


def test_a_device_objective_is_refused_by_the_class():
    import bboptpy_amd as bb

    class Fake(bb.DeviceObjective):
        def __init__(self):     # no compilation: the class refuses before it looks at the program
            self._handle = None

        def __del__(self):
            pass

    with pytest.raises(ValueError, match="LmCMAES does not take a DeviceObjective"):
        bb.LmCMAES(100, 1e-8, 6)._problem(Fake(), -np.ones(3), np.ones(3), np.zeros(3))


def test_no_base_of_a_restart_driver():
    import bboptpy_amd as bb
    for driver in (bb.IPopCMAES, bb.BiPopCMAES):
        with pytest.raises(TypeError) as ei:
            driver(bb.LmCMAES(100, 1e-8, 6), 1000)
        for legal in ("CMAES", "ActiveCMAES", "SepCMAES", "CholeskyCMAES"):
            assert legal in str(ei.value)
        assert "LmCMAES" in str(ei.value)
    # every other class as before
    with pytest.raises(TypeError, match="base must be a CMA-ES optimizer"):
        bb.IPopCMAES(bb.JADE(100, 6, 1e-8), 1000)
    bb.IPopCMAES(bb.SepCMAES(100, 1e-8, 6), 1000)


def test_the_methods_of_the_restart_drivers_engine_are_not_implemented():
    import bboptpy_amd as bb
    a = bb.LmCMAES(100, 1e-8, 6)
    for call in (lambda: a.inject_normals(np.zeros(3)), lambda: a.set_params(8, 1., 100), lambda: a.set_seed(3),
                 lambda: a.evaluate(np.zeros(3))):
        with pytest.raises(NotImplementedError, match="LmCMAES"):
            call()


def test_no_device_no_run():
    """without a GPU bbo_create returns BBO_ERR_NO_DEVICE: there is no CPU path"""
    import bboptpy_amd as bb
    from bboptpy_amd import _ffi
    if _ffi.lib().bbo_device_count() > 0:
        return      # a GPU is visible here: tests/test_lm_gpu.py runs
    p = _ffi.default_params(_ffi.ALGO_LM_CMAES)
    p.mfev, p.np = 100, 6
    h = C.c_void_p()
    assert _ffi.lib().bbo_create(C.byref(p), C.byref(h)) == -4 and not h.value
    with pytest.raises(_ffi.BboError) as ei:
        bb.LmCMAES(100, 1e-8, 6).optimize(bb.objectives.sphere, -np.ones(4), np.ones(4), np.zeros(4))
    assert ei.value.status == -4
