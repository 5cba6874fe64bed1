"""CPU checks of ACD at the drop-in boundary: the Python signature against
tests/golden/class_surface.json and the "signature" of tests/golden/acd_runs.json,
bbo_acd_params_default, the untouched layout of bbo_params, the statuses of the bbo_acd_* entry points
that need no handle, the limits the class names before a handle exists, and the refusal to run without
a device (the statuses that need a live handle are in tests/test_acd_gpu.py)."""
import ctypes as C
import inspect
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mfev", "ftol", "xtol", "ksucc", "kunsucc"]
SYMBOLS = ("bbo_acd_params_default", "bbo_acd_configure", "bbo_acd_phase")


def _golden(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as fh:
        return json.load(fh)


def test_algorithm_number_and_the_untouched_parameter_struct():
    import bboptpy_amd as bb
    from bboptpy_amd import _ffi
    assert bb.ACD._algo == _ffi.ALGO_ACD == 23
    base = _ffi.Params.stol.offset
    assert base == _ffi.Params.pcauchy.offset + 8 and C.sizeof(_ffi.Params) == base + 16
    # xtol travels in `stol`, so the defaults cover the long struct and nothing behind it
    fn = C.CDLL(_ffi.LIB_PATH).bbo_params_default
    fn.argtypes, fn.restype = [C.c_void_p, C.c_int], None
    size = C.sizeof(_ffi.Params)
    buf = (C.c_ubyte * (size + 64))(*([0xA5] * (size + 64)))
    fn(C.addressof(buf), _ffi.ALGO_ACD)
    assert C.c_int.from_buffer(buf, 0).value == 23 and bytes(buf[size:]) == b"\xA5" * 64
    assert C.c_double.from_buffer(buf, base).value == 0.
    p = _ffi.default_params(_ffi.ALGO_ACD)
    # poll_every = 0 asks for the engine's own chunk: one sweep
    assert (p.algo, p.np, p.populations, p.device, p.poll_every, p.stol) == (23, 0, 1, 0, 0, 0.)
    for other in (_ffi.ALGO_SSDE, _ffi.ALGO_HEES, _ffi.ALGO_CMAES):
        assert _ffi.default_params(other).poll_every == 8       # (the generational engines keep 8)
    assert _ffi.default_params(_ffi.ALGO_CRS).poll_every == 0
    text = open(os.path.join(ROOT, "include", "bbopt_hip.h")).read()
    assert "BBO_ALGO_ACD = 23" in text and "bbo_acd_params" in text
    for name in SYMBOLS:
        assert name in text


def test_acd_params_default_and_the_statuses_that_need_no_handle():
    from bboptpy_amd import _ffi
    L = _ffi.lib()
    d = _ffi.AcdParams()
    C.memset(C.byref(d), 0xA5, C.sizeof(d))
    L.bbo_acd_params_default(C.byref(d))
    assert (d.ksucc, d.kunsucc, d.from_guess, d.speculate) == (2., 0.5, 0, 0)
    assert C.sizeof(_ffi.AcdParams) == 24
    L.bbo_acd_params_default(None)      # tolerated
    assert L.bbo_acd_configure(None, C.byref(d)) == _ffi.ERR_ARG
    assert L.bbo_acd_phase(None, 0) == _ffi.ERR_ARG
    for name in SYMBOLS:
        assert name in _ffi.EXPORTED_SYMBOLS and hasattr(C.CDLL(_ffi.LIB_PATH), name)
    assert (_ffi.ACD_PHASE_ADVANCE, _ffi.ACD_PHASE_EVALUATE, _ffi.ACD_PHASE_ABSORB) == (0, 1, 2)
    assert (_ffi.ACD_FLAG_CONVERGED, _ffi.ACD_FLAG_BUDGET, _ffi.ACD_RULE_FTOL, _ffi.ACD_RULE_XTOL) == (1, 2, 1, 2)


def test_class_signature_is_the_reference_signature():
    import bboptpy_amd as bb
    E = inspect.Parameter.empty
    cls = bb.ACD
    ps = inspect.signature(cls.__init__).parameters
    positional = [(k, v.default) for k, v in ps.items()
                  if v.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD and k != "self"]
    surface = _golden("class_surface.json")["classes"]["ACD"]
    assert surface["base"] == "MultivariateSearch"
    want = [(a["name"], E if a["required"] else a["default"]) for a in surface["init"]["keywords"]]
    recorded = [(a["name"], E if a["required"] else a["default"]) for a in _golden("acd_runs.json")["signature"]]
    assert want == recorded == positional
    assert [k for k, _ in positional] == NAMES
    # the extensions are keyword-only: a positional sixth argument cannot hit them
    for k in ("from_guess", "speculate"):
        assert ps[k].kind is inspect.Parameter.KEYWORD_ONLY and ps[k].default is False
    assert any(v.kind is inspect.Parameter.VAR_KEYWORD for v in ps.values())
    with pytest.raises(TypeError):
        bb.ACD(1000, 1e-8, 1e-8, 2., 0.5, True)
    assert bb.MultivariateSearch in cls.__mro__[1:] and not issubclass(cls, bb.BaseCMAES)
    assert "ACD" in bb.__all__ and cls._accepts_program is False
    for name in ("optimize", "initialize", "iterate", "solution", "run", "phase"):
        assert callable(getattr(cls, name))


def test_constructor_marshals_both_structs():
    import bboptpy_amd as bb
    a = bb.ACD(5000, 1e-9, 1e-7, seed=9, populations=3, poll_every=2)
    p, s = a._params, a._acd
    assert (p.algo, p.mfev, p.tol, p.stol, p.seed, p.populations, p.poll_every) == (23, 5000, 1e-9, 1e-7, 9, 3, 2)
    assert (s.ksucc, s.kunsucc, s.from_guess, s.speculate) == (2., 0.5, 0, 0)
    a = bb.ACD(700, 0.25, 0.5, 3., 0.25, from_guess=True)
    assert (a._params.mfev, a._params.tol, a._params.stol, a._params.poll_every) == (700, 0.25, 0.5, 0)
    assert (a._acd.ksucc, a._acd.kunsucc, a._acd.from_guess) == (3., 0.25, 1)
    a = bb.ACD(mfev=700, ftol=0.5, xtol=0.125, kunsucc=0.75)
    assert (a._params.mfev, a._params.tol, a._params.stol, a._acd.ksucc, a._acd.kunsucc) == (700, 0.5, 0.125, 2., 0.75)
    for args in ((700,), (700, 1e-8)):
        with pytest.raises(TypeError):
            bb.ACD(*args)                   # ftol and xtol are required
    with pytest.raises(TypeError):
        bb.ACD(700, 1e-8, 1e-8, np=7)       # the reference's constructor has no such argument
    with pytest.raises(ValueError, match="speculative sweep was measured and dropped"):
        bb.ACD(700, 1e-8, 1e-8, speculate=True)


def test_a_device_objective_and_the_limits_are_refused_by_the_class():
    import bboptpy_amd as bb

    class Fake(bb.DeviceObjective):
        def __init__(self):     # no compilation: the class refuses before it looks at the program
            self._handle = None

        def __del__(self):
            pass

    with pytest.raises(ValueError, match="ACD does not take a DeviceObjective yet: objective programs are "
                                         "supported by CMAES"):
        bb.ACD(100, 0., 0.)._problem(Fake(), -np.ones(3), np.ones(3), np.zeros(3))
    # the limits the class names before a handle exists
    with pytest.raises(ValueError, match=r"ACD: dimension must be in \[1, 128\]"):
        bb.ACD(100, 0., 0.)._problem("sphere", -np.ones(129), np.ones(129), np.zeros(129))
    bb.ACD(100, 0., 0.)._problem("sphere", -np.ones(128), np.ones(128), np.zeros(128))
    with pytest.raises(ValueError, match="ACD draws x_best from .*finite"):
        bb.ACD(100, 0., 0.)._problem("sphere", -np.ones(3), np.array([1., np.inf, 1.]), np.zeros(3))
    with pytest.raises(ValueError, match="finite"):
        bb.ACD(100, 0., 0.)._problem("sphere", np.array([-np.inf, -1.]), np.ones(2), np.zeros(2))


def test_no_device_no_run():
    """without a GPU bbo_create returns BBO_ERR_NO_DEVICE: there is no CPU path"""
    import bboptpy_amd as bb
    from bboptpy_amd import _ffi
    if _ffi.lib().bbo_device_count() > 0:
        return      # a GPU is visible here: tests/test_acd_gpu.py runs
    p = _ffi.default_params(_ffi.ALGO_ACD)
    p.mfev = 100
    h = C.c_void_p()
    assert _ffi.lib().bbo_create(C.byref(p), C.byref(h)) == -4 and not h.value
    with pytest.raises(_ffi.BboError) as ei:
        bb.ACD(100, 0., 0.).optimize(bb.objectives.sphere, -np.ones(4), np.ones(4), np.zeros(4))
    assert ei.value.status == -4
