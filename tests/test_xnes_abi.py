"""CPU: what xNES adds to the C ABI and the Python surface -- the constructor against
tests/golden/class_surface.json, bbo_xnes_params_default, the enum value, the untouched layout of
bbo_params, the statuses of the bbo_xnes_* entry points that need no handle, the refusal of a
DeviceObjective and the refusal to run without a device (the statuses that need a live handle are
in tests/test_xnes_gpu.py)."""
import ctypes as C
import inspect
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mfev", "tol", "a0", "etamu"]
SYMBOLS = ("bbo_xnes_params_default", "bbo_xnes_configure", "bbo_xnes_phase", "bbo_xnes_inject_normals")


def _golden(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as fh:
        return json.load(fh)


def test_algorithm_number_and_the_untouched_parameter_struct():
    import bboptpy_amd as bb
    from bboptpy_amd import _ffi
    assert bb.xNES._algo == _ffi.ALGO_XNES == 18
    base = _ffi.Params.stol.offset
    assert base == _ffi.Params.pcauchy.offset + 8 and C.sizeof(_ffi.Params) == base + 16
    # mfev and tol travel in the part of the struct every caller has: nothing behind it is written
    fn = C.CDLL(_ffi.LIB_PATH).bbo_params_default
    fn.argtypes, fn.restype = [C.c_void_p, C.c_int], None
    buf = (C.c_ubyte * (base + 64))(*([0xA5] * (base + 64)))
    fn(C.addressof(buf), _ffi.ALGO_XNES)
    assert C.c_int.from_buffer(buf, 0).value == 18 and bytes(buf[base:]) == b"\xA5" * 64
    p = _ffi.default_params(_ffi.ALGO_XNES)
    assert (p.algo, p.populations, p.device, p.poll_every) == (18, 1, 0, 8)
    text = open(os.path.join(ROOT, "include", "bbopt_hip.h")).read()
    assert "BBO_ALGO_XNES = 18" in text and "bbo_xnes_params" in text
    for name in SYMBOLS:
        assert name in text


def test_xnes_params_default_and_the_statuses_that_need_no_handle():
    from bboptpy_amd import _ffi
    L = _ffi.lib()
    d = _ffi.XnesParams()
    C.memset(C.byref(d), 0xA5, C.sizeof(d))
    L.bbo_xnes_params_default(C.byref(d))
    assert (d.a0, d.etamu, d.from_guess) == (1., 1., 0)
    assert C.sizeof(_ffi.XnesParams) == 24
    L.bbo_xnes_params_default(None)      # tolerated
    assert L.bbo_xnes_configure(None, C.byref(d)) == _ffi.ERR_ARG
    assert L.bbo_xnes_phase(None, 0) == _ffi.ERR_ARG
    assert L.bbo_xnes_inject_normals(None, None, 0) == _ffi.ERR_ARG
    for name in SYMBOLS:
        assert name in _ffi.EXPORTED_SYMBOLS and hasattr(C.CDLL(_ffi.LIB_PATH), name)
    assert (_ffi.XNES_PHASE_SAMPLE, _ffi.XNES_PHASE_RANK, _ffi.XNES_PHASE_STEP, _ffi.XNES_PHASE_ADAPT) == (0, 1, 2, 3)


def test_class_signature_is_the_reference_signature():
    import bboptpy_amd as bb
    E = inspect.Parameter.empty
    cls = bb.xNES
    ps = inspect.signature(cls.__init__).parameters
    positional = [(k, v.default) for k, v in ps.items()
                  if v.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD and k != "self"]
    surface = _golden("class_surface.json")["classes"]["xNES"]
    assert surface["base"] == "MultivariateSearch"
    want = [(a["name"], E if a["required"] else a["default"]) for a in surface["init"]["keywords"]]
    assert [k for k, _ in positional] == [k for k, _ in want] == NAMES
    for (k, got), (_, exp) in zip(positional, want):
        assert (got is E) == (exp is E), k
        if exp is not E:
            assert got == exp and type(got) is type(exp), (k, got, exp)
    # the extensions are keyword-only
    assert ps["from_guess"].kind is inspect.Parameter.KEYWORD_ONLY and ps["from_guess"].default is False
    assert any(v.kind is inspect.Parameter.VAR_KEYWORD for v in ps.values())
    assert bb.MultivariateSearch in cls.__mro__[1:] and not issubclass(cls, bb.BaseCMAES)
    assert "xNES" in bb.__all__ and cls._accepts_program is False
    for name in ("optimize", "initialize", "iterate", "solution", "run", "phase", "inject_normals", "get_state"):
        assert callable(getattr(cls, name))


def test_constructor_marshals_both_structs():
    import bboptpy_amd as bb
    a = bb.xNES(5000, 1e-8, seed=9, populations=3, poll_every=2)
    p, s = a._params, a._xnes
    assert (p.algo, p.mfev, p.tol) == (18, 5000, 1e-8)
    assert (p.seed, p.populations, p.poll_every) == (9, 3, 2)
    assert (s.a0, s.etamu, s.from_guess) == (1., 1., 0)
    a = bb.xNES(700, 0., 0.5, 0.9, from_guess=True)
    assert (a._xnes.a0, a._xnes.etamu, a._xnes.from_guess) == (0.5, 0.9, 1)
    a = bb.xNES(mfev=700, tol=0., a0=2., etamu=0.5)
    assert (a._xnes.a0, a._xnes.etamu, a._params.mfev) == (2., 0.5, 700)
    with pytest.raises(TypeError):
        bb.xNES(700)                            # tol is required
    with pytest.raises(TypeError):
        bb.xNES(700, 1e-8, 1., 1., True)        # from_guess is keyword-only
    with pytest.raises(TypeError):
        bb.xNES(700, 1e-8, np=12)               # the population size is no parameter


def test_a_device_objective_is_refused_by_the_class():
    import bboptpy_amd as bb

    class Fake(bb.DeviceObjective):
        def __init__(self):     # no compilation: the class refuses before it looks at the program
            self._handle = None

        def __del__(self):
            pass

    with pytest.raises(ValueError, match="xNES does not take a DeviceObjective"):
        bb.xNES(100, 1e-8)._problem(Fake(), -np.ones(3), np.ones(3), np.zeros(3))


def test_no_base_of_a_restart_driver():
    import bboptpy_amd as bb
    with pytest.raises(TypeError):
        bb.IPopCMAES(bb.xNES(100, 1e-8), 1000)


def test_no_device_no_run():
    """without a GPU bbo_create returns BBO_ERR_NO_DEVICE: there is no CPU path"""
    import bboptpy_amd as bb
    from bboptpy_amd import _ffi
    if _ffi.lib().bbo_device_count() > 0:
        return      # a GPU is visible here: tests/test_xnes_gpu.py runs
    p = _ffi.default_params(_ffi.ALGO_XNES)
    p.mfev = 100
    h = C.c_void_p()
    assert _ffi.lib().bbo_create(C.byref(p), C.byref(h)) == -4 and not h.value
    with pytest.raises(_ffi.BboError) as ei:
        bb.xNES(100, 1e-8).optimize(bb.objectives.sphere, -np.ones(4), np.ones(4), np.zeros(4))
    assert ei.value.status == -4
