"""CPU: what AMALGAM adds to the C ABI and the Python surface -- the constructor against
tests/golden/class_surface.json, bbo_amalgam_params_default, the enum value, the untouched layout of
bbo_params, the statuses of the bbo_amalgam_* entry points that need no handle, the refusal of a
DeviceObjective and the refusal to run without a device (the statuses that need a live handle are
in tests/test_amalgam_gpu.py)."""
import ctypes as C
import inspect
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mfev", "tol", "stol", "np", "iamalgam", "noparam", "print"]
SYMBOLS = ("bbo_amalgam_params_default", "bbo_amalgam_configure", "bbo_amalgam_phase", "bbo_amalgam_inject_draws",
           "bbo_amalgam_inject_points")


def _golden(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as fh:
        return json.load(fh)


def test_algorithm_number_and_the_untouched_parameter_struct():
    import bboptpy_amd as bb
    from bboptpy_amd import _ffi
    assert bb.AMALGAM._algo == _ffi.ALGO_AMALGAM == 19
    # the layout every earlier caller knows: the struct ends 16 bytes behind `stol`, which follows `pcauchy`
    base = _ffi.Params.stol.offset
    assert base == _ffi.Params.pcauchy.offset + 8 and C.sizeof(_ffi.Params) == base + 16
    assert _ffi.Params.ranked.offset == base + 8
    # stol travels in the long struct (a caller that can name algorithm 19 has it): nothing behind it is written
    fn = C.CDLL(_ffi.LIB_PATH).bbo_params_default
    fn.argtypes, fn.restype = [C.c_void_p, C.c_int], None
    size = C.sizeof(_ffi.Params)
    buf = (C.c_ubyte * (size + 64))(*([0xA5] * (size + 64)))
    fn(C.addressof(buf), _ffi.ALGO_AMALGAM)
    assert C.c_int.from_buffer(buf, 0).value == 19 and bytes(buf[size:]) == b"\xA5" * 64
    assert C.c_double.from_buffer(buf, base).value == 0.
    p = _ffi.default_params(_ffi.ALGO_AMALGAM)
    assert (p.algo, p.populations, p.device, p.poll_every, p.np, p.stol) == (19, 1, 0, 8, 0, 0.)
    text = open(os.path.join(ROOT, "include", "bbopt_hip.h")).read()
    assert "BBO_ALGO_AMALGAM = 19" in text and "bbo_amalgam_params" in text
    for name in SYMBOLS:
        assert name in text


def test_amalgam_params_default_and_the_statuses_that_need_no_handle():
    from bboptpy_amd import _ffi
    L = _ffi.lib()
    d = _ffi.AmalgamParams()
    C.memset(C.byref(d), 0xA5, C.sizeof(d))
    L.bbo_amalgam_params_default(C.byref(d))
    assert (d.iamalgam, d.noparam, d.print, d.keep_elite, d.concurrent, d.substream) == (1, 1, 1, 0, 1, 0)
    assert C.sizeof(_ffi.AmalgamParams) == 24
    L.bbo_amalgam_params_default(None)      # tolerated
    assert L.bbo_amalgam_configure(None, C.byref(d)) == _ffi.ERR_ARG
    assert L.bbo_amalgam_phase(None, 0) == _ffi.ERR_ARG
    assert L.bbo_amalgam_inject_draws(None, None, 0, None, 0) == _ffi.ERR_ARG
    assert L.bbo_amalgam_inject_points(None, None, 0) == _ffi.ERR_ARG
    for name in SYMBOLS:
        assert name in _ffi.EXPORTED_SYMBOLS and hasattr(C.CDLL(_ffi.LIB_PATH), name)
    assert (_ffi.AMALGAM_PHASE_DISTRIBUTION, _ffi.AMALGAM_PHASE_SAMPLE, _ffi.AMALGAM_PHASE_ADAPT) == (0, 1, 2)


def test_class_signature_is_the_reference_signature():
    import bboptpy_amd as bb
    E = inspect.Parameter.empty
    cls = bb.AMALGAM
    ps = inspect.signature(cls.__init__).parameters
    positional = [(k, v.default) for k, v in ps.items()
                  if v.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD and k != "self"]
    surface = _golden("class_surface.json")["classes"]["AMALGAM"]
    assert surface["base"] == "MultivariateSearch"
    want = [(a["name"], E if a["required"] else a["default"]) for a in surface["init"]["keywords"]]
    assert [k for k, _ in positional] == [k for k, _ in want] == NAMES
    for (k, got), (_, exp) in zip(positional, want):
        assert (got is E) == (exp is E), k
        if exp is not E:
            assert got == exp and type(got) is type(exp), (k, got, exp)
    # the extensions are keyword-only
    for k, dflt in (("keep_elite", False), ("concurrent", True)):
        assert ps[k].kind is inspect.Parameter.KEYWORD_ONLY and ps[k].default is dflt
    assert any(v.kind is inspect.Parameter.VAR_KEYWORD for v in ps.values())
    assert bb.MultivariateSearch in cls.__mro__[1:] and not issubclass(cls, bb.BaseCMAES)
    assert "AMALGAM" in bb.__all__ and cls._accepts_program is False
    for name in ("optimize", "initialize", "iterate", "solution", "run", "phase", "inject_draws", "inject_points",
                 "get_state", "set_state"):
        assert callable(getattr(cls, name))


def test_constructor_marshals_both_structs():
    import bboptpy_amd as bb
    a = bb.AMALGAM(5000, 1e-6, 1e-8, seed=9, poll_every=2)
    p, s = a._params, a._amalgam
    assert (p.algo, p.mfev, p.tol, p.stol, p.np) == (19, 5000, 1e-6, 1e-8, 0)
    assert (p.seed, p.populations, p.poll_every) == (9, 1, 2)
    assert (s.iamalgam, s.noparam, s.print, s.keep_elite, s.concurrent, s.substream) == (1, 1, 1, 0, 1, 0)
    a = bb.AMALGAM(700, 0., 1e-9, 40, False, False, False, keep_elite=True, concurrent=False, populations=3,
                   substream=4)
    s = a._amalgam
    assert (a._params.np, a._params.populations) == (40, 3)
    assert (s.iamalgam, s.noparam, s.print, s.keep_elite, s.concurrent, s.substream) == (0, 0, 0, 1, 0, 4)
    a = bb.AMALGAM(mfev=700, tol=0., stol=1e-3, np=12, iamalgam=False, noparam=False, print=False)
    assert (a._params.stol, a._params.np, a._amalgam.iamalgam) == (1e-3, 12, 0)
    with pytest.raises(TypeError):
        bb.AMALGAM(700, 1e-8)                                       # stol is required
    with pytest.raises(TypeError):
        bb.AMALGAM(700, 1e-8, 1e-8, 0, True, True, True, True)      # keep_elite is keyword-only
    with pytest.raises(ValueError, match="populations=1"):
        bb.AMALGAM(700, 1e-8, 1e-8, populations=2)                  # the parameter-free mode is the default


def test_a_device_objective_is_refused_by_the_class():
    import bboptpy_amd as bb

    class Fake(bb.DeviceObjective):
        def __init__(self):     # no compilation: the class refuses before it looks at the program
            self._handle = None

        def __del__(self):
            pass

    with pytest.raises(ValueError, match="AMALGAM does not take a DeviceObjective"):
        bb.AMALGAM(100, 1e-8, 1e-8)._problem(Fake(), -np.ones(3), np.ones(3), np.zeros(3))


def test_no_device_no_run():
    """without a GPU bbo_create returns BBO_ERR_NO_DEVICE: there is no CPU path"""
    import bboptpy_amd as bb
    from bboptpy_amd import _ffi
    if _ffi.lib().bbo_device_count() > 0:
        return      # a GPU is visible here: tests/test_amalgam_gpu.py runs
    p = _ffi.default_params(_ffi.ALGO_AMALGAM)
    p.mfev = 100
    h = C.c_void_p()
    assert _ffi.lib().bbo_create(C.byref(p), C.byref(h)) == -4 and not h.value
    with pytest.raises(_ffi.BboError) as ei:
        bb.AMALGAM(100, 1e-8, 1e-8).optimize(bb.objectives.sphere, -np.ones(4), np.ones(4), np.zeros(4))
    assert ei.value.status == -4
