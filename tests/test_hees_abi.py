"""CPU checks of HEES at the drop-in boundary: the Python signature against
tests/golden/class_surface.json and the "signature" of tests/golden/hees_runs.json,
bbo_hees_params_default, the untouched layout of bbo_params, the statuses of bbo_hees_configure that
need no handle, and the refusal to run without a device (the statuses that need a live handle are
in tests/test_hees_gpu.py)."""
import ctypes as C
import inspect
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _golden(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as fh:
        return json.load(fh)


def test_algorithm_number_and_the_untouched_parameter_struct():
    import bboptpy_amd as bb
    from bboptpy_amd import _ffi
    assert bb.HEES._algo == _ffi.ALGO_HEES == 14
    base = _ffi.Params.stol.offset
    assert base == _ffi.Params.pcauchy.offset + 8 and C.sizeof(_ffi.Params) == base + 16
    # np and sigma0 travel in the part of the struct every caller has: nothing behind it is written
    fn = C.CDLL(_ffi.LIB_PATH).bbo_params_default
    fn.argtypes, fn.restype = [C.c_void_p, C.c_int], None
    buf = (C.c_ubyte * (base + 64))(*([0xA5] * (base + 64)))
    fn(C.addressof(buf), _ffi.ALGO_HEES)
    assert C.c_int.from_buffer(buf, 0).value == 14 and bytes(buf[base:]) == b"\xA5" * 64
    p = _ffi.default_params(_ffi.ALGO_HEES)
    assert (p.algo, p.np, p.sigma0, p.populations, p.device) == (14, 0, 2., 1, 0)
    text = open(os.path.join(ROOT, "include", "bbopt_hip.h")).read()
    assert "BBO_ALGO_HEES = 14" in text


def test_hees_params_default_and_the_statuses_that_need_no_handle():
    from bboptpy_amd import _ffi
    L = _ffi.lib()
    d = _ffi.HeesParams()
    C.memset(C.byref(d), 0xA5, C.sizeof(d))
    L.bbo_hees_params_default(C.byref(d))
    assert (d.mres, d.print) == (1, 0) and C.sizeof(_ffi.HeesParams) == 8
    L.bbo_hees_params_default(None)      # tolerated
    assert L.bbo_hees_configure(None, C.byref(d)) == _ffi.ERR_ARG
    assert L.bbo_hees_phase(None, 0) == _ffi.ERR_ARG
    assert L.bbo_hees_inject_normals(None, None, 0) == _ffi.ERR_ARG
    for name in ("bbo_hees_params_default", "bbo_hees_configure", "bbo_hees_phase",
                 "bbo_hees_inject_normals"):
        assert name in _ffi.EXPORTED_SYMBOLS and hasattr(C.CDLL(_ffi.LIB_PATH), name)


def test_class_signature_is_the_reference_signature():
    import bboptpy_amd as bb
    E = inspect.Parameter.empty
    cls = bb.HEES
    ps = inspect.signature(cls.__init__).parameters
    mine = [(k, v.default) for k, v in ps.items() if k not in ("self", "ext")]
    surface = _golden("class_surface.json")["classes"]["HEES"]
    assert surface["base"] == "MultivariateSearch"
    want = [(a["name"], E if a["required"] else a["default"]) for a in surface["init"]["keywords"]]
    recorded = [(a["name"], E if a["required"] else a["default"]) for a in _golden("hees_runs.json")["signature"]]
    assert want == recorded
    assert [k for k, _ in mine] == [k for k, _ in want] == ["mfev", "tol", "mres", "print", "np", "sigma0"]
    for (k, got), (_, exp) in zip(mine, want):
        assert (got is E) == (exp is E), k
        if exp is not E:
            assert got == exp and type(got) is type(exp), (k, got, exp)
    assert any(v.kind is inspect.Parameter.VAR_KEYWORD for v in ps.values())
    assert bb.MultivariateSearch in cls.__mro__[1:] and not issubclass(cls, bb.BaseCMAES)
    assert "HEES" in bb.__all__ and cls._accepts_program is False
    for name in ("optimize", "initialize", "iterate", "solution", "run", "phase", "inject_normals"):
        assert callable(getattr(cls, name))


def test_constructor_marshals_both_structs():
    import bboptpy_amd as bb
    a = bb.HEES(5000, 1e-6, seed=9, populations=3, poll_every=2)
    p, h = a._params, a._hees
    assert (p.algo, p.mfev, p.tol, p.np, p.sigma0, p.seed, p.populations, p.poll_every) \
        == (14, 5000, 1e-6, 0, 2., 9, 3, 2)
    assert (h.mres, h.print) == (1, 0)
    a = bb.HEES(5000, 1e-6, 3, True, 12, 0.5)
    assert (a._hees.mres, a._hees.print, a._params.np, a._params.sigma0) == (3, 1, 12, 0.5)
    with pytest.raises(ValueError, match="populations=1"):
        bb.HEES(5000, 1e-6, mres=2, populations=2)


def test_a_device_objective_is_refused_by_the_class():
    import bboptpy_amd as bb

    class Fake(bb.DeviceObjective):
        def __init__(self):     # no compilation: the class refuses before it looks at the program
            self._handle = None

        def __del__(self):
            pass

    with pytest.raises(ValueError, match="HEES does not take a DeviceObjective"):
        bb.HEES(100, 0.)._problem(Fake(), -np.ones(3), np.ones(3), np.zeros(3))


def test_no_device_no_run():
    """without a GPU bbo_create returns BBO_ERR_NO_DEVICE: there is no CPU path"""
    import bboptpy_amd as bb
    from bboptpy_amd import _ffi
    if _ffi.lib().bbo_device_count() > 0:
        pytest.skip("a GPU is visible here")
    p = _ffi.default_params(_ffi.ALGO_HEES)
    p.mfev = 100
    h = C.c_void_p()
    assert _ffi.lib().bbo_create(C.byref(p), C.byref(h)) == -4 and not h.value
    with pytest.raises(_ffi.BboError) as ei:
        bb.HEES(100, 0.).optimize(bb.objectives.sphere, -np.ones(4), np.ones(4), np.zeros(4))
    assert ei.value.status == -4
