"""CPU checks of CRS at the drop-in boundary: the Python signature against
tests/golden/class_surface.json and the "signature" of tests/golden/crs_runs.json,
bbo_crs_params_default, the untouched layout of bbo_params, the statuses of the bbo_crs_* entry points
that need no handle, and the refusal to run without a device (the statuses that need a live handle are
in tests/test_crs_gpu.py)."""
import ctypes as C
import inspect
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mfev", "np", "tol"]
SYMBOLS = ("bbo_crs_params_default", "bbo_crs_configure", "bbo_crs_phase", "bbo_crs_inject_draws")


def _golden(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as fh:
        return json.load(fh)


def test_algorithm_number_and_the_untouched_parameter_struct():
    import bboptpy_amd as bb
    from bboptpy_amd import _ffi
    assert bb.CRS._algo == _ffi.ALGO_CRS == 21
    base = _ffi.Params.stol.offset
    assert base == _ffi.Params.pcauchy.offset + 8 and C.sizeof(_ffi.Params) == base + 16
    # mfev, np and tol travel in the part of the struct every caller has: nothing behind it is written
    fn = C.CDLL(_ffi.LIB_PATH).bbo_params_default
    fn.argtypes, fn.restype = [C.c_void_p, C.c_int], None
    buf = (C.c_ubyte * (base + 64))(*([0xA5] * (base + 64)))
    fn(C.addressof(buf), _ffi.ALGO_CRS)
    assert C.c_int.from_buffer(buf, 0).value == 21 and bytes(buf[base:]) == b"\xA5" * 64
    p = _ffi.default_params(_ffi.ALGO_CRS)
    # np has no default; poll_every = 0 asks for the engine's own chunk of iterations
    assert (p.algo, p.np, p.populations, p.device, p.poll_every) == (21, 0, 1, 0, 0)
    assert _ffi.default_params(_ffi.ALGO_NSHS).poll_every == 0
    for other in (_ffi.ALGO_SLPSO, _ffi.ALGO_HEES, _ffi.ALGO_CMAES):
        assert _ffi.default_params(other).poll_every == 8       # (the generational engines keep 8)
    text = open(os.path.join(ROOT, "include", "bbopt_hip.h")).read()
    assert "BBO_ALGO_CRS = 21" in text and "bbo_crs_params" in text
    for name in SYMBOLS:
        assert name in text


def test_crs_params_default_and_the_statuses_that_need_no_handle():
    from bboptpy_amd import _ffi
    L = _ffi.lib()
    d = _ffi.CrsParams()
    C.memset(C.byref(d), 0xA5, C.sizeof(d))
    L.bbo_crs_params_default(C.byref(d))
    assert (d.max_depth, d.repair) == (4096, 0)
    assert C.sizeof(_ffi.CrsParams) == 8
    L.bbo_crs_params_default(None)      # tolerated
    assert L.bbo_crs_configure(None, C.byref(d)) == _ffi.ERR_ARG
    assert L.bbo_crs_phase(None, 0) == _ffi.ERR_ARG
    assert L.bbo_crs_inject_draws(None, None, 0) == _ffi.ERR_ARG
    for name in SYMBOLS:
        assert name in _ffi.EXPORTED_SYMBOLS and hasattr(C.CDLL(_ffi.LIB_PATH), name)
    assert (_ffi.CRS_PHASE_ADVANCE, _ffi.CRS_PHASE_EVALUATE, _ffi.CRS_PHASE_ABSORB) == (0, 1, 2)
    assert (_ffi.CRS_FLAG_TOL, _ffi.CRS_FLAG_BUDGET, _ffi.CRS_FLAG_DEPTH) == (1, 2, 3)


def test_class_signature_is_the_reference_signature():
    import bboptpy_amd as bb
    E = inspect.Parameter.empty
    cls = bb.CRS
    ps = inspect.signature(cls.__init__).parameters
    mine = [(k, v.default) for k, v in ps.items() if k not in ("self", "ext")]
    surface = _golden("class_surface.json")["classes"]["CRS"]
    assert surface["base"] == "MultivariateSearch"
    want = [(a["name"], E if a["required"] else a["default"]) for a in surface["init"]["keywords"]]
    recorded = [(a["name"], E if a["required"] else a["default"]) for a in _golden("crs_runs.json")["signature"]]
    assert want == recorded
    assert [k for k, _ in mine] == [k for k, _ in want] == NAMES
    for (k, got), (_, exp) in zip(mine, want):
        assert got is E and exp is E, k         # all three are required, as bound
    # the extensions are keyword-only (**ext): a positional reference call cannot hit them
    assert any(v.kind is inspect.Parameter.VAR_KEYWORD for v in ps.values())
    with pytest.raises(TypeError):
        bb.CRS(1000, 10, 1e-6, True)
    assert bb.MultivariateSearch in cls.__mro__[1:] and not issubclass(cls, bb.BaseCMAES)
    assert "CRS" in bb.__all__ and cls._accepts_program is False
    for name in ("optimize", "initialize", "iterate", "solution", "run", "phase", "inject_draws"):
        assert callable(getattr(cls, name))


def test_constructor_marshals_both_structs():
    import bboptpy_amd as bb
    a = bb.CRS(5000, 20, 1e-6, seed=9, populations=3, poll_every=2)
    p, s = a._params, a._crs
    assert (p.algo, p.mfev, p.np, p.tol, p.seed, p.populations, p.poll_every) == (21, 5000, 20, 1e-6, 9, 3, 2)
    assert (s.max_depth, s.repair) == (4096, 0) and a._record_draws is False
    a = bb.CRS(700, 7, 0.25, repair=True, max_depth=64, record_draws=True)
    assert (a._params.mfev, a._params.np, a._params.tol, a._params.poll_every) == (700, 7, 0.25, 0)
    assert (a._crs.max_depth, a._crs.repair) == (64, 1) and a._record_draws is True
    a = bb.CRS(mfev=700, np=7, tol=0.5)
    assert (a._params.mfev, a._params.np, a._params.tol) == (700, 7, 0.5)
    for args in ((700,), (700, 7)):
        with pytest.raises(TypeError):
            bb.CRS(*args)                   # np and tol are required
    with pytest.raises(TypeError):
        bb.CRS(700, 7, 1e-6, sigma0=2.)     # the reference's constructor has no such argument


def test_a_device_objective_is_refused_by_the_class():
    import bboptpy_amd as bb

    class Fake(bb.DeviceObjective):
        def __init__(self):     # no compilation: the class refuses before it looks at the program
            self._handle = None

        def __del__(self):
            pass

    with pytest.raises(ValueError, match="CRS does not take a DeviceObjective"):
        bb.CRS(100, 5, 0.)._problem(Fake(), -np.ones(3), np.ones(3), np.zeros(3))
    # the limits the class names before a handle exists
    with pytest.raises(ValueError, match="np must be in"):
        bb.CRS(100, 1, 0.)._problem("sphere", -np.ones(3), np.ones(3), np.zeros(3))
    with pytest.raises(ValueError, match="finite"):
        bb.CRS(100, 5, 0.)._problem("sphere", -np.ones(3), np.array([1., np.inf, 1.]), np.zeros(3))


def test_no_device_no_run():
    """without a GPU bbo_create returns BBO_ERR_NO_DEVICE: there is no CPU path"""
    import bboptpy_amd as bb
    from bboptpy_amd import _ffi
    if _ffi.lib().bbo_device_count() > 0:
        return      # a GPU is visible here: tests/test_crs_gpu.py runs
    p = _ffi.default_params(_ffi.ALGO_CRS)
    p.mfev, p.np = 100, 5
    h = C.c_void_p()
    assert _ffi.lib().bbo_create(C.byref(p), C.byref(h)) == -4 and not h.value
    with pytest.raises(_ffi.BboError) as ei:
        bb.CRS(100, 5, 0.).optimize(bb.objectives.sphere, -np.ones(4), np.ones(4), np.zeros(4))
    assert ei.value.status == -4
