"""CPU checks of SLPSO at the drop-in boundary: the enum value, the layout and the defaults of
bbo_slpso_params, the untouched base of bbo_params, the Python signature against
tests/golden/class_surface.json and the "signature" of tests/golden/slpso_runs.json, the statuses of the
bbo_slpso_* entry points that need no handle, the argument checks and the refusal to run without a
device (the statuses that need a live handle are in tests/test_slpso_gpu.py)."""
import ctypes as C
import inspect
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mfev", "stol", "np", "omegamin", "omegamax", "eta", "gamma", "vmax", "Ufmax"]
SYMBOLS = ("bbo_slpso_params_default", "bbo_slpso_configure", "bbo_slpso_phase", "bbo_slpso_inject_draws")


def _golden(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as fh:
        return json.load(fh)


def test_algorithm_number_and_the_parameter_structs():
    import bboptpy_amd as bb
    from bboptpy_amd import _ffi
    assert bb.SLPSO._algo == _ffi.ALGO_SLPSO == 20
    # bbo_params is unchanged: stol rides in its existing field behind the base, as for DSA
    base = _ffi.Params.stol.offset
    size = C.sizeof(_ffi.Params)
    assert base == _ffi.Params.pcauchy.offset + 8 and size == base + 16
    fn = C.CDLL(_ffi.LIB_PATH).bbo_params_default
    fn.argtypes, fn.restype = [C.c_void_p, C.c_int], None
    buf = (C.c_ubyte * (size + 64))(*([0xA5] * (size + 64)))
    fn(C.addressof(buf), _ffi.ALGO_SLPSO)
    assert C.c_int.from_buffer(buf, 0).value == 20 and bytes(buf[size:]) == b"\xA5" * 64
    p = _ffi.default_params(_ffi.ALGO_SLPSO)
    assert (p.algo, p.np, p.populations, p.device, p.poll_every, p.stol) == (20, 0, 1, 0, 8, 0.)
    text = open(os.path.join(ROOT, "include", "bbopt_hip.h")).read()
    assert "BBO_ALGO_SLPSO = 20" in text
    assert "typedef struct { double omegamin, omegamax, eta, gamma, vmax, Ufmax; } bbo_slpso_params;" in text
    for name in SYMBOLS:
        assert name in text


def test_slpso_params_default_and_the_statuses_that_need_no_handle():
    from bboptpy_amd import _ffi
    L = _ffi.lib()
    d = _ffi.SlpsoParams()
    C.memset(C.byref(d), 0xA5, C.sizeof(d))
    L.bbo_slpso_params_default(C.byref(d))
    assert (d.omegamin, d.omegamax, d.eta, d.gamma, d.vmax, d.Ufmax) == (0.4, 0.9, 1.496, 0.01, 0.2, 10.)
    assert C.sizeof(_ffi.SlpsoParams) == 48
    assert [f[0] for f in _ffi.SlpsoParams._fields_] == NAMES[3:]
    assert [getattr(_ffi.SlpsoParams, k).offset for k in NAMES[3:]] == [0, 8, 16, 24, 32, 40]
    L.bbo_slpso_params_default(None)      # tolerated
    assert L.bbo_slpso_configure(None, C.byref(d)) == _ffi.ERR_ARG
    assert L.bbo_slpso_phase(None, 0) == _ffi.ERR_ARG
    assert L.bbo_slpso_inject_draws(None, None, 0) == _ffi.ERR_ARG
    for name in SYMBOLS:
        assert name in _ffi.EXPORTED_SYMBOLS and hasattr(C.CDLL(_ffi.LIB_PATH), name)
    assert (_ffi.SLPSO_PHASE_ADVANCE, _ffi.SLPSO_PHASE_EVALUATE, _ffi.SLPSO_PHASE_ABSORB) == (0, 1, 2)


def test_class_signature_is_the_reference_signature():
    import bboptpy_amd as bb
    E = inspect.Parameter.empty
    cls = bb.SLPSO
    ps = inspect.signature(cls.__init__).parameters
    mine = [(k, v.default) for k, v in ps.items() if k not in ("self", "ext")]
    surface = _golden("class_surface.json")["classes"]["SLPSO"]
    assert surface["base"] == "MultivariateSearch"
    want = [(a["name"], E if a["required"] else a["default"]) for a in surface["init"]["keywords"]]
    recorded = [(a["name"], E if a["required"] else a["default"]) for a in _golden("slpso_runs.json")["signature"]]
    assert want == recorded
    assert [k for k, _ in mine] == [k for k, _ in want] == NAMES
    for (k, got), (_, exp) in zip(mine, want):
        assert (got is E) == (exp is E), k
        if exp is not E:
            assert got == exp and type(got) is type(exp), (k, got, exp)
    assert any(v.kind is inspect.Parameter.VAR_KEYWORD for v in ps.values())
    assert bb.MultivariateSearch in cls.__mro__[1:] and not issubclass(cls, bb.BaseCMAES)
    assert "SLPSO" in bb.__all__ and cls._accepts_program is False
    for name in ("optimize", "initialize", "iterate", "solution", "run", "phase", "inject_draws"):
        assert callable(getattr(cls, name))


def test_constructor_marshals_both_structs():
    import bboptpy_amd as bb
    a = bb.SLPSO(5000, 1e-6, 20, seed=9, populations=3, poll_every=2)
    p, s = a._params, a._slpso
    assert (p.algo, p.mfev, p.stol, p.np, p.seed, p.populations, p.poll_every) == (20, 5000, 1e-6, 20, 9, 3, 2)
    assert (s.omegamin, s.omegamax, s.eta, s.gamma, s.vmax, s.Ufmax) == (0.4, 0.9, 1.496, 0.01, 0.2, 10.)
    assert a._record_draws is False
    a = bb.SLPSO(700, 0.5, 7, 0.3, 0.8, 1.5, 0.02, 0.25, 4., record_draws=True)
    s = a._slpso
    assert (s.omegamin, s.omegamax, s.eta, s.gamma, s.vmax, s.Ufmax) == (0.3, 0.8, 1.5, 0.02, 0.25, 4.)
    assert a._record_draws is True
    a = bb.SLPSO(mfev=700, stol=0.5, np=7, Ufmax=1.)
    assert (a._params.mfev, a._params.stol, a._params.np, a._slpso.Ufmax) == (700, 0.5, 7, 1.)
    with pytest.raises(TypeError):
        bb.SLPSO(700, 1e-6)             # np is required
    with pytest.raises(TypeError):
        bb.SLPSO(700, 1e-6, 7, tol=1e-6)    # the reference's constructor has no tol


def test_argument_checks():
    """np < 2 and np > 4096 are refused by bbo_create with BBO_ERR_ARG before it looks for a device;
    the class refuses them, an infinite box, n > 512 and an objective program with a ValueError before it
    creates a handle (bbo_init refuses the same with BBO_ERR_ARG: tests/test_slpso_gpu.py)"""
    import bboptpy_amd as bb
    from bboptpy_amd import _ffi
    L = _ffi.lib()
    for bad in (0, 1, 4097):
        p = _ffi.default_params(_ffi.ALGO_SLPSO)
        p.mfev, p.np = 100, bad
        h = C.c_void_p()
        assert L.bbo_create(C.byref(p), C.byref(h)) == _ffi.ERR_ARG and not h.value
        assert b"SLPSO: np must be in [2, 4096]" in L.bbo_last_error(None)
    lo, up, x0 = -np.ones(3), np.ones(3), np.zeros(3)
    for bad in (1, 4097):
        with pytest.raises(ValueError, match=r"SLPSO: np must be in \[2, 4096\]"):
            bb.SLPSO(100, 1e-6, bad)._problem("sphere", lo, up, x0)
    for lo_bad, up_bad in ((np.array([-1., -np.inf, -1.]), up), (lo, np.array([1., 1., np.inf])),
                           (np.array([np.nan, -1., -1.]), up)):
        with pytest.raises(ValueError, match="the bounds must be finite"):
            bb.SLPSO(100, 1e-6, 5)._problem("sphere", lo_bad, up_bad, x0)
    with pytest.raises(ValueError, match=r"SLPSO: dimension must be in \[1, 512\]"):
        bb.SLPSO(100, 1e-6, 5)._problem("sphere", -np.ones(513), np.ones(513), np.zeros(513))
    bb.SLPSO(100, 1e-6, 5)._problem("sphere", -np.ones(512), np.ones(512), np.zeros(512))

    class Fake(bb.DeviceObjective):
        def __init__(self):     # no compilation: the class refuses before it looks at the program
            self._handle = None

        def __del__(self):
            pass

    with pytest.raises(ValueError, match="SLPSO does not take a DeviceObjective"):
        bb.SLPSO(100, 1e-6, 5)._problem(Fake(), lo, up, x0)


def test_no_device_no_run():
    """without a GPU bbo_create returns BBO_ERR_NO_DEVICE: there is no CPU path"""
    import bboptpy_amd as bb
    from bboptpy_amd import _ffi
    if _ffi.lib().bbo_device_count() > 0:
        return      # a GPU is visible here: tests/test_slpso_gpu.py runs
    p = _ffi.default_params(_ffi.ALGO_SLPSO)
    p.mfev, p.np = 100, 5
    h = C.c_void_p()
    assert _ffi.lib().bbo_create(C.byref(p), C.byref(h)) == -4 and not h.value
    with pytest.raises(_ffi.BboError) as ei:
        bb.SLPSO(100, 1e-6, 5).optimize(bb.objectives.sphere, -np.ones(4), np.ones(4), np.zeros(4))
    assert ei.value.status == -4
