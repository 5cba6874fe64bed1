"""CPU checks of SSDE at the drop-in boundary: the enum value, the layout and the defaults of
bbo_ssde_params, the untouched bbo_params, the Python signature against tests/golden/class_surface.json and
the "signature" of tests/golden/ssde_runs.json, the statuses of the bbo_ssde_* entry points that need no
handle, the argument checks and the refusal to run without a device (the statuses that need a live handle
are in tests/test_ssde_gpu.py)."""
import ctypes as C
import inspect
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mfev", "npinit", "tol", "patience", "npmin", "ptop", "h", "usede", "repaircr"]
SYMBOLS = ("bbo_ssde_params_default", "bbo_ssde_configure", "bbo_ssde_phase", "bbo_ssde_inject_draws")


def _golden(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as fh:
        return json.load(fh)


def test_algorithm_number_and_the_untouched_bbo_params():
    import bboptpy_amd as bb
    from bboptpy_amd import _ffi
    assert bb.SSDE._algo == _ffi.ALGO_SSDE == 22
    # bbo_params is unchanged: mfev, np (= npinit) and tol ride in the fields every caller has
    base = _ffi.Params.stol.offset
    size = C.sizeof(_ffi.Params)
    assert base == _ffi.Params.pcauchy.offset + 8 and size == base + 16
    fn = C.CDLL(_ffi.LIB_PATH).bbo_params_default
    fn.argtypes, fn.restype = [C.c_void_p, C.c_int], None
    buf = (C.c_ubyte * (size + 64))(*([0xA5] * (size + 64)))
    fn(C.addressof(buf), _ffi.ALGO_SSDE)
    # (SSDE has no long parameters: nothing behind the base is written)
    assert C.c_int.from_buffer(buf, 0).value == 22 and bytes(buf[base:]) == b"\xA5" * (size - base + 64)
    p = _ffi.default_params(_ffi.ALGO_SSDE)
    assert (p.algo, p.np, p.populations, p.device, p.poll_every) == (22, 0, 1, 0, 8)
    text = open(os.path.join(ROOT, "include", "bbopt_hip.h")).read()
    assert "BBO_ALGO_SSDE = 22" in text
    assert "typedef struct { int patience, npmin; double ptop; int h, usede, repaircr; } bbo_ssde_params;" in text
    for name in SYMBOLS:
        assert name in text


def test_ssde_params_default_and_the_statuses_that_need_no_handle():
    from bboptpy_amd import _ffi
    L = _ffi.lib()
    d = _ffi.SsdeParams()
    C.memset(C.byref(d), 0xA5, C.sizeof(d))
    L.bbo_ssde_params_default(C.byref(d))
    # the binding's defaults: usede is false there (the C++ header's own default is true)
    assert (d.patience, d.npmin, d.ptop, d.h, d.usede, d.repaircr) == (1000, 4, 0.11, 100, 0, 1)
    assert C.sizeof(_ffi.SsdeParams) == 32
    assert [f[0] for f in _ffi.SsdeParams._fields_] == NAMES[3:]
    assert [getattr(_ffi.SsdeParams, k).offset for k in NAMES[3:]] == [0, 4, 8, 16, 20, 24]
    L.bbo_ssde_params_default(None)      # tolerated
    assert L.bbo_ssde_configure(None, C.byref(d)) == _ffi.ERR_ARG
    assert L.bbo_ssde_phase(None, 0) == _ffi.ERR_ARG
    assert L.bbo_ssde_inject_draws(None, None, 0) == _ffi.ERR_ARG
    for name in SYMBOLS:
        assert name in _ffi.EXPORTED_SYMBOLS and hasattr(C.CDLL(_ffi.LIB_PATH), name)
    assert (_ffi.SSDE_PHASE_ADVANCE, _ffi.SSDE_PHASE_EVALUATE, _ffi.SSDE_PHASE_ABSORB) == (0, 1, 2)


def test_class_signature_is_the_reference_signature():
    import bboptpy_amd as bb
    E = inspect.Parameter.empty
    cls = bb.SSDE
    ps = inspect.signature(cls.__init__).parameters
    mine = [(k, v.default) for k, v in ps.items() if k not in ("self", "ext")]
    surface = _golden("class_surface.json")["classes"]["SSDE"]
    assert surface["base"] == "MultivariateSearch"
    want = [(a["name"], E if a["required"] else a["default"]) for a in surface["init"]["keywords"]]
    recorded = [(a["name"], E if a["required"] else a["default"]) for a in _golden("ssde_runs.json")["signature"]]
    assert want == recorded
    assert [k for k, _ in mine] == [k for k, _ in want] == NAMES
    for (k, got), (_, exp) in zip(mine, want):
        assert (got is E) == (exp is E), k
        if exp is not E:
            assert got == exp and type(got) is type(exp), (k, got, exp)
    assert any(v.kind is inspect.Parameter.VAR_KEYWORD for v in ps.values())
    assert bb.MultivariateSearch in cls.__mro__[1:] and not issubclass(cls, bb.BaseCMAES)
    assert "SSDE" in bb.__all__ and cls._accepts_program is False
    for name in ("optimize", "initialize", "iterate", "solution", "run", "phase", "inject_draws", "get_state",
                 "set_state"):
        assert callable(getattr(cls, name))


def test_constructor_marshals_both_structs():
    import bboptpy_amd as bb
    a = bb.SSDE(5000, 50, 1e-6, seed=9, populations=3, poll_every=2)
    p, s = a._params, a._ssde
    assert (p.algo, p.mfev, p.np, p.tol, p.seed, p.populations, p.poll_every) == (22, 5000, 50, 1e-6, 9, 3, 2)
    assert (s.patience, s.npmin, s.ptop, s.h, s.usede, s.repaircr) == (1000, 4, 0.11, 100, 0, 1)
    assert a._record_draws is False
    a = bb.SSDE(700, 30, 0.5, 7, 5, 0.2, 9, True, False, record_draws=True)
    s = a._ssde
    assert (s.patience, s.npmin, s.ptop, s.h, s.usede, s.repaircr) == (7, 5, 0.2, 9, 1, 0)
    assert a._record_draws is True
    a = bb.SSDE(mfev=700, npinit=12, tol=0.5, usede=True)
    assert (a._params.mfev, a._params.np, a._params.tol, a._ssde.usede) == (700, 12, 0.5, 1)
    with pytest.raises(TypeError):
        bb.SSDE(700, 12)                # tol is required
    with pytest.raises(TypeError):
        bb.SSDE(700, 12, 1e-6, np=12)   # the reference's constructor has no np


def test_argument_checks():
    """the class refuses npinit outside [4, 4096], an infinite box, n > 512 and an objective program with a
    ValueError before it creates a handle (bbo_init refuses the same, and what travels in bbo_ssde_params,
    with BBO_ERR_ARG: tests/test_ssde_gpu.py)"""
    import bboptpy_amd as bb
    lo, up, x0 = -np.ones(3), np.ones(3), np.zeros(3)
    for bad in (3, 4097):
        with pytest.raises(ValueError, match=r"SSDE: npinit must be in \[4, 4096\]"):
            bb.SSDE(100, bad, 1e-6)._problem("sphere", lo, up, x0)
    for lo_bad, up_bad in ((np.array([-1., -np.inf, -1.]), up), (lo, np.array([1., 1., np.inf])),
                           (np.array([np.nan, -1., -1.]), up)):
        with pytest.raises(ValueError, match="the bounds must be finite"):
            bb.SSDE(100, 5, 1e-6)._problem("sphere", lo_bad, up_bad, x0)
    with pytest.raises(ValueError, match=r"SSDE: dimension must be in \[1, 512\]"):
        bb.SSDE(100, 5, 1e-6)._problem("sphere", -np.ones(513), np.ones(513), np.zeros(513))
    bb.SSDE(100, 5, 1e-6)._problem("sphere", -np.ones(512), np.ones(512), np.zeros(512))

    class Fake(bb.DeviceObjective):
        def __init__(self):     # no compilation: the class refuses before it looks at the program
            self._handle = None

        def __del__(self):
            pass

    with pytest.raises(ValueError, match="SSDE does not take a DeviceObjective"):
        bb.SSDE(100, 5, 1e-6)._problem(Fake(), lo, up, x0)


def test_no_device_no_run():
    """without a GPU bbo_create returns BBO_ERR_NO_DEVICE: there is no CPU path"""
    import bboptpy_amd as bb
    from bboptpy_amd import _ffi
    if _ffi.lib().bbo_device_count() > 0:
        return      # a GPU is visible here: tests/test_ssde_gpu.py runs
    p = _ffi.default_params(_ffi.ALGO_SSDE)
    p.mfev, p.np = 100, 5
    h = C.c_void_p()
    assert _ffi.lib().bbo_create(C.byref(p), C.byref(h)) == -4 and not h.value
    with pytest.raises(_ffi.BboError) as ei:
        bb.SSDE(100, 5, 1e-6).optimize(bb.objectives.sphere, -np.ones(4), np.ones(4), np.zeros(4))
    assert ei.value.status == -4
