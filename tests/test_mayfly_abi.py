"""CPU checks of Mayfly at the drop-in boundary: the enum value and the header text, the exported symbols,
bbo_mayfly_params_default, the Python signature against the "signature" of tests/golden/mayfly_runs.json (the
names and defaults of the binding the reference writes out, commented away), and every refusal the class
names before a handle exists (the statuses that need a live handle are in tests/test_mayfly_gpu.py)."""
import ctypes as C
import inspect
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("bbo_mayfly_params_default", "bbo_mayfly_configure", "bbo_mayfly_inject_draws")
DEFAULTS = dict(a1=1., a2=1.5, a3=1.5, beta=2., dance=5., ddamp=0.8, fl=1., fldamp=0.99, gmin=0.8, gmax=0.8,
                vdamp=0.1, sigma=0.1, pmutdim=0.01, pmutnp=0.05, l=0.95)


def _signature():
    with open(os.path.join(ROOT, "tests", "golden", "mayfly_runs.json")) as fh:
        return json.load(fh)["signature"]


def test_algorithm_number_header_and_the_untouched_parameter_struct():
    import bboptpy_amd as bb
    from bboptpy_amd import _ffi
    assert bb.Mayfly._algo == _ffi.ALGO_MAYFLY == 24
    text = open(os.path.join(ROOT, "include", "bbopt_hip.h")).read()
    assert "BBO_ALGO_MAYFLY = 24" in text and "bbo_mayfly_params;" in text
    for name in SYMBOLS:
        assert name in text
    # np and mfev travel in the part of bbo_params every caller has: nothing behind it is written
    base = _ffi.Params.stol.offset
    fn = C.CDLL(_ffi.LIB_PATH).bbo_params_default
    fn.argtypes, fn.restype = [C.c_void_p, C.c_int], None
    buf = (C.c_ubyte * (base + 64))(*([0xA5] * (base + 64)))
    fn(C.addressof(buf), _ffi.ALGO_MAYFLY)
    assert C.c_int.from_buffer(buf, 0).value == 24 and bytes(buf[base:]) == b"\xA5" * 64
    p = _ffi.default_params(_ffi.ALGO_MAYFLY)
    assert (p.algo, p.np, p.mfev, p.populations, p.device, p.poll_every) == (24, 0, 0, 1, 0, 8)


def test_symbols_and_params_default():
    from bboptpy_amd import _ffi
    L = _ffi.lib()
    raw = C.CDLL(_ffi.LIB_PATH)
    for name in SYMBOLS:
        assert name in _ffi.EXPORTED_SYMBOLS and hasattr(raw, name)
    assert "bbo_mayfly_phase" not in _ffi.EXPORTED_SYMBOLS and not hasattr(raw, "bbo_mayfly_phase")
    d = _ffi.MayflyParams()
    C.memset(C.byref(d), 0xA5, C.sizeof(d))
    L.bbo_mayfly_params_default(C.byref(d))
    assert {k: getattr(d, k) for k in DEFAULTS} == DEFAULTS and (d.pgb, d.repair, d.substream) == (0, 0, 0)
    assert C.sizeof(_ffi.MayflyParams) == 15 * 8 + 16
    L.bbo_mayfly_params_default(None)       # tolerated
    assert L.bbo_mayfly_configure(None, C.byref(d)) == _ffi.ERR_ARG
    assert L.bbo_mayfly_inject_draws(None, None, 0) == _ffi.ERR_ARG


def test_class_signature_is_the_commented_binding():
    import bboptpy_amd as bb
    E = inspect.Parameter.empty
    ps = inspect.signature(bb.Mayfly.__init__).parameters
    positional = [(k, v.default) for k, v in ps.items()
                  if v.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD and k != "self"]
    want = [(a["name"], E if a["required"] else a["default"]) for a in _signature()]
    assert positional == want and [k for k, _ in want][:2] == ["np", "mfev"]
    keyword_only = {k for k, v in ps.items() if v.kind is inspect.Parameter.KEYWORD_ONLY}
    assert keyword_only == {"repair", "record_draws", "substream"} and ps["repair"].default is False
    assert any(v.kind is inspect.Parameter.VAR_KEYWORD for v in ps.values())     # seed, populations, poll_every
    with pytest.raises(TypeError):
        bb.Mayfly(20, 1000, 1., 1.5, 1.5, 2., 5., 0.8, 1., 0.99, 0.8, 0.8, 0.1, 0.1, 0.01, 0.05, 0.95, False, True)
    assert bb.MultivariateSearch in bb.Mayfly.__mro__[1:] and "Mayfly" in bb.__all__
    assert bb.Mayfly._accepts_program is False and bb.Mayfly._extension == "mayfly"
    for name in ("optimize", "initialize", "iterate", "solution", "run", "inject_draws"):
        assert callable(getattr(bb.Mayfly, name))


def test_constructor_marshals_both_structs():
    import bboptpy_amd as bb
    a = bb.Mayfly(20, 5000, seed=9, populations=3, poll_every=2)
    p, m = a._params, a._mayfly
    assert (p.algo, p.np, p.mfev, p.seed, p.populations, p.poll_every) == (24, 20, 5000, 9, 3, 2)
    assert {k: getattr(m, k) for k in DEFAULTS} == DEFAULTS and (m.pgb, m.repair) == (0, 0)
    a = bb.Mayfly(10, 700, 2., pmutnp=0.3, pgb=True, repair=True, record_draws=True)
    assert (a._mayfly.a1, a._mayfly.pmutnp, a._mayfly.pgb, a._mayfly.repair) == (2., 0.3, 1, 1) and a._record_draws
    with pytest.raises(TypeError):
        bb.Mayfly(20)                       # mfev is required
    with pytest.raises(TypeError):
        bb.Mayfly(20, 700, tol=1e-6)        # the reference's constructor has no such argument


def test_every_refusal_names_its_reason():
    import bboptpy_amd as bb

    class Fake(bb.DeviceObjective):
        def __init__(self):     # no compilation: the class refuses before it looks at the program
            self._handle = None

        def __del__(self):
            pass

    lo, up, g = -np.ones(3), np.ones(3), np.zeros(3)
    with pytest.raises(ValueError, match="Mayfly does not take a DeviceObjective"):
        bb.Mayfly(10, 1000)._problem(Fake(), lo, up, g)
    with pytest.raises(ValueError, match="np must be even.*zero vector of value 0"):
        bb.Mayfly(21, 1000)._problem("sphere", lo, up, g)
    with pytest.raises(ValueError, match=r"np must be in \[2, 4096\]"):
        bb.Mayfly(1, 1000)._problem("sphere", lo, up, g)
    with pytest.raises(ValueError, match=r"np must be in \[2, 4096\]"):
        bb.Mayfly(4098, 10 ** 6)._problem("sphere", lo, up, g)
    for mfev in (20, 19):
        with pytest.raises(ValueError, match="mfev must exceed 2 np.*g = 0/0"):
            bb.Mayfly(10, mfev)._problem("sphere", lo, up, g)
    with pytest.raises(ValueError, match="finite"):
        bb.Mayfly(10, 1000)._problem("sphere", lo, np.array([1., np.inf, 1.]), g)
    with pytest.raises(ValueError, match=r"dimension must be in \[1, 512\]"):
        bb.Mayfly(10, 1000)._problem("sphere", -np.ones(513), np.ones(513), np.zeros(513))
    # initialize() refuses the same way, before a handle is made
    a = bb.Mayfly(21, 1000)
    with pytest.raises(ValueError, match="np must be even"):
        a.initialize("sphere", lo, up, g)
    assert a._handle is None


def test_no_device_no_run():
    """without a GPU bbo_create returns BBO_ERR_NO_DEVICE: there is no CPU path; the parameter checks of the
    library come first"""
    import bboptpy_amd as bb
    from bboptpy_amd import _ffi
    L = _ffi.lib()
    for np_, mfev, why in ((21, 1000, "np must be even"), (0, 1000, "np must be in"), (10, 20, "mfev must exceed 2 np")):
        p = _ffi.default_params(_ffi.ALGO_MAYFLY)
        p.np, p.mfev = np_, mfev
        h = C.c_void_p()
        assert L.bbo_create(C.byref(p), C.byref(h)) == _ffi.ERR_ARG and not h.value
        assert why in L.bbo_last_error(None).decode()
    if L.bbo_device_count() > 0:
        return      # a GPU is visible here: tests/test_mayfly_gpu.py runs
    p = _ffi.default_params(_ffi.ALGO_MAYFLY)
    p.np, p.mfev = 10, 1000
    h = C.c_void_p()
    assert L.bbo_create(C.byref(p), C.byref(h)) == -4 and not h.value
    with pytest.raises(_ffi.BboError) as ei:
        bb.Mayfly(10, 1000).optimize(bb.objectives.sphere, -np.ones(4), np.ones(4), np.zeros(4))
    assert ei.value.status == -4
