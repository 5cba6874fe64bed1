"""CPU checks of DSA at the drop-in boundary: bbo_params_default for algorithm 13 (with `stol`
written) and for the older algorithms (nothing written behind the short struct),
bbo_dsa_params_default, the Python signature against the "signature" of
tests/golden/dsa_runs.json, and the refusal to run without a device (the statuses of
bbo_dsa_configure that need a live handle are in tests/test_dsa_gpu.py)."""
import ctypes as C
import inspect
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _signature():
    with open(os.path.join(ROOT, "tests", "golden", "dsa_runs.json")) as fh:
        return json.load(fh)["signature"]


def test_default_parameters_are_the_reference_defaults_with_stol_written():
    import bboptpy_amd as bb
    from bboptpy_amd import _ffi
    assert bb.DSA._algo == _ffi.ALGO_DSA == 13
    base = _ffi.Params.stol.offset
    assert base == _ffi.Params.pcauchy.offset + 8 and C.sizeof(_ffi.Params) == base + 16
    fn = C.CDLL(_ffi.LIB_PATH).bbo_params_default
    fn.argtypes, fn.restype = [C.c_void_p, C.c_int], None
    buf = (C.c_ubyte * (base + 64))(*([0xA5] * (base + 64)))
    fn(C.addressof(buf), _ffi.ALGO_DSA)
    assert C.c_int.from_buffer(buf, 0).value == 13
    assert bytes(buf[base:base + 16]) == b"\x00" * 16 and bytes(buf[base + 16:]) == b"\xA5" * 48
    p = _ffi.default_params(_ffi.ALGO_DSA)
    assert (p.algo, p.stol, p.populations, p.device) == (13, 0., 1, 0)


def test_older_algorithms_still_get_nothing_written_behind_the_short_struct():
    from bboptpy_amd import _ffi
    base = _ffi.Params.stol.offset
    fn = C.CDLL(_ffi.LIB_PATH).bbo_params_default
    fn.argtypes, fn.restype = [C.c_void_p, C.c_int], None
    for algo in range(13):
        if algo == _ffi.ALGO_CHOLESKY_CMAES:
            continue
        buf = (C.c_ubyte * (base + 64))(*([0xA5] * (base + 64)))
        fn(C.addressof(buf), algo)
        assert bytes(buf[base:]) == b"\xA5" * 64, algo
        assert C.c_int.from_buffer(buf, 0).value == algo


def test_dsa_params_default():
    from bboptpy_amd import _ffi
    L = _ffi.lib()
    d = _ffi.DsaParams()
    C.memset(C.byref(d), 0xA5, C.sizeof(d))
    L.bbo_dsa_params_default(C.byref(d))
    assert (d.adapt, d.nbatch) == (1, 100) and C.sizeof(_ffi.DsaParams) == 8
    L.bbo_dsa_params_default(None)      # tolerated
    assert L.bbo_dsa_configure(None, C.byref(d)) == _ffi.ERR_ARG
    for name in ("bbo_dsa_params_default", "bbo_dsa_configure"):
        assert name in _ffi.EXPORTED_SYMBOLS


def test_class_signature_is_the_reference_signature():
    import bboptpy_amd as bb
    E = inspect.Parameter.empty
    cls = bb.DSA
    ps = inspect.signature(cls.__init__).parameters
    mine = [(k, v.default) for k, v in ps.items() if k not in ("self", "ext")]
    want = [(a["name"], E if a["required"] else a["default"]) for a in _signature()]
    assert [k for k, _ in mine] == [k for k, _ in want] == ["mfev", "tol", "stol", "np", "adapt", "nbatch"]
    for (k, got), (_, exp) in zip(mine, want):
        assert (got is E) == (exp is E), k
        if exp is not E:
            assert got == exp and type(got) is type(exp), (k, got, exp)
    assert any(v.kind is inspect.Parameter.VAR_KEYWORD for v in ps.values())
    assert bb.MultivariateSearch in cls.__mro__[1:]
    assert "DSA" in bb.__all__ and cls._accepts_program is False
    for name in ("optimize", "initialize", "iterate", "solution"):
        assert callable(getattr(cls, name))


def test_constructor_marshals_both_structs():
    import bboptpy_amd as bb
    a = bb.DSA(5000, 1e-6, 1e-7, 40, seed=9, populations=3, poll_every=2)
    p, d = a._params, a._dsa
    assert (p.algo, p.mfev, p.tol, p.stol, p.np, p.seed, p.populations, p.poll_every) \
        == (13, 5000, 1e-6, 1e-7, 40, 9, 3, 2)
    assert (d.adapt, d.nbatch) == (1, 100)
    d = bb.DSA(5000, 1e-6, 1e-7, 40, False, 7)._dsa
    assert (d.adapt, d.nbatch) == (0, 7)


def test_no_device_no_run():
    """without a GPU bbo_create returns BBO_ERR_NO_DEVICE: there is no CPU path"""
    import bboptpy_amd as bb
    from bboptpy_amd import _ffi
    if _ffi.lib().bbo_device_count() > 0:
        pytest.skip("a GPU is visible here")
    p = _ffi.default_params(_ffi.ALGO_DSA)
    p.mfev, p.np = 100, 8
    h = C.c_void_p()
    assert _ffi.lib().bbo_create(C.byref(p), C.byref(h)) == -4 and not h.value
    with pytest.raises(_ffi.BboError) as ei:
        bb.DSA(100, 0., 0., 8).optimize(bb.objectives.sphere, -np.ones(4), np.ones(4), np.zeros(4))
    assert ei.value.status == -4
