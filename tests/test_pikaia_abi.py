"""CPU checks of PIKAIA at the drop-in boundary: the enum value and the header text, the exported symbols,
bbo_pikaia_params_default, the Python signature against the "signature" of tests/golden/pikaia_runs.json (the
names and defaults of the reference's constructor), both structs as the constructor marshals them, and every
refusal with its reason (the library's own refusals through bbo_pikaia_configure, which need a live handle, are
in tests/test_pikaia_gpu.py::test_the_library_refuses_what_the_class_refuses)."""
import ctypes as C
import inspect
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("bbo_pikaia_params_default", "bbo_pikaia_configure", "bbo_pikaia_inject_draws")
DEFAULTS = dict(pcross=0.85, pmut=0.005, pmutmn=0.0005, pmutmx=0.25, fdif=1., imut=2, irep=1, ielite=0)


def _signature():
    with open(os.path.join(ROOT, "tests", "golden", "pikaia_runs.json")) as fh:
        return json.load(fh)["signature"]


def test_algorithm_number_header_and_the_untouched_parameter_struct():
    import bboptpy_amd as bb
    from bboptpy_amd import _ffi
    assert bb.PIKAIA._algo == _ffi.ALGO_PIKAIA == 25
    text = open(os.path.join(ROOT, "include", "bbopt_hip.h")).read()
    assert "BBO_ALGO_PIKAIA = 25" in text and "bbo_pikaia_params;" in text
    for name in SYMBOLS:
        assert name in text
    # np, ngen and nd travel in the part of bbo_params every caller has: nothing behind it is written
    base = _ffi.Params.stol.offset
    fn = C.CDLL(_ffi.LIB_PATH).bbo_params_default
    fn.argtypes, fn.restype = [C.c_void_p, C.c_int], None
    buf = (C.c_ubyte * (base + 64))(*([0xA5] * (base + 64)))
    fn(C.addressof(buf), _ffi.ALGO_PIKAIA)
    assert C.c_int.from_buffer(buf, 0).value == 25 and bytes(buf[base:]) == b"\xA5" * 64


def test_symbols_and_params_default():
    from bboptpy_amd import _ffi
    L = _ffi.lib()
    raw = C.CDLL(_ffi.LIB_PATH)
    for name in SYMBOLS:
        assert name in _ffi.EXPORTED_SYMBOLS and hasattr(raw, name)
    assert "bbo_pikaia_phase" not in _ffi.EXPORTED_SYMBOLS and not hasattr(raw, "bbo_pikaia_phase")
    d = _ffi.PikaiaParams()
    C.memset(C.byref(d), 0xA5, C.sizeof(d))
    L.bbo_pikaia_params_default(C.byref(d))
    assert {k: getattr(d, k) for k in DEFAULTS} == DEFAULTS and (d.repair, d.raw, d.substream) == (0, 0, 0)
    assert C.sizeof(_ffi.PikaiaParams) == 5 * 8 + 6 * 4
    L.bbo_pikaia_params_default(None)       # tolerated
    assert L.bbo_pikaia_configure(None, C.byref(d)) == _ffi.ERR_ARG
    assert L.bbo_pikaia_inject_draws(None, None, 0) == _ffi.ERR_ARG


def test_class_signature_is_the_reference_constructor():
    import bboptpy_amd as bb
    from bboptpy_amd import multivariate
    E = inspect.Parameter.empty
    ps = inspect.signature(bb.PIKAIA.__init__).parameters
    positional = [(k, v.default) for k, v in ps.items()
                  if v.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD and k != "self"]
    want = [(a["name"], E if a["required"] else a["default"]) for a in _signature()]
    assert positional == want and [k for k, _ in want][:3] == ["np", "ngen", "nd"]
    keyword_only = {k for k, v in ps.items() if v.kind is inspect.Parameter.KEYWORD_ONLY}
    assert keyword_only == {"repair", "raw", "record_draws", "substream"}
    assert ps["repair"].default is False and ps["raw"].default is False
    assert any(v.kind is inspect.Parameter.VAR_KEYWORD for v in ps.values())     # seed, populations, poll_every, device
    with pytest.raises(TypeError):
        bb.PIKAIA(20, 10, 6, 0.85, 2, 0.005, 0.0005, 0.25, 1., 1, 0, True)
    assert bb.MultivariateSearch in bb.PIKAIA.__mro__[1:] and "PIKAIA" in bb.__all__
    assert bb.PIKAIA._accepts_program is True and bb.PIKAIA._extension == "pikaia"
    assert multivariate.PROGRAM_FAMILIES.endswith("PIKAIA") and "JADE" in multivariate.PROGRAM_FAMILIES
    for name in ("optimize", "initialize", "iterate", "solution", "run", "inject_draws", "table_len"):
        assert callable(getattr(bb.PIKAIA, name))


def test_constructor_marshals_both_structs():
    import bboptpy_amd as bb
    a = bb.PIKAIA(20, 50, 6, seed=9, populations=3, poll_every=2)
    p, g = a._params, a._pikaia
    assert (p.algo, p.np, p.mfev, p.h, p.seed, p.populations, p.poll_every) == (25, 20, 50, 6, 9, 3, 2)
    assert {k: getattr(g, k) for k in DEFAULTS} == DEFAULTS and (g.repair, g.raw, g.substream) == (0, 0, 0)
    a = bb.PIKAIA(10, 7, 9, 0.5, 6, 0.01, 0.001, 0.5, 0.25, 1, 1, repair=True, raw=True, record_draws=True, substream=4)
    g = a._pikaia
    assert (g.pcross, g.imut, g.pmut, g.pmutmn, g.pmutmx, g.fdif, g.irep, g.ielite) == (0.5, 6, 0.01, 0.001, 0.5, 0.25, 1, 1)
    assert (g.repair, g.raw, g.substream, a._params.h) == (1, 1, 4, 9) and a._record_draws
    with pytest.raises(TypeError):
        bb.PIKAIA(20, 50)                       # nd is required
    with pytest.raises(TypeError):
        bb.PIKAIA(20, 50, 6, tol=1e-6)          # the reference's constructor has no such argument


def test_every_refusal_names_its_reason():
    import bboptpy_amd as bb
    for irep in (2, 3):
        with pytest.raises(ValueError, match="irep must be 1.*steady-state.*sequential walk.*not built"):
            bb.PIKAIA(10, 5, 6, irep=irep)
    with pytest.raises(ValueError, match="np must be even.*zero vector"):
        bb.PIKAIA(11, 5, 6)
    for np_ in (0, 1, 4098):
        with pytest.raises(ValueError, match=r"np must be in \[2, 4096\]"):
            bb.PIKAIA(np_, 5, 6)
    for nd in (0, 10):
        with pytest.raises(ValueError, match=r"nd must be in \[1, 9\].*overflows an int"):
            bb.PIKAIA(10, 5, nd)
    for imut in (0, 7):
        with pytest.raises(ValueError, match=r"imut must be in \[1, 6\]"):
            bb.PIKAIA(10, 5, 6, imut=imut)
    with pytest.raises(ValueError, match="ielite is 0 or 1"):
        bb.PIKAIA(10, 5, 6, ielite=2)
    for kw in (dict(pcross=1.5), dict(pmut=-0.1), dict(pmutmn=2.), dict(pmutmx=-1.)):
        with pytest.raises(ValueError, match=r"%s is a probability and must lie in \[0, 1\]" % list(kw)[0]):
            bb.PIKAIA(10, 5, 6, **kw)
    with pytest.raises(ValueError, match="pmutmn must not exceed pmutmx"):
        bb.PIKAIA(10, 5, 6, pmutmn=0.3, pmutmx=0.2)
    for fdif in (-0.1, 1.5):
        with pytest.raises(ValueError, match=r"fdif must lie in \[0, 1\]"):
            bb.PIKAIA(10, 5, 6, fdif=fdif)
    with pytest.raises(ValueError, match="ngen must be >= 1"):
        bb.PIKAIA(10, 0, 6)
    with pytest.raises(ValueError, match="INT_MAX"):
        bb.PIKAIA(4096, 600000, 6)
    lo, up, g = -np.ones(3), np.ones(3), np.zeros(3)
    with pytest.raises(ValueError, match="finite"):
        bb.PIKAIA(10, 5, 6)._problem("sphere", lo, np.array([1., np.inf, 1.]), g)
    bb.PIKAIA(10, 5, 6, raw=True)._problem("sphere", lo, np.array([1., np.inf, 1.]), g)     # raw never reads the box
    with pytest.raises(ValueError, match=r"dimension must be in \[1, 512\]"):
        bb.PIKAIA(10, 5, 6)._problem("sphere", -np.ones(513), np.ones(513), np.zeros(513))
    # initialize() refuses the same way, before a handle is made
    a = bb.PIKAIA(10, 5, 6)
    with pytest.raises(ValueError, match="finite"):
        a.initialize("sphere", lo, np.array([1., np.inf, 1.]), g)
    assert a._handle is None


def test_no_device_no_run():
    """without a GPU bbo_create returns BBO_ERR_NO_DEVICE: there is no CPU path; the parameter checks of the
    library come first"""
    import bboptpy_amd as bb
    from bboptpy_amd import _ffi
    L = _ffi.lib()
    for np_, ngen, nd, why in ((11, 5, 6, "np must be even"), (0, 5, 6, "np must be in"), (10, 5, 10, "nd must be in"),
                               (10, 0, 6, "ngen must be >= 1"), (4096, 600000, 6, "int counter")):
        p = _ffi.default_params(_ffi.ALGO_PIKAIA)
        p.np, p.mfev, p.h = np_, ngen, nd
        h = C.c_void_p()
        assert L.bbo_create(C.byref(p), C.byref(h)) == _ffi.ERR_ARG and not h.value
        assert why in L.bbo_last_error(None).decode()
    if L.bbo_device_count() > 0:
        return      # a GPU is visible here: tests/test_pikaia_gpu.py runs
    p = _ffi.default_params(_ffi.ALGO_PIKAIA)
    p.np, p.mfev, p.h = 10, 5, 6
    h = C.c_void_p()
    assert L.bbo_create(C.byref(p), C.byref(h)) == -4 and not h.value
    with pytest.raises(_ffi.BboError) as ei:
        bb.PIKAIA(10, 5, 6).optimize(bb.objectives.sphere, -np.ones(4), np.ones(4), np.zeros(4))
    assert ei.value.status == -4
