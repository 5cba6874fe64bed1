"""CPU checks of NelderMead at the drop-in boundary: the Python signature and the two enums against the record
of the reference's header in tests/golden/neldermead_runs.json, bbo_nm_params_default, the entry points that
need no handle, and the arguments the class refuses before a handle exists."""
import ctypes as C
import inspect
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mfev", "tol", "rad0", "minit", "pinit", "checkev", "eps"]
SYMBOLS = ("bbo_nm_params_default", "bbo_nm_configure", "bbo_nm_phase")


def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "neldermead_runs.json")) as fh:
        return json.load(fh)


def test_algorithm_number_header_and_symbols():
    import bboptpy_amd as bb
    from bboptpy_amd import _ffi
    assert bb.NelderMead._algo == _ffi.ALGO_NELDER_MEAD == 26
    text = open(os.path.join(ROOT, "include", "bbopt_hip.h")).read()
    assert "BBO_ALGO_NELDER_MEAD = 26" in text and "bbo_nm_params;" in text
    raw = C.CDLL(_ffi.LIB_PATH)
    for name in SYMBOLS:
        assert name in text and name in _ffi.EXPORTED_SYMBOLS and hasattr(raw, name)
    p = _ffi.default_params(_ffi.ALGO_NELDER_MEAD)
    assert (p.algo, p.populations, p.poll_every) == (26, 1, 0)       # the engine's own chunk of steps
    assert _ffi.default_params(_ffi.ALGO_CMAES).poll_every == 8
    assert (_ffi.NM_PHASE_ADVANCE, _ffi.NM_PHASE_EVALUATE, _ffi.NM_PHASE_ABSORB) == (0, 1, 2)
    assert (_ffi.NM_FLAG_CONVERGED, _ffi.NM_FLAG_BUDGET) == (1, 2)


def test_nm_params_default_and_the_statuses_that_need_no_handle():
    from bboptpy_amd import _ffi
    L = _ffi.lib()
    d = _ffi.NmParams()
    C.memset(C.byref(d), 0xA5, C.sizeof(d))
    L.bbo_nm_params_default(C.byref(d))
    assert (d.minit, d.pinit, d.checkev, d.eps, d.repair, d.speculate, d.lds, d.substream) == (1, 3, 10, 1e-3, 0, 0, -1, 0)
    assert C.sizeof(_ffi.NmParams) == 40
    L.bbo_nm_params_default(None)       # tolerated
    assert L.bbo_nm_configure(None, C.byref(d)) == _ffi.ERR_ARG
    assert L.bbo_nm_phase(None, 0) == _ffi.ERR_ARG


def test_class_signature_is_the_reference_signature():
    import bboptpy_amd as bb
    E = inspect.Parameter.empty
    cls = bb.NelderMead
    ps = inspect.signature(cls.__init__).parameters
    positional = [(k, v.default) for k, v in ps.items()
                  if v.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD and k != "self"]
    recorded = _golden()["signature"]
    assert [k for k, _ in positional] == [a["name"] for a in recorded] == NAMES
    for (k, default), a in zip(positional, recorded):
        if a["required"]:
            assert default is E, k
        elif isinstance(a["default"], str):      # an enum's value, by its name in the header
            assert default.name == a["default"] and default == getattr(cls, a["default"]), k
        else:
            assert default == a["default"] and type(default) is type(a["default"]), k
    for k in ("repair", "speculate"):
        assert ps[k].kind is inspect.Parameter.KEYWORD_ONLY and ps[k].default is False
    assert ps["lds"].kind is inspect.Parameter.KEYWORD_ONLY and ps["lds"].default is None
    assert any(v.kind is inspect.Parameter.VAR_KEYWORD for v in ps.values())
    with pytest.raises(TypeError):
        bb.NelderMead(1000, 1e-8, 1., cls.spendley, cls.original, 10, 1e-3, True)
    assert bb.MultivariateSearch in cls.__mro__[1:] and not issubclass(cls, bb.BaseCMAES)
    assert "NelderMead" in bb.__all__ and cls._accepts_program is False
    for name in ("optimize", "initialize", "iterate", "solution", "run", "phase"):
        assert callable(getattr(cls, name))


def test_enums_are_the_reference_enums_with_exported_values():
    import bboptpy_amd as bb
    cls = bb.NelderMead
    enums = _golden()["enums"]
    for enum_cls, key in ((cls.NelderMead_SimplexInit, "simplex_initializer"),
                          (cls.NelderMead_ParamInit, "parameter_initializer")):
        assert [e.name for e in enum_cls] == enums[key]
        assert [int(e) for e in enum_cls] == list(range(len(enums[key])))
        for e in enum_cls:      # export_values: the values are attributes of the class as well
            assert getattr(cls, e.name) is e
    assert (cls.coordinate_axis, cls.spendley, cls.pfeffer, cls.random) == (0, 1, 2, 3)
    assert (cls.original, cls.gao2010, cls.mehta2019_crude, cls.mehta2019_refined) == (0, 1, 2, 3)


def test_constructor_marshals_both_structs():
    import bboptpy_amd as bb
    cls = bb.NelderMead
    a = cls(5000, 1e-9, 0.5, seed=9, populations=3, poll_every=2)
    p, s = a._params, a._nm
    assert (p.algo, p.mfev, p.tol, p.sigma0, p.seed, p.populations, p.poll_every) == (26, 5000, 1e-9, 0.5, 9, 3, 2)
    assert (s.minit, s.pinit, s.checkev, s.eps, s.repair, s.speculate, s.lds, s.substream) == (1, 3, 10, 1e-3, 0, 0, -1, 0)
    assert cls(700, 0.25, 2., lds=True)._nm.lds == 1
    a = cls(700, 0.25, 2., cls.pfeffer, cls.gao2010, 4, 1e-2, repair=True, lds=False, substream=5)
    s = a._nm
    assert (s.minit, s.pinit, s.checkev, s.eps, s.repair, s.lds, s.substream) == (2, 1, 4, 1e-2, 1, 0, 5)
    a = cls(mfev=700, tol=0.5, rad0=1., pinit=cls.NelderMead_ParamInit.original, minit=3)
    assert (a._nm.minit, a._nm.pinit) == (3, 0)
    for args in ((700,), (700, 1e-8)):
        with pytest.raises(TypeError):
            cls(*args)
    with pytest.raises(TypeError):
        cls(700, 1e-8, 1., np=7)


def test_invalid_arguments_are_refused():
    import bboptpy_amd as bb
    cls = bb.NelderMead
    with pytest.raises(ValueError, match=r"NelderMead: dimension must be in \[1, 128\]"):
        cls(100, 0., 1.)._problem("sphere", -np.ones(129), np.ones(129), np.zeros(129))
    cls(100, 0., 1.)._problem("sphere", -np.ones(128), np.ones(128), np.zeros(128))
    for checkev in (0, -3):
        with pytest.raises(ValueError, match="checkev must be >= 1"):
            cls(100, 0., 1., checkev=checkev)
    for rad0 in (np.inf, -np.inf, np.nan):
        with pytest.raises(ValueError, match="rad0 must be finite"):
            cls(100, 0., rad0)
    with pytest.raises(ValueError, match="minit = random draws the simplex from .*finite"):
        cls(100, 0., 1., minit=cls.random)._problem("sphere", -np.ones(3), np.array([1., np.inf, 1.]), np.zeros(3))
    cls(100, 0., 1., minit=cls.random)._problem("sphere", -np.ones(3), np.ones(3), np.zeros(3))
    # the search itself never reads the bounds
    cls(100, 0., 1.)._problem("sphere", np.full(3, -np.inf), np.full(3, np.inf), np.zeros(3))
    with pytest.raises(ValueError):
        cls(100, 0., 1., minit=4)
    with pytest.raises(ValueError):
        cls(100, 0., 1., pinit=-1)
    with pytest.raises(ValueError, match="speculative step was measured and dropped"):
        cls(100, 0., 1., speculate=True)

    class Fake(bb.DeviceObjective):
        def __init__(self):
            self._handle = None

        def __del__(self):
            pass

    with pytest.raises(ValueError, match="NelderMead does not take a DeviceObjective yet"):
        cls(100, 0., 1.)._problem(Fake(), -np.ones(3), np.ones(3), np.zeros(3))


def test_no_device_no_run():
    """without a GPU bbo_create returns BBO_ERR_NO_DEVICE: there is no CPU path"""
    import bboptpy_amd as bb
    from bboptpy_amd import _ffi
    if _ffi.lib().bbo_device_count() > 0:
        return
    with pytest.raises(_ffi.BboError) as ei:
        bb.NelderMead(100, 0., 1.).optimize(bb.objectives.sphere, -np.ones(4), np.ones(4), np.zeros(4))
    assert ei.value.status == -4
