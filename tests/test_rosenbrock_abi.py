"""CPU checks of Rosenbrock at the drop-in boundary: the Python signature against tests/golden/class_surface.json
and the record of the reference's header in tests/golden/rosenbrock_runs.json, bbo_rosen_params_default, the entry
points that need no handle, and the arguments the class refuses before a handle exists."""
import ctypes as C
import inspect
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mfev", "tol", "step0", "decf"]
SYMBOLS = ("bbo_rosen_params_default", "bbo_rosen_configure", "bbo_rosen_phase")


def _json(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as fh:
        return json.load(fh)


def test_algorithm_number_header_and_symbols():
    import bboptpy_amd as bb
    from bboptpy_amd import _ffi
    assert bb.Rosenbrock._algo == _ffi.ALGO_ROSENBROCK == 27
    text = open(os.path.join(ROOT, "include", "bbopt_hip.h")).read()
    assert "BBO_ALGO_ROSENBROCK = 27" in text and "bbo_rosen_params;" in text
    assert "typedef struct { double decf; int repair, wide, substream; } bbo_rosen_params;" in text
    raw = C.CDLL(_ffi.LIB_PATH)
    for name in SYMBOLS:
        assert name in text and name in _ffi.EXPORTED_SYMBOLS and hasattr(raw, name)
    p = _ffi.default_params(_ffi.ALGO_ROSENBROCK)
    assert (p.algo, p.populations, p.poll_every) == (27, 1, 0)       # the engine's own chunk of searches
    assert (_ffi.ROSEN_PHASE_ADVANCE, _ffi.ROSEN_PHASE_EVALUATE, _ffi.ROSEN_PHASE_ABSORB) == (0, 1, 2)
    assert (_ffi.ROSEN_FLAG_CONVERGED, _ffi.ROSEN_FLAG_BUDGET) == (1, 2)
    assert _ffi.EXTENSIONS["rosen"] == (_ffi.RosenParams, True, {})


def test_rosen_params_default_and_the_statuses_that_need_no_handle():
    from bboptpy_amd import _ffi
    L = _ffi.lib()
    d = _ffi.RosenParams()
    C.memset(C.byref(d), 0xA5, C.sizeof(d))
    L.bbo_rosen_params_default(C.byref(d))
    assert (d.decf, d.repair, d.wide, d.substream) == (0.1, 0, -1, 0)
    assert C.sizeof(_ffi.RosenParams) == 24
    L.bbo_rosen_params_default(None)       # tolerated
    assert L.bbo_rosen_configure(None, C.byref(d)) == _ffi.ERR_ARG
    assert L.bbo_rosen_phase(None, 0) == _ffi.ERR_ARG


def test_class_signature_is_the_reference_signature():
    import bboptpy_amd as bb
    E = inspect.Parameter.empty
    cls = bb.Rosenbrock
    ps = inspect.signature(cls.__init__).parameters
    positional = [(k, v.default) for k, v in ps.items()
                  if v.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD and k != "self"]
    recorded = _json("rosenbrock_runs.json")["signature"]
    surface = _json("class_surface.json")
    surface = surface.get("classes", surface)["Rosenbrock"]["init"]["keywords"]
    assert [k for k, _ in positional] == [a["name"] for a in recorded] == [a["name"] for a in surface] == NAMES
    for (k, default), a, b in zip(positional, recorded, surface):
        assert a["required"] == b["required"], k
        if a["required"]:
            assert default is E, k
        else:
            assert default == a["default"] == b["default"] and type(default) is type(a["default"]), k
    assert ps["repair"].kind is inspect.Parameter.KEYWORD_ONLY and ps["repair"].default is False
    assert ps["wide"].kind is inspect.Parameter.KEYWORD_ONLY and ps["wide"].default is None
    assert ps["substream"].kind is inspect.Parameter.KEYWORD_ONLY and ps["substream"].default == 0
    assert any(v.kind is inspect.Parameter.VAR_KEYWORD for v in ps.values())
    with pytest.raises(TypeError):
        cls(1000, 1e-8, 1., 0.1, True)
    assert bb.MultivariateSearch in cls.__mro__[1:] and not issubclass(cls, bb.BaseCMAES)
    assert "Rosenbrock" in bb.__all__ and cls._accepts_program is False
    assert bb.objectives.rosenbrock is not cls and callable(bb.objectives.rosenbrock)
    for name in ("optimize", "initialize", "iterate", "solution", "run", "phase"):
        assert callable(getattr(cls, name))
    assert "**On a budget exit optimize() returns the ZERO vector**" in cls.__doc__


def test_constructor_marshals_both_structs():
    import bboptpy_amd as bb
    cls = bb.Rosenbrock
    a = cls(5000, 1e-9, 0.5, seed=9, populations=3, poll_every=2)
    p, s = a._params, a._rosen
    assert (p.algo, p.mfev, p.tol, p.sigma0, p.seed, p.populations, p.poll_every) == (27, 5000, 1e-9, 0.5, 9, 3, 2)
    assert (s.decf, s.repair, s.wide, s.substream) == (0.1, 0, -1, 0)
    s = cls(700, 0.25, 2., 0.5, repair=True, wide=False, substream=5)._rosen
    assert (s.decf, s.repair, s.wide, s.substream) == (0.5, 1, 0, 5)
    assert cls(mfev=700, tol=0.5, step0=1., wide=True)._rosen.wide == 1
    for args in ((700,), (700, 1e-8)):
        with pytest.raises(TypeError):
            cls(*args)
    with pytest.raises(TypeError):
        cls(700, 1e-8, 1., np=7)


def test_invalid_arguments_are_refused():
    import bboptpy_amd as bb
    cls = bb.Rosenbrock
    with pytest.raises(ValueError, match=r"Rosenbrock: dimension must be in \[1, 128\]"):
        cls(100, 0., 1.)._problem("sphere", -np.ones(129), np.ones(129), np.zeros(129))
    cls(100, 0., 1.)._problem("sphere", -np.ones(128), np.ones(128), np.zeros(128))
    for mfev in (0, -3):
        with pytest.raises(ValueError, match="mfev must be positive"):
            cls(mfev, 0., 1.)
    for step0 in (np.inf, -np.inf, np.nan):
        with pytest.raises(ValueError, match="step0 must be finite"):
            cls(100, 0., step0)
    with pytest.raises(ValueError, match="decf must be finite"):
        cls(100, 0., 1., np.nan)
    # a step of 0 never leaves the doubling loop of a search but on the budget
    for bad in (dict(step0=0.), dict(step0=-0.), dict(step0=1., decf=0.), dict(step0=1., tol=-1e-8),
                dict(step0=1., tol=np.nan)):
        with pytest.raises(ValueError, match="Rosenbrock: (step0|decf|tol) must be"):
            cls(**dict(dict(mfev=100, tol=0.), **bad))
    cls(100, 0., -1.)       # a negative first step is the reference's search mirrored
    # no finite box is required: the search never reads the bounds
    cls(100, 0., 1.)._problem("sphere", np.full(3, -np.inf), np.full(3, np.inf), np.zeros(3))

    class Fake(bb.DeviceObjective):
        def __init__(self):
            self._handle = None

        def __del__(self):
            pass

    with pytest.raises(ValueError, match="Rosenbrock does not take a DeviceObjective yet"):
        cls(100, 0., 1.)._problem(Fake(), -np.ones(3), np.ones(3), np.zeros(3))


def test_no_device_no_run():
    """without a GPU bbo_create returns BBO_ERR_NO_DEVICE: there is no CPU path"""
    import bboptpy_amd as bb
    from bboptpy_amd import _ffi
    if _ffi.lib().bbo_device_count() > 0:
        return
    with pytest.raises(_ffi.BboError) as ei:
        bb.Rosenbrock(100, 0., 1.).optimize(bb.objectives.sphere, -np.ones(4), np.ones(4), np.zeros(4))
    assert ei.value.status == -4
