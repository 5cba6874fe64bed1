"""The host lifecycle every engine shares (Engine<Scal>, bbo_engine.hpp), pinned per class:
run() against iterate(), a spent budget, the guards' statuses and messages, NaN from a callable.

Characterisation: every assertion here held before the engines were moved onto the shared base
(no case needed its own pin), so a difference after a change to the base is a change of behaviour.
Shapes are the smallest the classes accept: n = 4, two populations, eight individuals.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, NP, POPS = 4, 8, 2
ERR_ARG, ERR_STATE = -1, -2      # bbo_status, include/bbopt_hip.h
LOWER, UPPER = -5. * np.ones(N), 5. * np.ones(N)
GUESS = np.random.default_rng(5).uniform(-3., 3., N * POPS)

# class -> (constructor from (package, mfev), one state vector, the fitness vectors)
CASES = {
    "CMAES": (lambda hip, mfev, **k: hip.CMAES(mfev, 1e-12, NP, **k), "xmean", ("fitness",)),
    "ActiveCMAES": (lambda hip, mfev, **k: hip.ActiveCMAES(mfev, 1e-12, NP, **k), "xmean", ("fitness",)),
    "SepCMAES": (lambda hip, mfev, **k: hip.SepCMAES(mfev, 1e-12, NP, **k), "xmean", ("fitness",)),
    "CholeskyCMAES": (lambda hip, mfev, **k: hip.CholeskyCMAES(mfev, 1e-12, 1e-12, NP, **k), "A", ("fitness",)),
    "JADE": (lambda hip, mfev, **k: hip.JADE(mfev, NP, 1e-12, **k), "f", ("f",)),
    "SHADE": (lambda hip, mfev, **k: hip.SHADE(mfev, NP, 1e-12, **k), "f", ("f",)),
    "SANSDE": (lambda hip, mfev, **k: hip.SANSDE(mfev, NP, 1e-12, **k), "f", ("f",)),
    "CSO": (lambda hip, mfev, **k: hip.CSO(mfev, 1e-12, NP, pcompete=2, **k), "f", ("f",)),
    "CCPSO": (lambda hip, mfev, **k: hip.CCPSO(mfev, 1e-12, NP, [2], **k), "fx", ("fx", "fy")),
    "APSO": (lambda hip, mfev, **k: hip.APSO(mfev, 1e-12, NP, **k), "fb", ("f", "fb")),
    "JAYA": (lambda hip, mfev, **k: hip.JAYA(mfev, 1e-12, NP, 2, **k), "f", ("f",)),
    "DSA": (lambda hip, mfev, **k: hip.DSA(mfev, 1e-12, 1e-12, NP, **k), "f", ("f",)),
}
NAMES = list(CASES)


def _make(hip, name, mfev, f):
    g = CASES[name][0](hip, mfev, seed=1234, populations=POPS)
    g.initialize(f, LOWER, UPPER, GUESS)
    return g


def _snapshot(g, key):
    out = []
    for p in range(POPS):
        s = g.solution(p)
        out += [np.array([s.n_evals], dtype=np.float64), s.x, g.get_state("fev", p), g.get_state(key, p)]
    return out


@pytest.mark.parametrize("objective", ["builtin", "callable"])
@pytest.mark.parametrize("name", NAMES)
def test_run_equals_iterate(hip, name, objective):
    """run(3) and three iterate() calls from the same seed: fev, x and a state vector bit-equal;
    a callable is called equally often"""
    calls = [0, 0]

    def counted(slot):
        def f(x):
            calls[slot] += 1
            return float(np.sum((x - 0.5) ** 2))
        return f

    fa = hip.objectives.rosenbrock if objective == "builtin" else counted(0)
    fb = hip.objectives.rosenbrock if objective == "builtin" else counted(1)
    a, b = _make(hip, name, 100000, fa), _make(hip, name, 100000, fb)
    assert a.run(3) == 3
    for _ in range(3):
        b.iterate()
    key = CASES[name][1]
    for va, vb in zip(_snapshot(a, key), _snapshot(b, key)):
        print(name, objective, key, va[:4], vb[:4])
        assert va.tobytes() == vb.tobytes()
    assert int(a.get_state("fev")[0]) > 0
    assert calls[0] == calls[1]
    if objective == "callable":
        assert calls[0] > 0


@pytest.mark.parametrize("name", NAMES)
def test_spent_budget_takes_no_generation(hip, name):
    """a run driven to the end of a small budget; a second run() then launches nothing"""
    g = _make(hip, name, 5 * NP, hip.objectives.sphere)
    assert g.run(1000) > 0
    before = [(g.solution(p).n_evals, g.solution(p).x.tobytes()) for p in range(POPS)]
    assert g.run(5) == 0
    after = [(g.solution(p).n_evals, g.solution(p).x.tobytes()) for p in range(POPS)]
    assert after == before
    for p in range(POPS):
        assert int(g.get_state("stop", p)[0]) != 0


@pytest.mark.parametrize("name", NAMES)
def test_guard_statuses(hip, name):
    """a handle that was never initialised: the state error from iterate, run, solution and
    get_state; an initialised one: the argument error for population == populations"""
    from bboptpy_amd import _ffi
    L = _ffi.lib()
    g = CASES[name][0](hip, 1000, seed=1, populations=POPS)
    h = g._ensure_handle()
    x, fev, conv, done = np.zeros(N), C.c_int(), C.c_int(), C.c_int()
    out = np.zeros(4)
    for status in (L.bbo_iterate(h), L.bbo_run(h, 1, C.byref(done)),
                   L.bbo_solution_of(h, 0, x, C.byref(fev), C.byref(conv)),
                   L.bbo_get(h, b"fev", 0, out.ctypes.data_as(C.c_void_p), 4)):
        assert status == ERR_STATE
        assert "before initialize" in L.bbo_last_error(h).decode()
    g.initialize(hip.objectives.sphere, LOWER, UPPER, GUESS)
    for call in (lambda: g.solution(POPS), lambda: g.get_state("fev", POPS),
                 lambda: g.set_state("profile", [0.], POPS)):
        with pytest.raises(_ffi.BboError) as ei:
            call()
        assert ei.value.status == ERR_ARG
        assert "out of range" in str(ei.value)


@pytest.mark.parametrize("name", NAMES)
def test_nan_objective_becomes_inf(hip, name):
    """a callable that returns NaN on every call: no NaN reaches the engine's fitness"""
    g = _make(hip, name, 100000, lambda x: float("nan"))
    g.iterate()
    for p in range(POPS):
        for key in CASES[name][2]:
            f = g.get_state(key, p)
            assert f.size > 0 and not np.isnan(f).any(), (key, f)
