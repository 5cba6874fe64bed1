"""GPU: the walk protocol the engines SLPSO, CRS, SSDE and ACD share (host side): a generation
entered and left at its evaluations.  A host callable sees the points of the built-in run, once per counted
evaluation, and a generation driven through phase() is the generation of iterate(), bit for bit, in every
population of a handle whose populations need different numbers of evaluations."""
import numpy as np
import pytest

from slpso_model import device_objective
from test_acd_gpu import KEYS as ACD_KEYS
from test_crs_gpu import KEYS as CRS_KEYS
from test_slpso_gpu import ALL_KEYS as SLPSO_KEYS
from test_ssde_gpu import KEYS as SSDE_KEYS

pytestmark = pytest.mark.gpu

N, NP, P, MFEV = 3, 6, 3, 300
LO, UP = -3. * np.ones(N), 3. * np.ones(N)


def _advance_test(g):
    """SLPSO, SSDE: absorb leaves the walk where it is, the next advance says whether a point is pending"""
    while g.phase(0):
        g.phase(1)
        g.phase(2)


def _absorb_advances(g):
    """CRS: absorb walks on to the next pending point"""
    pending = g.phase(0)
    while pending:
        g.phase(1)
        pending = g.phase(2)


def _one_step(g):
    """ACD: every population has its pair pending, and absorb ends the step"""
    assert g.phase(0) == P
    g.phase(1)
    g.phase(2)


# name -> constructor, the keys its own phase test compares, one generation through phase()
ENGINES = {
    "SLPSO": (lambda hip: hip.SLPSO(MFEV, 1e-12, NP, seed=11, populations=P), SLPSO_KEYS, _advance_test),
    "CRS": (lambda hip: hip.CRS(MFEV, NP, 0., seed=11, populations=P, max_depth=64), CRS_KEYS, _absorb_advances),
    "SSDE": (lambda hip: hip.SSDE(MFEV, NP, 1e-12, seed=11, populations=P), SSDE_KEYS + ("perm", "order"),
             _advance_test),
    "ACD": (lambda hip: hip.ACD(MFEV, 0., 0., seed=11, populations=P), ACD_KEYS, _one_step),
}


def _start(hip, name, f):
    g = ENGINES[name][0](hip)
    g.initialize(f, LO, UP, np.zeros(N * P))
    return g


def _counted():
    f, calls = device_objective("sphere", N), []

    def sphere(x):
        calls.append(1)
        return f(x)
    return sphere, calls


@pytest.mark.parametrize("name", list(ENGINES))
def test_a_callable_run_to_the_budget_is_the_builtin_run(hip, name):
    sphere, calls = _counted()
    a, b = _start(hip, name, "sphere"), _start(hip, name, sphere)
    a.run(1 << 30)
    b.run(1 << 30)
    fev = 0
    for p in range(P):
        sa, sb = a.solution(p), b.solution(p)
        assert sa.x.tobytes() == sb.x.tobytes(), (p, sa.x, sb.x)
        for k in ("fev", "flag"):
            assert a.get_state(k, p).tobytes() == b.get_state(k, p).tobytes(), (p, k)
        assert sb.n_evals == int(b.get_state("fev", p)[0]) and int(b.get_state("flag", p)[0]) != 0
        fev += sb.n_evals
    assert len(calls) == fev


@pytest.mark.parametrize("name", list(ENGINES))
def test_a_generation_through_phase_is_the_generation_of_iterate(hip, name):
    """the handle driven by phase() has the callable: phase 1 is then the host's evaluation loop"""
    _, keys, generation = ENGINES[name]
    sphere, calls = _counted()
    a, b = _start(hip, name, "sphere"), _start(hip, name, sphere)
    for it in range(3):
        a.iterate()
        generation(b)
        for p in range(P):
            assert int(b.get_state("pending", p)[0]) == 0
            for k in keys:
                ka, kb = a.get_state(k, p), b.get_state(k, p)
                assert ka.shape == kb.shape and ka.tobytes() == kb.tobytes(), (it, p, k)
    assert len(calls) == sum(int(b.get_state("fev", p)[0]) for p in range(P))
