"""Which kernels sample and update a CMA-ES generation (CmaEngine::sample_route and update_route, read back
through the keys `sample_route`, `sample_lean`, `update_route` and `small_fused`), case by case: every
branch of the two routes at the smallest shape that reaches it (tests/cma_route_cases.py).  The A/B tests
of the samplers, the Gram and the path kernels compare "the form under a knob" with the default; this file
is what shows that the two sides ran different kernels.  The expected kernels were read off a kernel trace
of the commit before the route functions existed (profiles/sample_update_routes.txt), not off those
functions.  Every case also checks what the kernels computed."""
import numpy as np
import pytest

import cma_route_cases as rc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(rc.SAMPLE_CASES))
def test_sample_route(hip, name):
    case = rc.SAMPLE_CASES[name]
    g = rc.make_handle(hip, case)
    assert int(g.get_state("sample_route")[0]) == -1           # no launch yet
    rc.run_sample(g)
    assert rc.SAMPLE_NAMES[int(g.get_state("sample_route")[0])] == case["want"]
    if case["lean"] is not None:
        assert int(g.get_state("sample_lean")[0]) == case["lean"]
    # the fitness is the objective of the stored row (rtol: the sum-on-draw check of tests/test_batch_gpu.py)
    n, lam = case["n"], case["lam"]
    for p in sorted({0, case["P"] - 1}):
        X = g.get_state("arx", p).reshape(lam, n)
        f = g.get_state("fitness", p)[:lam]
        assert np.isfinite(X).all()
        np.testing.assert_allclose(f, rc.objective_rows(case["obj"], X), rtol=1e-12, atol=0)


@pytest.mark.parametrize("name", sorted(rc.UPDATE_CASES))
def test_update_route(hip, name):
    case = rc.UPDATE_CASES[name]
    g = rc.make_handle(hip, case)
    assert g.get_state("update_route").size == 0               # no launch yet
    rc.run_update(g, case)
    want = list(case["want"])
    if want[0] is None:       # the whitening runs exactly when the one-wavefront ranking handed no norms down
        want = want[1:] if int(g.get_state("rank_route")[0]) == 0 else want[2:]
    got = [rc.UPDATE_NAMES[int(k)] for k in g.get_state("update_route")]
    assert got == [w.split("<")[0] for w in want]
    if case["mode"] == "generation":       # in front of cma_eigen_fx128: no cma_cov
        assert "cma_cov" not in got and int(g.get_state("cov_fused")[0]) == 1
    n = case["n"]
    for p in sorted({0, case["P"] - 1}):
        assert g.get_state("sigma", p)[0] > 0
        if case["algo"] == rc.SEP:
            Cm = g.get_state("csep", p)
        elif case["algo"] == rc.CHOL:
            A = g.get_state("A", p).reshape(n, n)
            Cm = A @ A.T
        else:
            Cm = g.get_state("C", p).reshape(n, n)
            np.testing.assert_array_equal(Cm, Cm.T)
        assert np.isfinite(Cm).all()


def test_small_fused(hip):
    """n = 8, lambda = 8, a builtin objective: a generation is one cma_small_generations launch; diagnostic bit 64
    keeps the nine-kernel sequence"""
    for dbg, want in ((0, 1), (64, 0)):
        g = hip.ActiveCMAES(10 ** 6, 1e-12, 8, seed=3)
        g.initialize(hip.objectives.sphere, -5. * np.ones(8), 5. * np.ones(8), np.ones(8))
        if dbg:
            g.set_state("dbg", [float(dbg)])
        assert int(g.get_state("small_fused")[0]) == 0
        g.iterate()
        assert int(g.get_state("small_fused")[0]) == want
        assert int(g.get_state("sample_route")[0]) == (-1 if want else rc.SAMPLE_NAMES.index("cma_sample_eval64<1, 8>"))
        assert np.isfinite(g.get_state("C")).all() and g.get_state("sigma")[0] > 0
