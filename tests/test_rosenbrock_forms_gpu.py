"""GPU: the two forms of rosen_walk (a wavefront per point of a batch / one wavefront, the points in turn)
and rosen_eval give the same bits."""
import numpy as np
import pytest

import objective_reference as R
import test_neldermead_forms_gpu  # noqa: F401  (its row: the table is complete only with every row registered)
import test_objective_forms_gpu as T
from slpso_model import device_objective

# Rosenbrock's row in the table of call sites of tests/test_objective_forms_gpu.py, registered at import as the
# rows of the engines before it are.  One form of evaluation whatever n is (eval_row_group<64> over a point in
# LDS).  The pair: the four interpolation points of the last search and their values, "cand" / "fs".
T.SITES["Rosenbrock"] = T.Site(lambda hip, n: hip.Rosenbrock(T.BUDGET, 0., 1., seed=3), [("cand", "fs")],
                               ns=(1, 17, 65, 128))
SITE = T.SITES["Rosenbrock"]


def test_the_row_is_in_the_table():
    """(no device)"""
    T.test_the_table_names_every_optimizer_class()
    assert SITE.ns == (1, 17, 65, 128) and SITE.clamp_kw is None and not SITE.extra


@pytest.mark.gpu
@pytest.mark.parametrize("n", SITE.ns)
def test_call_sites_inside_the_bound(hip, n):
    """initialize, two searches, the interpolation points and their values, all ten objectives, both forms"""
    for wide in (False, True):
        T._hold_site(hip, "Rosenbrock", n, R.OBJECTIVES, -5., 5.,
                     make=lambda hip, n: hip.Rosenbrock(T.BUDGET, 0., 1., wide=wide, seed=3))



@pytest.mark.gpu
@pytest.mark.parametrize("n", [5, 64, 65, 128])
def test_wide_and_narrow_walk_the_same_bits(hip, n):
    lo, up = -5. * np.ones(n), 5. * np.ones(n)
    guess = np.random.default_rng(n).uniform(-2., 2., (2, n))
    hs = []
    for wide in (False, True, None):
        g = hip.Rosenbrock(1 << 20, 1e-12, 1., populations=2, wide=wide, seed=1)
        g.initialize(hip.objectives.rosenbrock, lo, up, guess.ravel())
        assert g.run(n + 8) == n + 8
        hs.append(g)
    assert int(hs[2].get_state("wide")[0]) == 1         # two populations: the wide form at every n
    for p in range(2):
        for k in ("x", "v", "d", "stepi", "i", "fev", "fs", "path", "it", "orths"):
            a, b, c = (h.get_state(k, p) for h in hs)
            assert a.tobytes() == b.tobytes() == c.tobytes(), (n, p, k)
        assert int(hs[0].get_state("it", p)[0]) == n + 8


@pytest.mark.gpu
def test_the_default_form_is_narrow_for_many_small_searches(hip):
    """n <= 64 and at least four populations per CU"""
    for n, P, want in ((32, 4096, 0), (64, 4096, 0), (65, 4096, 1), (32, 64, 1)):
        g = hip.Rosenbrock(1000, 1e-8, 1., populations=P, seed=1)
        g.initialize(hip.objectives.sphere, -np.ones(n), np.ones(n), np.zeros(P * n))
        assert int(g.get_state("wide")[0]) == want, (n, P)


@pytest.mark.gpu
def test_rosen_eval_gives_the_values_of_the_fused_walk(hip):
    n = 33
    f = device_objective("rosenbrock", n)
    g = hip.Rosenbrock(1 << 20, 1e-12, 1., seed=1)
    g.initialize(hip.objectives.rosenbrock, -5. * np.ones(n), 5. * np.ones(n), np.linspace(-1., 1., n))
    seen = 0
    for _ in range(3):
        pending = g.phase(0)
        while pending:
            cnt = int(g.get_state("pending")[0])
            g.phase(1)
            cand = g.get_state("cand").reshape(4, n)
            assert g.get_state("value")[:cnt].tobytes() == np.array([f(cand[q]) for q in range(cnt)]).tobytes()
            seen += cnt
            pending = g.phase(2)
    assert seen == int(g.get_state("fev")[0])
