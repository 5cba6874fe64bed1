"""GPU: CholeskyCMAES against tests/chol_model.py (itself pinned to the recorded reference by
tests/test_chol_model.py) under the device's own normals, and against itself (phases / iterate,
batch / single), its stop rule from crafted states, whole runs, the restart drivers over it.

State tolerance 1e-9 relative to the largest entry, per generation, over 30 generations.  The
model of the shapes with n >= 64 factors C' with numpy.linalg.cholesky instead of walking the
rank-1 chain.  The drift between the two, whole state, same normals, is measured and asserted on
the CPU for these very shapes (tests/test_chol_model.py::
test_chain_and_factorisation_agree_at_the_large_shapes): 1.4e-14 at (64, 256), 2.1e-14 at
(128, 1024), 1.4e-14 at (130, 256), 2.0e-14 at (256, 512) after 30 generations, 2.8e-14 at
(128, 4096) after 10 -- all far inside 1e-9, so the constant stays."""
import math

import numpy as np
import pytest

from _golden import load
from chol_model import CholModel, objective, objective_rows

pytestmark = pytest.mark.gpu

RUNS = load("chol_runs.json")["runs"]
KEYS = ("arx", "xmean", "sigma", "pc", "ps", "A")


def _rel(a, b):
    a, b = np.asarray(a, float).ravel(), np.asarray(b, float).ravel()
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _models(n, lam, obj, lo, up, guess, ranked=False, bound=False, mfev=10 ** 8, tol=1e-12, stol=1e-12, sigma0=2.):
    fast = n >= 64
    ms = []
    for row in guess:
        m = CholModel(mfev, tol, stol, lam, sigma0, bound, ranked=ranked,
                      factor="cholesky" if fast else "chain", fast=fast)
        m.init((objective_rows if fast else objective)(obj, n), lo, up, row)
        ms.append(m)
    return ms


def _pair(hip, n, lam, obj, P=1, ranked=False, bound=False, seed=77, mfev=10 ** 8, tol=1e-12,
          stol=1e-12, box=5., lo_up=None, guess=None, sigma0=2.):
    """`lo_up`, `guess`, `sigma0`: other bounds, starting points and step than +-box, the drawn ones and 2"""
    lo, up = (-box * np.ones(n), box * np.ones(n)) if lo_up is None else lo_up
    if guess is None:
        guess = np.random.default_rng(n + lam).uniform(-0.9 * box, 0.9 * box, (P, n))
    g = hip.CholeskyCMAES(mfev, tol, stol, lam, sigma0, bound, seed=seed, populations=P, ranked=ranked)
    g.initialize(getattr(hip.objectives, obj), lo, up, guess.ravel())
    g.set_state("record_normals", [1.0])
    return g, _models(n, lam, obj, lo, up, guess, ranked, bound, mfev, tol, stol, sigma0)


@pytest.mark.parametrize("P", [1, 5])
@pytest.mark.parametrize("bound", [False, True])
@pytest.mark.parametrize("ranked", [False, True])
@pytest.mark.parametrize("n,lam", [(16, 32), (64, 256), (128, 1024), (128, 4096), (130, 256), (256, 512)])
def test_generations_match_the_model(hip, n, lam, ranked, bound, P):
    # (bounded: a box the population leaves, so that clamps bite)
    g, ms = _pair(hip, n, lam, "ellipsoid", P=P, ranked=ranked, bound=bound, box=2.5 if bound else 5.)
    worst = 0.
    for gen in range(1, 31):
        g.iterate()
        for p, m in enumerate(ms):
            m.generation(g.get_state("zlast", p))
            for key in KEYS:
                got = g.get_state(key, p)
                err = _rel(got, [m.sigma] if key == "sigma" else getattr(m, key))
                worst = max(worst, err)
                assert err <= 1e-9, "n %d lambda %d P %d pop %d gen %d %s: %.3e" % (n, lam, P, p, gen, key, err)
            assert _rel(g.get_state("fit_val", p), m.fit_val) <= 1e-9
            if gen <= 3:
                np.testing.assert_array_equal(g.get_state("fit_idx", p), m.fit_idx)
            assert (int(g.get_state("it", p)[0]), int(g.get_state("fev", p)[0])) == (m.it, m.fev)
            assert (int(g.get_state("flag", p)[0]) == 11) == m.converged()
            A = g.get_state("A", p).reshape(n, n)
            assert (np.triu(A, 1) == 0.).all()
            assert int(g.get_state("chol_repairs", p)[0]) == 0
        if bound and gen == 1:
            assert (np.abs(g.get_state("arx", 0)) == 2.5).any()
    print("n %d lambda %d ranked %d bound %d P %d: worst rel err %.3e" % (n, lam, ranked, bound, P, worst))


@pytest.mark.parametrize("n,lam,tri,route", [(37, 16, 1, "cma_sample_eval64<1, 32>"),
                                             (128, 16, 1, "cma_sample_eval<1, 8, true>"),
                                             (128, 16, 0, "cma_sample_eval<1, 8, false>")])
def test_the_clamp_takes_each_coordinates_own_bounds(hip, oracle_lib, n, lam, tri, route):
    """bound=True under tests/_boxes.py's box, whose bounds differ in every coordinate and lie on three sides of
    sphere's optimum; n = 37 is off every tile, n = 128 takes the triangular and the full operand.  First, on the
    model alone under the generator's normals as the oracle states them: coordinates on their lower bound, on
    their upper bound and strictly inside, three of each at least.  Then the walk of
    test_generations_match_the_model, its tolerance."""
    import cma_route_cases as rc
    from _boxes import binding_witness, percoord_box, percoord_centre
    seed, gens, sigma0 = 77, 6, 0.7
    lo, up = percoord_box(n)
    guess = percoord_centre(n)[None, :]
    (w,) = _models(n, lam, "sphere", lo, up, guess, bound=True, sigma0=sigma0)
    rows = []
    for gen in range(gens):
        z = np.zeros(lam * n)
        oracle_lib.f("philox_normals")(seed, w.it, lam, n, z)
        w.generation(z)
        rows.append(np.array(w.arx, float))
    binding_witness(rows, lo, up)
    g, (m,) = _pair(hip, n, lam, "sphere", bound=True, seed=seed, lo_up=(lo, up), guess=guess, sigma0=sigma0)
    g.set_state("chol_tri", [float(tri)])
    for gen in range(1, gens + 1):
        g.iterate()
        assert rc.SAMPLE_NAMES[int(g.get_state("sample_route")[0])] == route
        assert int(g.get_state("sample_lean")[0]) == 0
        m.generation(g.get_state("zlast"))
        for key in KEYS:
            err = _rel(g.get_state(key), [m.sigma] if key == "sigma" else getattr(m, key))
            assert err <= 1e-9, "n %d gen %d %s: %.3e" % (n, gen, key, err)
        assert _rel(g.get_state("fit_val"), m.fit_val) <= 1e-9
        X, Xm = g.get_state("arx").reshape(lam, n), np.asarray(m.arx, float).reshape(lam, n)
        assert (X >= lo).all() and (X <= up).all()
        np.testing.assert_array_equal(X == lo, Xm == lo)
        np.testing.assert_array_equal(X == up, Xm == up)
        assert (int(g.get_state("it")[0]), int(g.get_state("fev")[0])) == (m.it, m.fev)


def _state(g, p=0):
    return [g.get_state(k, p).copy() for k in KEYS + ("fit_val", "fit_idx", "it", "fev", "flag", "xold")]


@pytest.mark.parametrize("n,lam,P", [(16, 32, 1), (128, 1024, 1), (130, 256, 2), (10, 20, 1)])
def test_phases_one_at_a_time_equal_iterate(hip, n, lam, P):
    from bboptpy_amd import _ffi
    a, _ = _pair(hip, n, lam, "rosenbrock", P=P)
    b, _ = _pair(hip, n, lam, "rosenbrock", P=P)
    for _ in range(5):
        a.iterate()
        for ph in (_ffi.PHASE_SAMPLE_EVALUATE, _ffi.PHASE_RANK, _ffi.PHASE_UPDATE, _ffi.PHASE_EIGEN,
                   _ffi.PHASE_HISTORY_STOP):
            b.phase(ph)
        for p in range(P):
            for x, y in zip(_state(a, p), _state(b, p)):
                np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("n,lam", [(16, 32), (128, 1024), (128, 4096)])
def test_population_zero_of_a_batch_is_the_single_run(hip, n, lam):
    """few and many populations take different kernels (samplers, rankings): the same bits"""
    P = 16 if lam == 4096 else 5
    lo, up = -5. * np.ones(n), 5. * np.ones(n)
    guess = np.random.default_rng(3).uniform(-3, 3, (P, n))
    a = hip.CholeskyCMAES(10 ** 8, 1e-12, 1e-12, lam, seed=9, populations=P)
    a.initialize(hip.objectives.rosenbrock, lo, up, guess.ravel())
    b = hip.CholeskyCMAES(10 ** 8, 1e-12, 1e-12, lam, seed=9)
    b.initialize(hip.objectives.rosenbrock, lo, up, guess[0])
    for _ in range(6):
        a.iterate()
        b.iterate()
        for x, y in zip(_state(a, 0), _state(b, 0)):
            np.testing.assert_array_equal(x, y)


def test_dense_keys_are_refused_and_A_round_trips(hip):
    from bboptpy_amd import _ffi
    g, _ = _pair(hip, 10, 20, "sphere")
    g.iterate()
    for key in ("B", "C", "D", "invsqrtC"):
        with pytest.raises(_ffi.BboError) as ei:
            g.get_state(key)
        assert ei.value.status == -6
    A = g.get_state("A").reshape(10, 10)
    g.set_state("A", A)
    np.testing.assert_array_equal(g.get_state("A").reshape(10, 10), A)
    np.testing.assert_array_equal(g.get_state("BD").reshape(10, 10), A)    # the sampler's operand


def _crafted(hip, n=6, lam=12, tol=1e-6, stol=1e-8, mfev=12000):
    """one real generation on both sides, then the state is overwritten"""
    from bboptpy_amd import _ffi
    g, (m,) = _pair(hip, n, lam, "ellipsoid", tol=tol, stol=stol, mfev=mfev)
    for ph in (_ffi.PHASE_SAMPLE_EVALUATE, _ffi.PHASE_RANK, _ffi.PHASE_UPDATE):
        g.phase(ph)
    m.sample(g.get_state("zlast"))
    m.evaluate_sort()
    m.update()
    return g, m


def _stop(g, m, arx=None, f=None, fev=None):
    from bboptpy_amd import _ffi
    if arx is not None:
        g.set_state("arx", arx)
        m.arx = np.array(arx, float)
    if f is not None:
        g.set_state("fitness", f)
        m.fit_val = np.asarray(f, float)[m.fit_idx]       # (the ranking is the real generation's)
    if fev is not None:
        g.set_state("fev", [fev])
        m.fev = fev
    g.phase(_ffi.PHASE_HISTORY_STOP)
    m.update_history()
    assert int(g.get_state("it")[0]) == m.it
    return int(g.get_state("flag")[0]), int(g.get_state("stop")[0]), m.spread_parts()


def test_crafted_stop_states(hip):
    n, lam = 6, 12
    rng = np.random.default_rng(5)
    # nothing crafted: the run goes on
    g, m = _crafted(hip)
    assert _stop(g, m) == (0, 0, (False, False))
    # the population collapsed to a point: both parts hold
    g, m = _crafted(hip)
    assert _stop(g, m, arx=np.tile(rng.uniform(-1, 1, n), (lam, 1)), f=np.full(lam, 3.)) == (11, 1, (True, True))
    # spread radii, equal f: only the first part
    g, m = _crafted(hip)
    assert _stop(g, m, arx=rng.uniform(-1, 1, (lam, n)), f=np.full(lam, 3.)) == (0, 0, (True, False))
    # equal radii, spread f: only the second part
    u = rng.standard_normal((lam, n))
    u /= np.linalg.norm(u, axis=1)[:, None]
    g, m = _crafted(hip)
    assert _stop(g, m, arx=2. * u, f=np.arange(lam) + 1.) == (0, 0, (False, True))
    # equal radii (not a point), equal f: both
    g, m = _crafted(hip)
    assert _stop(g, m, arx=2. * u, f=np.full(lam, 3.)) == (11, 1, (True, True))
    # radii spread just above / below the bound (stol = 1e-8: sum of squares <= 11e-16)
    r = 2. + 3e-8 * np.linspace(-1, 1, lam)
    g, m = _crafted(hip)
    assert _stop(g, m, arx=r[:, None] * u, f=np.full(lam, 3.)) == (0, 0, (True, False))
    r = 2. + 3e-9 * np.linspace(-1, 1, lam)
    g, m = _crafted(hip)
    assert _stop(g, m, arx=r[:, None] * u, f=np.full(lam, 3.)) == (11, 1, (True, True))
    # the budget: fev >= mfev, no rule fired
    g, m = _crafted(hip)
    assert _stop(g, m, fev=12000) == (0, 2, (False, False))
    sol = g.solution()
    assert sol.n_evals == 12000 and not sol.converged


@pytest.mark.parametrize("obj,ranked", [("sphere", False), ("ellipsoid", False), ("rosenbrock", False),
                                        ("rosenbrock", True)])
def test_whole_runs_match_the_model_under_the_devices_normals(hip, obj, ranked):
    """optimize() against the model stepped with the normals the same seed draws (a second handle,
    generation by generation): evaluations, converged, x* (1e-9 of max(|x*|, 1): x* of a converged
    sphere run is itself of the size of the tolerance)"""
    n, lam, mfev, tol = 10, 20, 10000, 1e-8
    lo, up = -10. * np.ones(n), 10. * np.ones(n)
    guess = np.random.default_rng(8).uniform(-3, 3, n)
    a = hip.CholeskyCMAES(mfev, tol, tol, lam, seed=31, ranked=ranked)
    sol = a.optimize(getattr(hip.objectives, obj), lo, up, guess)
    b = hip.CholeskyCMAES(mfev, tol, tol, lam, seed=31, ranked=ranked)
    b.initialize(getattr(hip.objectives, obj), lo, up, guess)
    b.set_state("record_normals", [1.0])
    m = CholModel(mfev, tol, tol, lam, ranked=ranked)
    m.init(objective(obj, n), lo, up, guess)
    conv = False
    while m.fev < mfev:
        b.iterate()
        m.generation(b.get_state("zlast"))
        if m.converged():
            conv = True
            break
    print("%s ranked %d: model fev %d converged %s, device fev %d converged %s" % (
        obj, ranked, m.fev, conv, sol.n_evals, sol.converged))
    assert (sol.n_evals, sol.converged) == (m.fev, conv)
    err = np.abs(sol.x - m.best()).max() / max(np.abs(m.best()).max(), 1.)
    assert err <= 1e-9, err
    np.testing.assert_array_equal(sol.x, b.solution().x)          # run() == iterate() x k


def test_issue_example_converges(hip):
    n = 10
    lo, up = -10. * np.ones(n), 10. * np.ones(n)
    sol = hip.CholeskyCMAES(10000, 1e-8, 1e-8, 20, seed=4).optimize(
        hip.objectives.sphere, lo, up, np.random.default_rng(0).uniform(-3, 3, n))
    assert sol.converged and sol.n_evals < 10000 and hip.objectives.sphere(sol.x) < 1e-6


def test_host_objective_takes_the_same_path(hip):
    n = 6
    lo, up = -5. * np.ones(n), 5. * np.ones(n)
    guess = np.random.default_rng(2).uniform(-3, 3, n)
    a = hip.CholeskyCMAES(4000, 1e-8, 1e-8, 12, seed=6).optimize(hip.objectives.sphere, lo, up, guess)
    b = hip.CholeskyCMAES(4000, 1e-8, 1e-8, 12, seed=6).optimize(lambda x: float(np.dot(x, x)), lo, up, guess)
    assert a.converged and b.converged
    assert abs(a.n_evals - b.n_evals) <= 12 * 3        # (the sums of f round differently)


def test_generations_to_stop_lie_in_the_references_range(hip):
    ref = [r["generations"] for r in RUNS["results"]]
    n, lam = RUNS["n"], RUNS["lambda"]
    gens = []
    for seed in range(32):
        g = hip.CholeskyCMAES(RUNS["mfev"], RUNS["tol"], RUNS["stol"], lam, RUNS["sigma0"], seed=500 + seed)
        sol = g.optimize(hip.objectives.sphere, -10. * np.ones(n), 10. * np.ones(n),
                         np.random.default_rng(seed).uniform(-3, 3, n))
        assert sol.converged
        gens.append(sol.n_evals // lam)
    med = float(np.median(gens))
    print("reference %d..%d, device median %.1f (min %d max %d)" % (min(ref), max(ref), med, min(gens), max(gens)))
    assert min(ref) <= med <= max(ref)


def test_frozen_populations_keep_their_state(hip):
    n, lam, P = 5, 12, 4
    lo, up = -10. * np.ones(n), 10. * np.ones(n)
    g = hip.CholeskyCMAES(100000, 1e-8, 1e-8, lam, seed=12, populations=P)
    g.initialize(hip.objectives.sphere, lo, up, np.random.default_rng(1).uniform(-3, 3, P * n))
    g.run(400)
    its = [int(g.get_state("it", p)[0]) for p in range(P)]
    assert all(int(g.get_state("stop", p)[0]) == 1 for p in range(P)) and len(set(its)) > 1
    assert all(g.solution(p).converged and g.solution(p).n_evals == its[p] * lam for p in range(P))


# ---- restart drivers over a CholeskyCMAES base: the rules of tests/test_restart_gpu.py ----------
def _max_evals(n, lam, mfev, fev):
    maxit = int(100. + 50. * (n + 3) * (n + 3) / math.sqrt(1. * lam))
    return min(maxit * lam, mfev - fev)


def test_bipop_over_cholesky_follows_the_reference_rules(hip, capfd):
    n, mfev = 10, 80000
    lo, up = -5. * np.ones(n), 5. * np.ones(n)
    base = hip.CholeskyCMAES(1, 1e-6, 1e-6, 4, 2., True)       # bound: set_params switches it off
    drv = hip.BiPopCMAES(base, mfev=mfev, seed=21)
    drv.initialize(hip.objectives.rastrigin, lo, up, np.random.default_rng(1).uniform(-5, 5, n))
    assert "box bounding is no longer enabled" in capfd.readouterr().err
    lamdef = 4 + int(3. * math.log(n))
    assert int(drv.get_state("lambdadef")[0]) == lamdef
    fev = int(drv.get_state("fev")[0])
    assert fev == int(drv.get_state("last_inner_fev")[0]) + 1
    large = small = nl = 0
    best_regime, fbest = 1, drv.get_state("fxbest")[0]
    large_lambda = None
    for _ in range(60):
        if nl >= 9 or fev >= mfev:
            break
        want = (1 if large <= small * 2. else 2) if best_regime == 1 else (2 if small <= 2. * large else 1)
        drv.iterate()
        regime = int(drv.get_state("last_regime")[0])
        lam = int(drv.get_state("last_lambda")[0])
        sig = drv.get_state("last_sigma")[0]
        used = int(drv.get_state("last_inner_fev")[0])
        assert regime == want
        if regime == 1:
            assert lam == int(lamdef * 2 ** (nl + 1))
            assert sig == max(2. * (1. / 1.6) ** (nl + 1), 0.02)
            assert used <= max(_max_evals(n, lam, mfev, fev), 0) + lam
            large += used
            nl += 1
            large_lambda = lam
        else:
            assert lamdef <= lam <= max(lamdef, large_lambda // 2)
            assert 2e-2 * (1 - 1e-12) <= sig <= 2.
            assert used <= max(min(_max_evals(n, lam, mfev, fev), large >> 1), 0) + lam
            small += used
        fev += used + 1
        assert int(drv.get_state("fev")[0]) == fev
        fx = drv.get_state("fx")[0]
        if fx < fbest:
            fbest, best_regime = fx, regime
        assert drv.get_state("fxbest")[0] == fbest
        assert int(drv.get_state("bestregime")[0]) == best_regime
        assert (int(drv.get_state("largebudget")[0]), int(drv.get_state("smallbudget")[0])) == (large, small)
    assert nl >= 9 or fev >= mfev                       # ran to its budget / its last large run
    sol = drv.solution()
    assert hip.objectives.rastrigin(sol.x) == pytest.approx(fbest, rel=1e-9, abs=1e-9)
    assert int(base.get_state("chol_repairs")[0]) == 0


def test_ipop_over_cholesky_doubles_lambda_and_shrinks_sigma(hip):
    n, mfev = 10, 60000
    base = hip.CholeskyCMAES(1, 1e-6, 1e-6, 4)
    drv = hip.IPopCMAES(base, mfev=mfev, seed=5)
    drv.initialize(hip.objectives.rastrigin, -5. * np.ones(n), 5. * np.ones(n), np.zeros(n))
    lam = 4 + int(3. * math.log(n))
    sig = 2.
    fev = int(drv.get_state("fev")[0])
    for _ in range(40):
        if fev >= mfev:
            break
        drv.iterate()
        lam <<= 1
        if lam > 10 * n * n:
            lam = 10 * n * n if lam - 10 * n * n < 10 * n * n - (lam >> 1) else 4 + int(3. * math.log(n))
        sig = max(sig / 1.6, 0.02)
        assert int(drv.get_state("lambda")[0]) == lam
        assert drv.get_state("sigma")[0] == sig
        fev += int(drv.get_state("last_inner_fev")[0]) + 1
        assert int(drv.get_state("fev")[0]) == fev
    assert fev >= mfev
    sol = drv.solution()
    assert sol.n_evals == fev and not sol.converged
    # optimize() of a driver over this base, end to end
    drv2 = hip.IPopCMAES(hip.CholeskyCMAES(1, 1e-8, 1e-8, 4), mfev=20000, seed=7)
    s2 = drv2.optimize(hip.objectives.rastrigin, -5. * np.ones(n), 5. * np.ones(n), np.ones(n))
    assert np.isfinite(s2.x).all() and 0 < s2.n_evals <= 20000 + 1000


@pytest.mark.parametrize("guarded", [False, True])
@pytest.mark.parametrize("P", [1, 16])
def test_triangular_sampler_equals_the_full_operand_sampler(hip, P, guarded):
    """n = 128, lambda = 4096: P = 1 takes the tile-per-workgroup sampler, P = 16 the LDS-operand
    one; each has a triangular form (k-block <= column block, the default) and the full-operand
    form (`chol_tri` = 0).  The skipped products are exact zeros: same seed, same X, bit for bit
    (guarded: the general build of the tile loop -- box and recorded normals -- instead of the lean one)"""
    n, lam = 128, 4096
    lo, up = -5. * np.ones(n), 5. * np.ones(n)
    guess = np.random.default_rng(4).uniform(-3, 3, (P, n))
    hs = []
    for tri in (1., 0.):
        g = hip.CholeskyCMAES(10 ** 8, 1e-12, 1e-12, lam, 2., guarded, seed=13, populations=P)
        g.initialize(hip.objectives.rosenbrock, lo, up, guess.ravel())
        assert g.get_state("chol_tri")[0] == 1.            # the default
        g.set_state("chol_tri", [tri])
        if guarded:
            g.set_state("record_normals", [1.0])
        hs.append(g)
    for gen in range(4):
        for g in hs:
            g.iterate()
        for p in (0, P - 1):
            for key in ("arx", "fitness", "fit_idx", "xmean", "A", "sigma"):
                np.testing.assert_array_equal(hs[0].get_state(key, p), hs[1].get_state(key, p))
    # enum SampleKernel (bbo_cma.hpp): 8, 9 = cma_sample_eval<1, 8> and its triangular form, 6, 7 = cma_sample_eval128
    # and cma_sample_eval128_tri, whose lean build runs unless guarded
    assert [int(g.get_state("sample_route")[0]) for g in hs] == ([9, 8] if P == 1 else [7, 6])
    if P == 16:
        assert [int(g.get_state("sample_lean")[0]) for g in hs] == [0 if guarded else 1] * 2
    A = hs[0].get_state("A", 0).reshape(n, n)
    assert np.abs(np.tril(A, -1)).max() > 0.               # (a factor with off-diagonals was sampled through)
