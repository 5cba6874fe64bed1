"""GPU: the xNES kernels against the device form of tests/xnes_model.py under injected normals, the
two routes against each other, and the contract of the class.

Floats are held to 1e-9 relative to the largest entry of the key -- the project's constant for device
against model (tests/test_lm_gpu.py, tests/test_hees_gpu.py); integer keys are equal.  The model ties
in with the reference through tests/test_xnes_model.py and tests/test_xnes_golden_gpu.py.

Measured on an MI355X: device against model 2.7e-14 at most over the thirteen shapes (n = 31, fit_val;
1.7e-15 at n = 512, 4.4e-16 at n = 128); the two routes on the device at n = 24 5.1e-14; the 32
Rosenbrock runs converge after 10090 ... 11850 evaluations, median 10905, the reference's 16 after
9820 ... 12280."""
import ctypes as C

import numpy as np
import pytest

import xnes_model as xm
from _golden import load

pytestmark = pytest.mark.gpu

RTOL = 1e-9
GOLD = load("xnes_runs.json")
# the smallest shapes at which a path changes: G_B = 0; dense with np > n; the last plain-FMA shape;
# the first on the matrix pipe; the last dense; the first low-rank; ld padding; the wavefront's
# edge; two row tiles; a ragged column tile; the upper limit
SHAPES = [1, 2, 15, 16, 31, 32, 33, 63, 64, 65, 128, 130, 512]
FLOAT_KEYS = ("B", "xmean", "sigma", "gsigma", "arx", "arz", "ary", "fit_val", "fbest", "xbest", "u")
INT_KEYS = ("fit_idx", "np", "it", "fev", "stop", "conv", "fact_fail", "route")
ALL_KEYS = FLOAT_KEYS + INT_KEYS


def _bits(a, b, what):
    a, b = np.asarray(a, float).ravel(), np.asarray(b, float).ravel()
    assert a.shape == b.shape, what
    assert a.tobytes() == b.tobytes(), (what, np.flatnonzero(a != b)[:8], a[a != b][:4], b[a != b][:4])


def _rel(a, b):
    a, b = np.asarray(a, float).ravel(), np.asarray(b, float).ravel()
    assert a.shape == b.shape
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _snapshot(g, p=0, keys=ALL_KEYS):
    return {k: g.get_state(k, p).copy() for k in keys}


def _model_state(m):
    return {"B": m.B, "xmean": m.mu, "sigma": [m.sigma], "gsigma": [m.gsigma], "arx": m.x, "arz": m.z, "ary": m.y,
            "fit_val": m.f, "fbest": [m.fbest], "xbest": m.xbest, "u": m.u, "fit_idx": m.order, "np": [m.np],
            "it": [m.it], "fev": [m.fev], "stop": [m.stop], "conv": [int(m.conv)], "fact_fail": [m.fact_fail],
            "route": [m.route]}


def _generation(g, gen):
    """the generations alternate between iterate() and the four phases"""
    if gen % 2:
        g.iterate()
    else:
        for ph in range(4):
            g.phase(ph)


@pytest.mark.parametrize("n", SHAPES)
def test_generations_against_the_device_form_of_the_model(hip, n):
    P, gens = 3, 3 if n == 512 else 5
    obj = "sphere" if n == 1 else ["rosenbrock", "ellipsoid"][n % 2]
    a0, etamu = 0.7, 0.9
    rng = np.random.default_rng(4000 + n)
    np_ = xm.popsize(n)
    z = rng.standard_normal((gens, P, np_, n))
    g = hip.xNES(10 ** 9, 0., a0, etamu, seed=n, populations=P)
    g.initialize(obj, -5. * np.ones(n), 5. * np.ones(n), np.ones(P * n))
    g.inject_normals(z)
    f = xm.device_objective(obj, n)
    models = [xm.XNes(f, n, a0, etamu).init() for _ in range(P)]
    assert int(g.get_state("route")[0]) == models[0].route == (1 if n >= 32 else 0)
    _bits(g.get_state("xmean", 1), np.zeros(n), "the mean starts at the origin whatever the guess")
    worst = (-1., "")
    for gen in range(1, gens + 1):
        _generation(g, gen)
        for p in range(P):
            models[p].iterate_device(z[gen - 1, p])
            want, have = _model_state(models[p]), _snapshot(g, p)
            for k in INT_KEYS:
                assert have[k].astype(int).tolist() == [int(v) for v in want[k]], (k, gen, p)
            for k in FLOAT_KEYS:
                err = _rel(have[k], want[k])
                worst = max(worst, (err, "%s generation %d population %d" % (k, gen, p)))
                assert err <= RTOL, (k, gen, p, err)
    print("n = %d, np = %d: worst relative deviation from the model over %d generations %.3e (%s)"
          % ((n, np_, gens) + worst))
    if n == 1:
        for p in range(P):
            assert abs(float(g.get_state("B", p)[0]) - 1.) <= 1e-15     # G_B = 0: B stays 1
    with pytest.raises(Exception, match="used up"):
        g.iterate()
    g.inject_normals(None)
    g.iterate()
    assert int(g.get_state("it")[0]) == gens + 1


def test_the_two_routes_agree_on_the_device_at_n24(hip):
    n, P, gens = 24, 3, 5
    np_ = xm.popsize(n)
    z = np.random.default_rng(24).standard_normal((gens, P, np_, n))
    lo, up = -5. * np.ones(n), 5. * np.ones(n)
    a = hip.xNES(10 ** 9, 0., seed=1, populations=P)
    b = hip.xNES(10 ** 9, 0., seed=1, populations=P)
    for h in (a, b):
        h.initialize("rosenbrock", lo, up, np.zeros(P * n))
        h.inject_normals(z)
    a.set_state("lowrank_min_n", [16.])
    assert (int(a.get_state("route")[0]), int(b.get_state("route")[0])) == (1, 0)
    assert int(a.get_state("lowrank_min_n")[0]) == 16 and int(b.get_state("lowrank_min_n")[0]) == 32
    worst = (-1., "")
    for gen in range(1, gens + 1):
        _generation(a, gen)
        _generation(b, gen + 1)
        for p in range(P):
            sa, sb = _snapshot(a, p), _snapshot(b, p)
            for k in INT_KEYS:
                if k != "route":
                    assert np.array_equal(sa[k], sb[k]), (k, gen, p)
            for k in FLOAT_KEYS:
                err = _rel(sa[k], sb[k])
                worst = max(worst, (err, "%s generation %d population %d" % (k, gen, p)))
                assert err <= RTOL, (k, gen, p, err)
    print("n = 24: worst relative deviation between the routes on the device %.3e (%s)" % worst)
    for bad in (15., 33., 16.5):
        with pytest.raises(Exception, match="lowrank_min_n"):
            a.set_state("lowrank_min_n", [bad])


def test_same_seed_same_bits_and_populations_draw_their_own_streams(hip):
    n, P = 20, 3
    lo, up = -5. * np.ones(n), 5. * np.ones(n)
    a, b, c = (hip.xNES(10 ** 9, 0., seed=s, populations=P) for s in (7, 7, 8))
    one = hip.xNES(10 ** 9, 0., seed=7)
    for h in (a, b, c):
        h.initialize("ellipsoid", lo, up, np.zeros(P * n))
        assert h.run(9) == 9
    one.initialize("ellipsoid", lo, up, np.zeros(n))
    assert one.run(9) == 9
    for p in range(P):
        sa, sb = _snapshot(a, p), _snapshot(b, p)
        for k in sa:
            _bits(sa[k], sb[k], k)
    sa, s1 = _snapshot(a, 0), _snapshot(one, 0)
    for k in sa:
        _bits(sa[k], s1[k], "populations=1 against population 0 of three: " + k)
    z = [a.get_state("arz", p) for p in range(P)]
    assert not np.array_equal(z[0], z[1]) and not np.array_equal(z[1], z[2])
    assert not np.array_equal(z[0], c.get_state("arz", 0))
    assert abs(z[0].mean()) < 0.6 and 0.5 < z[0].std() < 1.5 and np.unique(z[0]).size == z[0].size


@pytest.mark.parametrize("obj", ["sphere", "rosenbrock"])
def test_a_callable_in_the_builtins_order_gives_the_builtins_run(hip, obj):
    n = 70
    np_ = xm.popsize(n)
    lo, up, guess = -5. * np.ones(n), 5. * np.ones(n), np.zeros(n)
    f = xm.device_objective(obj, n)
    calls = []

    def host(x):
        calls.append(1)
        return float(f(np.asarray(x, float))[0])

    a, b = hip.xNES(10 ** 9, 0., seed=5), hip.xNES(10 ** 9, 0., seed=5)
    a.initialize(obj, lo, up, guess)
    b.initialize(host, lo, up, guess)
    assert a.run(8) == 8 and b.run(8) == 8
    assert len(calls) == 8 * np_
    sa, sb = _snapshot(a), _snapshot(b)
    for k in sa:
        _bits(sa[k], sb[k], k)
    _bits(a.solution().x, b.solution().x, "solution")
    _bits(a.solution().x, sa["arx"].reshape(np_, n)[int(sa["fit_idx"][0])], "the best candidate of the last generation")


def test_the_mean_starts_at_the_origin_or_at_the_guess(hip):
    n, P = 7, 2
    lo, up = np.ones(n), 3. * np.ones(n)
    guess = np.linspace(1.5, 2.5, P * n)
    g = hip.xNES(1000, 0., seed=1, populations=P)
    g.initialize("sphere", lo, up, guess)
    h = hip.xNES(1000, 0., seed=1, populations=P, from_guess=True)
    h.initialize("sphere", lo, up, guess)
    for p in range(P):
        _bits(g.get_state("xmean", p), np.zeros(n), "default: the reference's start at the origin")
        _bits(h.get_state("xmean", p), guess[p * n:(p + 1) * n], "from_guess")
        _bits(g.solution(p).x, np.zeros(n), "before the first generation the reference's point is the origin")
    assert float(g.get_state("sigma")[0]) == 1. and np.array_equal(g.get_state("B").reshape(n, n), np.eye(n))
    # the reference's converged() on the zero points of init(): 0 < tol; the stop flag is not set
    assert g.solution().converged is False and g.solution().n_evals == 0
    a = hip.xNES(1000, 1e-8, 0.25, seed=1)
    a.initialize("sphere", lo, up, guess[:n])
    assert a.solution().converged is True and int(a.get_state("stop")[0]) == 0
    assert float(a.get_state("sigma")[0]) == 0.25 and np.array_equal(a.get_state("B").reshape(n, n), np.eye(n))


def test_budget_stop_and_converged_stop(hip):
    bud = GOLD["runs"]["budget"]
    n = bud["n"]
    np_ = xm.popsize(n)
    lo, up = -5. * np.ones(n), 5. * np.ones(n)
    g = hip.xNES(bud["mfev"], bud["tol"], seed=3)
    sol = g.optimize("rosenbrock", lo, up, np.zeros(n))
    # the loop overshoots to a multiple of np, as the reference's did
    assert sol.n_evals == bud["fev"] == 510 and sol.n_evals % np_ == 0 and sol.n_evals >= bud["mfev"]
    assert sol.converged is False and int(g.get_state("stop")[0]) == 2
    arx, idx = g.get_state("arx").reshape(np_, n), g.get_state("fit_idx").astype(int)
    _bits(sol.x, arx[idx[0]], "solution() is the best point of the last generation")
    assert g.run(5) == 0        # the budget is spent
    g = hip.xNES(10 ** 6, 1e-8, seed=3)
    sol = g.optimize("sphere", lo, up, np.zeros(n))
    assert sol.converged is True and int(g.get_state("stop")[0]) == 1 and int(g.get_state("conv")[0]) == 1
    assert sol.n_evals % np_ == 0 and sol.n_evals < 10 ** 6
    fv = g.get_state("fit_val")[g.get_state("fit_idx").astype(int)]
    assert abs(fv[0] - fv[-1]) < 1e-8
    assert float(g.get_state("fbest")[0]) <= fv[0]


def test_a_stopped_population_freezes_while_the_others_go_on(hip):
    n, P = 6, 3
    g = hip.xNES(10 ** 9, 1e-300, seed=3, populations=P)
    g.initialize("sphere", -np.ones(n), np.ones(n), np.zeros(P * n))
    assert g.run(2) == 2
    np_ = xm.popsize(n)
    g.inject_normals(np.concatenate([np.random.default_rng(1).standard_normal((1, 1, np_, n)),
                                     np.zeros((1, 1, np_, n)),       # equal points: f_best = f_worst
                                     np.random.default_rng(2).standard_normal((1, 1, np_, n))], axis=1))
    assert g.run(1) == 1
    g.inject_normals(None)
    assert [int(g.get_state("stop", p)[0]) for p in range(P)] == [0, 1, 0]
    frozen = _snapshot(g, 1)
    assert g.run(5) == 5
    after = _snapshot(g, 1)
    for k in frozen:
        _bits(frozen[k], after[k], k)
    assert [int(g.get_state("it", p)[0]) for p in range(P)] == [8, 3, 8]


def test_equal_rows_fail_the_factorisation_and_leave_B(hip):
    n = 64
    np_ = xm.popsize(n)
    rng = np.random.default_rng(5)
    z = rng.standard_normal((2, 1, np_, n))
    z[1, 0, 7] = z[1, 0, 3]
    g = hip.xNES(10 ** 9, 0., seed=1)
    g.initialize("sphere", -np.ones(n), np.ones(n), np.zeros(n))
    g.inject_normals(z)
    g.iterate()
    assert int(g.get_state("fact_fail")[0]) == 0
    B0 = g.get_state("B").copy()
    assert not np.array_equal(B0.reshape(n, n), np.eye(n))
    g.iterate()
    assert int(g.get_state("fact_fail")[0]) == 1
    _bits(g.get_state("B"), B0, "B is unchanged by the generation whose factorisation failed")
    for k in FLOAT_KEYS:
        assert np.isfinite(g.get_state(k)).all(), k
    assert int(g.get_state("it")[0]) == 2 and int(g.get_state("fev")[0]) == 2 * np_
    m = xm.XNes(xm.device_objective("sphere", n), n).init()
    m.iterate_device(z[0, 0])
    m.iterate_device(z[1, 0])
    assert m.fact_fail == 1 and _rel(g.get_state("xmean"), m.mu) <= RTOL and _rel(g.get_state("sigma"), [m.sigma]) <= RTOL
    g.inject_normals(None)
    g.iterate()             # the next generation adapts again
    assert int(g.get_state("fact_fail")[0]) == 1 and not np.array_equal(g.get_state("B"), B0)


def test_limits_and_refusals_through_the_c_abi(hip):
    from bboptpy_amd import _ffi
    L = _ffi.lib()
    g = hip.xNES(1000, 1e-8, seed=1)
    with pytest.raises(_ffi.BboError) as ei:
        g.initialize("sphere", -np.ones(513), np.ones(513), np.zeros(513))
    assert ei.value.status == _ffi.ERR_ARG and "dimension must be in [1, 512]" in str(ei.value)
    for a0 in (0., -1., float("inf"), float("nan")):
        with pytest.raises(_ffi.BboError) as ei:
            hip.xNES(1000, 1e-8, a0, seed=1)._ensure_handle()
        assert ei.value.status == _ffi.ERR_ARG

    d = _ffi.XnesParams()
    L.bbo_xnes_params_default(C.byref(d))
    other = hip.HEES(1000, 1e-6, seed=1)
    oh = other._ensure_handle()
    assert L.bbo_xnes_configure(oh, C.byref(d)) == _ffi.ERR_ARG
    assert "not an xNES handle" in L.bbo_last_error(oh).decode()
    assert L.bbo_xnes_phase(oh, 0) == _ffi.ERR_ARG and L.bbo_xnes_inject_normals(oh, None, 0) == _ffi.ERR_ARG
    n = 6
    np_ = xm.popsize(n)
    lo, up = -np.ones(n), np.ones(n)
    g = hip.xNES(1000, 1e-8, seed=1)
    h = g._ensure_handle()
    assert L.bbo_xnes_configure(h, None) == _ffi.ERR_ARG
    assert L.bbo_xnes_phase(h, 0) == -2 and "before initialize" in L.bbo_last_error(h).decode()
    # an objective program: refused by the class and by the library, naming who takes one
    prog = hip.DeviceObjective('extern "C" __device__ double bbo_user_objective(const double *x, int n, '
                               'const double *data) { return x[0] * x[0]; }')
    with pytest.raises(ValueError, match="xNES does not take a DeviceObjective"):
        g.initialize(prog, lo, up, np.zeros(n))
    ob = _ffi.Objective()
    ob.kind, ob.user = _ffi.OBJ_PROGRAM, prog._handle
    st = L.bbo_init(h, n, lo, up, np.zeros(n), C.byref(ob))
    msg = L.bbo_last_error(h).decode()
    assert st == -1 and "xNES" in msg and "CMAES" in msg and "SHADE" in msg, (st, msg)
    g.initialize("sphere", lo, up, np.zeros(n))
    assert L.bbo_xnes_configure(h, C.byref(d)) == -2            # BBO_ERR_STATE
    assert "after bbo_init" in L.bbo_last_error(h).decode()
    assert L.bbo_xnes_phase(h, 4) == _ffi.ERR_ARG and L.bbo_xnes_phase(h, -1) == _ffi.ERR_ARG
    with pytest.raises(_ffi.BboError, match="populations \\* np \\* n"):
        g.inject_normals(np.zeros(np_ * n - 1))
    g.inject_normals(np.zeros(np_ * n))
    g.iterate()
    _bits(g.get_state("arx"), np.zeros((np_, n)), "z = 0: every candidate is the mean")
    with pytest.raises(_ffi.BboError, match="used up") as ei:
        g.iterate()
    assert ei.value.status == -2
    g.initialize("sphere", lo, up, np.zeros(n))               # bbo_init returns to the device generator
    g.iterate()
    assert g.get_state("arx").any()
    with pytest.raises(_ffi.BboError):
        g.get_state("no_such_key")


def test_outcome_distribution_of_the_rosenbrock_runs(hip):
    """device generator, so not comparable draw by draw: 32 seeds as one handle of 32 populations;
    every run converges (every reference run did) and the median of fev lies inside the
    reference's [min, max] over its 16"""
    runs = GOLD["runs"]
    ref = runs["converging"]
    assert len(ref) == 16 and all(r["converged"] for r in ref)
    n, P = runs["n"], 32
    g = hip.xNES(runs["mfev"], runs["tol"], runs["a0"], runs["etamu"], seed=900, populations=P, poll_every=64)
    g.initialize("rosenbrock", -5. * np.ones(n), 5. * np.ones(n), np.zeros(P * n))
    g.run(10 ** 9)
    sols = [g.solution(p) for p in range(P)]
    assert all(s.converged is True for s in sols)
    assert [int(g.get_state("stop", p)[0]) for p in range(P)] == [1] * P
    fev = [s.n_evals for s in sols]
    lo_ref, hi_ref = min(r["fev"] for r in ref), max(r["fev"] for r in ref)
    print("device fev min %d median %.0f max %d; the reference [%d, %d]"
          % (min(fev), np.median(fev), max(fev), lo_ref, hi_ref))
    assert lo_ref <= np.median(fev) <= hi_ref
