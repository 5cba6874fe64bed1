"""GPU: the LmCMAES kernels against the device form of tests/lm_model.py under injected NumPy draws,
and the engine's contract.

The device form of the model adds every dot product and every built-in objective in the device's
order, so given the same draws the two differ only where libm and the device's exp may (the sigma
rule): the state is held to 1e-9 relative to the largest entry of the key -- the project's constant
for device against model (tests/test_hees_gpu.py, tests/test_chol_gpu.py) -- and fit_idx, jarr,
larr, memlen, it, fev and the stop state are equal.  The shapes are the ones at which the kernels
take another path: n below, at and above one wavefront and one workgroup of columns, n = 1000 and
4096 with 4 and 16 columns per thread, lambda = 2, odd, a multiple of the block of four "+"
candidates and several blocks, memory 1, 2, 3 and the default, both sampling modes, both `usenew`,
three populations with their own guesses, m t + 3 generations so that the slot list wraps.  Ties
(n = 1, 2 with Rademacher draws repeat candidates) are ranked in index order by both.

Measured on an MI355X: the largest deviation from the model over all shapes is 4.0e-15 (n = 2,
lambda = 33, generation 4, d), seven of the thirteen shapes agree in every bit; the runs of "stops"
end with the reference's flags after 10, 184, 484 and 2 generations (the reference: 10, 183, 511,
61); the median fev over 32 seeds is 2148 with Gaussian and 2736 with Rademacher draws (the
reference's ranges: [2040, 2232] and [2640, 2832])."""
import ctypes as C
import math

import numpy as np
import pytest

import lm_model as lm
from _boxes import binding_witness, percoord_box, percoord_guess
from test_lm_model import GOLD, KEYS, INT_KEYS

pytestmark = pytest.mark.gpu

RTOL = 1e-9
SNAP = KEYS + ("stop", "conv", "xold")

# (n, lambda, memory, rademacher, usenew, objective)
SHAPES = [
    (1, 2, 1, 1, 1, "sphere"),
    (1, 7, 2, 0, 0, "sphere"),
    (2, 8, 0, 1, 1, "rosenbrock"),
    (2, 33, 3, 0, 1, "ellipsoid"),
    (63, 7, 0, 1, 1, "rosenbrock"),
    (64, 2, 3, 0, 0, "ellipsoid"),
    (64, 33, 2, 1, 1, "cigar"),
    (65, 8, 0, 0, 1, "rosenbrock"),
    (257, 7, 2, 1, 0, "ellipsoid"),
    (257, 33, 1, 0, 1, "sphere"),
    (1000, 8, 3, 1, 1, "ellipsoid"),
    (1000, 7, 1, 0, 0, "rosenbrock"),
]


def _bits(a, b, what):
    a, b = np.asarray(a, float).ravel(), np.asarray(b, float).ravel()
    assert a.shape == b.shape, what
    assert a.tobytes() == b.tobytes(), (what, np.flatnonzero(a != b)[:8], a[a != b][:4], b[a != b][:4])


def _snapshot(g, p=0, keys=SNAP):
    return {k: g.get_state(k, p).copy() for k in keys}


def _models(P, lam, memory, usenew, bound, obj, lo, up, guess):
    models = []
    for p in range(P):
        m = lm.LmModel(10 ** 9, 0., lam, memory, 1.5, bound, bool(usenew), device=True)
        m.init(obj, lo, up, guess[p])
        models.append(m)
    return models


def _against_model(hip, n, lam, memory, rad, usenew, obj, gens, P=3, bound=False, seed=1, box=None, guess=None,
                   before=None):
    """`box`, `guess`: other bounds and starting points than +-5 and the drawn ones; `before(models, table)`
    is called with models of their own, before the device has done anything"""
    rng = np.random.default_rng(1000 * n + 10 * lam + memory)
    if guess is None:
        guess = rng.uniform(-3., 3., (P, n))
    lo, up = (-5. * np.ones(n), 5. * np.ones(n)) if box is None else box
    g = hip.LmCMAES(10 ** 9, 0., lam, memory, 1.5, bound, bool(rad), bool(usenew), seed=seed, populations=P)
    g.initialize(obj, lo, up, guess.ravel())
    models = _models(P, lam, memory, usenew, bound, obj, lo, up, guess)
    table = np.array([[m.draw(rng, bool(rad)) for m in models] for _ in range(gens)])
    if before is not None:
        before(_models(P, lam, memory, usenew, bound, obj, lo, up, guess), table)
    g.inject_draws(table)
    worst = (0., None)
    for gen in range(gens):
        # (not run(): the tiny shapes raise EqualFunVals on their ties, and run() honours a stop)
        if gen % 2:
            g.iterate()
        else:
            for ph in range(5):
                g.phase(ph)
        for p, m in enumerate(models):
            m.generation(table[gen, p])
            want = m.state()
            for k in KEYS:
                have = g.get_state(k, p)
                tag = "n%d l%d generation %d population %d %s" % (n, lam, gen + 1, p, k)
                assert have.shape == want[k].shape, tag
                if k in INT_KEYS:
                    assert np.array_equal(have, want[k]), (tag, have, want[k])
                    continue
                err = float(np.abs(have - want[k]).max() / max(np.abs(want[k]).max(), 1e-300))
                assert err <= RTOL, (tag, err)
                if err > worst[0]:
                    worst = (err, tag)
    print("n=%d lambda=%d memory=%d: largest deviation from the model %.3e (%s)" % (n, lam, models[0].m, *worst))
    return g, models


@pytest.mark.parametrize("n,lam,memory,rad,usenew,obj", SHAPES,
                         ids=["n%d_l%d_m%d_rad%d_new%d" % s[:5] for s in SHAPES])
def test_wrapping_runs_against_the_device_form_of_the_model(hip, n, lam, memory, rad, usenew, obj):
    m = memory if memory > 0 else lm.default_memory(n)
    t = max(1, int(math.log(n))) if usenew else 1
    g, models = _against_model(hip, n, lam, memory, rad, usenew, obj, m * t + 3)
    assert int(g.get_state("memlen")[0]) == m == models[0].m
    assert sorted(g.get_state("jarr").astype(int)) == list(range(m))


def percoord_witness(models, table):
    """from the models alone: the clamp of the mean binds under tests/_boxes.py's box"""
    lo, up = models[0].lower, models[0].upper
    for p, m in enumerate(models):
        means = []
        for gen in range(table.shape[0]):
            m.generation(table[gen, p])
            means.append(np.array(m.xmean, float))
        binding_witness(means, np.asarray(lo, float), np.asarray(up, float))


@pytest.mark.parametrize("n,lam,memory,rad", [(33, 8, 0, 1), (257, 8, 2, 0)])
def test_the_mean_is_clamped_to_each_coordinates_own_bounds(hip, n, lam, memory, rad):
    """bound=True under bounds that differ in every coordinate (tests/_boxes.py): sphere drives the mean
    onto its lower bound in a third of the coordinates, onto its upper bound in a third, and leaves a third
    free -- asserted on the models alone before the device runs; then the walk of this file, its tolerance.
    n = 33 is off every tile, 257 the first n past one pass of the workgroup."""
    lo, up = percoord_box(n)
    g, models = _against_model(hip, n, lam, memory, rad, 1, "sphere", 12, bound=True, box=(lo, up),
                               guess=percoord_guess(n, 3), before=percoord_witness)
    for p in range(3):
        xm = g.get_state("xmean", p)
        assert (xm >= lo).all() and (xm <= up).all()
        # on a bound exactly where the model's mean is
        np.testing.assert_array_equal(xm == lo, np.asarray(models[p].xmean) == lo)
        np.testing.assert_array_equal(xm == up, np.asarray(models[p].xmean) == up)


def test_n4096_three_generations(hip):
    g, models = _against_model(hip, 4096, 8, 0, 1, 1, "ellipsoid", 3, P=2)
    assert int(g.get_state("memory")[0]) == 128 and int(g.get_state("memlen")[0]) == 1


def test_the_mean_is_clamped_and_never_a_candidate(hip):
    n, lam = 6, 8
    # the mean starts next to a corner and the optimum lies outside the box
    lo, up = 1. * np.ones(n), 2. * np.ones(n)
    g = hip.LmCMAES(10 ** 9, 0., lam, 2, 3., True, False, True, seed=4)
    m = lm.LmModel(10 ** 9, 0., lam, 2, 3., True, True, device=True)
    guess = np.full(n, 1.05)
    g.initialize("sphere", lo, up, guess)
    m.init("sphere", lo, up, guess)
    rng = np.random.default_rng(8)
    outside = clamped = 0
    for _ in range(6):
        tab = m.draw(rng, False)
        g.inject_draws(tab)
        g.iterate()
        m.generation(tab)
        x, xm = g.get_state("arx").reshape(lam, n), g.get_state("xmean")
        assert (xm >= lo).all() and (xm <= up).all()
        _bits(xm, m.xmean, "xmean")
        _bits(x, m.arx, "arx")
        outside += int(((x < lo) | (x > up)).any())
        clamped += int((xm == lo).any())
    assert outside == 6 and clamped > 0


def test_run_is_iterate_is_the_five_phases(hip):
    n, lam, P = 37, 9, 2
    lo, up = -5. * np.ones(n), 5. * np.ones(n)
    guess = np.linspace(-2., 2., P * n)
    for rad in (True, False):
        hs = [hip.LmCMAES(10 ** 9, 0., lam, 3, 2., False, rad, True, seed=21, populations=P) for _ in range(3)]
        for h in hs:
            h.initialize("rosenbrock", lo, up, guess)
        assert hs[0].run(12) == 12
        for _ in range(12):
            hs[1].iterate()
            for ph in range(5):
                hs[2].phase(ph)
        for p in range(P):
            sa, sb, sc = (_snapshot(h, p) for h in hs)
            for k in sa:
                _bits(sa[k], sb[k], k)
                _bits(sa[k], sc[k], k)
            assert int(sa["it"][0]) == 12 and int(sa["fev"][0]) == 12 * lam


def test_same_seed_same_bits_and_populations_draw_their_own_streams(hip):
    n, lam, P = 20, 8, 3
    lo, up, guess = -5. * np.ones(n), 5. * np.ones(n), np.tile(np.linspace(-2., 2., n), P)
    for rad in (True, False):
        a, b, c = (hip.LmCMAES(10 ** 9, 0., lam, 0, 2., False, rad, True, seed=s, populations=P) for s in (7, 7, 8))
        for h in (a, b, c):
            h.initialize("ellipsoid", lo, up, guess)
            assert h.run(9) == 9
        for p in range(P):
            sa, sb = _snapshot(a, p), _snapshot(b, p)
            for k in sa:
                _bits(sa[k], sb[k], k)
        # the same guess everywhere: what differs comes from the streams
        z = [a.get_state("z", p) for p in range(P)]
        assert not np.array_equal(z[0], z[1]) and not np.array_equal(z[1], z[2])
        assert not np.array_equal(a.get_state("xmean", 0), a.get_state("xmean", 1))
        assert not np.array_equal(a.get_state("z", 0), c.get_state("z", 0))
        zz = a.get_state("z", 0)
        if rad:
            assert set(np.unique(zz)) == {-1., 1.} and abs(zz.mean()) < 0.5
        else:
            assert abs(zz.mean()) < 0.6 and 0.5 < zz.std() < 1.5 and np.unique(zz).size == zz.size
        assert abs(a.get_state("g", 0)).max() < 8.


@pytest.mark.parametrize("obj", ["sphere", "rosenbrock"])
def test_a_callable_in_the_builtins_order_gives_the_builtins_run(hip, obj):
    n, lam = 70, 7
    lo, up, guess = -5. * np.ones(n), 5. * np.ones(n), np.linspace(-2., 2., n)
    f = lm.device_objective(obj, n)
    calls = []

    def host(x):
        calls.append(1)
        return f(np.asarray(x, float))

    a = hip.LmCMAES(10 ** 9, 0., lam, 3, 2., seed=5)
    b = hip.LmCMAES(10 ** 9, 0., lam, 3, 2., seed=5)
    a.initialize(obj, lo, up, guess)
    b.initialize(host, lo, up, guess)
    assert a.run(8) == 8 and b.run(8) == 8
    assert len(calls) == 8 * lam
    sa, sb = _snapshot(a), _snapshot(b)
    for k in sa:
        _bits(sa[k], sb[k], k)
    _bits(a.solution().x, b.solution().x, "solution")
    _bits(a.solution().x, sa["arx"].reshape(lam, n)[int(sa["fit_idx"][0])], "the best candidate of the last generation")


def test_a_stopped_population_freezes_while_the_others_go_on(hip):
    n, lam, P = 12, 8, 3
    lo, up = -5. * np.ones(n), 5. * np.ones(n)
    g = hip.LmCMAES(10 ** 9, 0., lam, seed=3, populations=P)
    g.initialize("sphere", lo, up, np.linspace(-2., 2., P * n))
    assert g.run(2) == 2
    g.set_state("sigma", [1e-17], population=1)
    assert g.run(1) == 1
    assert [int(g.get_state("flag", p)[0]) for p in range(P)] == [0, 11, 0]
    assert [int(g.get_state("stop", p)[0]) for p in range(P)] == [0, 1, 0]
    frozen = _snapshot(g, 1)
    assert g.run(5) == 5
    after = _snapshot(g, 1)
    for k in frozen:
        _bits(frozen[k], after[k], k)
    assert [int(g.get_state("it", p)[0]) for p in range(P)] == [8, 3, 8]
    assert g.solution(1).converged is True and g.solution(0).converged is False
    assert g.solution(1).n_evals == 3 * lam and g.solution(0).n_evals == 8 * lam
    # iterate() (and the phases) do not look at the stop flag, like the reference's iterate()
    g.iterate()
    assert int(g.get_state("it", 1)[0]) == 4


@pytest.mark.parametrize("name", [r["name"] for r in GOLD["runs"]["stops"]])
def test_every_stop_test_is_reached_with_the_references_flag(hip, name):
    rec = {r["name"]: r for r in GOLD["runs"]["stops"]}[name]
    n = rec["n"]
    rng = np.random.default_rng(rec["seed"])
    g = hip.LmCMAES(rec["mfev"], rec["tol"], rec["lambda"], 0, 2., False, bool(rec["rademacher"]), True, seed=rec["seed"])
    sol = g.optimize("sphere", -10. * np.ones(n), 10. * np.ones(n), rng.uniform(-3., 3., n))
    flag, it = int(g.get_state("flag")[0]), int(g.get_state("it")[0])
    print("%s: flag %d after %d generations (the reference: %d after %d)" % (name, flag, it, rec["flag"], rec["generations"]))
    assert flag == rec["flag"] and sol.converged is True and sol.n_evals == it * rec["lambda"]
    if name == "maxiter":
        assert it == rec["generations"] == rec["mfev"] // rec["lambda"]
    if name == "sigma":
        assert float(g.get_state("sigma")[0]) < 1e-16


def test_a_nan_value_ranks_last(hip):
    n, lam = 5, 8
    calls = []

    def f(x):
        calls.append(1)
        return float("nan") if len(calls) % lam == 3 else float(x @ x)

    g = hip.LmCMAES(10 ** 9, 0., lam, seed=2, rademacher=False)
    g.initialize(f, -5. * np.ones(n), 5. * np.ones(n), np.linspace(-2., 2., n))
    for _ in range(3):
        g.iterate()
        assert int(g.get_state("fit_idx")[-1]) == 2 and g.get_state("fit_val")[-1] == np.inf
        assert np.isfinite(g.get_state("fit_val")[:-1]).all() and np.isfinite(g.get_state("xmean")).all()
        assert np.isfinite(g.get_state("sigma")).all()


def test_limits_and_refusals_through_the_c_abi(hip):
    from bboptpy_amd import _ffi
    L = _ffi.lib()

    def refused(n, np_, memory=0, sigma0=2.):
        g = hip.LmCMAES(1000, 1e-8, np_, memory, sigma0, seed=1)
        with pytest.raises(_ffi.BboError) as ei:
            g.initialize("sphere", -np.ones(n), np.ones(n), np.zeros(n))
        assert ei.value.status == _ffi.ERR_ARG
        return str(ei.value)

    assert "dimension must be in [1, 4096]" in refused(4097, 8)
    assert "np (lambda) must be in [2, 4096]" in refused(8, 1)
    assert "np (lambda) must be in [2, 4096]" in refused(8, 4097)
    assert "must be in [1, 256]" in refused(8, 8, memory=257)
    assert "sigma0 must be finite" in refused(8, 8, sigma0=float("inf"))
    assert "sigma0 must be finite" in refused(8, 8, sigma0=float("nan"))
    # the limits themselves are served
    g = hip.LmCMAES(10 ** 6, 1e-8, 2, 256, seed=1)
    g.initialize("sphere", -np.ones(8), np.ones(8), np.zeros(8))
    assert g.run(2) == 2 and int(g.get_state("memory")[0]) == 256

    d = _ffi.LmParams()
    L.bbo_lm_params_default(C.byref(d))
    other = hip.HEES(1000, 1e-6, seed=1)
    oh = other._ensure_handle()
    assert L.bbo_lm_configure(oh, C.byref(d)) == _ffi.ERR_ARG
    assert "not an LmCMAES handle" in L.bbo_last_error(oh).decode()
    assert L.bbo_lm_phase(oh, 0) == _ffi.ERR_ARG and L.bbo_lm_inject_draws(oh, None, 0) == _ffi.ERR_ARG
    n, lam = 6, 7
    lo, up = -np.ones(n), np.ones(n)
    g = hip.LmCMAES(1000, 1e-8, lam, seed=1)
    h = g._ensure_handle()
    assert L.bbo_lm_configure(h, None) == _ffi.ERR_ARG
    assert L.bbo_lm_phase(h, 0) == -2 and "before initialize" in L.bbo_last_error(h).decode()
    # an objective program: refused by the class and by the library, naming who takes one
    prog = hip.DeviceObjective('extern "C" __device__ double bbo_user_objective(const double *x, int n, '
                               'const double *data) { return x[0] * x[0]; }')
    with pytest.raises(ValueError, match="LmCMAES does not take a DeviceObjective"):
        g.initialize(prog, lo, up, np.zeros(n))
    ob = _ffi.Objective()
    ob.kind, ob.user = _ffi.OBJ_PROGRAM, prog._handle
    st = L.bbo_init(h, n, lo, up, np.zeros(n), C.byref(ob))
    msg = L.bbo_last_error(h).decode()
    assert st == -1 and "LmCMAES" in msg and "CMAES" in msg and "SHADE" in msg, (st, msg)
    g.initialize("sphere", lo, up, np.zeros(n))
    assert L.bbo_lm_configure(h, C.byref(d)) == -2            # BBO_ERR_STATE
    assert "after bbo_init" in L.bbo_last_error(h).decode()
    assert L.bbo_lm_phase(h, 5) == _ffi.ERR_ARG and L.bbo_lm_phase(h, -1) == _ffi.ERR_ARG
    with pytest.raises(_ffi.BboError, match="rows of n \\+ 1 values"):
        g.inject_draws(np.zeros(4 * (n + 1) - 1))             # ceil(7 / 2) = 4 rows of n + 1
    g.inject_draws(np.zeros(4 * (n + 1)))
    g.iterate()
    _bits(g.get_state("arx"), np.zeros((lam, n)), "z = 0: every candidate is the mean")
    with pytest.raises(_ffi.BboError, match="used up"):
        g.iterate()
    g.initialize("sphere", lo, up, np.zeros(n))               # bbo_init returns to the device generator
    g.iterate()
    assert g.get_state("arx").any()
    with pytest.raises(_ffi.BboError):
        g.get_state("no_such_key")
    # no base of a restart driver
    p = _ffi.default_params(_ffi.ALGO_IPOP)
    p.mfev, p.np = 1000, 8
    out = C.c_void_p()
    fn = C.CDLL(_ffi.LIB_PATH).bbo_create_restart
    fn.argtypes, fn.restype = [C.c_void_p, C.c_void_p, C.c_void_p], C.c_int
    assert fn(C.byref(p), h, C.byref(out)) == _ffi.ERR_ARG and not out.value
    assert "CMA-ES handle" in L.bbo_last_error(None).decode()


@pytest.mark.parametrize("mode", ["gauss", "rademacher"])
def test_outcome_distribution_of_the_sphere_runs(hip, mode):
    """device generator, so not comparable draw by draw: over 32 seeds every run converges (every
    reference run did) and the median of fev lies inside the reference's [min, max] over its 16"""
    runs = GOLD["runs"]
    ref = runs[mode]
    assert all(r["converged"] for r in ref)
    n, lam = runs["n"], runs["lambda"]
    lo, up = -runs["box"] * np.ones(n), runs["box"] * np.ones(n)
    fev = []
    for seed in range(32):
        rng = np.random.default_rng(500 + seed)
        g = hip.LmCMAES(runs["mfev"], runs["tol"], lam, 0, runs["sigma0"], False, mode == "rademacher", True, seed=900 + seed)
        sol = g.optimize("sphere", lo, up, rng.uniform(-3., 3., n))
        assert sol.converged is True, seed
        fev.append(sol.n_evals)
    lo_ref, hi_ref = min(r["fev"] for r in ref), max(r["fev"] for r in ref)
    print("%s: device fev min %d median %.0f max %d; the reference [%d, %d]"
          % (mode, min(fev), np.median(fev), max(fev), lo_ref, hi_ref))
    assert lo_ref <= np.median(fev) <= hi_ref
