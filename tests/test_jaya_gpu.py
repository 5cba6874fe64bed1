"""GPU: the JAYA kernels against tests/jaya_model.py in its synchronous order.

The model is fed what the device recorded of a generation (`occ`, `len`, `draws`, `ftrial`) and
must then hold the same state BIT FOR BIT for the original, tent_map and logistic mutations: the
trial is the same IEEE operations in the same order, the chaotic chain is recomputed by the model
from `xchaos`.  Under levy the model's pow is the C library's and the device's is ocml's, so X is
compared at LEVY_RTOL (relative to the largest |x| of the pool).  The reference ties in through the
outcome bands of tests/golden/jaya_runs.json (criterion: tests/test_jaya_model.py::band, shown
there to hold for the model in this order and between halves of the reference itself)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import jaya_model as jm
from slpso_model import device_objective
from test_jaya_model import GOLD, band, _h

pytestmark = pytest.mark.gpu

# measured worst over the levy cases below: see DESIGN.md section 5; the margin is one decade
LEVY_MEASURED = 1.110e-16
LEVY_RTOL = 10. * LEVY_MEASURED


def _bits(a, b, what):
    a, b = np.asarray(a, float).ravel(), np.asarray(b, float).ravel()
    assert a.shape == b.shape, what
    assert a.tobytes() == b.tobytes(), (what, np.flatnonzero(a != b)[:8], a[a != b][:4], b[a != b][:4])


def _model_of(g, p, n, np_, npmin, lo, up, mut, k0, adapt, **kw):
    m = jm.Jaya(None, lo, up, np_, npmin, adapt=adapt, k0=k0, mutation=mut, order="sync", **kw)
    m.start(g.get_state("X", p), g.get_state("f", p), g.get_state("xchaos", p)[0])
    return m


def _step_model(g, m, p, levy_err=None):
    """one device generation has just run: replay it in the model and compare"""
    np_, n = m.np, m.n
    C_ = 5 if m.mutation == jm.LEVY else 2
    raw = g.get_state("draws", p)
    assert raw.size == np_ * n * C_ + 1
    d = raw[:-1].reshape(np_, n, C_)
    occ = g.get_state("occ", p).astype(int)
    lens = g.get_state("len", p).astype(int)
    assert lens[:m.k].sum() == np_ and lens[:m.k].min() >= np_ // m.k
    levy = (d[..., 0], d[..., 1], d[..., 2]) if m.mutation == jm.LEVY else None
    m.iterate_sync(occ, lens, d[..., C_ - 2], d[..., C_ - 1], levy=levy, uroul=raw[-1],
                   ftrial=g.get_state("ftrial", p))
    X = g.get_state("X", p).reshape(np_, n)
    if m.mutation == jm.LEVY:
        err = np.abs(X - m.X).max() / np.abs(m.X).max()
        levy_err.append(err)
        print("levy: relative deviation of X from the model %.3e" % err)
        assert err <= LEVY_RTOL, err
        m.X = X.copy()              # the next generation starts from the device's pool
        if m.fgbest == float(g.get_state("fgbest", p)[0]):
            m.bestx = g.get_state("bestx", p).copy()
    else:
        _bits(g.get_state("trial", p), m.trial, "trial")
        _bits(X, m.X, "X")
        _bits(g.get_state("bestx", p), m.bestx, "bestx")
        _bits(g.get_state("xchaos", p), [m.xchaos], "xchaos")
    _bits(g.get_state("f", p), m.f, "f")
    _bits(g.get_state("best", p), [m.best], "best")
    _bits(g.get_state("fgbest", p), [m.fgbest], "fgbest")
    assert int(g.get_state("k", p)[0]) == m.k and int(g.get_state("fev", p)[0]) == m.fev
    assert int(g.get_state("gen", p)[0]) == m.gen


# (mutation, n, np, npmin, k0, P, objective): n in {1, 3, 64, 65, 130}, np in {2, 7, 70},
# k in {1, 3, nks} with np % k != 0, P in {1, 3}
CASES = [
    ("original", 1, 2, 1, 1, 1, "sphere"),
    ("original", 3, 7, 2, 3, 3, "rosenbrock"),
    ("original", 130, 70, 5, 14, 1, "rastrigin"),
    ("logistic", 64, 70, 5, 3, 1, "rosenbrock"),
    ("logistic", 65, 7, 1, 7, 1, "ellipsoid"),
    ("tent_map", 130, 70, 10, 3, 3, "sphere"),
    ("tent_map", 3, 7, 2, 1, 1, "sphere"),
    ("levy", 65, 70, 5, 3, 1, "rosenbrock"),
    ("levy", 3, 7, 2, 3, 3, "sphere"),
    # rows past one pass of a 256-thread workgroup: one live lane in the second pass (257), in the
    # third (513), and the cap (1024: four full passes)
    ("original", 257, 7, 2, 3, 1, "rosenbrock"),
    ("logistic", 513, 7, 1, 7, 1, "ellipsoid"),
    ("tent_map", 1024, 8, 2, 3, 1, "rosenbrock"),
    ("original", 1024, 7, 2, 3, 3, "ellipsoid"),
]


@pytest.mark.parametrize("mut,n,np_,npmin,k0,P,obj", CASES,
                         ids=["%s-n%d-np%d-k%d-P%d" % (c[0], c[1], c[2], c[4], c[5]) for c in CASES])
def test_three_generations_against_the_synchronous_model(hip, mut, n, np_, npmin, k0, P, obj):
    lo, up = -3. * np.ones(n), 4. * np.ones(n)
    g = hip.JAYA(10 ** 7, 0., np_, npmin, k0=k0, mutation=jm.MUTATIONS[mut], seed=31 + n, populations=P)
    g.initialize(getattr(hip.objectives, obj), lo, up, np.zeros((P, n)))
    g.set_state("record_draws", [1.])
    models = [_model_of(g, p, n, np_, npmin, lo, up, jm.MUTATIONS[mut], k0, True) for p in range(P)]
    for p, m in enumerate(models):
        _bits(g.get_state("fgbest", p), [m.fgbest], "init fgbest")
        _bits(g.get_state("bestx", p), m.bestx, "init bestx")
        assert int(g.get_state("fev", p)[0]) == np_ and int(g.get_state("nks", p)[0]) == m.nks
        assert ((g.get_state("X", p).reshape(np_, n) >= lo) & (g.get_state("X", p).reshape(np_, n) <= up)).all()
    errs = []
    # past one pass of a row loop the trial's value is held too: the sum in the device's order
    # (eval_row_group<64>, slpso_model.device_objective), bit for bit
    fdev = device_objective(obj, n) if n > 256 else None
    for _ in range(3):
        g.iterate()
        for p, m in enumerate(models):
            _step_model(g, m, p, errs)
            if fdev is not None:
                T = g.get_state("trial", p).reshape(np_, n)
                _bits(g.get_state("ftrial", p), [fdev(t) for t in T], "ftrial")
    if errs:
        print("levy: worst relative deviation of X from the model %.3e" % max(errs))
    if P > 1:       # the populations are independent streams
        assert not np.array_equal(g.get_state("X", 0), g.get_state("X", 1))


def _percoord_pool(n, np_, rng):
    """rows under tests/_boxes.py's box from which the clamp binds on both sides and leaves a third of the
    coordinates alone: the trial is x + r1 (best - |x|) - r2 (worst - |x|), so the coordinates that are
    negative throughout (class 1) move by up to twice their size and meet both bounds, those packed next to
    their lower bound (class 0) meet it, and those packed in [0.9, 1.1], well inside (class 2), stay inside"""
    from _boxes import percoord_box
    lo, up = percoord_box(n)
    j, U = np.arange(n), rng.random((np_, n))
    return lo, up, np.where(j % 3 == 0, lo + 0.3 * U, np.where(j % 3 == 1, lo + (up - lo) * U, 0.9 + 0.2 * U))


def _percoord_handle(hip, n, np_, npmin, k0, P, seed, lo, up, pools, f):
    g = hip.JAYA(10 ** 7, 0., np_, npmin, k0=k0, mutation=jm.MUTATIONS["original"], seed=seed, populations=P)
    g.initialize(hip.objectives.sphere, lo, up, np.zeros((P, n)))
    for p in range(P):
        X = g.get_state("X", p).reshape(np_, n)
        assert ((X >= lo) & (X <= up)).all()        # the initial draw, coordinate by coordinate
        assert ((X.max(0) - X.min(0)) > 0.25 * (up - lo)).sum() >= n // 2
        g.set_state("X", pools[p], p)
        g.set_state("f", [f(x) for x in pools[p]], p)
    g.set_state("record_draws", [1.])
    return g


def _percoord_model(g, p, n, np_, npmin, k0, lo, up, f=None):
    m = jm.Jaya(f, lo, up, np_, npmin, adapt=True, k0=k0, mutation=jm.ORIGINAL, order="sync")
    m.start(g.get_state("X", p), g.get_state("f", p), g.get_state("xchaos", p)[0])
    # (the incumbent is the best point ever evaluated, the drawn pool's included)
    m.fgbest, m.bestx = float(g.get_state("fgbest", p)[0]), g.get_state("bestx", p).copy()
    m.best = m.pbest = float(g.get_state("best", p)[0])
    return m


@pytest.mark.parametrize("n,np_,npmin,k0,P", [(37, 7, 2, 3, 2), (513, 7, 2, 3, 1)])
def test_the_clamp_of_the_trial_under_bounds_that_differ_in_every_coordinate(hip, n, np_, npmin, k0, P):
    """tests/_boxes.py's box: the initial draw and the clamp of every trial (jaya_trials) read another pair of
    bounds in every coordinate.  The witness is established before anything is compared: a first handle only
    hands over its starting state and what its generator drew (the shuffle and the uniforms), and the model runs
    alone on them with its own objective; over its trials at least three coordinates sit on their lower bound,
    three on their upper bound and three stay strictly inside in every row.  Then a second handle of the same
    seed walks beside a second model as in test_three_generations_against_the_synchronous_model.  n = 37 is
    off every tile, 513 puts one live lane into the third pass."""
    from _boxes import binding_witness
    seed = 31 + n
    rng = np.random.default_rng(seed)
    f = device_objective("sphere", n)
    pools = []
    for _ in range(P):
        lo, up, X = _percoord_pool(n, np_, rng)
        pools.append(X)
    # ---- the witness: the model alone on the generator's draws
    a = _percoord_handle(hip, n, np_, npmin, k0, P, seed, lo, up, pools, f)
    alone = [_percoord_model(a, p, n, np_, npmin, k0, lo, up, f) for p in range(P)]
    trials = [[] for _ in range(P)]
    for _ in range(3):
        a.iterate()
        for p, w in enumerate(alone):
            raw = a.get_state("draws", p)
            d = raw[:-1].reshape(np_, n, 2)
            w.iterate_sync(a.get_state("occ", p).astype(int), a.get_state("len", p).astype(int), d[..., 0],
                           d[..., 1], uroul=raw[-1])
            trials[p].append(np.array(w.trial))
    for p in range(P):
        binding_witness(trials[p], lo, up)
    # ---- the walk
    g = _percoord_handle(hip, n, np_, npmin, k0, P, seed, lo, up, pools, f)
    models = [_percoord_model(g, p, n, np_, npmin, k0, lo, up) for p in range(P)]
    for gen in range(3):
        g.iterate()
        for p, m in enumerate(models):
            _step_model(g, m, p)
            T = g.get_state("trial", p).reshape(np_, n)
            assert ((T >= lo) & (T <= up)).all()
            if n > 256:     # (as there: past one pass the trial's value is the sum in the device's order)
                _bits(g.get_state("ftrial", p), [f(t) for t in T], "ftrial")


def test_bounded_pool_at_a_corner_and_a_nan_objective(hip):
    """a crafted pool next to the upper corner (the trials are clamped to the box) and a callback
    that returns NaN for part of the trials (they rank last: +inf, never accepted)"""
    n, np_, npmin = 5, 7, 2
    lo, up = -1. * np.ones(n), 2. * np.ones(n)
    calls = []

    def f(x):
        calls.append(1)
        return float("nan") if x[0] > 1.99 else float(np.sum(x * x))

    g = hip.JAYA(10 ** 6, 0., np_, npmin, k0=3, mutation=hip.JAYA.original, seed=3)
    g.initialize(f, lo, up, np.zeros(n))
    assert len(calls) == np_
    rng = np.random.default_rng(1)
    X = up - 0.02 * rng.random((np_, n))
    g.set_state("X", X)
    g.set_state("f", [float(np.sum(x * x)) for x in X])
    g.set_state("record_draws", [1.])
    m = _model_of(g, 0, n, np_, npmin, lo, up, jm.ORIGINAL, 3, True)
    m.fgbest, m.bestx = float(g.get_state("fgbest")[0]), g.get_state("bestx").copy()
    m.best = m.pbest = float(g.get_state("best")[0])
    clamped = nan = 0
    for _ in range(3):
        g.iterate()
        _step_model(g, m, 0)
        T, ft = g.get_state("trial").reshape(np_, n), g.get_state("ftrial")
        assert (T >= lo).all() and (T <= up).all()
        clamped += int((T == up).sum())
        nan += int(np.isinf(ft).sum())
    assert clamped > 0 and nan > 0 and len(calls) == 4 * np_
    assert np.isfinite(g.get_state("f")).all()


@pytest.mark.parametrize("name", ["sphere", "rosenbrock", "rastrigin", "ellipsoid", "ackley",
                                  "griewank", "cigar", "discus", "diffpow", "schwefel12"])
def test_trial_fitness_is_the_objective_of_the_trial(hip, name):
    n, np_ = 65, 7
    obj = getattr(hip.objectives, name)
    lo, up = -2. * np.ones(n), 3. * np.ones(n)
    g = hip.JAYA(10 ** 6, 0., np_, 2, k0=2, seed=17)
    g.initialize(obj, lo, up, np.zeros(n))
    g.set_state("record_draws", [1.])
    g.iterate()
    T, ft = g.get_state("trial").reshape(np_, n), g.get_state("ftrial")
    want = np.array([obj(t) for t in T])
    assert np.all(np.abs(ft - want) <= 1e-12 * np.abs(want)), (ft, want)


def _state(g, p=0):
    return {k: g.get_state(k, p).copy() for k in ("X", "f", "occ", "k", "pstrat", "perfindex", "xchaos",
                                                  "best", "fgbest", "bestx", "fev", "gen", "stop")}


def _device_sphere3(x):
    """the built-in sphere at n = 3 in the device's order: one term per lane, then the butterfly"""
    return float((x[0] * x[0] + x[2] * x[2]) + x[1] * x[1])


def test_same_seed_same_run_and_callback_path_equals_builtin(hip):
    n, np_ = 3, 70
    lo, up = -5. * np.ones(n), 5. * np.ones(n)
    runs = []
    for f in (hip.objectives.sphere, hip.objectives.sphere, _device_sphere3):
        g = hip.JAYA(10 ** 6, 0., np_, 5, seed=77)
        g.initialize(f, lo, up, np.zeros(n))
        for _ in range(4):
            g.iterate()
        runs.append(_state(g))
    for other in runs[1:]:
        for k, v in runs[0].items():
            _bits(v, other[k], k)
    g = hip.JAYA(10 ** 6, 0., np_, 5, seed=78)
    g.initialize(hip.objectives.sphere, lo, up, np.zeros(n))
    for _ in range(4):
        g.iterate()
    assert not np.array_equal(g.get_state("X"), runs[0]["X"])       # another seed, another run


def test_a_frozen_population_keeps_its_state(hip):
    n, np_, P = 4, 7, 3
    lo, up = -5. * np.ones(n), 5. * np.ones(n)
    g = hip.JAYA(10 ** 6, 1e-3, np_, 2, seed=5, populations=P, poll_every=1)
    g.initialize(hip.objectives.sphere, lo, up, np.zeros((P, n)))
    g.set_state("X", np.tile([1., 2., 0.5, 3.], (np_, 1)), population=1)     # a collapsed pool
    assert g.run(1) == 1
    assert [int(g.get_state("stop", p)[0]) for p in range(P)] == [0, 1, 0]
    before = _state(g, 1)
    assert g.run(3) == 3
    after = _state(g, 1)
    for k, v in before.items():
        _bits(v, after[k], k)
    assert int(g.get_state("fev", 0)[0]) == np_ * 5 and int(g.get_state("fev", 1)[0]) == np_ * 2
    assert g.solution(1).converged and not g.solution(0).converged


def test_stop_rules(hip):
    n, np_ = 4, 7
    lo, up = -5. * np.ones(n), 5. * np.ones(n)
    # the budget: whole generations, so fev overshoots mfev like the reference's loop
    g = hip.JAYA(100, 0., np_, 2, seed=6)
    g.initialize(hip.objectives.rosenbrock, lo, up, np.zeros(n))
    g.run(10 ** 6)
    assert int(g.get_state("stop")[0]) == 2 and int(g.get_state("fev")[0]) == 105
    assert g.run(5) == 0
    # the spread of the radii, on a crafted collapsed pool
    g = hip.JAYA(10 ** 6, 1e-6, np_, 2, seed=6)
    g.initialize(hip.objectives.rosenbrock, lo, up, np.zeros(n))
    g.iterate()
    assert int(g.get_state("stop")[0]) == 0
    g.set_state("X", np.tile([1., 1.5, 2., 2.5], (np_, 1)))
    g.iterate()
    assert int(g.get_state("stop")[0]) == 1 and g.solution().converged
    # the budget is looked at before the spread (jaya.cpp:184-196)
    g = hip.JAYA(14, 1e-6, np_, 2, seed=6)
    g.initialize(hip.objectives.rosenbrock, lo, up, np.zeros(n))
    g.set_state("X", np.tile([1., 1.5, 2., 2.5], (np_, 1)))
    g.iterate()
    assert int(g.get_state("stop")[0]) == 2 and int(g.get_state("conv")[0]) == 1


def test_configure_statuses_and_parameter_checks(hip):
    from bboptpy_amd import _ffi
    L = _ffi.lib()
    j = _ffi.JayaParams()
    L.bbo_jaya_params_default(C.byref(j))
    other = hip.CSO(1000, 1e-6, 12, seed=1)
    assert L.bbo_jaya_configure(other._ensure_handle(), C.byref(j)) == _ffi.ERR_ARG
    g = hip.JAYA(1000, 1e-6, 12, 3, seed=1)         # nks = 4
    h = g._ensure_handle()
    assert L.bbo_jaya_configure(h, C.byref(j)) == 0
    assert L.bbo_jaya_configure(h, None) == _ffi.ERR_ARG
    for field, bad in (("k0", 0), ("k0", 5), ("beta", 0.), ("beta", 2.5), ("mutation", 4)):
        b = _ffi.JayaParams()
        L.bbo_jaya_params_default(C.byref(b))
        setattr(b, field, bad)
        assert L.bbo_jaya_configure(h, C.byref(b)) == _ffi.ERR_ARG, (field, bad)
    g.initialize(hip.objectives.sphere, -np.ones(2), np.ones(2), np.zeros(2))
    assert L.bbo_jaya_configure(h, C.byref(j)) == -2          # BBO_ERR_STATE
    for np_, npmin in ((1, 1), (4, 0), (4, 5)):
        with pytest.raises(_ffi.BboError) as e:
            hip.JAYA(1000, 1e-6, np_, npmin)._ensure_handle()
        assert e.value.status == _ffi.ERR_ARG
    with pytest.raises(_ffi.BboError):                        # the default k0 = 2 with nks = 1
        hip.JAYA(1000, 1e-6, 7, 5)._ensure_handle()


def test_optimize_converges_on_the_sphere(hip):
    n = 10
    g = hip.JAYA(400000, 1e-5, 40, 5, seed=12)
    sol = g.optimize(hip.objectives.sphere, -5. * np.ones(n), 5. * np.ones(n), np.zeros(n))
    print("optimize: fev %d f %.3e" % (sol.n_evals, hip.objectives.sphere(sol.x)))
    assert sol.converged and hip.objectives.sphere(sol.x) < 1e-6 and sol.n_evals < 400000


@pytest.mark.parametrize("obj", ["sphere", "rosenbrock"])
def test_outcome_bands_match_the_reference(hip, obj):
    b, P = GOLD["bands"], 64
    n = b["n"]
    g = hip.JAYA(b["mfev"], b["tol"], b["np"], b["npmin"], seed=2024, populations=P)
    g.initialize(getattr(hip.objectives, obj), -b["box"] * np.ones(n), b["box"] * np.ones(n), np.zeros((P, n)))
    g.run(10 ** 6)
    got = [float(g.get_state("fgbest", p)[0]) for p in range(P)]
    assert all(int(g.get_state("fev", p)[0]) == 4000 for p in range(P))
    print("device %s: quartiles of log10 f" % obj, np.percentile(np.log10(got), [25, 50, 75]))
    band(got, _h(b[obj]), obj + " device")


def test_a_row_matrix_round_trips_at_odd_n_in_the_second_population(hip):
    """n = 3 (ld = 4), six rows, population 1: set_state -> get_state bit-equal, no padding column"""
    n, np_, P = 3, 6, 2
    g = hip.JAYA(10 ** 6, 0., np_, 2, seed=4, populations=P)
    g.initialize(hip.objectives.sphere, -2. * np.ones(n), 2. * np.ones(n), np.zeros((P, n)))
    X = np.random.default_rng(9).uniform(-1., 1., (np_, n))
    g.set_state("X", X, population=1)
    got = g.get_state("X", 1)
    assert got.size == np_ * n and got.tobytes() == X.tobytes()
