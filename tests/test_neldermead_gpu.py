"""GPU: the NelderMead engine against tests/neldermead_model.py, and its behaviour at the C ABI.

With a Python callable that computes the model's own formula every value is the model's, so a whole optimize()
-- the steps, the stop test, the factorial test, the restarts, the budget exit -- must be the model's bit for
bit, and the callable must have seen the reference's points in its order, each once.  The model is held to the
reference by tests/test_neldermead_model.py.  With the built-in objective: tests/test_neldermead_golden_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import chol_model
import neldermead_model as nm
from slpso_model import device_objective
from test_neldermead_golden_gpu import _bits, device_of, inject
from test_neldermead_model import GOLDEN, guess_of, model_of

pytestmark = pytest.mark.gpu

KEYS = ("p", "y", "ilo", "ylo", "jcount", "fev", "conv", "branch", "it", "flag", "restarts", "stage", "pending")


class Logged:
    """a callable that keeps the points it was handed"""

    def __init__(self, f):
        self.f, self.seen = f, []

    def __call__(self, x):
        self.seen.append([float(v) for v in x])
        return self.f(x)


def _whole_run(hip, rec, f=None, **kw):
    n = rec["n"]
    f = f or chol_model.objective(rec["objective"], n)
    m = model_of(rec, repair=kw.get("repair", False))
    m.f = f
    x, icount, conv = m.optimize(guess_of(rec))
    log = Logged(f)
    g, _, lo, up = device_of(hip, rec, **kw)
    sol = g.optimize(log, lo, up, guess_of(rec))
    tag = rec["name"] + ": "
    assert len(log.seen) == len(m.evals) == sol.n_evals == icount, tag + "the callable is called once per counted evaluation"
    _bits(log.seen, [e[0] for e in m.evals], tag + "the points the callable saw, in order")
    _bits(sol.x, x, tag + "x")
    assert sol.converged == conv, tag
    assert int(g.get_state("restarts")[0]) == m.restarts and int(g.get_state("it")[0]) == m.it, tag
    assert int(g.get_state("flag")[0]) == (1 if conv else 2), tag
    _bits(g.get_state("xmin"), x, tag + "xmin")
    _bits(g.get_state("p"), m.p, tag + "the last simplex")
    _bits(g.get_state("y"), m.y, tag + "its values")
    return m, g


@pytest.mark.parametrize("rec", GOLDEN["runs"], ids=lambda r: r["name"])
def test_whole_optimize_is_the_model_bit_for_bit(hip, rec):
    m, g = _whole_run(hip, rec)
    assert [list(e) for e in m.events] == rec["events"] and m.icount == rec["icount"]      # (the reference's run)


@pytest.mark.parametrize("name", ["run_n2_loose", "run_n3_loose", "run_n2_wide", "run_n65_budget"])
def test_the_built_in_run_crosses_restarts_on_the_device_as_the_callable_run_does(hip, name):
    """optimize() with the built-in: the stop test, the factorial test (all 2 n probes evaluated at once, counted
    up to the first that improved), the restarts and the budget exit inside the launches; against the same run
    driven from the host with a callable that sums as the device does"""
    rec = next(r for r in GOLDEN["runs"] if r["name"] == name)
    log = Logged(device_objective(rec["objective"], rec["n"]))
    a, _, lo, up = device_of(hip, rec)
    b, _, _, _ = device_of(hip, rec, f=log)
    sa = a.optimize(getattr(hip.objectives, rec["objective"]), lo, up, guess_of(rec))
    sb = b.optimize(log, lo, up, guess_of(rec))
    _bits(sa.x, sb.x, name + ": x")
    assert (sa.n_evals, sa.converged) == (sb.n_evals, sb.converged) and len(log.seen) == sb.n_evals
    for k in ("p", "y", "xmin", "start", "fev", "it", "restarts", "flag", "del", "ilo", "jcount"):
        _bits(a.get_state(k), b.get_state(k), name + ": " + k)
    if name.endswith("_loose"):
        assert int(a.get_state("restarts")[0]) >= 1


def test_a_run_that_ends_on_the_budget(hip):
    rec = next(r for r in GOLDEN["runs"] if r["events"][-1] == ["budget"] and r["n"] == 65)
    m, g = _whole_run(hip, rec, lds=False)
    assert m.icount > rec["params"]["mfev"] and int(g.get_state("flag")[0]) == 2


@pytest.mark.parametrize("repair", [False, True])
def test_the_refused_outside_contraction_literal_and_repaired(hip, repair):
    rec = next(r for r in GOLDEN["runs"] if r["paths"]["outside_refused"])
    m, g = _whole_run(hip, rec, repair=repair)
    assert m.paths["outside_refused"] >= 1


def test_a_nan_from_the_callable_counts_as_inf(hip):
    rec = next(r for r in GOLDEN["runs"] if r["name"] == "run_n3_sphere")
    base = chol_model.objective("sphere", 3)
    calls = [0]

    def f(x):       # a pure function of the point: NaN in a shell the run crosses
        v = base(x)
        return float("nan") if 0.5 < v < 0.9 else v

    m, g = _whole_run(hip, rec, f=f)
    assert any(v == nm.INF for _, v in m.evals), "the run never met the shell: choose another"
    assert not np.isnan(g.get_state("y")).any()


def test_a_nan_from_the_built_in_counts_as_inf(hip):
    cls = hip.NelderMead
    g = cls(1000, 1e-8, 1., cls.coordinate_axis, cls.original, seed=1)
    g.initialize(hip.objectives.rosenbrock, -5. * np.ones(3), 5. * np.ones(3), [np.inf, np.inf, 1.])    # inf - inf
    assert (g.get_state("y") == np.inf).all() and int(g.get_state("fev")[0]) == 4
    g.iterate()
    assert not np.isnan(g.get_state("y")).any() and int(g.get_state("branch")[0]) in range(1, 8)


def _snap(g, P):
    return [{k: g.get_state(k, p).copy() for k in KEYS} for p in range(P)]


def _same(a, b, tag):
    for p, (sa, sb) in enumerate(zip(a, b)):
        for k in KEYS:
            _bits(sa[k], sb[k], "%s population %d %s" % (tag, p, k))


@pytest.mark.parametrize("n,lds", [(3, True), (17, False), (65, True), (128, True)])
def test_phase_walk_and_callable_are_the_iterate_run(hip, n, lds):
    """three populations that need different numbers of evaluations per step; 12 steps: iterate() with the
    built-in, the same through phase(), the same with a callable that sums as the device does"""
    P, steps, cls = 3, 12, hip.NelderMead
    rng = np.random.default_rng(n)
    guess = rng.uniform(-3., 3., (P, n))
    guess[1] *= 0.01        # near the minimum of the sphere part: contractions, where the others expand
    lo, up = -5. * np.ones(n), 5. * np.ones(n)

    def make(f):
        g = cls(1 << 20, 1e-300, 2., cls.coordinate_axis, cls.gao2010, 3, populations=P, lds=lds, seed=2)
        g.initialize(f, lo, up, guess.ravel())
        return g

    a, b = make(hip.objectives.rosenbrock), make(hip.objectives.rosenbrock)
    log = Logged(device_objective("rosenbrock", n))
    c = make(log)
    assert len(log.seen) == P * (n + 1)
    _same(_snap(a, P), _snap(b, P), "initialize")
    _same(_snap(a, P), _snap(c, P), "initialize, callable")
    counts = set()
    for k in range(steps):
        before = [int(a.get_state("fev", p)[0]) for p in range(P)]
        a.iterate()
        seen0 = len(log.seen)
        c.iterate()
        # the walk protocol: advance, then evaluate and absorb while a batch is pending
        pending = b.phase(0)
        assert pending == P and all(int(b.get_state("stage", p)[0]) == 1 for p in range(P))
        rounds = 0
        while pending:
            want = [int(b.get_state("pending", p)[0]) for p in range(P)]
            assert b.phase(1) is None
            for p in range(P):
                if want[p]:
                    vals = b.get_state("value", p)[:want[p]]
                    assert np.isfinite(vals).all()
            pending = b.phase(2)
            rounds += 1
        assert 1 <= rounds <= 3 and b.phase(2) == 0         # nothing pending: absorb is a no-op
        sa = _snap(a, P)
        _same(sa, _snap(b, P), "step %d, phase walk" % k)
        _same(sa, _snap(c, P), "step %d, callable" % k)
        spent = [int(sa[p]["fev"][0]) - before[p] for p in range(P)]
        assert all(s in (1, 2, n + 3) for s in spent) and len(log.seen) - seen0 == sum(spent)
        counts.add(tuple(spent))
        assert all(int(s["it"][0]) == k + 1 and int(s["pending"][0]) == 0 and int(s["stage"][0]) == 0 for s in sa)
    assert any(len(set(t)) > 1 for t in counts), "the populations never differed in their evaluations: %s" % counts
    # run() is the same walk: 5 more steps in one call equal 5 iterate() calls while no stop test fires
    assert a.run(5) == 5
    for _ in range(5):
        b.iterate()
    sa, sb = _snap(a, P), _snap(b, P)
    for p in range(P):
        for k in ("p", "y", "fev", "it", "ilo"):
            _bits(sa[p][k], sb[p][k], "run against iterate, population %d %s" % (p, k))
    with pytest.raises(hip._ffi.BboError):
        b.phase(3)


def test_shrink_from_a_crafted_state(hip):
    """y set so that the reflection and the inside contraction both lose: the shrink, its n + 1 evaluations as
    one batch, and the return before the stop test's bookkeeping"""
    n, cls = 5, hip.NelderMead
    rec = dict(n=n, objective="rosenbrock", minit="spendley", pinit="mehta2019_refined",
               params=dict(mfev=1 << 20, tol=1e-8, rad0=1., checkev=10, eps=1e-3))
    f = chol_model.objective("rosenbrock", n)
    guess = [0.3, -0.2, 0.5, 0.1, -0.4]
    for ilo in (0, 2, n):
        m = model_of(rec)
        m.init(guess)
        m.first_simplex()
        log = Logged(f)
        g, _, lo, up = device_of(hip, rec, f=log)
        g.initialize(log, lo, up, guess)
        y = [-1e6 + j for j in range(n + 1)]        # far below anything the objective returns
        y[ilo] = -2e6
        m.y, m.ilo, m.ylo, m.jcount = list(y), ilo, y[ilo], 1
        inject(g, m)
        log.seen, m.evals = [], []
        m.iterate()
        g.iterate()
        assert m.branch == nm.SHRINK and int(g.get_state("branch")[0]) == nm.SHRINK
        _bits(log.seen, [e[0] for e in m.evals], "ilo %d: the points of the shrink step" % ilo)
        assert len(log.seen) == n + 3
        _bits(g.get_state("p"), m.p, "the shrunk simplex")
        _bits(g.get_state("y"), m.y, "its values")
        got = [int(g.get_state(q)[0]) for q in ("ilo", "fev", "jcount", "conv")]
        assert got == [m.ilo, m.icount, 1, 0]       # jcount untouched: the shrink returns before :207


def test_speculate_is_refused(hip):
    """the speculative step was measured slower everywhere and dropped"""
    from bboptpy_amd import _ffi
    with pytest.raises(ValueError, match="speculative step was measured and dropped"):
        hip.NelderMead(100, 0., 1., speculate=True)
    L = _ffi.lib()
    p = _ffi.default_params(_ffi.ALGO_NELDER_MEAD)
    p.mfev, p.sigma0 = 100, 1.
    h = C.c_void_p()
    _ffi.check(L.bbo_create(C.byref(p), C.byref(h)))
    try:
        s = _ffi.NmParams()
        L.bbo_nm_params_default(C.byref(s))
        s.speculate = 1
        assert L.bbo_nm_configure(h, C.byref(s)) == _ffi.ERR_ARG
        assert b"measured and dropped" in L.bbo_last_error(h)
        s.speculate, s.checkev = 0, 0
        assert L.bbo_nm_configure(h, C.byref(s)) == _ffi.ERR_ARG
        s.checkev = 3
        assert L.bbo_nm_configure(h, C.byref(s)) == 0
    finally:
        L.bbo_destroy(h)


def test_the_library_refuses_what_the_class_refuses(hip):
    from bboptpy_amd import _ffi
    cls = hip.NelderMead
    g = cls(100, 0., 1., minit=cls.random, seed=1)
    g._problem = lambda f, lo, up, x: hip.MultivariateSearch._problem(g, f, lo, up, x)     # past the class's checks
    with pytest.raises(_ffi.BboError, match="bounds must be finite"):
        g.initialize(hip.objectives.sphere, -np.ones(3), np.array([1., np.inf, 1.]), np.zeros(3))
    g = cls(100, 0., 1., seed=1)
    g._problem = lambda f, lo, up, x: hip.MultivariateSearch._problem(g, f, lo, up, x)
    with pytest.raises(_ffi.BboError, match=r"dimension must be in \[1, 128\]"):
        g.initialize(hip.objectives.sphere, -np.ones(129), np.ones(129), np.zeros(129))
    p = _ffi.default_params(_ffi.ALGO_NELDER_MEAD)
    p.mfev, p.sigma0 = 100, float("inf")
    h = C.c_void_p()
    assert _ffi.lib().bbo_create(C.byref(p), C.byref(h)) == _ffi.ERR_ARG


def test_random_simplex_stays_in_the_box_and_follows_the_seed(hip):
    n, cls = 17, hip.NelderMead
    lo, up = np.linspace(-4., -1., n), np.linspace(0.5, 3., n)
    guess = np.zeros(n)

    def first(seed, **kw):
        g = cls(1000, 1e-8, 1., cls.random, seed=seed, **kw)
        g.initialize(hip.objectives.sphere, lo, up, guess)
        return g.get_state("p").reshape(n + 1, n)

    a, b, c = first(11), first(11), first(12)
    _bits(a, b, "the same seed")
    assert (a[:n] >= lo).all() and (a[:n] < up).all() and (a[n] == guess).all()
    assert (a[:n] != c[:n]).all() and len(np.unique(a[:n])) == n * n
    g = cls(1000, 1e-8, 1., cls.random, seed=11, populations=2)
    g.initialize(hip.objectives.sphere, lo, up, np.zeros(2 * n))
    _bits(g.get_state("p", 1), first(11, substream=1), "population 1 draws sub-stream 1")
    _bits(g.get_state("p", 0), a, "population 0 draws sub-stream 0")


def test_results_do_not_depend_on_the_population_index(hip):
    n, P, cls = 9, 70, hip.NelderMead
    lo, up = -5. * np.ones(n), 5. * np.ones(n)
    rng = np.random.default_rng(4)
    kinds = rng.uniform(-3., 3., (3, n))
    guess = np.stack([kinds[p % 3] for p in range(P)])
    g = cls(600, 1e-6, 1., populations=P, seed=3)
    g.initialize(hip.objectives.rosenbrock, lo, up, guess.ravel())
    g.run(1 << 20)
    for p in range(3, P):
        for k in ("p", "y", "fev", "it", "flag", "restarts", "xmin"):
            _bits(g.get_state(k, p), g.get_state(k, p % 3), "population %d against %d: %s" % (p, p % 3, k))
        a, b = g.solution(p), g.solution(p % 3)
        _bits(a.x, b.x, "solution")
        assert (a.n_evals, a.converged) == (b.n_evals, b.converged)
    assert all(int(g.get_state("flag", p)[0]) in (1, 2) for p in range(P))
    # and a population of the batch is the single run from its row of guess
    s = cls(600, 1e-6, 1., seed=3)
    sol = s.optimize(hip.objectives.rosenbrock, lo, up, guess[1])
    _bits(sol.x, g.get_state("xmin", 1), "the single run")
    assert sol.n_evals == int(g.get_state("fev", 1)[0])


def test_ccpso_takes_neldermead_as_its_local_optimizer(hip):
    n = 12
    calls = [0]

    def f(x):
        calls[0] += 1
        return float(np.sum(x * x) + 0.5 * np.sum(x[:-1] * x[1:]))

    loc = hip.NelderMead(200, 1e-10, 0.05, seed=1)
    g = hip.CCPSO(mfev=10 ** 8, sigmatol=1e-12, np=6, pps=[3], local=loc, localfreq=2, seed=31)
    assert not g._local_native
    g.initialize(f, -5. * np.ones(n), 5. * np.ones(n), np.zeros(n))
    before = float(g.get_state("fyhat")[0])
    for _ in range(6):
        g.iterate()
    assert g._nlocal == 3
    assert int(g.get_state("fev")[0]) == calls[0]       # every evaluation of the local searches is counted
    assert float(g.get_state("fyhat")[0]) <= before


def test_the_cap_launches_two_handles_of_two_populations(hip):
    """n = 128: 129 KiB of simplex per workgroup in LDS"""
    n, cls = 128, hip.NelderMead
    lo, up = -5. * np.ones(n), 5. * np.ones(n)
    guess = np.random.default_rng(8).uniform(-2., 2., (2, n))
    hs = []
    for _ in range(2):
        g = cls(1 << 20, 1e-12, 1., populations=2, seed=1)
        g.initialize(hip.objectives.rosenbrock, lo, up, guess.ravel())
        hs.append(g)
    for g in hs:
        assert int(g.get_state("lds")[0]) == 1
        assert g.run(40) == 40
    hbm = cls(1 << 20, 1e-12, 1., populations=2, lds=False, seed=1)
    hbm.initialize(hip.objectives.rosenbrock, lo, up, guess.ravel())
    assert hbm.run(40) == 40
    for p in range(2):
        for k in ("p", "y", "fev", "it"):
            _bits(hs[0].get_state(k, p), hs[1].get_state(k, p), "two handles, %s" % k)
            _bits(hs[0].get_state(k, p), hbm.get_state(k, p), "LDS against HBM, %s" % k)
        assert int(hs[0].get_state("it", p)[0]) == 40 and hs[0].get_state("y", p).min() < 1e5
