"""GPU: the Rosenbrock engine against tests/rosenbrock_model.py, and its behaviour at the C ABI.

With a Python callable that computes the model's own formula every value is the model's, so a whole optimize() --
the searches, the extra search of a stage, the orthogonalisations, the shrinking step, both ends -- must be the
model's bit for bit, and the callable must have seen the reference's points in its order, each as often as the
reference evaluates it.  The model is held to the reference by tests/test_rosenbrock_model.py.  With the built-in
objective: tests/test_rosenbrock_golden_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import rosenbrock_model as rm
from slpso_model import device_objective
from test_rosenbrock_golden_gpu import _bits, device_of, inject
from test_rosenbrock_model import GOLDEN, flat_evals, guess_of, model_of

pytestmark = pytest.mark.gpu

KEYS = ("x", "v", "d", "stepi", "i", "fev", "x1", "flag", "path", "fs", "it", "orths", "stage", "pending")


class Logged:
    """a callable that keeps the points it was handed"""

    def __init__(self, f):
        self.f, self.seen = f, []

    def __call__(self, x):
        self.seen.append([float(v) for v in x])
        return self.f(self.seen[-1])


def _run(name):
    return next(r for r in GOLDEN["runs"] if r["name"] == name)


def _whole_run(hip, rec, f=None, **kw):
    f = f or rm.objective(rec["objective"], rec["n"])
    m = model_of(rec, repair=kw.get("repair", False))
    m.f = f
    x, fev, conv = m.optimize(guess_of(rec))
    log = Logged(f)
    g, _, lo, up = device_of(hip, rec, **kw)
    sol = g.optimize(log, lo, up, guess_of(rec))
    tag = rec["name"] + ": "
    assert len(log.seen) == len(m.evals) == sol.n_evals == fev, tag + "the callable is called once per counted evaluation"
    _bits(log.seen, [e[0] for e in m.evals], tag + "the points the callable saw, in order")
    _bits(sol.x, x, tag + "x")
    assert sol.converged == conv, tag
    assert int(g.get_state("it")[0]) == m.searches and int(g.get_state("orths")[0]) == m.orths, tag
    assert int(g.get_state("flag")[0]) == (1 if conv else 2), tag
    _bits(g.get_state("x"), m.x, tag + "the rows")
    _bits(g.get_state("v"), m.v, tag + "the directions")
    _bits(g.get_state("d"), m.d, tag + "d")
    _bits(g.get_state("x1"), m.x1, tag + "x1")
    s = g.solution()
    _bits(s.x, x, tag + "solution()")
    assert (s.n_evals, s.converged) == (fev, conv)
    return m, g


@pytest.mark.parametrize("rec", GOLDEN["runs"], ids=lambda r: r["name"])
def test_whole_optimize_is_the_model_bit_for_bit(hip, rec):
    m, g = _whole_run(hip, rec)
    # (the reference's run)
    assert (rm.crc(flat_evals(m)), m.fev, [v.hex() for v in m.solution()[0]]) == (rec["evals_crc"], rec["fev"], rec["x"])


def test_the_budget_exit_returns_the_zero_vector_and_repair_the_last_end_point(hip):
    rec = _run("run_n128_budget")
    m, g = _whole_run(hip, rec, repair=True)
    x = np.array(m.solution()[0])
    assert m.ierr == 1 and np.any(x != 0.) and m.f(list(x)) < m.f(guess_of(rec))
    _bits(g.get_state("x1"), np.zeros(rec["n"]), "x1 stays zero")
    literal = hip.Rosenbrock(3000, 1e-8, 1., seed=1)
    sol = literal.optimize(hip.objectives.rosenbrock, -5. * np.ones(128), 5. * np.ones(128), guess_of(rec))
    assert not sol.converged and (sol.x == 0.).all() and sol.n_evals > 3000


@pytest.mark.parametrize("name", ["run_n2_rosen", "run_n65_sphere", "run_n128_budget"])
def test_the_built_in_run_reaches_the_verdict_of_the_callable_run(hip, name):
    rec = _run(name)
    a, f, lo, up = device_of(hip, rec)
    b, _, _, _ = device_of(hip, rec)
    sa = a.optimize(f, lo, up, guess_of(rec))
    sb = b.optimize(Logged(rm.objective(rec["objective"], rec["n"])), lo, up, guess_of(rec))
    assert sa.converged == sb.converged == bool(rec["converged"])
    assert int(a.get_state("flag")[0]) == int(b.get_state("flag")[0]) == (1 if rec["converged"] else 2)
    if rec["converged"]:
        assert np.abs(sa.x - sb.x).max() < 1e-5
    else:
        assert (sa.x == 0.).all() and sa.n_evals > rec["params"]["mfev"]


def _snap(g, P):
    return [{k: g.get_state(k, p).copy() for k in KEYS} for p in range(P)]


def _same(a, b, tag):
    for p, (sa, sb) in enumerate(zip(a, b)):
        for k in KEYS:
            _bits(sa[k], sb[k], "%s population %d %s" % (tag, p, k))


@pytest.mark.parametrize("n,wide", [(3, False), (17, True), (65, False), (128, True)])
def test_phase_walk_and_callable_are_the_iterate_run(hip, n, wide):
    """three populations whose searches take different paths: iterate() with the built-in, the same through
    phase(), the same with a callable that sums as the device does.  2 n + 6 searches up to n = 65 -- past the
    first stage, so the extra search, dnrm2 and the step test with its orthogonalisation or shrink are entered
    through the re-entry of the walk as well -- and 40 at n = 128"""
    P, steps, cls = 3, (2 * n + 6 if n <= 65 else 40), hip.Rosenbrock
    rng = np.random.default_rng(n)
    guess = rng.uniform(-2., 2., (P, n))
    guess[1] *= 0.01
    lo, up = -5. * np.ones(n), 5. * np.ones(n)

    def make(f):
        g = cls(1 << 20, 1e-300, 0.5, populations=P, wide=wide, seed=2)
        g.initialize(f, lo, up, guess.ravel())
        return g

    a, b = make(hip.objectives.rosenbrock), make(hip.objectives.rosenbrock)
    log = Logged(device_objective("rosenbrock", n))
    c = make(log)
    assert len(log.seen) == 0                   # init() evaluates nothing
    _same(_snap(a, P), _snap(b, P), "initialize")
    batches = set()
    for k in range(steps):
        before = [int(a.get_state("fev", p)[0]) for p in range(P)]
        a.iterate()
        seen0 = len(log.seen)
        c.iterate()
        pending = b.phase(0)
        assert pending == P and all(int(b.get_state("pending", p)[0]) == 2 for p in range(P))
        while pending:
            want = [int(b.get_state("pending", p)[0]) for p in range(P)]
            batches.update(want)
            assert b.phase(1) is None
            if n == 3:      # rosen_eval's values are the fused walk's bits: the callable sums as the device does
                for p in range(P):
                    f = device_objective("rosenbrock", n)
                    cand = b.get_state("cand", p).reshape(4, n)
                    _bits(b.get_state("value", p)[:want[p]], [f(cand[q]) for q in range(want[p])], "rosen_eval")
            pending = b.phase(2)
        assert b.phase(2) == 0          # nothing pending: absorb is a no-op
        sa = _snap(a, P)
        _same(sa, _snap(b, P), "search %d, phase walk" % k)
        _same(sa, _snap(c, P), "search %d, callable" % k)
        spent = [int(sa[p]["fev"][0]) - before[p] for p in range(P)]
        assert all(s >= 6 for s in spent) and len(log.seen) - seen0 == sum(spent)
        assert all(int(s["it"][0]) == k + 1 and int(s["pending"][0]) == 0 and int(s["stage"][0]) == 0 for s in sa)
    # (0: a population whose search ended while another's goes on)
    assert batches == {0, 1, 2, 4}
    if n <= 65:
        assert all(int(a.get_state("it", p)[0]) > 2 * n + 2 for p in range(P))
        assert sum(int(a.get_state("orths", p)[0]) for p in range(P)) >= 1
    assert a.run(5) == 5
    for _ in range(5):
        b.iterate()
    _same(_snap(a, P), _snap(b, P), "run against iterate")
    with pytest.raises(hip._ffi.BboError):
        b.phase(3)


def test_populations_are_independent_of_each_other_and_of_their_index(hip):
    n, P, cls = 17, 70, hip.Rosenbrock
    lo, up = -5. * np.ones(n), 5. * np.ones(n)
    guess = np.random.default_rng(4).uniform(-2., 2., (P, n))
    guess[69] = guess[3]            # the same start at two indices
    g = cls(1500, 1e-4, 1., populations=P, seed=3)
    g.initialize(hip.objectives.rosenbrock, lo, up, guess.ravel())
    g.run(1 << 20)
    assert all(int(g.get_state("flag", p)[0]) in (1, 2) for p in range(P))
    assert len({int(g.get_state("fev", p)[0]) for p in range(P)}) > 10
    for k in KEYS:
        _bits(g.get_state(k, 69), g.get_state(k, 3), "population 69 against 3: " + k)
    for p in range(P):
        s = cls(1500, 1e-4, 1., seed=3)
        s.initialize(hip.objectives.rosenbrock, lo, up, guess[p])
        s.run(1 << 20)
        for k in KEYS:
            _bits(g.get_state(k, p), s.get_state(k), "population %d against its single run: %s" % (p, k))
        a, b = g.solution(p), s.solution()
        _bits(a.x, b.x, "solution")
        assert (a.n_evals, a.converged) == (b.n_evals, b.converged)


def _crafted(hip, n, obj, state):
    rec = dict(n=n, objective=obj, params=dict(mfev=1 << 20, tol=1e-8, step0=1., decf=0.1))
    m = model_of(rec)
    m.init([0.] * n)
    state(m)
    log = Logged(rm.objective(obj, n))
    g, _, lo, up = device_of(hip, rec)
    g.initialize(log, lo, up, [0.] * n)
    inject(g, m)
    m.iterate()
    g.iterate()
    _bits(log.seen, [e[0] for e in m.evals], "the points")
    for k, want in (("x", m.x), ("v", m.v), ("d", m.d), ("stepi", [m.stepi]), ("i", [m.i]), ("fev", [m.fev])):
        _bits(g.get_state(k), want, k)
    return m, g


def test_rows_whose_trailing_d_are_zero_keep_their_vectors(hip):
    n = 4

    def state(m):
        m.x[0] = [2., -1., 0.5, 1.5]
        m.x[n] = [0.5, 0.25, 0.5, 1.5]
        m.v[n + 1] = [0.6, 0.8, 0., 0.]
        m.d = [0., -1.5, 1.25, 0., 0., 0.]
        m.i = n + 1

    m, g = _crafted(hip, n, "sphere", state)
    assert m.orth and int(g.get_state("orth")[0]) == 1 and m.i == 2
    V = g.get_state("v").reshape(n + 2, n)
    assert (V[3] == [0., 0., 1., 0.]).all() and (V[4] == [0., 0., 0., 1.]).all() and V[1][0] != 1.


def test_a_stage_that_did_not_move_shrinks_the_step_without_the_extra_search(hip):
    n = 3

    def state(m):
        m.i = n         # every row at the minimum of the sphere: the search returns to its start

    m, g = _crafted(hip, n, "sphere", state)
    assert m.paths["zero_norm"] == 1 and m.i == 1 and m.stepi == 0.1 and m.d[n + 1] == 0.
    assert int(g.get_state("it")[0]) == 1 and int(g.get_state("flag")[0]) == 0


def test_a_nan_from_the_callable_counts_as_inf(hip):
    rec = _run("run_n3_sphere")
    base = rm.objective("sphere", 3)

    def f(x):       # a pure function of the point: NaN in a shell the run crosses
        v = base(x)
        return float("nan") if 0.5 < v < 2.5 else v

    m, g = _whole_run(hip, rec, f=f)
    assert any(v == rm.INF for _, v in m.evals), "the run never met the shell: choose another"


def test_a_nan_from_the_built_in_counts_as_inf(hip):
    g = hip.Rosenbrock(1000, 1e-8, 1., seed=1)
    g.initialize(hip.objectives.rosenbrock, -5. * np.ones(3), 5. * np.ones(3), [np.inf, np.inf, 1.])    # inf - inf
    g.iterate()
    assert (g.get_state("fs") == np.inf).all() and float(g.get_state("fx0")[0]) == np.inf
    assert int(g.get_state("fev")[0]) >= 6 and not np.isnan(g.get_state("d")).any()


def test_the_constant_objective_ends_its_search_at_1e30(hip):
    g = hip.Rosenbrock(1 << 20, 1e-8, 1., seed=1)
    g.initialize(hip.objectives.rosenbrock, [-5.], [5.], [0.5])        # n = 1: the empty sum
    g.iterate()
    assert [int(q) for q in g.get_state("path")] == [rm.FORWARD, 100, 0, rm.NO_FINAL]
    assert int(g.get_state("fev")[0]) == 106 and float(g.get_state("d")[1]) == -2. ** 99


def test_the_library_refuses_what_the_class_refuses(hip):
    from bboptpy_amd import _ffi
    cls = hip.Rosenbrock
    with pytest.raises(ValueError, match=r"dimension must be in \[1, 128\]"):
        cls(100, 0., 1.).initialize(hip.objectives.sphere, -np.ones(129), np.ones(129), np.zeros(129))
    g = cls(100, 0., 1., seed=1)
    g._problem = lambda f, lo, up, x: hip.MultivariateSearch._problem(g, f, lo, up, x)     # past the class's checks
    with pytest.raises(_ffi.BboError, match=r"dimension must be in \[1, 128\]"):
        g.initialize(hip.objectives.sphere, -np.ones(129), np.ones(129), np.zeros(129))
    with pytest.raises(ValueError, match="mfev must be positive"):
        cls(0, 0., 1.)
    for mfev in (0, -5):
        p = _ffi.default_params(_ffi.ALGO_ROSENBROCK)
        p.mfev, p.sigma0 = mfev, 1.
        h = C.c_void_p()
        assert _ffi.lib().bbo_create(C.byref(p), C.byref(h)) == _ffi.ERR_ARG
    p = _ffi.default_params(_ffi.ALGO_ROSENBROCK)
    p.mfev, p.sigma0 = 100, 1.
    h = C.c_void_p()
    _ffi.check(_ffi.lib().bbo_create(C.byref(p), C.byref(h)))
    try:
        s = _ffi.RosenParams()
        _ffi.lib().bbo_rosen_params_default(C.byref(s))
        s.wide = 2
        assert _ffi.lib().bbo_rosen_configure(h, C.byref(s)) == _ffi.ERR_ARG
        s.wide = 1
        assert _ffi.lib().bbo_rosen_configure(h, C.byref(s)) == 0
    finally:
        _ffi.lib().bbo_destroy(h)

    class Fake(hip.DeviceObjective):
        def __init__(self):
            self._handle = None

        def __del__(self):
            pass

    with pytest.raises(ValueError, match="Rosenbrock does not take a DeviceObjective yet"):
        cls(100, 0., 1.).initialize(Fake(), -np.ones(3), np.ones(3), np.zeros(3))
    # a real objective program: refused by the class and by the library, naming who takes one
    L, lo, up = _ffi.lib(), -np.ones(3), np.ones(3)
    prog = hip.DeviceObjective('extern "C" __device__ double bbo_user_objective(const double *x, int n, '
                               'const double *data) { return x[0] * x[0]; }')
    g = cls(100, 0., 1., seed=1)
    with pytest.raises(ValueError, match="Rosenbrock does not take a DeviceObjective yet"):
        g.initialize(prog, lo, up, np.zeros(3))
    h = g._ensure_handle()
    ob = _ffi.Objective()
    ob.kind, ob.user = _ffi.OBJ_PROGRAM, prog._handle
    st = L.bbo_init(h, 3, lo, up, np.zeros(3), C.byref(ob))
    msg = L.bbo_last_error(h).decode()
    assert st == _ffi.ERR_ARG and "Rosenbrock" in msg and "CMAES" in msg and "SHADE" in msg, (st, msg)
    # a step of 0 (the doubling loop would end on the budget alone) and a negative tol, by the library as well
    for field, v in (("sigma0", 0.), ("tol", -1.), ("tol", float("nan")), ("sigma0", float("inf"))):
        p = _ffi.default_params(_ffi.ALGO_ROSENBROCK)
        p.mfev, p.sigma0, p.tol = 100, 1., 1e-8
        setattr(p, field, v)
        out = C.c_void_p()
        assert L.bbo_create(C.byref(p), C.byref(out)) == _ffi.ERR_ARG, (field, v)
    g.initialize(hip.objectives.sphere, lo, up, np.zeros(3))
    with pytest.raises(_ffi.BboError):
        g.set_state("stepi", [0.])


def test_ccpso_takes_rosenbrock_as_its_local_optimizer(hip):
    n = 12
    calls = [0]

    def f(x):
        calls[0] += 1
        return float(np.sum(x * x) + 0.5 * np.sum(x[:-1] * x[1:]))

    loc = hip.Rosenbrock(200, 1e-10, 0.05, repair=True, seed=1)
    g = hip.CCPSO(mfev=10 ** 8, sigmatol=1e-12, np=6, pps=[3], local=loc, localfreq=2, seed=31)
    assert not g._local_native
    g.initialize(f, -5. * np.ones(n), 5. * np.ones(n), np.zeros(n))
    before = float(g.get_state("fyhat")[0])
    for _ in range(6):
        g.iterate()
    assert g._nlocal == 3
    assert int(g.get_state("fev")[0]) == calls[0]       # every evaluation of the local searches is counted
    assert float(g.get_state("fyhat")[0]) <= before
