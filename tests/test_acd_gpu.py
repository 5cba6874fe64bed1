"""GPU: the ACD kernels against tests/acd_model.py, and the engine's behaviour at the C ABI.

The device's basis cannot be the reference's from the second update on, so the
model is fed the DEVICE's own B, invB and diagd behind every update and everything else -- every point,
value, sigma, m, p, C, the ranking -- must be the device's bit for bit (the model's device form sums the
objective as the device does).  Against the recorded reference: tests/test_acd_golden_gpu.py."""
import json
import math
import os

import numpy as np
import pytest

import acd_model as am
from slpso_model import device_objective
from test_acd_golden_gpu import _bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("xbest", "fbest", "sigma", "B", "invB", "C", "p", "m", "diagd", "x", "f", "order", "ix", "it", "itae",
        "improved", "fev", "flag", "rule", "colmax", "fhist")
MIN_GAP = 1e-6


def _snapshot(g, p=0):
    return {k: g.get_state(k, p).copy() for k in KEYS}


def _same_state(sa, sb, tag=""):
    for k in KEYS:
        _bits(sa[k], sb[k], tag + k)


def _start(hip, n, obj, x0=None, P=1, mfev=1 << 30, ftol=0., xtol=0., box=5., seed=7, **kw):
    g = hip.ACD(mfev, ftol, xtol, seed=seed, populations=P, from_guess=x0 is not None, **kw)
    g.initialize(obj, -box * np.ones(n), box * np.ones(n), np.zeros(P * n) if x0 is None else np.asarray(x0, float))
    return g


def _model(n, obj, x0, decompose=am.eigh_decompose, mfev=1 << 30, ftol=0., xtol=0., box=5., f=None):
    m = am.Acd(f or device_objective(obj, n), n, [-box] * n, [box] * n, mfev, ftol, xtol, decompose=decompose)
    return m.start(x0)


def _device_basis(g):
    def decompose(model):
        n = model.n
        model.C = [list(r) for r in g.get_state("C").reshape(n, n)]      # (the diagonal a repair shifted)
        return ([list(r) for r in g.get_state("B").reshape(n, n)],
                [list(r) for r in g.get_state("invB").reshape(n, n)], list(g.get_state("diagd")))
    return decompose


def _quiet_start(n, obj, sweeps, first):
    """a start point from which the stand-in run (numpy's eigh) meets no comparison closer than 1e-6"""
    for seed in range(first, first + 64):
        x0 = np.random.default_rng(seed).uniform(-5., 5., n)
        m = _model(n, obj, x0)
        margin = math.inf
        for _ in range(sweeps * n):
            m.iterate()
            margin = min(margin, m.margin)
        if margin >= MIN_GAP:
            return seed, x0
    raise AssertionError("no start point without a close decision among 64")


@pytest.mark.parametrize("n,obj,first", [(5, "ellipsoid", 0), (17, "rosenbrock", 0), (65, "sphere", 0)])
def test_the_device_is_the_model_fed_its_own_basis(hip, n, obj, first):
    sweeps = 6
    seed, x0 = _quiet_start(n, obj, sweeps, first)
    g = _start(hip, n, obj, x0)
    m = _model(n, obj, x0, decompose=_device_basis(g))
    _bits(g.get_state("xbest"), x0, "from_guess")
    margin, updates = math.inf, 0
    for k in range(sweeps * n):
        tag = "n %d start %d step %d: " % (n, seed, k)
        ix = m.ix
        g.iterate()
        c_before = [list(r) for r in m.C]
        m.iterate()
        margin = min(margin, m.margin)
        assert margin >= MIN_GAP, "the device run from start point %d meets a close decision (%.3e) at step %d: " \
            "choose another `first`" % (seed, margin, k)
        rows = g.get_state("x").reshape(2 * n, n)
        _bits(rows[2 * ix:2 * ix + 2], [m.evals[0][0], m.evals[1][0]], tag + "points")
        _bits(g.get_state("f")[2 * ix:2 * ix + 2], [m.evals[0][1], m.evals[1][1]], tag + "values")
        _bits(g.get_state("xbest"), m.xbest, tag + "xbest")
        _bits(g.get_state("fbest"), [m.fbest], tag + "fbest")
        _bits(g.get_state("sigma"), m.sigma, tag + "sigma")
        got = {q: int(g.get_state(q)[0]) for q in ("ix", "it", "fev", "improved", "itae", "flag")}
        assert got == dict(ix=m.ix, it=m.it, fev=m.fev, improved=int(m.improved), itae=m.itae, flag=0), tag
        if m.updated:
            updates += 1
            assert [int(v) for v in g.get_state("order")] == m.order, tag + "order"
            _bits(g.get_state("m"), m.m, tag + "m")
            _bits(g.get_state("p"), m.p, tag + "p")
            if m.itae > 1:
                # C before the repair's shift (none here): the model's own update of the C it held
                c1 = m.c1
                want = [[(1. - c1) * c_before[i][j] + c1 * m.p[i] * m.p[j] for j in range(n)] for i in range(n)]
                _bits(g.get_state("C"), want, tag + "C")
                r1, r2 = am.residuals(m.B, m.invB, m.C)
                assert r1 <= 64 * n * 2. ** -52 and r2 <= 1e-9, (tag, r1, r2)
    assert updates >= 3


@pytest.mark.parametrize("n", [37, 65])
def test_the_first_sweep_under_bounds_that_differ_in_every_coordinate(hip, n):
    """tests/_boxes.py's box: sigma[j] starts at (up[j] - lo[j]) / 4, another value in every coordinate, and the
    two points of step j are clamp(x_best[j] -+ sigma[j]) to that coordinate's own bounds.  The first sweep only:
    its basis is the identity on both sides, and from a strictly interior start no trial point equals x_best
    (once x_best lies on a bound the clamped trial point IS x_best, an exact tie, which the decision-gap guard of
    this file's walk rejects by construction).  First the model alone: at least three coordinates whose trial
    point is clamped to the lower bound, three to the upper bound, three that stay strictly inside throughout,
    and no decision closer than MIN_GAP.  Then the device, bit for bit."""
    from _boxes import binding_witness, percoord_box, percoord_guess
    lo, up = percoord_box(n)
    x0 = percoord_guess(n, 3)[1]
    f = device_objective("sphere", n)

    def model():
        return am.Acd(f, n, lo, up, 1 << 30, 0., 0.).start(x0)
    w = model()
    pts, margin = [], math.inf
    for _ in range(n):
        w.iterate()
        margin = min(margin, w.margin)
        pts.append(np.array([w.evals[0][0], w.evals[1][0]]))
    binding_witness(pts, lo, up)
    assert margin >= MIN_GAP and w.updated
    g = hip.ACD(1 << 30, 0., 0., seed=7, from_guess=True)
    g.initialize("sphere", lo, up, x0)
    _bits(g.get_state("xbest"), x0, "from_guess")
    _bits(g.get_state("sigma"), (up - lo) / 4., "initial sigma")
    m = model()
    for k in range(n):
        tag = "n %d step %d: " % (n, k)
        ix = m.ix
        g.iterate()
        m.iterate()
        rows = g.get_state("x").reshape(2 * n, n)
        _bits(rows[2 * ix:2 * ix + 2], [m.evals[0][0], m.evals[1][0]], tag + "points")
        assert (rows[2 * ix:2 * ix + 2] >= lo).all() and (rows[2 * ix:2 * ix + 2] <= up).all(), tag
        _bits(g.get_state("f")[2 * ix:2 * ix + 2], [m.evals[0][1], m.evals[1][1]], tag + "values")
        _bits(g.get_state("xbest"), m.xbest, tag + "xbest")
        _bits(g.get_state("fbest"), [m.fbest], tag + "fbest")
        _bits(g.get_state("sigma"), m.sigma, tag + "sigma")
        got = {q: int(g.get_state(q)[0]) for q in ("ix", "it", "fev", "improved", "itae", "flag")}
        assert got == dict(ix=m.ix, it=m.it, fev=m.fev, improved=int(m.improved), itae=m.itae, flag=0), tag
    assert m.updated
    _bits(g.get_state("m"), m.m, "m after the first sweep")
    _bits(g.get_state("p"), m.p, "p after the first sweep")


@pytest.mark.parametrize("n,obj", [(2, "rosenbrock"), (33, "ellipsoid"), (128, "rosenbrock")])
def test_run_iterate_and_a_chunk_of_one_give_the_same_bits(hip, n, obj):
    steps = 3 * n + 1
    a, b, c = _start(hip, n, obj), _start(hip, n, obj, poll_every=1), _start(hip, n, obj)
    sq = _start(hip, n, obj, poll_every=3)
    assert int(a.get_state("chunk")[0]) == n and int(b.get_state("chunk")[0]) == 1
    assert a.run(steps) == steps and b.run(steps) == steps
    assert sq.run(steps) == steps
    for _ in range(steps):
        c.iterate()
    sa = _snapshot(a)
    assert int(sa["it"][0]) == steps and int(sa["fev"][0]) == 2 * steps
    assert int(sa["itae"][0]) >= (2 if n > 2 else 1)        # (decompositions behind: not every sweep of n = 2 improves)
    _same_state(sa, _snapshot(b), "chunk 1: ")
    _same_state(sa, _snapshot(c), "iterate: ")
    _same_state(sa, _snapshot(sq), "chunks of 3: ")
    if n == 128:
        C = sa["C"].reshape(n, n)
        r1, r2 = am.residuals(sa["B"].reshape(n, n), sa["invB"].reshape(n, n), C)
        assert r1 <= 64 * n * 2. ** -52 and r2 <= 1e-9, (r1, r2)


def test_a_python_callable_is_called_in_the_reference_order(hip):
    n, obj = 5, "rosenbrock"
    f = device_objective(obj, n)
    calls = []

    def py(x):
        calls.append(np.array(x))
        return f(x)

    x0 = np.random.default_rng(2).uniform(-5., 5., n)
    a, b = _start(hip, n, obj, x0), _start(hip, n, py, x0)
    steps = 4 * n
    assert a.run(steps) == steps and b.run(steps) == steps
    _same_state(_snapshot(a), _snapshot(b), "callable: ")
    assert len(calls) == b.solution().n_evals == 2 * steps
    # x1, then x2: the model fed the device's basis names every call
    g = _start(hip, n, obj, x0)
    m = _model(n, obj, x0, decompose=_device_basis(g))
    for k in range(steps):
        g.iterate()
        m.iterate()
        _bits(calls[2 * k], m.evals[0][0], "call %d" % (2 * k))
        _bits(calls[2 * k + 1], m.evals[1][0], "call %d" % (2 * k + 1))


def test_a_converged_population_freezes_and_the_others_go_on(hip):
    n, obj, P = 5, "sphere", 3
    g = _start(hip, n, obj, P=P, xtol=1e-8, seed=21)
    g.set_state("xbest", np.zeros(n), 1)
    g.set_state("sigma", 1e-12 * np.ones(n), 1)
    assert g.run(1) == 1
    assert [int(g.get_state("flag", p)[0]) for p in range(P)] == [0, 1, 0]
    assert int(g.get_state("rule", 1)[0]) == 2 and g.solution(1).converged and g.solution(1).n_evals == 2
    frozen = _snapshot(g, 1)
    assert g.run(10 * n) == 10 * n
    _same_state(frozen, _snapshot(g, 1), "frozen: ")
    for p in (0, 2):
        s = _start(hip, n, obj, xtol=1e-8, seed=21)
        s.set_state("substream", [p])
        assert s.run(10 * n + 1) == 10 * n + 1
        _same_state(_snapshot(s), _snapshot(g, p), "population %d: " % p)
    assert not np.array_equal(g.get_state("xbest", 0), g.get_state("xbest", 2))


@pytest.mark.parametrize("diag", [(1., 1., 1e15), (2., -1., 4.)])
def test_both_repairs_against_the_model(hip, diag):
    """C and p set before the sweep that ends in the second update.  Either solver finds an eigenvalue
    within a few n eps ||C|| of the true one, so that is how close the device's diagd^2 and shifted
    diagonal of C are to the model's (numpy's eigh); the small eigenvalues of diag(1, 1, 1e15) are decided
    by the repair, whose invariants are tested on the device's own numbers."""
    n, obj = 3, "sphere"
    x0 = [1.5, -2.5, 0.5]
    g = _start(hip, n, obj, x0)
    pre = []

    def decompose(model):
        pre.append(np.array(model.C))
        return am.eigh_decompose(model)

    m = _model(n, obj, x0, decompose=decompose)
    for _ in range(n):              # one sweep: the first update forms m
        g.iterate()
        m.iterate()
    assert m.itae == 1 and int(g.get_state("itae")[0]) == 1
    m.C = [[diag[i] if i == j else 0. for j in range(n)] for i in range(n)]
    m.p = [0.] * n
    m.improved = True               # the sweep ends in an update whether or not it improves
    g.set_state("C", np.array(m.C))
    g.set_state("p", m.p)
    g.set_state("improved", [1.])
    for _ in range(n):
        g.iterate()
        m.iterate()
    assert m.itae == 2 and int(g.get_state("itae")[0]) == 2 and len(pre) == 1
    _bits(g.get_state("p"), m.p, "p")
    C = g.get_state("C").reshape(n, n)
    _bits(C - np.diag(np.diag(C)), pre[0] - np.diag(np.diag(pre[0])), "C off the diagonal")
    d = g.get_state("diagd")
    bound = 16 * n * 2. ** -52 * max(d) ** 2
    shift = np.diag(C) - np.diag(pre[0])
    print("diag %s: device diagd %s, model %s, shift of the diagonal %s" % (diag, d, m.diagd, shift))
    assert (shift > 0.).all() and np.ptp(shift) <= bound                   # a repair ran, the same for every i
    assert np.abs(np.diag(C) - np.diag(np.array(m.C))).max() <= bound
    assert np.abs(d * d - np.array(m.diagd) ** 2).max() <= bound
    assert np.all(np.diff(d) >= 0.) and d[0] > 0. and d[n - 1] ** 2 <= 1e14 * d[0] ** 2 * (1. + 1e-9)
    # B B^T is C with its eigenvalues repaired (a clamped negative one is not C's any more): the model's
    B, invB, Bm = g.get_state("B").reshape(n, n), g.get_state("invB").reshape(n, n), np.array(m.B)
    assert np.abs(B @ B.T - Bm @ Bm.T).max() <= 4 * bound and np.abs(invB @ B - np.eye(n)).max() <= 1e-6


def test_the_history_rule_stops_where_the_model_says(hip):
    n, obj = 1, "sphere"
    x0 = [3.25]
    g = _start(hip, n, obj, x0, ftol=1e-3)
    m = _model(n, obj, x0, ftol=1e-3)
    assert m.period == 30 == int(g.get_state("cp")[0])
    while not m.converged():
        m.iterate()
        assert m.it < 500
    assert m.converged() == 1 and m.it > m.period
    done = g.run(10000)
    assert done >= m.it and int(g.get_state("it")[0]) == m.it
    assert (int(g.get_state("flag")[0]), int(g.get_state("rule")[0])) == (1, 1)
    _bits(g.get_state("fbest"), [m.fbest], "fbest")
    _bits(g.get_state("sigma"), m.sigma, "sigma")
    sol = g.solution()
    assert sol.converged and sol.n_evals == m.fev
    # frozen: another run() does nothing
    assert g.run(10) == 0 and int(g.get_state("it")[0]) == m.it


def test_the_budget_ends_a_run(hip):
    n = 5
    g = _start(hip, n, "rosenbrock", mfev=101)
    sol = g.optimize("rosenbrock", -5. * np.ones(n), 5. * np.ones(n), np.zeros(n))
    assert sol.n_evals in (101, 102) and not sol.converged
    assert int(g.get_state("flag")[0]) == 2 and int(g.get_state("rule")[0]) == 0


def test_seeds_guesses_and_refusals(hip):
    n = 9
    a, b, c = _start(hip, n, "sphere", seed=5), _start(hip, n, "sphere", seed=5), _start(hip, n, "sphere", seed=6)
    _bits(a.get_state("xbest"), b.get_state("xbest"), "same seed")
    xa = a.get_state("xbest")
    assert not np.array_equal(xa, c.get_state("xbest")) and (np.abs(xa) <= 5.).all()
    _bits(a.get_state("sigma"), 2.5 * np.ones(n), "sigma")
    assert a.get_state("fbest")[0] == math.inf and not a.solution().converged
    assert a.run(4 * n) == 4 * n and b.run(4 * n) == 4 * n
    _same_state(_snapshot(a), _snapshot(b), "same seed: ")
    x0 = np.linspace(-4., 4., 2 * n)
    d = _start(hip, n, "sphere", x0, P=2)
    _bits(d.get_state("xbest", 0), x0[:n], "guess 0")
    _bits(d.get_state("xbest", 1), x0[n:], "guess 1")
    with pytest.raises(ValueError, match=r"ACD: dimension must be in \[1, 128\]"):
        _start(hip, 129, "sphere")
    with pytest.raises(ValueError, match="the bounds must be finite"):
        hip.ACD(100, 0., 0.).initialize("sphere", -np.ones(3), np.array([1., np.inf, 1.]), np.zeros(3))
    # the library says the same to a caller that is not the class
    e = hip.ACD(100, 0., 0.)
    e.MAX_N = 1000
    with pytest.raises(hip._ffi.BboError, match=r"ACD: dimension must be in \[1, 128\]"):
        e.initialize("sphere", -np.ones(129), np.ones(129), np.zeros(129))
    with pytest.raises(hip._ffi.BboError, match="unknown or read-only state key"):
        a.set_state("rule", [1.])


@pytest.mark.parametrize("obj", ["sphere", "rosenbrock", "schwefel12"])
def test_whole_runs_lie_in_the_band_of_the_reference(hip, obj):
    """64 populations at the fixture's n, tolerances and budget.  The margins are quantiles of the
    reference's own spread over its 256 recorded runs."""
    with open(os.path.join(ROOT, "tests", "golden", "acd_runs.json")) as fh:
        b = json.load(fh)["bands"]
    n, P = b["n"], 64
    g = _start(hip, n, obj, P=P, mfev=b["mfev"], ftol=b["ftol"], xtol=b["xtol"], box=b["box"], seed=77)
    g.run(1 << 30)
    sols = [g.solution(p) for p in range(P)]
    fev = np.array([s.n_evals for s in sols])
    fb = np.array([g.get_state("fbest", p)[0] for p in range(P)])
    share = np.mean([int(g.get_state("flag", p)[0]) == 1 for p in range(P)])
    ref_fev = np.array(b[obj]["n_evals"], float)
    ref_fb = np.array([float.fromhex(v) for v in b[obj]["fbest"]])
    lo, hi = np.percentile(ref_fev, [10, 90])
    print("%s: median n_evals %.0f (reference 10th .. 90th percentile %.0f .. %.0f), converged share %.3f "
          "(reference %.3f), median f_best %.3e (reference 90th percentile %.3e)" % (
              obj, np.median(fev), lo, hi, share, b[obj]["converged_share"], np.median(fb), np.percentile(ref_fb, 90)))
    assert lo <= np.median(fev) <= hi
    assert share >= b[obj]["converged_share"] - 0.10
    assert np.median(fb) <= np.percentile(ref_fb, 90)
    h = _start(hip, n, obj, P=P, mfev=b["mfev"], ftol=b["ftol"], xtol=b["xtol"], box=b["box"], seed=77)
    h.run(1 << 30)
    assert [h.solution(p).n_evals for p in range(P)] == list(fev)
