"""GPU: acd_sweep, acd_ae and the decomposition against the recorded runs of the reference's ACD
(tests/golden/acd_runs.json).

For every recorded shape and every recorded sweep the state the reference held before that sweep is
injected (tests/acd_model.py replays the record bit for bit, tests/test_acd_model.py, so its state IS the
reference's) and the sweep is run, as one launch and cut after every coordinate step.  Every point handed
to the objective, x_best, sigma, ix, it, fev, improved and the archive are the reference's bit for bit;
the values within n 2^-52 relative: the objectives of the fixture are sums of at most n non-negative
terms that the device forms bit for bit and adds in another order (schwefel12 in the same order), so
either sum is within (n - 1) 2^-53 of the exact sum of those terms.  Where an update follows, order, m, p
and C are the reference's bit for bit.  The decomposition cannot be (a degenerate
eigenspace, whose basis rounding decides): the device's B, invB and diagd satisfy the invariants within
10 times the reference's own recorded residuals, floored at n 2^-52.
The fixture's seed rule (no comparison closer than 1e-6 relative) is what makes the decisions the
reference's: there is no skip path.  The speculative sweep was built, passed this test as a third leg bit
for bit, measured slower at 4096 populations and was dropped: no leg is left."""
import numpy as np
import pytest

import acd_model as am
from test_acd_model import SHAPES, hx, reference_model

pytestmark = pytest.mark.gpu


def _bits(a, b, what):
    a, b = np.asarray(a, float).ravel(), np.asarray(b, float).ravel()
    assert a.shape == b.shape, what
    assert a.tobytes() == b.tobytes(), (what, np.flatnonzero(a != b)[:8], a[a != b][:4], b[a != b][:4])


def inject(g, m, p=0):
    """the model's state into population p of the device"""
    for k, v in (("xbest", m.xbest), ("fbest", [m.fbest]), ("sigma", m.sigma), ("B", m.B), ("invB", m.invB),
                 ("C", m.C), ("p", m.p), ("m", m.m), ("mold", m.mold), ("diagd", m.diagd), ("x", m.X),
                 ("f", m.fx), ("order", m.order), ("fhist", m.fhist), ("ix", [m.ix]), ("it", [m.it]),
                 ("itae", [m.itae]), ("improved", [int(m.improved)]), ("fev", [m.fev])):
        g.set_state(k, np.asarray(v, float), p)


def _close(dev, ref, n, what, worst):
    dev, ref = np.asarray(dev, float).ravel(), np.asarray(ref, float).ravel()
    rel = np.abs(dev - ref) / np.maximum(np.abs(ref), 1e-300)
    rel[dev == ref] = 0.
    worst[0] = max(worst[0], float(rel.max()))
    assert rel.max() <= n * 2. ** -52, (what, rel.max())


def _after_sweep(g, m, n, tag, worst):
    """the device behind a sweep against the model behind the same sweep (before its update's effects
    on B, invB and diagd, which are the decomposition's)"""
    _bits(g.get_state("x"), m.X, tag + "points")
    _close(g.get_state("f"), m.fx, n, tag + "values", worst)
    _bits(g.get_state("xbest"), m.xbest, tag + "xbest")
    _close(g.get_state("fbest"), [m.fbest], n, tag + "fbest", worst)
    _bits(g.get_state("sigma"), m.sigma, tag + "sigma")
    got = {k: int(g.get_state(k)[0]) for k in ("ix", "it", "fev", "improved", "itae", "due", "pending")}
    want = dict(ix=m.ix, it=m.it, fev=m.fev, improved=int(m.improved), itae=m.itae, due=0, pending=0)
    assert got == want, (tag, got, want)
    _close(g.get_state("fhist")[(m.it - 1) % m.period], m.fbest, n, tag + "fhist", worst)


def _after_update(g, m, u, n, tag):
    assert [int(v) for v in g.get_state("order")] == u["order"] == m.order, tag + "order"
    _bits(g.get_state("m"), hx(u["m"]), tag + "m")
    if u["itae"] == 1:
        return
    _bits(g.get_state("p"), hx(u["p"]), tag + "p")
    C = g.get_state("C").reshape(n, n)
    _bits(C, hx(u["C"]), tag + "C")
    B, invB, d = g.get_state("B").reshape(n, n), g.get_state("invB").reshape(n, n), g.get_state("diagd")
    r1, r2 = am.residuals(B, invB, C)
    b1 = max(10. * float.fromhex(u["res_bbt"]), n * 2. ** -52)
    b2 = max(10. * float.fromhex(u["res_inv"]), n * 2. ** -52)
    print("%s ||B B^T - C|| / ||C|| %.3e (reference %.3e), ||invB B - I|| %.3e (reference %.3e)" % (
        tag, r1, float.fromhex(u["res_bbt"]), r2, float.fromhex(u["res_inv"])))
    assert r1 <= b1 and r2 <= b2, (tag, r1, b1, r2, b2)
    assert np.all(np.diff(d) >= 0.), tag + "diagd ascending"
    S = np.tril(C) + np.tril(C, -1).T
    w = np.linalg.eigvalsh(S)
    assert np.abs(d * d - w).max() <= b1 * np.abs(w).max(), (tag, d * d, w)
    _bits(g.get_state("colmax"), np.abs(B).max(axis=0), tag + "colmax")


@pytest.mark.parametrize("leg", ["whole", "cut"])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_every_recorded_sweep_from_the_recorded_state(hip, name, leg):
    rec = SHAPES[name]
    n, box = rec["n"], rec["box"]
    cut = leg == "cut"
    g = hip.ACD(1 << 30, 0., 0., seed=1, poll_every=1 if cut else None)
    g.initialize(rec["objective"], -box * np.ones(n), box * np.ones(n), np.zeros(n))
    assert int(g.get_state("cp")[0]) == rec["init"]["cp"] and int(g.get_state("chunk")[0]) == (1 if cut else n)
    m = reference_model(rec)
    worst = [0.]
    for s in range(rec["sweeps"]):
        tag = "%s sweep %d %s: " % (name, s, leg)
        inject(g, m)
        assert g.run(n) == n
        for st in rec["steps"][s * n:(s + 1) * n]:
            m.iterate()
        _after_sweep(g, m, n, tag, worst)
        u = rec["steps"][(s + 1) * n - 1].get("update")
        assert (u is not None) == m.updated
        if u:
            _after_update(g, m, u, n, tag)
    print("%s: values within %.3e relative of the reference's (bound %.3e)" % (name, worst[0], n * 2. ** -52))


def test_the_step_by_step_walk_hands_the_objective_the_recorded_points(hip):
    """bbo_acd_phase: the pair of every step of the first two recorded sweeps, in the order x1, x2"""
    rec = SHAPES["n5_rosenbrock"]
    n, box = rec["n"], rec["box"]
    g = hip.ACD(1 << 30, 0., 0., seed=1)
    g.initialize(rec["objective"], -box * np.ones(n), box * np.ones(n), np.zeros(n))
    m = reference_model(rec)
    inject(g, m)
    worst = [0.]
    for k, st in enumerate(rec["steps"][:2 * n]):
        assert g.phase(0) == 1
        ev = hx(st["evals"])
        _bits(g.get_state("cand"), ev[:n] + ev[n + 1:2 * n + 1], "step %d cand" % k)
        g.phase(1)
        _close(g.get_state("value"), [ev[n], ev[2 * n + 1]], n, "step %d value" % k, worst)
        g.phase(2)
        m.iterate()
        if m.updated and m.itae > 1:
            # from here on the device walks with its own basis: the model follows it
            inject(g, m)
        _bits(g.get_state("xbest"), m.xbest, "step %d xbest" % k)
        assert int(g.get_state("fev")[0]) == m.fev and int(g.get_state("ix")[0]) == m.ix
