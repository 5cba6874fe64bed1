"""GPU: one iterate() of the device from every recorded state of the reference
(tests/golden/neldermead_runs.json), with the built-in objective.

The fixture keeps sums of the states, not the states: tests/neldermead_model.py replays the recorded run (bit for
bit, tests/test_neldermead_model.py holds it to the sums) and its state before step g is set on the device -- p, y,
ilo, ylo, jcount, fev.  After one iterate() the device must report the reference's branch, ihi, ilo, fev and
jcount, and row ihi of the simplex must be the reference's point bit for bit, on every step the fixture marks ok
(no comparison within 1e-6 relative of a tie: the built-in sums the objective in another order than the
reference).  The value the device stored for that row is held to the bound every built-in form is held to
(tests/test_objective_forms_gpu.py: objective_reference.reference_at and ratio <= 1)."""
import numpy as np
import pytest

import neldermead_model as nm
import objective_reference as R
from test_neldermead_model import GOLDEN, guess_of, model_of

pytestmark = pytest.mark.gpu


def _bits(a, b, what):
    a, b = np.asarray(a, float).ravel(), np.asarray(b, float).ravel()
    assert a.shape == b.shape, what
    assert a.tobytes() == b.tobytes(), (what, np.flatnonzero(a != b)[:8], a[a != b][:4], b[a != b][:4])


def inject(g, m, p=0):
    """the model's state between steps into population p of the device"""
    g.set_state("p", [v for r in m.p for v in r], p)
    g.set_state("y", m.y, p)
    g.set_state("ilo", [m.ilo], p)
    g.set_state("ylo", [m.ylo], p)
    g.set_state("jcount", [m.jcount], p)
    g.set_state("fev", [m.icount], p)


def device_of(hip, rec, f=None, **kw):
    par, cls, n = rec["params"], hip.NelderMead, rec["n"]
    g = cls(par["mfev"], par["tol"], par["rad0"], cls.NelderMead_SimplexInit[rec["minit"]],
            cls.NelderMead_ParamInit[rec["pinit"]], par["checkev"], par["eps"], seed=5, **kw)
    return g, (f or getattr(hip.objectives, rec["objective"])), -5. * np.ones(n), 5. * np.ones(n)


@pytest.mark.parametrize("lds", [True, False], ids=["lds", "hbm"])
@pytest.mark.parametrize("rec", GOLDEN["steps"], ids=lambda r: r["name"])
def test_one_step_from_every_recorded_state(hip, rec, lds):
    n, obj = rec["n"], rec["objective"]
    g, f, lo, up = device_of(hip, rec, lds=lds)
    g.initialize(f, lo, up, guess_of(rec))
    m = model_of(rec)
    m.init(guess_of(rec))
    m.first_simplex()
    _bits(g.get_state("coef"), [m.ccoef, m.ecoef, m.rcoef, m.scoef], "coef")
    # the first simplex: the reference's rows bit for bit, the values inside the bound
    _bits(g.get_state("p"), m.p, "first simplex")
    assert int(g.get_state("fev")[0]) == rec["init"]["icount"] == n + 1
    worst, held = 0., 0
    for x, v in zip(m.p, g.get_state("y")):
        worst = max(worst, R.ratio(v, *R.reference_at(obj, x)))
    assert worst <= 1., "first simplex: %.4g bounds" % worst
    for k, st in enumerate(rec["states"]):
        tag = "%s step %d: " % (rec["name"], k)
        inject(g, m)
        m.evals = []
        m.iterate()
        assert m.branch == st["branch"] and m.state_crc() == st["state_crc"], tag + "the model left the record"
        g.iterate()
        if not st["ok"]:
            continue
        held += 1
        got = {q: int(g.get_state(q)[0]) for q in ("branch", "ihi", "ilo", "fev", "jcount", "conv")}
        assert got == {q: st[q] for q in ("branch", "ihi", "ilo", "jcount", "conv")} | {"fev": st["icount"]}, tag
        P, Y = g.get_state("p").reshape(n + 1, n), g.get_state("y")
        if st["branch"] == nm.SHRINK:
            _bits(P, m.p, tag + "the shrunk simplex")
            pairs = list(zip(m.p, Y))
        else:
            _bits(P[st["ihi"]], m.p[m.ihi], tag + "the new row")
            # (the refused outside contraction stores pstar with the value of p2star, the last point evaluated)
            at = m.evals[-1][0] if st["branch"] == nm.OUTSIDE_REFUSED else m.p[m.ihi]
            pairs = [(at, Y[st["ihi"]])]
            keep = [j for j in range(n + 1) if j != st["ihi"]]
            _bits(P[keep], [m.p[j] for j in keep], tag + "the other rows")
            _bits(Y[keep], [m.y[j] for j in keep], tag + "the other values")
        for x, v in pairs:
            r = R.ratio(v, *R.reference_at(obj, x))
            worst = max(worst, r)
            assert r <= 1., tag + "the value %r is %.4g bounds from the reference at its point" % (v, r)
    assert held >= 12
    print("RATIO NelderMead %s %s: %.3f over %d steps" % (rec["name"], "lds" if lds else "hbm", worst, held))
