"""GPU: one iterate() of the device from every recorded state of the reference
(tests/golden/rosenbrock_runs.json), with the built-in objective, in both forms of the walk.

The fixture keeps sums of the states, not the states: tests/rosenbrock_model.py replays the recorded run (bit for
bit, tests/test_rosenbrock_model.py holds it to the sums) and its state before search k is set on the device -- x,
v, d, stepi, i, fev.  After one iterate() the device must report the reference's i, fev and path on every search
the fixture marks ok (no deciding comparison within 1e-6 relative of a tie: the built-in sums the objective in
another order than the reference).  Behind an orthogonalisation the whole of v must be the record's bit for bit
(it depends on the state alone).  x[i], d[i] and stepi are held bit for bit to the model's arithmetic: the
interpolated step is a continuous function of the four values fs and the final value, so the model takes the
device's own stored values there ("fs", "fx") -- where they are the reference's bits, as at n = 2, that is the
record itself; imin 0 / 3 and a restored point do not depend on them at all.  The stored values are held to the
bound every built-in form is held to (tests/test_objective_forms_gpu.py: objective_reference.reference_at and
ratio <= 1)."""
import copy

import numpy as np
import pytest

import objective_reference as R
import rosenbrock_model as rm
from test_rosenbrock_model import GOLDEN, GOOD_OK, at_window, guess_of, search_record

pytestmark = pytest.mark.gpu


def _bits(a, b, what):
    a, b = np.asarray(a, float).ravel(), np.asarray(b, float).ravel()
    assert a.shape == b.shape, what
    assert a.tobytes() == b.tobytes(), (what, np.flatnonzero(a != b)[:8], a[a != b][:4], b[a != b][:4])


def inject(g, m, p=0):
    """the model's state between searches into population p of the device"""
    g.set_state("x", m.flat(m.x), p)
    g.set_state("v", m.flat(m.v), p)
    g.set_state("d", m.d, p)
    g.set_state("stepi", [m.stepi], p)
    g.set_state("i", [m.i], p)
    g.set_state("fev", [m.fev], p)


def device_of(hip, rec, f=None, **kw):
    par, n = rec["params"], rec["n"]
    g = hip.Rosenbrock(par["mfev"], par["tol"], par["step0"], par["decf"], seed=5, **kw)
    return g, (f or getattr(hip.objectives, rec["objective"])), -5. * np.ones(n), 5. * np.ones(n)


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
@pytest.mark.parametrize("rec", GOLDEN["steps"], ids=lambda r: r["name"])
def test_one_search_from_every_recorded_state(hip, rec, wide):
    n, obj = rec["n"], rec["objective"]
    g, f, lo, up = device_of(hip, rec, wide=wide)
    g.initialize(f, lo, up, guess_of(rec))
    assert int(g.get_state("wide")[0]) == int(wide) and int(g.get_state("fev")[0]) == 0
    m = at_window(rec)
    worst, held, orths = 0., 0, 0
    for k, st in enumerate(rec["states"]):
        tag = "%s search %d: " % (rec["name"], rec["skip"] + k)
        inject(g, m)
        dev = copy.deepcopy(m)          # the model that takes the device's values at the interpolation
        m.evals, i0 = [], m.i
        m.iterate()
        assert search_record(m, i0) == st, tag + "the model left the record"
        g.iterate()
        if not st["ok"]:
            continue
        held += 1
        got = (int(g.get_state("i")[0]), int(g.get_state("fev")[0]), [int(q) for q in g.get_state("path")],
               int(g.get_state("orth")[0]))
        assert got == (st["i1"], st["fev"], st["path"], st["orth"]), tag
        fs, fx = g.get_state("fs"), float(g.get_state("fx")[0])
        dev.evals, dev.fs_override = [], [float(q) for q in fs]
        dev.final_override = fx if st["path"][3] in (rm.KEPT, rm.RESTORED) else None
        dev.iterate()
        assert dev.path == st["path"] and dev.i == st["i1"], tag + "the device's values decide as the reference's"
        X, V, D = g.get_state("x").reshape(n + 2, n), g.get_state("v").reshape(n + 2, n), g.get_state("d")
        _bits(X[i0], dev.x[i0], tag + "x[i]")
        _bits(D[i0], dev.d[i0], tag + "d[i]")
        _bits(g.get_state("stepi"), [float.fromhex(st["stepi"])], tag + "stepi")
        _bits(X, dev.x, tag + "x")
        _bits(D, dev.d, tag + "d")
        if list(fs) == m.fs and (dev.final_override is None or fx == m.evals[-1][1]):
            assert [rm.crc(X.ravel()), rm.crc(V.ravel()), rm.crc(D)] == st["state_crc"], tag + "the record itself"
        if st["orth"]:
            orths += 1
            _bits(V, m.v, tag + "v behind the orthogonalisation")
            assert rm.crc(V.ravel()) == st["state_crc"][1]
        else:
            _bits(V, dev.v, tag + "v")
        # the stored values against the extended-precision reference at their points
        final = st["path"][3] in (rm.KEPT, rm.RESTORED)
        pts = [e[0] for e in (m.evals[-5:-1] if final else m.evals[-4:])]
        pairs = list(zip(pts, fs)) + ([(dev.evals[-1][0], fx)] if final else [])
        for x, v in pairs:
            r = R.ratio(v, *R.reference_at(obj, x))
            worst = max(worst, r)
            assert r <= 1., tag + "the value %r is %.4g bounds from the reference at its point" % (v, r)
    assert held >= GOOD_OK
    assert orths == sum(s["orth"] and s["ok"] for s in rec["states"])
    print("RATIO Rosenbrock %s %s: %.3f over %d searches" % (rec["name"], "wide" if wide else "narrow", worst, held))


def test_the_orthogonalisation_is_met_at_every_size():
    assert {r["n"] for r in GOLDEN["steps"] if any(s["orth"] and s["ok"] for s in r["states"])} >= {2, 17, 33, 128}
