"""GPU: SpiralSearch fed the reference's own initial points and uniforms against the recorded
reference (tests/golden/spiral_runs.json, "steps").

The device takes the recorded initial points through set_state("x") (which re-evaluates them and
re-selects the best) and, per generation, the uniforms the reference made of its recorded mt19937
words through inject_uniforms; a conditional value the reference did not draw is padded with 0.5
and never used.  After each of the 4 recorded generations the points, their values, xbest, rs and
thetas are held against the reference's at 1e-10 relative to the largest entry -- the constant of
tests/test_hees_golden_gpu.py and tests/test_chol_golden_gpu.py for the same comparison: the device
rotates the difference x_i - xbest once (tests/test_spiral_model.py measures 3.1e-15 between the two
forms) and its cos and sin may differ from libm's in the last place.  ibest, fev and it must be
equal.

Measured on an MI355X: the worst deviation over the 12 runs is 3.1e-15 (bound 1e-10)."""
import numpy as np
import pytest

import jaya_model as jm
import spiral_model as sm
from test_spiral_model import GOLD, _h

pytestmark = pytest.mark.gpu

RTOL = 1e-10


def _close(a, b, what):
    a, b = np.asarray(a, float).ravel(), np.asarray(b, float).ravel()
    assert a.shape == b.shape, what
    err = float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))
    assert err <= RTOL, (what, err)
    return err


@pytest.mark.parametrize("rec", GOLD["steps"], ids=[r["name"] for r in GOLD["steps"]])
def test_injected_reference_uniforms_reproduce_reference_states(hip, rec):
    n, np_ = rec["n"], rec["np"]
    lo, up = -rec["box"] * np.ones(n), rec["box"] * np.ones(n)
    g = hip.SpiralSearch(1000000, 0., np_, taur=rec["taur"], tautheta=rec["tautheta"], seed=5)
    g.initialize(rec["objective"], lo, up, np.zeros(n))
    ini = rec["init"]
    g.set_state("x", _h(ini["x"]))
    assert int(g.get_state("fev")[0]) == ini["fev"] == np_ and int(g.get_state("it")[0]) == 0
    assert int(g.get_state("ibest")[0]) == ini["ibest"]
    worst = max(_close(g.get_state("f"), _h(ini["f"]), "init f"),
                _close(g.get_state("xbest"), _h(ini["xbest"]), "init xbest"))
    assert g.get_state("r").tobytes() == _h(ini["rs"]).tobytes()
    assert g.get_state("theta").tobytes() == _h(ini["thetas"]).tobytes()
    for gen, st in enumerate(rec["states"], 1):
        w = jm.Words(st["words"])
        u = sm.uniforms_of(w, np_, rec["taur"], rec["tautheta"])
        assert w.exhausted()
        g.inject_uniforms(u)
        g.iterate()
        tag = "%s gen %d " % (rec["name"], gen)
        errs = [
            _close(g.get_state("x"), _h(st["x"]), tag + "x"),
            _close(g.get_state("f"), _h(st["f"]), tag + "f"),
            _close(g.get_state("xbest"), _h(st["xbest"]), tag + "xbest"),
            _close(g.get_state("r"), _h(st["rs"]), tag + "rs"),
            _close(g.get_state("theta"), _h(st["thetas"]), tag + "thetas"),
        ]
        worst = max(worst, max(errs))
        assert int(g.get_state("ibest")[0]) == st["ibest"], tag + "ibest"
        assert int(g.get_state("it")[0]) == gen and int(g.get_state("fev")[0]) == st["fev"], tag
        assert g.solution().converged is False and int(g.get_state("flag")[0]) == 0, tag
    print("%s: worst relative deviation from the reference over 4 generations %.3e" % (rec["name"], worst))
    g.inject_uniforms(None)
    g.iterate()     # back on the device generator
    assert int(g.get_state("it")[0]) == len(rec["states"]) + 1
