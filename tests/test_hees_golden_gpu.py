"""GPU: HEES fed the reference's own normals against the recorded reference
(tests/golden/hees_runs.json, "steps").

The normals of a generation are what the reference's polar method made of the recorded mt19937
words (jaya_model.Words.normal, its spare value carried from generation to generation); the device
takes the full (B n) x n table and uses its first mu rows.  After each of the 4 recorded
generations the state is held against the reference's at 1e-10 relative to the largest entry -- the
constant of tests/test_chol_golden_gpu.py for the same comparison; the device's low-rank update of
A and its tree reductions differ from the reference's serial sums by reduction order alone
(tests/test_hees_model.py measures 6e-12 at most between the two forms).  The ranking, `it`, `fev`
and converged() must be equal."""
import numpy as np
import pytest

import jaya_model as jm
from test_hees_model import GOLD, _h

pytestmark = pytest.mark.gpu

RTOL = 1e-10


def _close(a, b, what):
    a, b = np.asarray(a, float).ravel(), np.asarray(b, float).ravel()
    assert a.shape == b.shape, what
    err = float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))
    assert err <= RTOL, (what, err)
    return err


@pytest.mark.parametrize("rec", GOLD["steps"], ids=[r["name"] for r in GOLD["steps"]])
def test_injected_reference_normals_reproduce_reference_states(hip, rec):
    n = rec["n"]
    lo, up = -rec["box"] * np.ones(n), rec["box"] * np.ones(n)
    g = hip.HEES(1000000, rec["tol"], np=rec["np"], sigma0=rec["sigma0"], seed=5)
    g.initialize(rec["objective"], lo, up, _h(rec["guess"]))
    ini = rec["init"]
    mu, B = ini["mu"], ini["B"]
    assert (int(g.get_state("mu")[0]), int(g.get_state("B")[0])) == (mu, B)
    assert int(g.get_state("fev")[0]) == ini["fev"] == 1 and int(g.get_state("it")[0]) == 0
    _close(g.get_state("fm"), _h(ini["scalars"])[2:3], "init fm")
    _close(g.get_state("fbest"), _h(ini["scalars"])[3:4], "init fbest")
    assert g.solution().converged is bool(ini["converged"]) is True
    have, saved, worst = False, 0., 0.
    for gen, st in enumerate(rec["states"], 1):
        w = jm.Words(st["words"])
        w.have, w.saved = have, saved
        z = np.array([[w.normal() for _ in range(n)] for _ in range(B * n)])
        assert w.exhausted()
        have, saved = w.have, w.saved
        g.inject_normals(z)
        g.iterate()
        tag = "%s gen %d " % (rec["name"], gen)
        sc = _h(st["scalars"])
        errs = [
            _close(g.get_state("A"), _h(st["A"]), tag + "A"),
            _close(g.get_state("xmean"), _h(st["xmean"]), tag + "xmean"),
            _close(g.get_state("ps"), _h(st["ps"]), tag + "ps"),
            _close(g.get_state("b"), _h(st["b"])[:mu * n], tag + "b"),
            _close(g.get_state("norms"), _h(st["norms"])[:mu], tag + "norms"),
            _close(g.get_state("arx"), _h(st["x"]), tag + "arx"),
            _close(g.get_state("fit_val"), _h(st["fit_val"]), tag + "fit_val"),
            _close(g.get_state("hess"), _h(st["hess"]), tag + "hess"),
            _close(g.get_state("q"), _h(st["q"]), tag + "q"),
            _close(g.get_state("xbest"), _h(st["xbest"]), tag + "xbest"),
            _close(g.get_state("sigma"), sc[0:1], tag + "sigma"),
            _close(g.get_state("gs"), sc[1:2], tag + "gs"),
            _close(g.get_state("fm"), sc[2:3], tag + "fm"),
            _close(g.get_state("fbest"), sc[3:4], tag + "fbest"),
        ]
        worst = max(worst, max(errs))
        order = sorted(range(2 * mu), key=lambda i: st["rank"][i])
        assert g.get_state("fit_idx").astype(int).tolist() == order, tag + "fit_idx"
        assert int(g.get_state("it")[0]) == gen and int(g.get_state("fev")[0]) == st["fev"], tag
        assert g.solution().converged is bool(st["converged"]), tag
        assert int(g.get_state("flag")[0]) == (1 if st["converged"] else 0), tag
    print("%s: worst relative deviation from the reference over 4 generations %.3e" % (rec["name"], worst))
    g.inject_normals(None)
    g.iterate()     # back on the device generator
    assert int(g.get_state("it")[0]) == len(rec["states"]) + 1
