"""GPU: NSHS fed the reference's own initial memory and uniforms against the recorded reference
(tests/golden/nshs_runs.json, "steps").

The device takes the recorded initial memory through set_state("x") (which re-evaluates it and
re-selects fstd, the best and the worst) and, per iteration, the uniforms the reference made of its
recorded mt19937 words through inject_uniforms; a value the reference did not draw is padded with
0.5 and never used.  After each of the 12 recorded iterations the memory and the candidate are the
reference's BIT FOR BIT (every operation of the improvisation is one IEEE operation in the
reference's order); the values f and fcand are held at 1e-10 relative -- the constant of
tests/test_spiral_golden_gpu.py, tests/test_hees_golden_gpu.py and tests/test_chol_golden_gpu.py for
an objective summed in another order; fstd, which the device forms in two passes over a tree sum,
within FSTD_BOUND of tests/test_nshs_model.py (3.1e-14, a hundred times what the two forms differ
by on the same values); ibest, iworst, it and fev are equal.  The odd iterations run through the
three phase kernels, the even ones through the fused kernel.

Measured on an MI355X over the 10 runs: f deviates by 2.6e-16 at most, fstd by 3.7e-16."""
import numpy as np
import pytest

import jaya_model as jm
import nshs_model as nm
from test_nshs_model import FSTD_BOUND, GOLD, PERCOORD, _h, box_of

pytestmark = pytest.mark.gpu

RTOL = 1e-10


def _close(a, b, what, rtol=RTOL):
    a, b = np.asarray(a, float).ravel(), np.asarray(b, float).ravel()
    assert a.shape == b.shape, what
    err = float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))
    assert err <= rtol, (what, err)
    return err


def _bits(a, b, what):
    a, b = np.asarray(a, float).ravel(), np.asarray(b, float).ravel()
    assert a.shape == b.shape, what
    assert a.tobytes() == b.tobytes(), (what, np.flatnonzero(a != b)[:8], a[a != b][:4], b[a != b][:4])


def _fstd_close(g, st, tag):
    ref = float.fromhex(st["fstd"])
    err = abs(float(g.get_state("fstd")[0]) - ref) / ref
    assert err <= FSTD_BOUND, (tag, err)
    return err


# (the last record: bounds that differ in every coordinate, tests/golden/nshs_percoord.json)
@pytest.mark.parametrize("rec", GOLD["steps"] + PERCOORD["steps"],
                         ids=[r["name"] for r in GOLD["steps"] + PERCOORD["steps"]])
def test_injected_reference_uniforms_reproduce_reference_states(hip, rec):
    n, hms = rec["n"], rec["hms"]
    lo, up = (np.asarray(v, float) for v in box_of(rec))
    g = hip.NSHS(rec["mfev"], hms, rec["fstdmin"], seed=5)
    g.initialize(rec["objective"], lo, up, np.zeros(n))
    ini = rec["init"]
    g.set_state("x", _h(ini["x"]))
    assert int(g.get_state("fev")[0]) == ini["fev"] == hms and int(g.get_state("it")[0]) == 0
    assert int(g.get_state("ibest")[0]) == ini["ibest"] and int(g.get_state("iworst")[0]) == ini["iworst"]
    worst_f = _close(g.get_state("f"), _h(ini["f"]), "init f")
    worst_s = _fstd_close(g, ini, "init fstd")
    hmcr = float(g.get_state("hmcr")[0])
    assert hmcr == 1.0 - 1.0 / (n + 1)
    for it, st in enumerate(rec["states"], 1):
        w = jm.Words(st["words"])
        u = nm.uniforms_of(w, n, hms, hmcr)
        assert w.exhausted()
        g.inject_uniforms(u)
        assert int(g.get_state("wide")[0]) == int(rec["wide"])
        if it % 2:
            g.iterate()
        else:
            assert g.run(1) == 1
        tag = "%s iteration %d " % (rec["name"], it)
        _bits(g.get_state("cand"), _h(st["cand"]), tag + "cand")
        _bits(g.get_state("x"), _h(st["x"]), tag + "x")
        ferr = max(_close(g.get_state("f"), _h(st["f"]), tag + "f"),
                   _close(g.get_state("fcand"), [float.fromhex(st["fcand"])], tag + "fcand"))
        worst_f = max(worst_f, ferr)
        worst_s = max(worst_s, _fstd_close(g, st, tag + "fstd"))
        got = [int(g.get_state(k)[0]) for k in ("ibest", "iworst", "it", "fev")]
        assert got == [st["ibest"], st["iworst"], st["it"], st["fev"]], (tag, got)
        assert g.solution().converged is False and int(g.get_state("flag")[0]) == 0, tag
    print("%s: worst relative deviation from the reference over 12 iterations: f %.3e, fstd %.3e"
          % (rec["name"], worst_f, worst_s))
    g.inject_uniforms(None)
    g.iterate()     # back on the device generator
    assert int(g.get_state("it")[0]) == len(rec["states"]) + 1
