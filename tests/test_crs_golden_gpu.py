"""GPU: CRS against the recorded reference (tests/golden/crs_runs.json).

Per recorded shape the device starts from the reference's initial pool (set_state("x")) and every
iteration is fed the reference's own draws: the model reads the recorded mt19937 words and logs them as
the records of bbo_crs_inject_draws.  After each iteration the row that changed, "cand", "cand2" and
"order" must be the reference's bit for bit -- every operation that forms them is one IEEE operation in
the reference's order -- and fev, the trials, the deepest stack and the stale count must be equal.  The
values hold within 1e-10 relative, the constant of the other golden GPU tests for an objective summed in
another order.  Odd iterations go through bbo_crs_phase, even ones through the fused kernel.

Worst relative deviation of a value measured on an MI355X (the test prints it): 3.5e-16 (n9_np20), 2.3e-16
at n = 17, 2.2e-16 at n = 5 and 2.1e-16 at n = 3, and 0 on the two one-term shapes (n = 1 and n = 2)."""
import numpy as np
import pytest

import crs_model as cm
import jaya_model as jm
from test_crs_model import STEPS, _h, expand, start_model

pytestmark = pytest.mark.gpu

RTOL = 1e-10


def _bits(a, b, what):
    a, b = np.asarray(a, float).ravel(), np.asarray(b, float).ravel()
    assert a.shape == b.shape, what
    assert a.tobytes() == b.tobytes(), (what, np.flatnonzero(a != b)[:8], a[a != b][:4], b[a != b][:4])


class Worst:
    def __init__(self):
        self.v, self.at = 0., ""

    def rel(self, got, want, what):
        got, want = np.asarray(got, float).ravel(), np.asarray(want, float).ravel()
        assert got.shape == want.shape, what
        err = float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300)))
        if err > self.v:
            self.v, self.at = err, what
        return err


@pytest.mark.parametrize("name", sorted(STEPS))
def test_the_device_walks_the_recorded_reference(hip, name):
    rec = STEPS[name]
    n, np_, box = rec["n"], rec["np"], rec["box"]
    m, x0 = start_model(rec)
    m.start(x0)
    g = hip.CRS(rec["mfev"], np_, 0., seed=5)
    g.initialize(rec["objective"], -box * np.ones(n), box * np.ones(n), np.zeros(n))
    g.set_state("x", np.asarray(x0))
    assert [int(v) for v in g.get_state("order")] == list(range(np_)) and int(g.get_state("fev")[0]) == np_
    worst = Worst()
    errs = [worst.rel(g.get_state("f"), _h(rec["init"]["f"]), name + " init f")]
    for k, raw in enumerate(rec["states"]):
        st = expand(raw, n)
        tag = "%s iteration %d " % (name, k)
        w = jm.Words(st["words"])
        assert m.iterate(cm.WordsSource(w, n, np_)) and w.exhausted()
        g.inject_draws(m.records)
        if k % 2:
            pending = g.phase(0)
            while pending:
                g.phase(1)
                pending = g.phase(2)
        else:
            g.iterate()
        assert int(g.get_state("starved")[0]) == 0 and int(g.get_state("irec")[0]) == len(m.records), tag
        x = g.get_state("x").reshape(np_, n)
        _bits(x[st["slot"]], st["trial"], tag + "the row that changed")
        _bits(x, m.x(), tag + "x")
        _bits(g.get_state("cand"), st["trial"], tag + "cand")
        _bits(g.get_state("cand2"), m.t2, tag + "cand2")
        assert [int(v) for v in g.get_state("order")] == m.order, tag + "order"
        errs.append(worst.rel(g.get_state("f"), m.fsorted(), tag + "f"))      # (the reference's: test_crs_model.py)
        errs.append(worst.rel(g.get_state("fcand"), [st["ftrial"]], tag + "fcand"))
        errs.append(worst.rel(g.get_state("fcand2"), [m.ft2], tag + "fcand2"))
        got = [int(g.get_state(key)[0]) for key in ("fev", "trials", "muts", "depth", "maxdepth", "stale", "it", "flag")]
        assert got == [st["fev"], m.trials, m.muts, 0, m.maxdepth, m.stale, k + 1, 0], (tag, got)
    print("%s: worst relative deviation of a value %.3e (%s)" % (name, worst.v, worst.at))
    assert max(errs) <= RTOL, (worst.v, worst.at)
    if (rec["objective"], n) in (("sphere", 1), ("rosenbrock", 2)):
        assert worst.v == 0.       # one term: the same bits, which is why these shapes may hold ties

