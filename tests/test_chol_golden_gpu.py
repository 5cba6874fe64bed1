"""GPU <-> REFERENCE directly for CholeskyCMAES (tests/golden/chol_runs.json was written by the
compiled reference, scripts/gen_chol_golden.py): the reference's own normals of its first three
generations are injected into the device and the device's state after each generation is held
against the reference's recorded state.

Tolerance: 1e-11 relative to the largest entry in generation 1 (A = I: pure GEMM / reduction
rounding), 1e-10 in generations 2-3 -- what tests/test_cma_golden_gpu.py holds for the same
comparison through an eigendecomposition; factoring C = I + O(0.1) is better conditioned."""
import numpy as np
import pytest

from _golden import load, unhex

pytestmark = pytest.mark.gpu

STEPS = load("chol_runs.json")["steps"]


def _close(a, b, rtol, what):
    a, b = np.asarray(a), np.asarray(b)
    scale = max(np.abs(b).max(), 1e-300)
    err = np.abs(a - b).max() / scale
    print("%s: rel err %.3e" % (what, err))
    assert err <= rtol, "%s: rel err %.3e > %.1e" % (what, err, rtol)


@pytest.mark.parametrize("idx", range(len(STEPS)))
def test_injected_reference_normals_reproduce_reference_states(hip, idx):
    rec = STEPS[idx]
    n, lam, box = rec["n"], rec["lambda"], rec["box"]
    g = hip.CholeskyCMAES(rec["mfev"], rec["tol"], rec["stol"], lam, rec["sigma0"],
                          bool(rec["bound"]), seed=1)
    g.initialize(getattr(hip.objectives, rec["objective"]), -box * np.ones(n), box * np.ones(n),
                 unhex(rec["guess"]))
    for st in rec["states"]:
        gen = st["gen"]
        g.inject_normals(unhex(st["normals"]))
        g.iterate()
        tol = 1e-11 if gen == 1 else 1e-10
        for key in ("arx", "xmean", "sigma", "pc", "ps", "A", "fit_val"):
            _close(g.get_state(key), unhex(st[key]), tol, "%s gen %d %s" % (rec["name"], gen, key))
        np.testing.assert_array_equal(g.get_state("fit_idx"), unhex(st["fit_idx"]))
        assert int(g.get_state("it")[0]) == st["it"]
        assert int(g.get_state("fev")[0]) == st["fev"]
        assert (int(g.get_state("flag")[0]) == 11) == bool(st["converged"])
        A = g.get_state("A").reshape(n, n)
        assert (np.triu(A, 1) == 0.).all() and (np.diag(A) > 0.).all()
        assert int(g.get_state("chol_repairs")[0]) == 0
    g.inject_normals(None)
