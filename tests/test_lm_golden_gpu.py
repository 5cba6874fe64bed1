"""GPU: LmCMAES fed the reference's own draws against the recorded reference
(tests/golden/lm_runs.json, "steps").

The device takes the recorded guess and, for all generations of a run at once, the recorded draws
through inject_draws; at each recorded generation its state is held against the fixture relative to
the largest entry of the key.  fit_idx, jarr, larr, memlen, it, fev and the stop state must be
exactly equal.  Bounds: 1e-11 at generation 1 and 1e-10 at generations 2-3, as
tests/test_chol_golden_gpu.py and tests/test_cma_golden_gpu.py hold for the same kind of comparison.
For the later generations the bound is 100 x the largest deviation of the model's device form from
the reference (tests/test_lm_model.py measures 7.3e-15: the two differ in summation order only, two
decades cover the device's own exp and fused reductions), but not below 1e-10: that floor is the
bound, LATE_BOUND = 1e-10.  The generations alternate between iterate(), run(1) and the five
phases.

Measured on an MI355X over the five runs: 3.6e-16 at most at generation 1, 1.9e-15 at generations
2-3, 7.3e-15 later (n16_l12_rad, generation 17, s)."""
import numpy as np
import pytest

from test_lm_model import GOLD, INT_KEYS, KEYS, draws_of, recorded, unpack

pytestmark = pytest.mark.gpu

FIRST_BOUND, EARLY_BOUND, LATE_BOUND = 1e-11, 1e-10, 1e-10
assert LATE_BOUND >= 100 * 7.3e-15


def bound_of(gen):
    return FIRST_BOUND if gen == 1 else EARLY_BOUND if gen <= 3 else LATE_BOUND


@pytest.mark.parametrize("rec", GOLD["steps"], ids=[r["name"] for r in GOLD["steps"]])
def test_injected_reference_draws_reproduce_reference_states(hip, rec):
    n, lam, box = rec["n"], rec["lambda"], rec["box"]
    g = hip.LmCMAES(rec["mfev"], rec["tol"], lam, 0, rec["sigma0"], bool(rec["bound"]), bool(rec["rademacher"]),
                    bool(rec["usenew"]), seed=5)
    g.initialize(rec["objective"], -box * np.ones(n), box * np.ones(n), unpack(rec["guess"]))
    assert [int(g.get_state(k)[0]) for k in ("memory", "t", "nsteps")] == [rec["memory"], rec["t"], rec["nsteps"]]
    g.inject_draws(np.array([draws_of(rec, st) for st in rec["states"]]))
    worst = {}
    for st in rec["states"]:
        gen = st["gen"]
        if gen % 3 == 0:
            g.iterate()
        elif gen % 3 == 1:
            assert g.run(1) == 1
        else:
            for ph in range(5):
                g.phase(ph)
        assert int(g.get_state("it")[0]) == st["it"] == gen
        if gen not in rec["recorded"]:
            continue
        memlen = int(g.get_state("memlen")[0])
        for k in KEYS:
            want = recorded(st, k, n)
            have = g.get_state(k)
            if k in ("pcmat", "vmat"):
                assert not have[memlen * n:].any(), (k, gen)
                have = have[:memlen * n]
            tag = "%s generation %d %s" % (rec["name"], gen, k)
            assert have.shape == want.shape, tag
            if k in INT_KEYS:
                assert np.array_equal(have, want), (tag, have, want)
                continue
            err = float(np.abs(have - want).max() / max(np.abs(want).max(), 1e-300))
            print("%-40s %.3e" % (tag, err))
            worst[gen] = max(worst.get(gen, 0.), err)
            assert err <= bound_of(gen), (tag, err)
        assert int(g.get_state("stop")[0]) == (1 if st["flag"] else 0)
        assert g.solution().converged is bool(st["flag"]) and g.solution().n_evals == st["fev"]
    print("%s: worst relative deviation from the reference per recorded generation: %s"
          % (rec["name"], ", ".join("%d: %.2e" % kv for kv in sorted(worst.items()))))
    with pytest.raises(Exception, match="used up"):
        g.iterate()     # the table is consumed: no silent return to the generator
    g.inject_draws(None)
    g.iterate()         # back on the device generator
    assert int(g.get_state("it")[0]) == len(rec["states"]) + 1
