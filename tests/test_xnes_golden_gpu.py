"""GPU: xNES fed the reference's own draws against the recorded reference
(tests/golden/xnes_runs.json, "steps": n = 2, 5, 12 on the dense route, n = 33 on the low-rank one).

The device takes, for all generations of a run at once, the recorded draws through inject_normals;
at each recorded generation its state is held against the fixture relative to the largest entry of
the key (arx and fit_val in the reference's ranked order).  fit_idx, it and fev must be equal.  The
generations alternate between iterate(), run(1) and the four phases.

The bound follows the rule of tests/test_xnes_model.py: the next power of ten at least 100 times
above the largest deviation measured, capped at the project's 1e-9.  Measured on an MI355X over the
four runs: 2.2e-14 (n12_ellipsoid, generation 12, fit_val; per run 2.4e-15, 1.4e-14, 2.2e-14 and
2.6e-15), so BOUND = 1e-11."""
import numpy as np
import pytest

from test_xnes_model import FLOAT_KEYS, GOLD, unpack

pytestmark = pytest.mark.gpu

MEASURED = 2.2e-14
BOUND = 1e-11
assert 100 * MEASURED <= BOUND <= 1e-9


@pytest.mark.parametrize("rec", GOLD["steps"], ids=[r["name"] for r in GOLD["steps"]])
def test_injected_reference_draws_reproduce_reference_states(hip, rec):
    n, np_ = rec["n"], rec["np"]
    g = hip.xNES(10 ** 9, 0., rec["a0"], rec["etamu"], seed=5)
    g.initialize(rec["objective"], -5. * np.ones(n), 5. * np.ones(n), np.zeros(n))
    assert int(g.get_state("np")[0]) == np_
    assert int(g.get_state("route")[0]) == (1 if n >= 32 else 0)
    g.inject_normals(np.array([unpack(st["z"]) for st in rec["states"]]))
    worst = {}
    for st in rec["states"]:
        gen = st["gen"]
        if gen % 3 == 0:
            g.iterate()
        elif gen % 3 == 1:
            assert g.run(1) == 1
        else:
            for ph in range(4):
                g.phase(ph)
        assert int(g.get_state("it")[0]) == gen
        if gen not in rec["recorded"]:
            continue
        idx = g.get_state("fit_idx").astype(int)
        assert idx.tolist() == st["fit_idx"], gen
        assert int(g.get_state("fev")[0]) == st["fev"] and st["it"] == gen
        for k in FLOAT_KEYS:
            want, have = unpack(st[k]), g.get_state(k)
            if k == "arx":
                have = have.reshape(np_, n)[idx].ravel()
            elif k == "fit_val":
                have = have[idx]
            tag = "%s generation %d %s" % (rec["name"], gen, k)
            assert have.shape == want.shape, tag
            err = float(np.abs(have - want).max() / max(np.abs(want).max(), 1e-300))
            print("%-40s %.3e" % (tag, err))
            worst[gen] = max(worst.get(gen, 0.), err)
            assert err <= BOUND, (tag, err)
        assert g.solution().n_evals == st["fev"]
        assert g.solution().x.tobytes() == g.get_state("arx").reshape(np_, n)[idx[0]].tobytes()
    print("%s: worst relative deviation from the reference per recorded generation: %s"
          % (rec["name"], ", ".join("%d: %.2e" % kv for kv in sorted(worst.items()))))
    with pytest.raises(Exception, match="used up"):
        g.iterate()     # the table is consumed: no silent return to the generator
