"""GPU: the AMALGAM kernels against the states recorded from the reference
(tests/golden/amalgam_runs.json), under injected initial points, normals and shifted rows (the points and the first normals regenerated
from the recorded seed, tests/amalgam_model.py).

The generations alternate between iterate(), run(1) and the three phases.  fit_idx, t, fev and nis are
equal.  Floats are relative to the key's largest entry, under the bound rule of
tests/test_amalgam_model.py: the next power of ten at least 100 times the largest deviation measured,
capped at 1e-9.  Measured on an MI355X over all recorded states: 7.5e-15 at most (n2_iamalgam,
generation 5, fit_val: Rosenbrock's sum in the device's order), so BOUND = 1e-12."""
import base64

import numpy as np
import pytest

import amalgam_model as am
from _golden import load

pytestmark = pytest.mark.gpu

GOLD = load("amalgam_runs.json")
STEPS = {s["name"]: s for s in GOLD["steps"]}
FLOAT_KEYS = ("arx", "fit_val", "mu", "mushift", "cov", "chol", "cmult")
BOUND = 1e-12


def unpack(s):
    return np.frombuffer(base64.b64decode(s), dtype="<f8").astype(np.float64)


def rel(a, b):
    a, b = np.asarray(a, float).ravel(), np.asarray(b, float).ravel()
    assert a.shape == b.shape
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("name", list(STEPS))
def test_device_reproduces_the_recorded_states(hip, name):
    rec = STEPS[name]
    n, np_, nams = rec["n"], rec["np"], rec["nams"]
    g = hip.AMALGAM(10 ** 9, 0., 0., 0, bool(rec["iamalgam"]), False, False, seed=3)
    x0, zs = am.fixture_draws(rec, unpack)
    g.inject_points(x0)
    g.initialize(rec["objective"], -5. * np.ones(n), 5. * np.ones(n), np.zeros(n))
    assert [int(g.get_state(k)[0]) for k in ("np", "ss", "nams")] == [np_, rec["ss"], nams]
    assert float(g.get_state("etasigma")[0]) == float.fromhex(rec["etasigma"])
    assert float(g.get_state("etashift")[0]) == float.fromhex(rec["etashift"])
    worst = (-1., "")
    for key, want in (("mu", rec["mu0"]), ("cov", rec["cov0"])):
        err = rel(g.get_state(key), unpack(want))
        worst = max(worst, (err, key + " after init"))
        assert err <= BOUND, (key, err)
    assert g.get_state("fit_idx").astype(int).tolist() == list(range(np_)) and int(g.get_state("fev")[0]) == np_
    z = np.array(zs)
    rows = np.array([st["perm"][1:nams + 1] for st in rec["states"]], dtype=np.int32)
    g.inject_draws(z, rows)
    seen = 0
    for st in rec["states"]:
        how = st["gen"] % 3
        if how == 1:
            g.iterate()
        elif how == 2:
            assert g.run(1) == 1
        else:
            for ph in range(3):
                g.phase(ph)
        assert sorted(np.flatnonzero(g.get_state("shifted")).tolist()) == sorted(st["perm"][1:nams + 1])
        if st["gen"] not in rec["recorded"]:
            continue
        seen += 1
        assert g.get_state("fit_idx").astype(int).tolist() == st["fit_idx"], st["gen"]
        assert [int(g.get_state(k)[0]) for k in ("t", "fev", "nis")] == [st["t"], st["fev"], st["nis"]]
        for key in FLOAT_KEYS:
            if key not in st:       # (arx is recorded up to n = 5)
                continue
            err = rel(g.get_state(key), unpack(st[key]))
            worst = max(worst, (err, "%s generation %d" % (key, st["gen"])))
            assert err <= BOUND, (key, st["gen"], err)
    assert seen == len(rec["recorded"])
    print("%s: worst relative deviation of the device from the recorded reference %.3e (%s)" % ((name,) + worst))
    with pytest.raises(Exception, match="used up"):
        g.iterate()
