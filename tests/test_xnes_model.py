"""CPU: tests/xnes_model.py against the recorded reference (tests/golden/xnes_runs.json) and its two
forms against each other.

Form (a) of the model, the reference's order, replays the recorded draws and must hold every
recorded state; it differs from the real class only by eigh against tred2 / tql2 and by NumPy's
sums.  Measured over all recorded states, relative to the largest entry of the key: 1.6e-14
(n12_ellipsoid, generation 12, fit_val); the bound REFERENCE_FORM_BOUND = 1e-11 is the next power of
ten at least 100 times above that.

Form (b), the device's form, against form (a) under the same draws at n = 16, 31, 32, 33, 64 over 40
generations: measured 9.0e-14 (n = 31, generation 3, gsigma, a sum that cancels), bound
DEVICE_FORM_BOUND = 1e-11 by the same rule; the rankings are identical.  The two routes of form (b)
against each other at n = 24: measured 1.9e-14, the same bound."""
import base64

import numpy as np
import pytest

import chol_model
import xnes_model as xm
from _golden import load

GOLD = load("xnes_runs.json")
STEPS = {s["name"]: s for s in GOLD["steps"]}
FLOAT_KEYS = ("arx", "fit_val", "xmean", "sigma", "gsigma", "B")
REFERENCE_FORM_BOUND = 1e-11
DEVICE_FORM_BOUND = 1e-11
CAP = 1e-9


def unpack(s):
    """an array of the fixture: base64 of little-endian IEEE doubles"""
    return np.frombuffer(base64.b64decode(s), dtype="<f8").astype(np.float64)


def rel(a, b):
    a, b = np.asarray(a, float).ravel(), np.asarray(b, float).ravel()
    assert a.shape == b.shape
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def model_state(m, key):
    """the model's state under the fixture's names: arx and fit_val ranked, as the reference holds them"""
    o = m.order
    return {"arx": m.x[o], "fit_val": m.f[o], "xmean": m.mu, "sigma": [m.sigma], "gsigma": [m.gsigma],
            "B": m.B}[key]


def model_of(rec, frows=None, **kw):
    n = rec["n"]
    return xm.XNes(frows or chol_model.objective_rows(rec["objective"], n), n, rec["a0"], rec["etamu"], **kw).init()


def test_bounds_respect_the_cap():
    assert REFERENCE_FORM_BOUND <= CAP and DEVICE_FORM_BOUND <= CAP


@pytest.mark.parametrize("name", list(STEPS))
def test_reference_form_reproduces_the_recorded_states(name):
    rec = STEPS[name]
    n, np_ = rec["n"], rec["np"]
    m = model_of(rec)
    assert m.np == np_ == xm.popsize(n)
    worst, seen = (-1., (0, "")), 0
    for st in rec["states"]:
        m.iterate_reference(unpack(st["z"]).reshape(np_, n))
        if st["gen"] not in rec["recorded"]:
            continue
        seen += 1
        assert m.order == st["fit_idx"], st["gen"]
        assert m.it == st["it"] == st["gen"] and m.fev == st["fev"] == st["gen"] * np_
        for key in FLOAT_KEYS:
            err = rel(model_state(m, key), unpack(st[key]))
            worst = max(worst, (err, (st["gen"], key)))
            assert err <= REFERENCE_FORM_BOUND, (key, st["gen"], err)
    assert seen == len(rec["recorded"])
    print("%s: worst relative deviation of form (a) from the recorded reference %.3e at %s" % ((name,) + worst))


def _pair(n, gens, obj, seed, **kw):
    """form (a) and form (b) under the same draws; the worst deviation of (b) from (a)"""
    f = xm.device_objective(obj, n)
    a = xm.XNes(f, n).init()
    b = xm.XNes(f, n, **kw).init()
    rng = np.random.default_rng(seed)
    worst = (-1., (0, ""))
    for gen in range(1, gens + 1):
        z = rng.standard_normal((a.np, n))
        a.iterate_reference(z)
        b.iterate_device(z)
        assert a.order == b.order, (n, gen)
        for key in FLOAT_KEYS:
            err = rel(model_state(b, key), model_state(a, key))
            worst = max(worst, (err, (gen, key)))
    assert b.fact_fail == 0
    return worst, b


@pytest.mark.parametrize("n", [16, 31, 32, 33, 64])
def test_device_form_against_reference_form(n):
    worst, b = _pair(n, 40, ["rosenbrock", "ellipsoid"][n % 2], 7000 + n)
    assert b.route == (1 if n >= 32 else 0)
    print("n = %d (route %d): worst relative deviation of form (b) from form (a) over 40 generations %.3e at %s"
          % ((n, b.route) + worst))
    assert worst[0] <= DEVICE_FORM_BOUND


def test_the_two_routes_of_the_device_form_agree_at_n24():
    n = 24
    f = xm.device_objective("rosenbrock", n)
    lo = xm.XNes(f, n, lowrank_min_n=16).init()
    de = xm.XNes(f, n).init()
    assert (lo.route, de.route) == (1, 0)
    rng = np.random.default_rng(24)
    worst = (-1., (0, ""))
    for gen in range(1, 41):
        z = rng.standard_normal((lo.np, n))
        lo.iterate_device(z)
        de.iterate_device(z)
        assert lo.order == de.order, gen
        for key in FLOAT_KEYS:
            worst = max(worst, (rel(model_state(lo, key), model_state(de, key)), (gen, key)))
    print("n = 24: worst relative deviation between the routes of form (b) over 40 generations %.3e at %s" % worst)
    assert lo.fact_fail == 0 and worst[0] <= DEVICE_FORM_BOUND


def test_equal_rows_fail_the_factorisation_and_leave_B():
    n = 64
    m = xm.XNes(xm.device_objective("sphere", n), n).init()
    rng = np.random.default_rng(5)
    m.iterate_device(rng.standard_normal((m.np, n)))
    B0 = m.B.copy()
    z = rng.standard_normal((m.np, n))
    z[7] = z[3]
    m.iterate_device(z)
    assert m.fact_fail == 1 and m.skipped and (m.B == B0).all() and np.isfinite(m.mu).all()


def test_the_utilities_sum_to_zero_and_the_run_loop_overshoots_to_a_multiple_of_np():
    n = 10
    rng = np.random.default_rng(1)
    m = xm.XNes(xm.device_objective("rosenbrock", n), n, tol=1e-8, mfev=505).init()
    assert abs(m.u.sum()) < 1e-15 and m.np == 10
    xm.run(m, lambda gen: rng.standard_normal((m.np, n)))
    assert m.fev == 510 and m.stop == 2 and not m.conv
