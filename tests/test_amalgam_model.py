"""CPU: tests/amalgam_model.py against the recorded reference (tests/golden/amalgam_runs.json) and its
two forms against each other.

The reference form replays the reference's initial points and first normals (regenerated from the
recorded seed by amalgam_model.reference_draws, which the recording script holds to the class bit for
bit), the recorded later normals and the recorded shuffles, and must hold every
recorded state, in both inner modes (iAMaLGaM and AMaLGaM).  The integers (np, ss, nams, fev, t, nis,
the ranking) and the two etas are exact.  Floats: the largest deviation measured over all recorded
states is 0 -- the model's reference form does the reference's operations in its order -- so the rule
(the next power of ten at least 100 times above the measured value, capped at 1e-9) gives no bound
above zero and the states are asserted EQUAL, bit for bit.

The device form against the reference form under the same NumPy draws at n = 16, 17, 33 and 130 over
30 generations, relative to the key's largest entry: measured 1.8e-14 (n = 33,
generation 30, mu), DEVICE_FORM_BOUND = 1e-11 by that rule; the rankings are identical.

The crafted non-positive pivots (n = 8, a rank-5 matrix with 1e-3 taken off the rest of the diagonal;
n = 20, the same at rank 17, so that the failure falls in the second panel of 16): the model's
partial factor equals the recorded one bit for bit.

The parameter-free driver: given the recorded outcomes of the inner runs, the stage sequence, the
budget accounting, the stop and the printed rows of the three recorded runs are exact."""
import base64

import numpy as np
import pytest

import _tabular
import amalgam_model as am
from _golden import load

GOLD = load("amalgam_runs.json")
STEPS = {s["name"]: s for s in GOLD["steps"]}
FLOAT_KEYS = ("arx", "fit_val", "mu", "mushift", "cov", "chol", "cmult")
REFERENCE_FORM_BOUND = 0.
DEVICE_FORM_BOUND = 1e-11
CAP = 1e-9
WIDTHS = [5, 5, 10, 25, 25, 10]


def unpack(s):
    """an array of the fixture: base64 of little-endian IEEE doubles"""
    return np.frombuffer(base64.b64decode(s), dtype="<f8").astype(np.float64)


def rel(a, b):
    a, b = np.asarray(a, float).ravel(), np.asarray(b, float).ravel()
    assert a.shape == b.shape
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def model_state(m, key):
    return {"arx": m.X, "fit_val": m.fit, "mu": m.mu, "mushift": m.mushift, "cov": m.cov, "chol": m.chol,
            "cmult": [m.cmult]}[key]


def model_of(rec, **kw):
    n = rec["n"]
    m = am.Amalgam(am.objective(rec["objective"], n), n, 10 ** 9, 0., 0, bool(rec["iamalgam"]), **kw)
    x0, zs = am.fixture_draws(rec, unpack)
    m.init(x0)
    return m, zs


def test_the_fixture_holds_both_modes_and_the_named_shapes():
    assert {(s["n"], s["iamalgam"]) for s in STEPS.values()} == {(2, 1), (2, 0), (5, 1), (5, 0), (17, 0), (33, 1)}
    assert STEPS["n17_amalgam"]["np"] == 227 and STEPS["n33_iamalgam"]["np"] == 57


@pytest.mark.parametrize("name", list(STEPS))
def test_reference_form_reproduces_the_recorded_states(name):
    rec = STEPS[name]
    n, np_ = rec["n"], rec["np"]
    m, zs = model_of(rec)
    c = m.c
    assert (c["np"], c["ss"], c["nams"]) == (np_, rec["ss"], rec["nams"]) and np_ == am.default_np(n, rec["iamalgam"])
    assert c["etasigma"] == float.fromhex(rec["etasigma"]) and c["etashift"] == float.fromhex(rec["etashift"])
    assert list(m.order) == list(range(np_))       # the regenerated points come sorted, as the class holds them
    assert rel(m.mu, unpack(rec["mu0"])) <= REFERENCE_FORM_BOUND
    assert rel(m.cov, unpack(rec["cov0"])) <= REFERENCE_FORM_BOUND
    worst, seen = (-1., (0, "")), 0
    for st, z in zip(rec["states"], zs):
        m.iterate(z, perm=st["perm"])
        if st["gen"] not in rec["recorded"]:
            continue
        seen += 1
        assert [int(i) for i in m.order] == st["fit_idx"], st["gen"]
        assert m.t == st["t"] == st["gen"] and m.fev == st["fev"] == (st["gen"] + 1) * np_ and m.nis == st["nis"]
        assert ("arx" in st) == (n <= 5)
        for key in FLOAT_KEYS:
            if key not in st:
                continue
            err = rel(model_state(m, key), unpack(st[key]))
            worst = max(worst, (err, (st["gen"], key)))
            assert err <= REFERENCE_FORM_BOUND, (key, st["gen"], err)
    assert seen == len(rec["recorded"])
    assert m.calls == np_ + m.t * (np_ - 1)
    print("%s: worst relative deviation of the reference form from the recorded reference %.3e at %s"
          % ((name,) + worst))


@pytest.mark.parametrize("n,iam", [(16, True), (17, False), (33, True), (130, True)])
def test_device_form_against_reference_form(n, iam):
    f = am.rosenbrock_fast
    a = am.Amalgam(f, n, 10 ** 9, 0., 0, iam)
    b = am.Amalgam(f, n, 10 ** 9, 0., 0, iam, form="device")
    rng = np.random.default_rng(1000 + n)
    x0 = rng.uniform(-5., 5., (a.np, n))
    a.init(x0)
    b.init(x0)
    draws = am.numpy_draws(rng)
    worst = (-1., (0, ""))
    for gen in range(1, 31):
        z, sh = draws(a)
        a.iterate(z, sh)
        b.iterate(z, sh)
        assert list(a.order) == list(b.order) and (a.nis, a.t, a.fev) == (b.nis, b.t, b.fev), gen
        for key in FLOAT_KEYS + ("sdr",):
            va = [a.sdr] if key == "sdr" else model_state(a, key)
            vb = [b.sdr] if key == "sdr" else model_state(b, key)
            err = rel(vb, va)
            worst = max(worst, (err, (gen, key)))
            assert err <= DEVICE_FORM_BOUND, (key, gen, err)
    print("n = %d: worst relative deviation of the device form from the reference form %.3e at %s" % ((n,) + worst))


@pytest.mark.parametrize("k", range(len(GOLD["pivot"])))
def test_crafted_pivot_failure_leaves_the_reference_partial_factor(k):
    rec = GOLD["pivot"][k]
    n = rec["n"]
    cov = am.crafted(n, rec["rank"], rec["drop"])
    chol, fail = am.factor(cov, 1.)
    assert fail == rec["fail_at"] == {8: 5, 20: 17}[n]
    want = unpack(rec["chol"]).reshape(n, n)
    assert np.array_equal(chol, want)
    assert np.all(np.triu(want, 1) == 0.) and want[fail, fail] < 0. and np.any(want[fail + 1:, fail:] != 0.)


@pytest.mark.parametrize("k", range(len(GOLD["noparam"])))
def test_parameter_free_driver_replays_the_recorded_runs(k):
    rec = GOLD["noparam"][k]
    copies = iter(rec["copies"])
    caps = []

    def inner(s, r, np_, cap):
        cp = next(copies)
        assert (cp["s"], cp["r"], cp["np"], cp["cap"]) == (s, r, np_, cap)
        caps.append(cap)
        return cp["fev"], float.fromhex(cp["f"])

    assert rec["nbase"] == am.default_np(rec["n"], rec["iamalgam"])
    rows = am.parameter_free(rec["nbase"], rec["mfev"], rec["tol"], inner)
    assert next(copies, None) is None
    assert rows[-1][5] == rec["fev"] and rows[-1][4] == float.fromhex(rec["f"])
    assert [(s, runs) for s, runs, *_ in rows] == [(s, 1 << (s >> 1) if s % 2 == 0 else 1) for s in range(len(rows))]
    text = [_tabular.fmt_row(["iter", "runs", "pop", "f*", "best f*", "fev"], WIDTHS), _tabular.rule(WIDTHS)]
    text += [_tabular.fmt_row(list(r), WIDTHS) for r in rows]
    assert text == rec["table"]
    if k == 2:      # the budget binds inside the two copies of stage 2: the last copy starts below zero
        assert rows[-1][1] == 2 and caps[-1] < 0 < caps[-2] < rec["copies"][-2]["fev"]


def test_recorded_outcomes_count_np_per_generation():
    runs = GOLD["runs"]
    np_ = am.default_np(runs["n"], True)
    for r in runs["converging"] + [runs["budget"]]:
        gens = r["fev"] // np_ - 1
        assert r["fev"] == np_ * (gens + 1) and r["calls"] == np_ + gens * (np_ - 1)
    b = runs["budget"]
    assert b["fev"] >= b["mfev"] > b["fev"] - np_
