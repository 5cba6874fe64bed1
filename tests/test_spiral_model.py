"""CPU: tests/spiral_model.py against the recorded reference (tests/golden/spiral_runs.json).

The reference form, fed the uniforms the reference made of its recorded mt19937 words, reproduces
every recorded state bit for bit with libm's cos and sin.  The device form (the difference
x_i - xbest rotated once) runs beside it from the same initial points and the same uniforms; its
largest deviation, relative to the largest coordinate of the generation, is measured over all
recorded generations and held below 1e-12."""
import json
import os

import numpy as np
import pytest

import chol_model
import jaya_model as jm
import spiral_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "spiral_runs.json")) as fh:
    GOLD = json.load(fh)

FORM_BOUND = 1e-12


def _h(v):
    return np.array([float.fromhex(s) for s in v])


def _same(a, b, what):
    a, b = np.asarray(a, float).ravel(), np.asarray(b, float).ravel()
    assert a.shape == b.shape, what
    assert a.tobytes() == b.tobytes(), (what, float(np.abs(a - b).max()))


def model_of(rec, form):
    n, np_ = rec["n"], rec["np"]
    m = sm.Spiral(chol_model.objective(rec["objective"], n), np_, taur=rec["taur"], tautheta=rec["tautheta"],
                  form=form)
    m.start(_h(rec["init"]["x"]).reshape(np_, n))
    return m


def uniforms_of(rec, st):
    w = jm.Words(st["words"])
    u = sm.uniforms_of(w, rec["np"], rec["taur"], rec["tautheta"])
    assert w.exhausted(), rec["name"]
    return u


def _check(m, st, tag):
    _same(m.x, _h(st["x"]), tag + "x")
    _same(m.fs, _h(st["f"]), tag + "f")
    _same(m.rs, _h(st["rs"]), tag + "rs")
    _same(m.thetas, _h(st["thetas"]), tag + "thetas")
    _same(m.xbest, _h(st["xbest"]), tag + "xbest")
    assert (m.ibest, m.fev) == (st["ibest"], st["fev"]), tag


@pytest.mark.parametrize("rec", GOLD["steps"], ids=[r["name"] for r in GOLD["steps"]])
def test_reference_form_reproduces_the_recorded_states_bit_for_bit(rec):
    m = model_of(rec, "reference")
    _check(m, rec["init"], rec["name"] + " init ")
    for g, st in enumerate(rec["states"], 1):
        m.iterate(uniforms_of(rec, st))
        _check(m, st, "%s gen %d " % (rec["name"], g))


def test_device_form_deviates_from_the_reference_form_by_rounding_alone():
    """Measured over the 12 recorded runs of 4 generations: 3.1e-15 relative to the largest
    coordinate at most; the bound is 1e-12.  Every generation picks the same ibest."""
    worst = 0.
    for rec in GOLD["steps"]:
        ref, dev = model_of(rec, "reference"), model_of(rec, "device")
        for g, st in enumerate(rec["states"], 1):
            u = uniforms_of(rec, st)
            ref.iterate(u)
            dev.iterate(u)
            a, b = np.array(dev.x), np.array(ref.x)
            err = float(np.abs(a - b).max() / np.abs(b).max())
            worst = max(worst, err)
            assert dev.ibest == ref.ibest == st["ibest"], (rec["name"], g)
            assert err < FORM_BOUND, (rec["name"], g, err)
    print("device form against reference form: largest relative deviation %.3e" % worst)
    assert worst < FORM_BOUND


def test_a_point_at_xbest_stays_and_n1_only_contracts():
    x = [0.3, -1.2, 2.5]
    for step in (sm.step_reference, sm.step_device):
        assert step(x, x, 0.95, 0.1, 0.9) == x
        assert step([2.], [0.5], 0.5, 0.3, 0.7) == [0.5 * 2. - 0.5 * 0.5 + 0.5 if step is sm.step_reference
                                                       else 0.5 * (2. - 0.5) + 0.5]


def test_the_row_wise_device_form_is_the_scalar_one_bit_for_bit():
    rng = np.random.default_rng(3)
    for n in (1, 2, 5, 12):
        X, xb = rng.uniform(-5., 5., (7, n)), rng.uniform(-5., 5., n)
        r, th = rng.uniform(0.9, 1., 7), rng.uniform(0., 6.28, 7)
        c, s = np.cos(th), np.sin(th)
        rows = sm.step_device_rows(X, xb, r, c, s)
        for i in range(7):
            _same(rows[i], sm.step_device(list(X[i]), list(xb), float(r[i]), float(c[i]), float(s[i])), "row %d" % i)


def test_the_fixture_keeps_its_arg_min_gap_and_its_signature():
    for rec in GOLD["steps"]:
        for st in [rec["init"]] + rec["states"]:
            f = np.sort(_h(st["f"]))
            assert abs(f[1] - f[0]) > 1e-6 * max(abs(f[0]), abs(f[1])), rec["name"]
    assert [a["name"] for a in GOLD["signature"]] == ["mfev", "tol", "np", "r", "theta", "taur", "tautheta", "rlow",
                                                     "rhigh", "thetalow", "thetahigh"]
    assert sorted((r["n"], r["np"]) for r in GOLD["steps"][::2]) == [(1, 3), (2, 5), (3, 7), (5, 20), (9, 20), (17, 4)]
    assert len(_h(GOLD["bands"]["sphere"])) == len(_h(GOLD["bands"]["rosenbrock"])) == 256
