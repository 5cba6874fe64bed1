"""tests/neldermead_model.py against the recorded runs of the reference (tests/golden/neldermead_runs.json): every
step's branch, ihi, ilo, counters, the CRC-32 of the whole simplex and its values and of every point handed to
the objective with its value; every whole run's result, evaluations, restarts and events, bit for bit.  The
generator (scripts/gen_neldermead_golden.py) compared the same replay with the full arrays before it kept the
sums."""
import json
import os

import pytest

import chol_model
import neldermead_model as nm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "neldermead_runs.json")) as fh:
    GOLDEN = json.load(fh)


def model_of(rec, **kw):
    par = rec["params"]
    return nm.Model(chol_model.objective(rec["objective"], rec["n"]), rec["n"], par["mfev"], par["tol"], par["rad0"],
                    nm.MINIT[rec["minit"]], nm.PINIT[rec["pinit"]], par["checkev"], par["eps"], **kw)


def guess_of(rec):
    return [float.fromhex(v) for v in rec["guess"]]


def flat_evals(m):
    return [v for x, fx in m.evals for v in x + [fx]]


def test_the_fixture_covers_the_shapes_and_every_path():
    assert sorted({r["n"] for r in GOLDEN["steps"]}) == [2, 3, 17, 33, 65, 128]
    assert {r["n"] for r in GOLDEN["runs"]} >= {2, 3, 17, 33, 65, 128}
    recs = GOLDEN["steps"] + GOLDEN["runs"]
    assert {r["objective"] for r in recs} == {"sphere", "rosenbrock"}
    assert {r["pinit"] for r in recs} == set(nm.PINIT)
    assert {r["minit"] for r in recs} == set(nm.MINIT) - {"random"}
    assert set(GOLDEN["paths"]) == set(nm.PATHS)
    for k in nm.PATHS:
        assert GOLDEN["paths"][k] >= 2, k
    for rec in GOLDEN["steps"]:
        assert len(rec["states"]) == 20 and sum(s["ok"] for s in rec["states"]) >= 12, rec["name"]


@pytest.mark.parametrize("key", sorted(GOLDEN["coef"]))
def test_coefficients_are_the_reference_s(key):
    pinit, n = key.split(":")
    assert list(nm.coefficients(nm.PINIT[pinit], int(n))) == [float.fromhex(v) for v in GOLDEN["coef"][key]]


@pytest.mark.parametrize("rec", GOLDEN["steps"], ids=lambda r: r["name"])
def test_steps_replay_bit_for_bit(rec):
    m = model_of(rec)
    m.init(guess_of(rec))
    m.first_simplex()
    assert (m.state_crc(), m.ilo, m.icount) == (rec["init"]["state_crc"], rec["init"]["ilo"], rec["init"]["icount"])
    for g, st in enumerate(rec["states"]):
        m.evals = []
        m.iterate()
        got = {"branch": m.branch, "ihi": m.ihi, "ilo": m.ilo, "icount": m.icount, "jcount": m.jcount,
               "conv": int(m.conv), "state_crc": m.state_crc(), "evals_crc": nm.crc(flat_evals(m)),
               "nevals": len(m.evals), "ok": bool(m.ok())}
        assert got == st, "%s step %d" % (rec["name"], g)


@pytest.mark.parametrize("rec", GOLDEN["runs"], ids=lambda r: r["name"])
def test_whole_runs_replay_bit_for_bit(rec):
    m = model_of(rec)
    x, icount, conv = m.optimize(guess_of(rec))
    assert [v.hex() for v in x] == rec["x"] and (icount, int(conv)) == (rec["icount"], rec["converged"])
    assert (nm.crc(flat_evals(m)), len(m.evals)) == (rec["evals_crc"], rec["nevals"])
    assert (m.it, m.restarts, [list(e) for e in m.events]) == (rec["steps"], rec["restarts"], rec["events"])
    assert m.paths == rec["paths"]


def test_repair_changes_the_refused_outside_contraction_only():
    rec = next(r for r in GOLDEN["runs"] if r["paths"]["outside_refused"])
    a, b = model_of(rec), model_of(rec, repair=True)
    a.init(guess_of(rec)), b.init(guess_of(rec))
    a.first_simplex(), b.first_simplex()
    while True:
        a.iterate(), b.iterate()
        if a.branch == nm.OUTSIDE_REFUSED:
            break
        assert a.p == b.p and a.y == b.y
    assert a.p == b.p and a.y != b.y
    assert b.y[b.ihi] == b.f(b.p[b.ihi]) and a.y[a.ihi] != a.f(a.p[a.ihi])
