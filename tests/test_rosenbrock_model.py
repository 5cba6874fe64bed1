"""tests/rosenbrock_model.py against the recorded runs of the reference (tests/golden/rosenbrock_runs.json): every
search's i before and after, fev, stepi, d[i], path, the CRC-32 of x, v and d and of every point handed to the
objective with its value; every whole run's result, evaluations, searches and paths, bit for bit.  The generator
(scripts/gen_rosenbrock_golden.py) compared the same replay with the full arrays before it kept the sums."""
import json
import os

import pytest

import rosenbrock_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "rosenbrock_runs.json")) as fh:
    GOLDEN = json.load(fh)
WINDOW, GOOD_OK = 24, 16


def model_of(rec, **kw):
    par = rec["params"]
    return rm.Model(rm.objective(rec["objective"], rec["n"]), rec["n"], par["mfev"], par["tol"], par["step0"],
                    par["decf"], **kw)


def guess_of(rec):
    return [float.fromhex(v) for v in rec["guess"]]


def flat_evals(m):
    return [v for x, fx in m.evals for v in x + [fx]]


def at_window(rec):
    """the model at the state the record's window begins with"""
    m = model_of(rec)
    m.init(guess_of(rec))
    for _ in range(rec["skip"]):
        m.iterate()
    return m


def search_record(m, i0):
    return {"i0": i0, "i1": m.i, "fev": m.fev, "stepi": m.stepi.hex(), "di": m.d[i0].hex(), "path": list(m.path),
            "orth": int(m.orth), "state_crc": m.state_crcs(), "evals_crc": rm.crc(flat_evals(m)),
            "nevals": len(m.evals), "ok": bool(m.ok())}


def test_the_fixture_covers_the_shapes_and_every_path():
    assert sorted({r["n"] for r in GOLDEN["steps"]}) == [2, 17, 33, 65, 128]
    assert {(r["objective"], r["n"]) for r in GOLDEN["runs"]} >= {
        ("sphere", 1), ("sphere", 3), ("sphere", 65), ("sphere", 128), ("rosenbrock", 2), ("rosenbrock", 17),
        ("rosenbrock", 128), ("rosenbrock", 1)}
    assert {r["objective"] for r in GOLDEN["steps"]} == {"sphere", "rosenbrock", "rastrigin"}
    assert set(GOLDEN["paths"]) == set(rm.PATHS)
    for k in rm.PATHS:
        assert GOLDEN["paths"][k] >= 2, k
    for rec in GOLDEN["steps"]:
        assert len(rec["states"]) == WINDOW and sum(s["ok"] for s in rec["states"]) >= GOOD_OK, rec["name"]
        if not rec["name"].endswith(("_rare", "_orth")):
            assert rec["skip"] == max(0, rec["n"] + 1 - 12)
        assert rec["guess"] == [v.hex() for v in guess_of(rec)]
    # the windows hold the first extra search and, where the stage moved, the first orthogonalisation
    assert all(r["paths"]["extra"] >= 1 for r in GOLDEN["steps"])
    assert {r["n"] for r in GOLDEN["steps"] if any(s["orth"] and s["ok"] for s in r["states"])} >= {2, 17, 33, 65, 128}
    for rec in GOLDEN["runs"]:
        if rec["objective"] == "sphere" and rec["n"] <= 65:
            assert rec["converged"] == 1 and rec["paths"]["zero_norm"] >= 1, rec["name"]
    budget = next(r for r in GOLDEN["runs"] if r["name"] == "run_n128_budget")
    assert budget["converged"] == 0 and budget["fev"] > budget["params"]["mfev"]
    assert all(float.fromhex(v) == 0. for v in budget["x"])         # the zero vector of the reference


def test_dnrm2_scaled_form():
    assert rm.dnrm2([3., 4.]) == 5. and rm.dnrm2([-2.]) == 2. and rm.dnrm2([0., 0., 0.]) == 0.
    assert rm.dnrm2([1e200, 1e200]) == 1e200 * 2. ** 0.5        # the plain sum of squares overflows
    assert rm.dnrm2([1e-200, 1e-200]) > 0.


def test_cos_2pi_is_near_the_cosine():
    import math
    for k in range(-40, 41):
        x = k / 16. + 0.013 * k
        assert abs(rm.cos_2pi(x) - math.cos(2. * math.pi * x)) < 1e-13


@pytest.mark.parametrize("rec", GOLDEN["steps"], ids=lambda r: r["name"])
def test_windows_replay_bit_for_bit(rec):
    m = at_window(rec)
    assert (m.state_crcs(), m.i, m.fev) == (rec["before"]["state_crc"], rec["before"]["i"], rec["before"]["fev"])
    for g, st in enumerate(rec["states"]):
        m.evals = []
        i0 = m.i
        m.iterate()
        assert search_record(m, i0) == st, "%s search %d" % (rec["name"], rec["skip"] + g)


@pytest.mark.parametrize("rec", GOLDEN["runs"], ids=lambda r: r["name"])
def test_whole_runs_replay_bit_for_bit(rec):
    m = model_of(rec)
    x, fev, conv = m.optimize(guess_of(rec))
    assert [v.hex() for v in x] == rec["x"] and (fev, int(conv)) == (rec["fev"], rec["converged"])
    assert (rm.crc(flat_evals(m)), len(m.evals)) == (rec["evals_crc"], rec["nevals"])
    assert (m.searches, m.orths, m.paths) == (rec["searches"], rec["orths"], rec["paths"])


def test_repair_returns_the_end_of_the_last_completed_search():
    rec = next(r for r in GOLDEN["runs"] if r["name"] == "run_n128_budget")
    a, b = model_of(rec), model_of(rec, repair=True)
    xa, fa, ca = a.optimize(guess_of(rec))
    xb, fb, cb = b.optimize(guess_of(rec))
    assert (fa, ca) == (fb, cb) and a.x == b.x and a.v == b.v
    assert xa == [0.] * rec["n"] and xb == b.x[b.i - 1] and b.f(xb) < b.f(guess_of(rec))
    rec = next(r for r in GOLDEN["runs"] if r["name"] == "run_n2_rosen")
    assert model_of(rec).optimize(guess_of(rec)) == model_of(rec, repair=True).optimize(guess_of(rec))


def test_the_constant_objective_doubles_until_1e30():
    rec = next(r for r in GOLDEN["runs"] if r["name"] == "run_n1_constant")
    m = model_of(rec)
    m.init(guess_of(rec))
    m.iterate()
    # 100 rounds: s = 2^100 >= 1e30 ends the loop; halved, and imin 0 of four equal values steps back by it
    assert m.path == [rm.FORWARD, 100, 0, rm.NO_FINAL] and m.d[1] == -2. ** 99 and m.fev == 106
