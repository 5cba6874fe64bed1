"""CPU: tests/basinhopping_model.py against the runs of the reference's BasinHopping recorded in
tests/golden/basinhopping_runs.json (scripts/gen_basinhopping_golden.py).  Every run is replayed on the reference's
draws, regenerated from the run's seed: the table's rows, the start handed to the minimiser and what it returned on
every hop (CRC-32 sums of their bits), the counts, the strategy's state afterwards -- bit for bit; no hop of the
fixture is a close decision, so none is left out."""
import json
import math
import os

import pytest

import basinhopping_model as bm
import rosenbrock_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "basinhopping_runs.json")) as _fh:
    GOLDEN = json.load(_fh)
RUNS = GOLDEN["runs"]


def guess_of(rec):
    """start_point() of the generator"""
    return [rec["base"] + 0.0625 * (i % 7) for i in range(rec["n"])]


def strategy_of(rec):
    st = rec["strategy"]
    if st["adaptive"]:
        return bm.Strategy(st["stepsize"], st["accept_rate"], st["interval"], st["factor"])
    return bm.Strategy(st["stepsize"])


def minimizer_of(rec, f):
    mn, n = rec["minimizer"], rec["n"]
    if mn["kind"] == "nm":
        return bm.nm_minimizer(f, n, mn["mfev"], mn["tol"], mn["rad0"])
    return bm.rosen_minimizer(f, n, mn["mfev"], mn["tol"], mn["step0"], mn["decf"])


def model_of(rec, strategy):
    n, box = rec["n"], rec["box"]
    f = rm.objective(rec["objective"], n)
    return bm.Model(f, [-box] * n, [box] * n, minimizer_of(rec, f), strategy, rec["mit"], rec["temp"])


def table_of(rec, k):
    """the draws of call k of the run: the calls of a run draw from one stream"""
    mit = rec["mit"]
    return bm.reference_draws(rec["seed"], rec["n"], mit * (k + 1))[mit * k:]


_REPLAYED = {}


def replayed(rec):
    """the model's runs of the record's calls, walked once per process: [(model, strategy state afterwards)]"""
    if rec["name"] not in _REPLAYED:
        strat, out = strategy_of(rec), []
        for k in range(len(rec["calls"])):
            m = model_of(rec, strat)
            m.result = m.optimize(guess_of(rec), table_of(rec, k))
            out.append((m, (strat.nstep, strat.naccept, strat.stepsize.hex())))
        _REPLAYED[rec["name"]] = out
    return _REPLAYED[rec["name"]]


def same_rows(rows, call, tag):
    """rows: dicts with it, f, conv, step, accept, fbest, fev, inner_fev, start, sol as floats / ints"""
    assert len(rows) == len(call["rows"]), tag
    for r, w in zip(rows, call["rows"]):
        t = "%s row %d: " % (tag, w["it"])
        for k in ("it", "conv", "accept", "fev", "inner_fev"):
            assert int(r[k]) == w[k], t + k
        for k in ("f", "step", "fbest"):
            assert float(r[k]).hex() == w[k], t + k
        assert rm.crc(r["start"]) == w["start_crc"], t + "start"
        assert rm.crc(r["sol"]) == w["sol_crc"], t + "sol"


@pytest.mark.parametrize("rec", RUNS, ids=lambda r: r["name"])
def test_the_model_replays_the_recorded_run(rec):
    before = (0, 0, float(rec["strategy"]["stepsize"]).hex())
    for k, (call, (m, after)) in enumerate(zip(rec["calls"], replayed(rec))):
        tag = "%s call %d" % (rec["name"], k)
        assert before == (call["nstep0"], call["naccept0"], call["stepsize0"]), tag
        xbest, fev, conv = m.result
        same_rows(m.rows, call, tag)
        assert conv is False and fev == call["fev"] == m.rows[-1]["fev"], tag
        assert (rm.crc(xbest), rm.crc(m.x)) == (call["xbest_crc"], call["x_crc"]), tag
        assert after == (call["nstep"], call["naccept"], call["stepsize"]), tag
        assert m.close() == [] and call["close"] == 0, tag
        before = after


def test_the_fixture_covers_what_it_claims():
    names = [r["name"] for r in RUNS]
    for n in (2, 17, 65, 128):      # both strategies x both minimisers at every size
        for kind in ("nm", "rosen"):
            for st in ("plain", "adapt"):
                assert any(v.startswith("n%d_" % n) and v.endswith("_%s_%s" % (kind, st)) for v in names), (n, kind, st)
    assert all(r["mit"] == 8 for r in RUNS) and GOLDEN["close"] == 0
    assert sum(r["temp"] == 0. for r in RUNS) == 2 and any(len(r["calls"]) == 2 for r in RUNS)
    assert all(v >= 2 for v in GOLDEN["coverage"].values()), GOLDEN["coverage"]
    rows = [row for r in RUNS for c in r["calls"] for row in c["rows"]]
    assert {row["conv"] for row in rows} == {0, 1} and {row["accept"] for row in rows[1:]} == {0, 1}
    # a Rosenbrock minimiser that ends on its budget returns the zero vector, which is evaluated and hopped from
    for r in RUNS:
        for c in r["calls"]:
            budget = sum(not row["conv"] for row in c["rows"])
            assert c["zeros"] == (budget if r["minimizer"]["kind"] == "rosen" else 0), r["name"]
    assert sum(c["zeros"] for r in RUNS for c in r["calls"]) >= 2
    run = next(r for r in RUNS if r["name"] == "n128_rosenbrock_rosen_plain")
    assert all(rm.crc([0.] * 128) == row["sol_crc"] for row in run["calls"][0]["rows"])


def test_the_reused_strategy_keeps_its_history():
    rec = next(r for r in RUNS if len(r["calls"]) == 2)
    first, second = rec["calls"]
    assert first["nstep0"] == 0 and second["nstep0"] == first["nstep"] == rec["mit"]
    assert second["naccept0"] == first["naccept"] and second["stepsize0"] == first["stepsize"]
    assert second["nstep"] == 2 * rec["mit"]


def test_the_metropolis_test_at_temperature_zero():
    inf, nan = math.inf, math.nan
    # beta = +inf: better accepts (w = 1), worse has w = 0, equal energies give 0 * inf = NaN, which std::min(0., v)
    # passes on as 0: w = 1, accepted
    assert bm.metropolis_w(1., 2., 0.) == 1. and bm.metropolis_w(2., 1., 0.) == 0.
    assert bm.metropolis_w(1., 1., 0.) == 1.
    assert bm.metropolis_w(inf, inf, 1.) == 1.          # inf - inf
    assert bm.metropolis_w(inf, 1., 1.) == 0. and bm.metropolis_w(1., inf, 1.) == 1.
    assert bm.metropolis_w(2., 1., 1.) == math.exp(-1.) and bm.metropolis_w(2., 1., 0.5) == math.exp(-2.)
    assert bm.metropolis_w(nan, 1., 1.) == 1.           # (the model's callers turn a NaN energy into +inf first)
    for rec in (r for r in RUNS if r["temp"] == 0.):
        for k, call in enumerate(rec["calls"]):
            rows, energy = call["rows"], None
            for row, u in zip(rows[1:], table_of(rec, k)):
                energy = float.fromhex(rows[0]["f"]) if energy is None else energy
                f = float.fromhex(row["f"])
                assert row["accept"] == int(f <= energy or u[-1] == 0.), (rec["name"], row["it"])
                if row["accept"]:
                    energy = f


def test_the_step_is_clamped_to_the_box_less_five_percent():
    st = bm.Strategy(1.)
    x = [0., 4., -4., 0.]
    st.take_step(x, [-5.] * 4, [5.] * 4, [0.999, 0.5, -0.5, 0.25])
    assert x == [4.5, 4.5, -4.5, 2.5]
    ad = bm.Strategy(1., 0.5, 2, 0.5)
    ad.naccept = 2
    for want in (1., 2., 2., 1.):       # nstep 1 .. 4: 2 / 2 > 0.5 widens, 2 / 4 > 0.5 is false and narrows
        ad.take_step([0.], [-1.], [1.], [0.])
        assert ad.stepsize == want


def test_the_global_case_of_the_fixture():
    g = GOLDEN["global"]
    assert (g["n"], g["box"], g["mit"]) == (2, 5.12, 8) and g["chains"] >= 24
    assert 0 <= g["first_in_global_basin"] < g["best_in_global_basin"] <= g["chains"]
