"""GPU: BasinHopping on the device against the runs of the reference's BasinHopping recorded in
tests/golden/basinhopping_runs.json.

Whole runs: with a callable objective (the serial sums of the fixture's harness) and the reference's draws injected
(regenerated from the run's seed), every run is the reference's bit for bit -- the table's rows, the start handed to
the minimiser and what it returned on every hop (the fixture's CRC-32 sums, and the bits of the model's replay,
which tests/test_basinhopping_model.py holds to the same sums), the minimiser's counts, the best point, n_evals,
converged = False.  Both minimisers, both strategies,
temp = 0, a strategy object used for two optimize() calls.
The step alone: from the state before every recorded hop (x, stepsize, nstep, naccept set, the hop's draws
injected) one iterate() with the built-in objective hands the minimiser the reference's start bit for bit and logs
the reference's adjusted stepsize; the records hold coordinates that hit either clamp."""
import numpy as np
import pytest

import rosenbrock_model as rm
from test_basinhopping_model import RUNS, guess_of, replayed, same_rows, table_of

pytestmark = pytest.mark.gpu


def strategy_of(hip, rec):
    st = rec["strategy"]
    if st["adaptive"]:
        return hip.BasinHopping_AdaptStrategy(st["stepsize"], st["accept_rate"], st["interval"], st["factor"])
    return hip.BasinHopping_StepStrategy(st["stepsize"])


def minimizer_of(hip, rec, **kw):
    mn = rec["minimizer"]
    if mn["kind"] == "nm":
        return hip.NelderMead(mn["mfev"], mn["tol"], mn["rad0"], seed=5, **kw)
    return hip.Rosenbrock(mn["mfev"], mn["tol"], mn["step0"], mn["decf"], seed=5, **kw)


def rows_of(b, n, p=0):
    log = b.get_state("log", p).reshape(-1, 7)
    start, sol = b.get_state("log_start", p).reshape(-1, n), b.get_state("log_sol", p).reshape(-1, n)
    fev = b.get_state("log_fev", p)
    return [{"it": r[0], "f": r[1], "conv": r[2], "step": r[3], "accept": r[4], "fbest": r[5], "fev": r[6],
             "inner_fev": fev[k], "start": start[k], "sol": sol[k]} for k, r in enumerate(log)]


@pytest.mark.parametrize("rec", RUNS, ids=lambda r: r["name"])
def test_whole_runs_are_the_reference_bit_for_bit(hip, rec):
    n, box = rec["n"], rec["box"]
    fobj = rm.objective(rec["objective"], n)
    calls = [0]

    def f(x):
        calls[0] += 1
        return fobj(x.tolist())

    strat = strategy_of(hip, rec)
    b = hip.BasinHopping(minimizer_of(hip, rec), strat, False, rec["mit"], rec["temp"], seed=3)
    for k, call in enumerate(rec["calls"]):
        tag = "%s call %d" % (rec["name"], k)
        calls[0] = 0
        b.inject_draws(table_of(rec, k))
        sol = b.optimize(f, -box * np.ones(n), box * np.ones(n), guess_of(rec))
        got = rows_of(b, n)
        same_rows(got, call, tag)
        for r, w in zip(got, replayed(rec)[k][0].rows):
            assert r["start"].tolist() == w["start"] and r["sol"].tolist() == w["sol"], (tag, w["it"])
        assert sol.converged is False and sol.n_evals == call["fev"] == calls[0], tag
        assert rm.crc(sol.x) == call["xbest_crc"] and rm.crc(b.get_state("x")) == call["x_crc"], tag
        assert rm.crc(b.get_state("xbest")) == call["xbest_crc"], tag
        assert float(b.get_state("fbest")[0]).hex() == call["rows"][-1]["fbest"], tag
        assert (int(b.get_state("it")[0]), int(b.get_state("flag")[0])) == (rec["mit"], 2), tag
        # the caller's strategy object carries the chain's history on, as the reference's does
        assert (strat.nstep, strat.naccept, float(strat.stepsize).hex()) == (call["nstep"], call["naccept"], call["stepsize"]), tag


@pytest.mark.parametrize("rec", RUNS, ids=lambda r: r["name"])
def test_the_step_alone_from_every_recorded_state(hip, rec):
    n, box, adaptive = rec["n"], rec["box"], rec["strategy"]["adaptive"]
    lo, up = -box * np.ones(n), box * np.ones(n)
    clamped = 0
    for c, call in enumerate(rec["calls"]):
        model = replayed(rec)[c][0].rows
        b = hip.BasinHopping(minimizer_of(hip, rec), strategy_of(hip, rec), False, rec["mit"], rec["temp"], seed=3)
        b.initialize(getattr(hip.objectives, rec["objective"]), lo, up, guess_of(rec))
        b.inject_draws(table_of(rec, c))
        rows = call["rows"]
        x, nacc = model[0]["sol"], call["naccept0"]
        for k in range(rec["mit"]):
            tag = "%s hop %d: " % (rec["name"], k)
            b.set_state("x", x)
            b.set_state("stepsize", [float.fromhex(rows[k]["step"] if k else call["stepsize0"])])
            b.set_state("nstep", [call["nstep0"] + k if adaptive else 0])
            b.set_state("naccept", [nacc])
            b.iterate()
            got = b.get_state("log_start").reshape(-1, n)[k + 1]
            assert got.tolist() == model[k + 1]["start"] and rm.crc(got) == rows[k + 1]["start_crc"], tag + "xtrial"
            assert float(b.get_state("log").reshape(-1, 7)[k + 1, 3]).hex() == rows[k + 1]["step"], tag + "stepsize"
            clamped += int(np.sum(np.abs(got) == box - 0.05 * (box + box)))
            if rows[k + 1]["accept"]:
                x = model[k + 1]["sol"]
                nacc += adaptive
    # (the n = 17 shapes start near the edges of the box: above for temp = 1, below for temp = 0)
    if rec["n"] == 17 and adaptive:
        assert clamped >= 1, "no coordinate of %s hit a clamp" % rec["name"]
