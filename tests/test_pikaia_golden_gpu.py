"""GPU: PIKAIA against the recorded reference (tests/golden/pikaia_runs.json).

Per recorded shape the model (tests/pikaia_model.py, held to the reference bit for bit by
tests/test_pikaia_model.py) replays the reference's run; for every generation marked "ok" the device is SET to
the reference's state before it (ph, fitns, order, pmut, ig, fev), handed the reference's own draws (the table
the model logs while it reads the mt19937 words) and runs that one generation.  It never runs two in a row, so
nothing compounds.

Bit for bit: the parents of every mating, the crossover window, the kind of mutation of every child, every new
phenotype and every mapped point (nothing transcendental is upstream of them: no tolerance).  Also exact: the
elite decision, the rank order after the generation (the stable order from the reference's state: where the
reference's quicksort ranks two copies of one row the other way round the rows are the same row), pmut, fev, ig
and the flag.  The objective values are held within a relative bound: the device sums the terms of an objective
in another order.

FTOL is 16 times the largest relative deviation of a value from the reference's measured on an MI355X (the test
prints it per shape): 7.9e-16 (7.827e-16 at n65_np66: 64 terms of Rosenbrock summed by 64 lanes and a butterfly
instead of left to right; 5.4e-16 at n = 33, 4.4e-16 at n = 17, 0 at n <= 3).  Nothing compounds over a single
generation, and a wrong formula is wrong by orders more.

Bands: the final best f of 256 device seeds per setting and objective against the reference's 256 recorded
runs, by the comparison of the sibling engines (the median of log10 f inside the reference's quartiles,
tests/test_hees_model.band)."""
import numpy as np
import pytest

import pikaia_model as pm
from test_hees_model import band
from test_pikaia_model import GOLD, STEPS, model_of, params_of, walk

pytestmark = pytest.mark.gpu

FTOL = 16 * 7.9e-16     # relative


def _ints(g, key):
    return [int(v) for v in g.get_state(key)]


def _rel(got, want):
    got, want = np.asarray(got, float).ravel(), np.asarray(want, float).ravel()
    assert got.shape == want.shape
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300)))


@pytest.mark.parametrize("name", sorted(STEPS))
def test_every_recorded_generation_from_the_reference_state(hip, name):
    rec = STEPS[name]
    n, np_ = rec["n"], rec["np"]
    lo, up = rec["lower"] * np.ones(n), rec["upper"] * np.ones(n)
    par = params_of(rec)
    par.pop("irep")
    g = hip.PIKAIA(np_, 1 << 20, rec["nd"], seed=5, **par)
    g.initialize(rec["objective"], lo, up, np.zeros(n))
    assert g.table_len() == pm.table_layout(n, np_, rec["nd"])["len"]
    assert [g.get_state("z")[0].hex(), g.get_state("zinv")[0].hex()] == GOLD["pow10"][str(rec["nd"])]
    d = model_of(rec, order="stable")
    worst, ran = 0., 0
    for k, st, before, m in walk(rec):
        if not st["ok"]:
            continue
        ran += 1
        tag = "%s generation %d " % (name, k)
        g.set_state("ph", np.asarray(before["ph"], float))
        g.set_state("fitns", np.asarray(before["fitns"], float))
        g.set_state("order", np.asarray(before["order"], float))
        for key in ("pmut", "ig", "fev"):
            g.set_state(key, [float(before[key])])
        g.inject_draws(m.table)
        g.iterate()
        assert _ints(g, "parents") == [v for pr in m.parents for v in pr], tag + "parents"
        assert _ints(g, "cross") == [v for cr in m.cross for v in cr], tag + "crossover windows"
        assert _ints(g, "mode") == m.mode, tag + "kinds of mutation"
        ph = np.asarray(m.ph, float)
        assert g.get_state("new_ph").tobytes() == ph.tobytes(), tag + "new phenotypes"
        assert g.get_state("ph").tobytes() == ph.tobytes(), tag + "the population"
        x = np.asarray([m.map(r) for r in m.ph], float)
        assert g.get_state("new_x").tobytes() == x.tobytes() and g.get_state("x").tobytes() == x.tobytes(), tag + "points"
        assert int(g.get_state("elite")[0]) == m.elite == st["elite"], tag + "elite"
        # the rank order: the stable order from the reference's state
        d.start(**before)
        d.iterate(pm.TableSource(m.table))
        assert d.state_crc() == st["state_crc"], tag
        assert _ints(g, "order") == d.order, tag + "rank order"
        assert g.get_state("pmut")[0] == m.pmut == float.fromhex(st["pmut"]), tag + "pmut"
        got = [int(g.get_state(key)[0]) for key in ("fev", "ig", "flag")]
        assert got == [m.fev, m.ig, 0], (tag, got)
        worst = max(worst, _rel(g.get_state("fitns"), m.fitns), _rel(g.get_state("new_f"), [-v for v in m.fitns]))
    assert ran == sum(st["ok"] for st in rec["states"]) >= 12
    print("%s: %d generations; worst deviation of a value %.3e relative" % (name, ran, worst))
    assert worst <= FTOL, worst


@pytest.mark.parametrize("run", range(4))
def test_outcome_bands_match_the_reference(hip, run):
    b = GOLD["bands"]
    r = b["runs"][run]
    n, P = b["n"], b["count"]
    g = hip.PIKAIA(b["np"], b["ngen"], b["nd"], imut=r["imut"], ielite=r["ielite"], seed=2024 + run, populations=P)
    g.initialize(r["objective"], b["lower"] * np.ones(n), b["upper"] * np.ones(n), np.zeros(P * n))
    g.run(10 ** 6)
    assert all(int(g.get_state("flag", p)[0]) == 1 and int(g.get_state("fev", p)[0]) == r["fev"] for p in range(P))
    # what the reference reports: the best row of the final population
    got = [-float(np.max(g.get_state("fitns", p))) for p in range(P)]
    band(got, r["fbest"], "imut %d ielite %d %s device" % (r["imut"], r["ielite"], r["objective"]))
