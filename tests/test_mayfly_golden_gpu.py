"""GPU: Mayfly against the recorded reference (tests/golden/mayfly_runs.json).

Per recorded shape the model (tests/mayfly_model.py, held to the reference bit for bit by
tests/test_mayfly_model.py) replays the reference's run; for every generation marked "ok" the device is SET
to the reference's state before it, handed the reference's own draws (the table the model logs while it
reads the recorded mt19937 words) and runs that one generation.  It never runs two in a row, so nothing
compounds.

Exact: which velocity form every fly took, both rank orders of the swarms, both rank orders of the
selections, the record that landed in every slot, which evaluation took fbest last, fev, nmut, it, the two
shuffles, and every position and velocity produced by a random flight, a crossover, a mutation or a copy.
Within a tolerance: the positions and velocities of the flies that took an exp() form and what descends
from them within the generation (relative to the box width), and the objective values (relative: the device
sums them in another order).  Up to the selection the device is held to the reference itself; the selection
is held to the model's stable order from the reference's state (beyond 16 records the reference's std::sort
is not stable; where a generation is marked "stable" the two are the same state, test_mayfly_model.py).

The bounds are 16 times the largest deviation measured on an MI355X (the test prints it per shape): positions
and velocities of the exp() descendants 3.5e-17 of the box width (n33_np40_pgb; 3.5e-16 absolute on a box of
10, under two ulps of a coordinate: a single exp() of <= 1 ulp scales one term of a velocity that is at most
a tenth of the box, and a generation restarted from the recorded state cannot accumulate), values 9.8e-16
relative (n65_np66: 64 terms summed in another order); both 0 on the one-term shapes n = 1 and n = 2.  A
wrong formula is wrong by orders more.

Bands: the final fbest of 256 device seeds at n = 10, np = 20 and the recorded budget against the reference's
256 recorded runs, by the comparison of the sibling engines (the median of log10 f inside the reference's
quartiles, tests/test_hees_model.band)."""
import numpy as np
import pytest

import mayfly_model as mm
from test_hees_model import band
from test_mayfly_model import GOLD, PERCOORD, STEPS, _h, bounds_of, percoord_witness, walk

pytestmark = pytest.mark.gpu

XTOL = 16 * 3.5e-17     # of the box width
FTOL = 16 * 9.8e-16     # relative
SET_KEYS = ("males_x", "males_v", "males_bx", "males_f", "males_bf", "females_x", "females_v", "females_f",
            "xbest", "fbest", "g", "dance", "fl", "it", "itmax", "fev")


class Worst:
    def __init__(self):
        self.x, self.f, self.at = 0., 0., ""

    def rows(self, got, want, taint, width, what):
        """rows of positions or velocities: bit for bit where no exp() is upstream, else within XTOL"""
        got, want = np.asarray(got, float).reshape(len(taint), -1), np.asarray(want, float).reshape(len(taint), -1)
        for j, t in enumerate(taint):
            if not t:
                assert got[j].tobytes() == want[j].tobytes(), (what, j, got[j][got[j] != want[j]][:3],
                                                                want[j][got[j] != want[j]][:3])
            else:
                err = float(np.max(np.abs(got[j] - want[j]) / width))
                if err > self.x:
                    self.x, self.at = err, "%s row %d" % (what, j)

    def vals(self, got, want, what):
        got, want = np.asarray(got, float).ravel(), np.asarray(want, float).ravel()
        assert got.shape == want.shape, what
        err = float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300)))
        if err > self.f:
            self.f = err


def _ints(g, key):
    return [int(v) for v in g.get_state(key)]


# (the last record: bounds that differ in every coordinate, tests/golden/mayfly_percoord.json)
@pytest.mark.parametrize("name", sorted(STEPS) + sorted(PERCOORD))
def test_every_recorded_generation_from_the_reference_state(hip, name):
    rec = STEPS.get(name) or PERCOORD[name]
    n, np_ = rec["n"], rec["np"]
    lo, up = (np.asarray(v, float) for v in bounds_of(rec))
    if name in PERCOORD:
        percoord_witness(rec)
    width = up - lo
    g = hip.Mayfly(np_, rec["mfev"], seed=5, **rec["params"])
    g.initialize(rec["objective"], lo, up, np.zeros(n))
    worst, ran = Worst(), 0
    for k, st, before, m in walk(rec):
        if not st["ok"]:
            continue
        ran += 1
        tag = "%s generation %d " % (name, k)
        for key in SET_KEYS:
            g.set_state(key, np.asarray(before[key], float))
        g.inject_draws(m.table)
        g.iterate()
        # ---- up to the selection: the reference itself
        assert _ints(g, "branch_f") == m.branch_f and _ints(g, "branch_m") == m.branch_m, tag + "branches"
        for sex, flies in (("females", m.moved_females), ("males", m.moved_males)):
            taint = [y.taint for y in flies]
            worst.rows(g.get_state("moved_%s_x" % sex), [y.x for y in flies], taint, width, tag + sex + " x")
            worst.rows(g.get_state("moved_%s_v" % sex), [y.v for y in flies], taint, width, tag + sex + " v")
            worst.vals(g.get_state("moved_%s_f" % sex), [y.f for y in flies], tag + sex + " f")
        assert _ints(g, "rank_m") == m.rank_m and _ints(g, "rank_f") == m.rank_f, tag + "ranks"
        worst.rows(g.get_state("off_x"), [y.x for y in m.offspring], [y.taint for y in m.offspring], width, tag + "off x")
        worst.vals(g.get_state("off_f"), [y.f for y in m.offspring], tag + "off f")
        assert _ints(g, "perm_o") == m.perm_o and _ints(g, "perm_u") == m.perm_u, tag + "shuffles"
        if m.nmut:
            worst.rows(g.get_state("mut_x"), [y.x for y in m.mutated], [y.taint for y in m.mutated], width, tag + "mut x")
            worst.vals(g.get_state("mut_f"), [y.f for y in m.mutated], tag + "mut f")
        got = [int(g.get_state(key)[0]) for key in ("took", "fev", "nmut", "it", "flag")]
        assert got == [m.took, m.fev, m.nmut, m.it, 0], (tag, got)
        worst.vals(g.get_state("fbest"), [m.fbest], tag + "fbest")
        worst.rows(g.get_state("xbest"), [m.best], [m.best_taint], width, tag + "xbest")
        assert g.get_state("g")[0] == m.g and g.get_state("dance")[0] == m.dance_now and g.get_state("fl")[0] == m.fl_now
        # ---- the selection: the stable order from the reference's state
        d = mm.Mayfly(m.fun, n, np_, m.lower, m.upper, rec["mfev"], **rec["params"])
        d.stable_sort = True
        d.start(before)
        d.iterate(mm.TableSource(m.table, n, np_, m.nmut, m.nmd))
        if st["stable"]:
            assert mm.state_crc(d.state()) == st["state_crc"], tag
        assert _ints(g, "sel_m") == d.sel_m and _ints(g, "sel_f") == d.sel_f, tag + "selection ranks"
        assert _ints(g, "src_m") == d.src_m and _ints(g, "src_f") == d.src_f, tag + "selection sources"
        tm, tf = [y.taint for y in d.males], [y.taint for y in d.females]
        worst.rows(g.get_state("males_x"), [y.x for y in d.males], tm, width, tag + "males_x")
        worst.rows(g.get_state("males_v"), [y.v for y in d.males], tm, width, tag + "males_v")
        worst.rows(g.get_state("males_bx"), [y.bx for y in d.males], tm, width, tag + "males_bx")
        worst.rows(g.get_state("females_x"), [y.x for y in d.females], tf, width, tag + "females_x")
        worst.rows(g.get_state("females_v"), [y.v for y in d.females], tf, width, tag + "females_v")
        worst.vals(g.get_state("males_f"), [y.f for y in d.males], tag + "males_f")
        worst.vals(g.get_state("males_bf"), [y.bf for y in d.males], tag + "males_bf")
        worst.vals(g.get_state("females_f"), [y.f for y in d.females], tag + "females_f")
    assert ran == sum(st["ok"] for st in rec["states"]) >= 4
    print("%s: %d generations; worst deviation of an exp() descendant %.3e of the box width (%s), of a value "
          "%.3e relative" % (name, ran, worst.x, worst.at, worst.f))
    assert worst.x <= XTOL and worst.f <= FTOL, (worst.x, worst.at, worst.f)


@pytest.mark.parametrize("obj", ["sphere", "rosenbrock"])
def test_outcome_bands_match_the_reference(hip, obj):
    b = GOLD["bands"]
    n, P = b["n"], b["count"]
    g = hip.Mayfly(b["np"], b["mfev"], seed=2024, populations=P)
    g.initialize(obj, -b["box"] * np.ones(n), b["box"] * np.ones(n), np.zeros(P * n))
    g.run(10 ** 6)
    got = [float(g.get_state("fbest", p)[0]) for p in range(P)]
    lo, hi = b[obj + "_fev"]
    assert all(int(g.get_state("flag", p)[0]) == 2 and lo <= int(g.get_state("fev", p)[0]) <= hi for p in range(P))
    band(got, _h(b[obj]), obj + " device")
