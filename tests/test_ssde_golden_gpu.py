"""GPU: SSDE fed the reference's own states and draws against the recorded reference
(tests/golden/ssde_runs.json, "steps").  The draws are the outcomes the reference arrived at from its
recorded mt19937 words, in the table tests/ssde_model.py writes while it replays them (a draw the reference
did not make stays 0 and is never used).

Tier 1, generation by generation.  Before each recorded generation the device is SET to the reference's
state before it (x -- which re-evaluates and re-sorts --, L1 L2 LCR k kCR fev convcount) and fed its draws,
then runs one generation: odd ones through iterate(), even ones through the phase path, one evaluation at a
time.  x, np, k, kCR, fev, convcount, perm (x is in rank order, so this is the rank order too) and, on the
phase path, every point handed to the objective are the reference's BIT FOR BIT.  f is held to 1e-10
relative -- the repository's constant for an objective summed in another order
(tests/test_slpso_golden_gpu.py) --, and bit for bit at n = 1 and n = 2, where the objective is one term.
The entries of L1 L2 LCR written in the generation are weighted Lehmer means whose weights are differences
f_i - fy of such values: they are held to 4 * 1e-10 * max_i (|f_i| + |fy_i|) / (f_i - fy_i) over that
generation's successes, a bound the test derives from the fixture (a weighted mean's error is at most the
largest relative error of its weights); every other entry is bit for bit.

Tier 2, six generations without re-setting: same draws, against the recorded states.  The integers stay
exact.  The tolerances are 100 times the worst deviation measured once on an MI355X (MEASURED below; the
test prints the worst deviation per key before it asserts).  L2 enters y only through ci, and the table
carries the ci the reference accepted, so on this path the memories' last-bit drift never reaches a point:
x was measured at 0 and is therefore held bit for bit here too.

Measured on an MI355X, worst over the six records.  Tier 1: f 3.9e-16 relative (0 at n = 1 and 2), the
written memory entries within 5.2e-16 of the reference (their bounds lie between 1e-9 and 1e-5).  Tier 2
after six generations: x 0, f 3.9e-16, L1 2.0e-16, L2 5.2e-16, LCR 1.1e-16."""
import json
import os

import numpy as np
import pytest

import chol_model
import ssde_model as sm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-10
# tier 2: the worst relative deviation from the reference after six generations, measured on an MI355X
MEASURED = {"x": 0., "f": 3.878e-16, "L1": 2.037e-16, "L2": 5.163e-16, "LCR": 1.110e-16}

with open(os.path.join(ROOT, "tests", "golden", "ssde_runs.json")) as _fh:
    STEPS = sm.load_steps(json.load(_fh))
# one record under bounds that differ in every coordinate: held generation by generation (tier 1); the tier 2
# bounds below were measured on the records of ssde_runs.json
with open(os.path.join(ROOT, "tests", "golden", "ssde_percoord.json")) as _fh:
    PERCOORD = sm.load_steps(json.load(_fh))
_CACHE = {}


def tables(rec):
    """the record's draw tables and successes, made once"""
    if rec["name"] not in _CACHE:
        _CACHE[rec["name"]] = sm.tables_of(rec, chol_model.objective(rec["objective"], rec["n"]))
    return _CACHE[rec["name"]]


def bits(a, b, what):
    a, b = np.asarray(a, float).ravel(), np.asarray(b, float).ravel()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert a.tobytes() == b.tobytes(), (what, np.flatnonzero(a != b)[:8], a[a != b][:4], b[a != b][:4])


def rel(a, b):
    a, b = np.asarray(a, float).ravel(), np.asarray(b, float).ravel()
    assert a.shape == b.shape
    if a.tobytes() == b.tobytes():
        return 0.
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def make(hip, rec):
    n = rec["n"]
    g = hip.SSDE(rec["mfev"], rec["npinit"], rec["tol"], rec.get("patience", 1000), rec.get("npmin", 4),
                 rec.get("ptop", 0.11), rec.get("h", 100), bool(rec.get("usede", 0)), bool(rec.get("repaircr", 1)),
                 seed=5)
    lo, up = (np.asarray(v, float) for v in sm.box_of(rec))
    g.initialize(rec["objective"], lo, up, np.zeros(n))
    return g


def load(g, st):
    g.set_state("x", st["x"])
    for k in ("L1", "L2", "LCR"):
        g.set_state(k, st[k])
    for k in ("k", "kCR", "fev", "convcount"):
        g.set_state(k, [st[k]])


def ints(g, st, tag):
    for k in sm.INT_KEYS:
        assert int(g.get_state(k)[0]) == st[k], (tag, k, g.get_state(k)[0], st[k])
    assert [int(v) for v in g.get_state("perm")] == st["perm"], tag


def phase_generation(g, pts, tag):
    """one generation through the phase path, every pending point against the reference's"""
    evals = 0
    while g.phase(0):
        assert evals < len(pts), tag
        bits(g.get_state("cand"), pts[evals], "%s point %d" % (tag, evals))
        g.phase(1)
        g.phase(2)
        evals += 1
    return evals


def memory_bound(pairs):
    return 4. * RTOL * max((abs(fi) + abs(fy)) / (fi - fy) for fi, fy in pairs)


@pytest.mark.parametrize("rec", STEPS + PERCOORD, ids=[r["name"] for r in STEPS + PERCOORD])
def test_generation_by_generation_from_the_reference_state(hip, rec):
    tabs, successes = tables(rec)
    if rec["box"] == "percoord":        # the reference's run redrew three coordinates or more past each bound
        assert min(rec["repairs"].values()) >= 3
    g = make(hip, rec)
    exact_f = rec["n"] <= 2
    worst_f = worst_m = 0.
    before = rec["init"]
    for it, (st, tab, (ss, de)) in enumerate(zip(rec["states"], tabs, successes), 1):
        tag = "%s generation %d" % (rec["name"], it)
        load(g, before)
        bits(g.get_state("x"), before["x"], tag + " loaded x")
        assert int(g.get_state("np")[0]) == before["np"]
        g.inject_draws(tab)
        if it % 2:
            g.iterate()
        else:
            assert phase_generation(g, st["pts"], tag) == st["fev"] - before["fev"] == len(st["pts"])
        assert int(g.get_state("pending")[0]) == 0
        bits(g.get_state("x"), st["x"], tag + " x")
        ints(g, st, tag)
        bits(g.solution().x, st["x"][:rec["n"]], tag + " solution")
        err = rel(g.get_state("f"), st["f"])
        worst_f = max(worst_f, err)
        assert err <= (0. if exact_f else RTOL), (tag, "f", err)
        for key, slot, pairs in (("L1", before["k"] - 1, ss), ("L2", before["k"] - 1, ss),
                                 ("LCR", before["kCR"] - 1, de)):
            dev, ref = g.get_state(key), st[key]
            written = np.zeros(len(ref), bool)
            if pairs:
                written[slot] = True
                e = abs(dev[slot] - ref[slot]) / abs(ref[slot])
                worst_m = max(worst_m, e)
                assert e <= (0. if exact_f else memory_bound(pairs)), (tag, key, e, memory_bound(pairs))
            bits(dev[~written], ref[~written], tag + " " + key)
        before = st
    print("%s: tier 1 worst relative deviation: f %.3e, written memory entries %.3e" % (rec["name"], worst_f, worst_m))
    g.inject_draws(None)
    g.iterate()     # back on the device generator
    assert int(g.get_state("gen")[0]) >= 1


@pytest.mark.parametrize("rec", STEPS, ids=[r["name"] for r in STEPS])
def test_six_generations_without_resetting(hip, rec):
    tabs, _ = tables(rec)
    g = make(hip, rec)
    load(g, rec["init"])
    worst = {k: 0. for k in sm.FLOAT_KEYS}
    for it, (st, tab) in enumerate(zip(rec["states"], tabs), 1):
        tag = "%s generation %d" % (rec["name"], it)
        g.inject_draws(tab)
        g.iterate()
        ints(g, st, tag)
        for k in sm.FLOAT_KEYS:
            worst[k] = max(worst[k], rel(g.get_state(k), st[k]))
    print("%s: tier 2 worst relative deviation after %d generations: %s"
          % (rec["name"], len(tabs), " ".join("%s %.3e" % (k, worst[k]) for k in sm.FLOAT_KEYS)))
    for k in sm.FLOAT_KEYS:
        assert worst[k] <= 100. * MEASURED[k], (rec["name"], k, worst[k], MEASURED[k])
