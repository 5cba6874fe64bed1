"""GPU: SLPSO fed the reference's own initial swarm and draws against the recorded reference
(tests/golden/slpso_runs.json, "steps").

The device takes the recorded initial positions through set_state("x") (which re-evaluates them, resets
pbest and abest in index order and zeroes the velocities) and the recorded permutation through
set_state("perm"); per generation it takes the draws the reference made of its recorded mt19937 words
through inject_draws, in the table tests/slpso_model.py writes while it replays the words (a draw the
reference did not make stays 0 and is never used).  Odd generations run through the fused kernel
(iterate), even ones through the phase path, one evaluation at a time.

After each recorded generation x v pb abest s vdavg perm Uf Pl alpha omega and every integer and flag (g
G m CF PF mfes fev) are the reference's BIT FOR BIT.  fx fpb fp fabest are held to 1e-10 relative -- the
repository's constant for an objective summed in another order (tests/test_nshs_golden_gpu.py).  p
accumulates differences of f and cannot be bit-exact where f is not: it is held to the same 1e-10.  The
test prints the worst deviations.

Measured on an MI355X over the five runs of eight generations: fx fpb fp fabest deviate by 4.4e-16 relative
at most, p by 1.3e-15 (n = 5; bit-exact at n = 2, where Rosenbrock is a single term), s by nothing."""
import numpy as np
import pytest

from test_slpso_model import GOLD, PERCOORD, _h, box_of, replay

pytestmark = pytest.mark.gpu

RTOL = 1e-10
BIT_KEYS = ("x", "v", "pb", "abest", "s", "vdavg", "Uf", "Pl")
INT_KEYS = ("g", "G", "m", "CF", "PF", "perm")
F_KEYS = ("fx", "fpb", "fp")


def close(a, b, what, rtol=RTOL):
    a, b = np.asarray(a, float).ravel(), np.asarray(b, float).ravel()
    assert a.shape == b.shape, what
    if a.tobytes() == b.tobytes():
        return 0.
    err = float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))
    assert err <= rtol, (what, err)
    return err


def bits(a, b, what):
    a, b = np.asarray(a, float).ravel(), np.asarray(b, float).ravel()
    assert a.shape == b.shape, what
    assert a.tobytes() == b.tobytes(), (what, np.flatnonzero(a != b)[:8], a[a != b][:4], b[a != b][:4])


def compare(g, want, tag, worst, population=0):
    """the device's state against a state of the reference (hex strings) or of the model (arrays)"""
    def val(k):
        v = want[k]
        if isinstance(v, str):
            return [float.fromhex(v)]
        if isinstance(v, list) and v and isinstance(v[0], str):
            return _h(v)
        return np.atleast_1d(np.asarray(v, float))

    def dev(k):
        return g.get_state(k, population)

    serr = close(dev("s"), val("s"), tag + "s", rtol=np.inf)
    if serr > worst["s"]:
        print("%ss deviates by %.3e relative" % (tag, serr))
    worst["s"] = max(worst["s"], serr)
    for k in BIT_KEYS + ("alpha", "omega"):
        bits(dev(k), val(k), tag + k)
    for k in INT_KEYS + ("mfes", "fev"):
        assert [int(v) for v in dev(k)] == [int(v) for v in val(k)], tag + k
    for k in F_KEYS + ("fabest",):
        worst["f"] = max(worst["f"], close(dev(k), val(k), tag + k))
    worst["p"] = max(worst["p"], close(dev("p"), val("p"), tag + "p"))


def phase_generation(g):
    """one generation through the phase path; returns the evaluations it made"""
    evals = 0
    while g.phase(0):
        g.phase(1)
        g.phase(2)
        evals += 1
    return evals


# (the last record: bounds that differ in every coordinate, tests/golden/slpso_percoord.json)
@pytest.mark.parametrize("rec", GOLD["steps"] + PERCOORD["steps"],
                         ids=[r["name"] for r in GOLD["steps"] + PERCOORD["steps"]])
def test_injected_reference_draws_reproduce_reference_states(hip, rec):
    n, np_ = rec["n"], rec["np"]
    lo, up = (np.asarray(v, float) for v in box_of(rec))
    if rec["box"] == "percoord":        # the reference's run redrew three coordinates or more at each wall
        assert min(rec["repairs"].values()) >= 3
    _, tables = replay(rec, check=False)
    g = hip.SLPSO(rec["mfev"], rec["stol"], np_, Ufmax=rec["Ufmax"], seed=5)
    g.initialize(rec["objective"], lo, up, np.zeros(n))
    ini = rec["init"]
    g.set_state("x", _h(ini["x"]))
    g.set_state("perm", ini["perm"])
    worst = {"f": 0., "p": 0., "s": 0.}
    compare(g, ini, rec["name"] + " init ", worst)
    fev = ini["fev"]
    for it, (st, tab) in enumerate(zip(rec["states"], tables), 1):
        g.inject_draws(tab)
        if it % 2:
            g.iterate()
        else:
            assert phase_generation(g) == st["fev"] - fev
        fev = st["fev"]
        compare(g, st, "%s generation %d " % (rec["name"], it), worst)
        assert int(g.get_state("it")[0]) == it and int(g.get_state("pending")[0]) == 0
        bits(g.solution().x, _h(st["abest"]), "solution")
    print("%s: worst relative deviation from the reference over %d generations: f %.3e, p %.3e, s %.3e"
          % (rec["name"], len(tables), worst["f"], worst["p"], worst["s"]))
    g.inject_draws(None)
    g.iterate()     # back on the device generator
    assert int(g.get_state("it")[0]) == len(rec["states"]) + 1
