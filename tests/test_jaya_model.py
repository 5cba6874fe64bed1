"""CPU: tests/jaya_model.py against the recorded reference (tests/golden/jaya_runs.json, written
by scripts/gen_jaya_golden.py from the real JayaSearch).

Reference order: every recorded state of the first three generations of six shapes, BIT FOR BIT
for all four mutations (the same IEEE operations in the same order; levy's pow and sigma_u's
tgamma go through the same C library as the harness did -- no tolerance is needed or given),
and every generation consumes exactly the words the reference consumed.

Synchronous order (the device's): the outcome-band criterion of tests/test_bands_gpu.py for a
fixed budget (APSO's: the median of log10 f inside the reference's inter-quartile band widened by
one decade), first on two disjoint halves of the reference's own 256 seeds, then on the model
with NumPy draws -- before tests/test_jaya_gpu.py uses it on the device."""
import json
import os

import numpy as np
import pytest

import chol_model
import jaya_model as jm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

with open(os.path.join(ROOT, "tests", "golden", "jaya_runs.json")) as _fh:
    GOLD = json.load(_fh)


def _h(v):
    return np.array([float.fromhex(x) for x in v])


def _same(a, b, what):
    a, b = np.asarray(a, float).ravel(), np.asarray(b, float).ravel()
    assert a.shape == b.shape, what
    assert a.tobytes() == b.tobytes() or all(
        (x == y and np.signbit(x) == np.signbit(y)) or (x != x and y != y) for x, y in zip(a, b)), \
        (what, a, b)


def band(dev_f, ref_f, what):
    """median of log10 f inside the reference's inter-quartile band widened by one decade"""
    dev = np.log10(np.asarray(dev_f, float) + 1e-300)
    ref = np.log10(np.asarray(ref_f, float) + 1e-300)
    q1, q3 = np.percentile(ref, [25, 75])
    assert q1 - 1. <= np.median(dev) <= q3 + 1., (what, np.median(dev), q1, q3)


@pytest.mark.parametrize("rec", GOLD["steps"], ids=[r["name"] for r in GOLD["steps"]])
def test_reference_order_reproduces_the_recorded_states_bit_for_bit(rec):
    n, np_ = rec["n"], rec["np"]
    lo, up = -rec["box"] * np.ones(n), rec["box"] * np.ones(n)
    m = jm.Jaya(chol_model.objective(rec["objective"], n), lo, up, np_, rec["npmin"],
                adapt=rec["adapt"], k0=rec["k0"], mutation=jm.MUTATIONS[rec["mutation"]],
                scale=rec["scale"], beta=rec["beta"], temper=rec["temper"], tol=rec["tol"],
                order="reference")
    ini = rec["init"]
    m.start(_h(ini["X"]), _h(ini["f"]), _h(ini["xchaos"])[0])
    _same(m.fgbest, _h(ini["fgbest"]), "init fgbest")
    _same(m.bestx, _h(ini["bestx"]), "init bestx")
    _same(m.best, _h(ini["best"]), "init best")
    assert m.fev == ini["fev"] and m.k == ini["k"] and m.converged() == bool(ini["converged"])
    for g, st in enumerate(rec["states"], 1):
        w = jm.Words(st["words"])
        m.iterate_reference(w)
        assert w.exhausted() and not w.have, (g, w.i, len(w.w))
        tag = "%s gen %d " % (rec["name"], g)
        _same(m.X[m.occ], _h(st["X"]), tag + "X")          # the pool in slot order
        _same(m.f[m.occ], _h(st["f"]), tag + "f")
        assert m.len == [int(v) for v in _h(st["len"])], tag + "len"
        _same(m.xchaos, _h(st["xchaos"]), tag + "xchaos")
        _same(m.pstrat, _h(st["pstrat"]), tag + "pstrat")
        _same(m.perfindex, _h(st["perfindex"]), tag + "perfindex")
        _same(m.best, _h(st["best"]), tag + "best")
        _same(m.fgbest, _h(st["fgbest"]), tag + "fgbest")
        _same(m.bestx, _h(st["bestx"]), tag + "bestx")
        assert (m.k, m.fev) == (st["k"], st["fev"]), tag
        assert m.converged() == bool(st["converged"]), tag


def test_fixture_covers_what_it_claims():
    steps = GOLD["steps"]
    assert {r["mutation"] for r in steps} == set(jm.MUTATIONS)
    assert {r["adapt"] for r in steps} == {0, 1} and any(r["k0"] == 1 for r in steps)
    assert any(r["np"] % r["k0"] for r in steps)
    assert any(r["k0"] == jm.count_ks(r["np"], r["npmin"]) > 1 for r in steps)
    b = GOLD["bands"]
    assert len(b["sphere"]) == len(b["rosenbrock"]) == b["count"] == 256
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "jaya_runs.json")) < 300 * 1024


@pytest.mark.parametrize("obj", ["sphere", "rosenbrock"])
def test_band_criterion_holds_between_halves_of_the_reference(obj):
    """the criterion separates nothing that is the same: 128 seeds against the other 128.  The
    recorded values are sorted, so the halves are drawn by a fixed permutation."""
    v = _h(GOLD["bands"][obj])
    idx = np.random.default_rng(0).permutation(v.size)
    a, b = v[idx[:128]], v[idx[128:]]
    band(a, b, obj + " first half")
    band(b, a, obj + " second half")


@pytest.mark.parametrize("obj", ["sphere", "rosenbrock"])
def test_synchronous_order_stays_inside_the_reference_bands(obj):
    """64 runs of the model in the device's order (NumPy draws), like the device's 64 populations"""
    b = GOLD["bands"]
    n = b["n"]
    rows = chol_model.objective_rows(obj, n)
    lo, up = -b["box"] * np.ones(n), b["box"] * np.ones(n)
    got = [jm.run_sync(np.random.default_rng(7000 + s), rows, lo, up, b["np"], b["npmin"], b["mfev"])
           for s in range(64)]
    print("sync model %s: quartiles of log10 f" % obj, np.percentile(np.log10(got), [25, 50, 75]),
          "reference", np.percentile(np.log10(_h(b[obj])), [25, 50, 75]))
    band(got, _h(b[obj]), obj + " sync model")
