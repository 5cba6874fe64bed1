"""CPU: tests/dsa_model.py against the recorded reference (tests/golden/dsa_runs.json, written by
scripts/gen_dsa_golden.py from the real DSSearch).

Reference order: every recorded state of the first four generations of six shapes, BIT FOR BIT
(the same IEEE operations in the same order; log and exp go through the same C library as the
harness did -- no tolerance is needed or given), and every generation consumes exactly the words
the reference consumed.

Keyed order (the device's draws): the outcome-band criterion -- the median of log10 f inside the
reference's inter-quartile band widened by 0.25 decade, the margin of tests/test_pop_bands_gpu.py
-- first on two fixed halves of the reference's own 256 seeds, then on 64 runs of the model with
NumPy draws, before tests/test_dsa_gpu.py uses it on the device.  Measured here with the compiled
reference: sphere quartiles -2.69 / -2.47 / -2.23 (the halves' medians -2.465 and -2.463),
Rosenbrock 1.14 / 1.30 / 1.48 (1.313 and 1.280): the reference passes with no widening at all."""
import json
import os

import numpy as np
import pytest

import chol_model
import dsa_model as dm
import jaya_model as jm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAND_MARGIN = 0.25      # decades

with open(os.path.join(ROOT, "tests", "golden", "dsa_runs.json")) as _fh:
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
    """median of log10 f inside the reference's inter-quartile band widened by BAND_MARGIN"""
    dev = np.log10(np.asarray(dev_f, float) + 1e-300)
    ref = np.log10(np.asarray(ref_f, float) + 1e-300)
    q1, q3 = np.percentile(ref, [25, 75])
    print("%s: median of log10 f %.3f, reference quartiles %.3f .. %.3f" % (what, np.median(dev), q1, q3))
    assert q1 - BAND_MARGIN <= np.median(dev) <= q3 + BAND_MARGIN, (what, np.median(dev), q1, q3)


def _model(rec):
    n = rec["n"]
    m = dm.Dsa(chol_model.objective(rec["objective"], n), -rec["box"] * np.ones(n), rec["box"] * np.ones(n),
               rec["np"], adapt=rec["adapt"], nbatch=rec["nbatch"], tol=rec["tol"], stol=rec["stol"])
    m.start(_h(rec["init"]["X"]), _h(rec["init"]["f"]))
    return m


@pytest.mark.parametrize("rec", GOLD["steps"], ids=[r["name"] for r in GOLD["steps"]])
def test_reference_order_reproduces_the_recorded_states_bit_for_bit(rec):
    m = _model(rec)
    ini = rec["init"]
    _same(m.w, _h(ini["w"]), "init w")
    _same(m.p, _h(ini["p"]), "init p")
    assert m.fev == ini["fev"] and m.it == ini["it"] and m.converged() == bool(ini["converged"])
    for g, st in enumerate(rec["states"], 1):
        w = jm.Words(st["words"])
        m.iterate_reference(w, st["imethd"] if rec["adapt"] else None)
        assert w.exhausted() and not w.have, (g, w.i, len(w.w))
        tag = "%s gen %d " % (rec["name"], g)
        assert m.imethd == st["imethd"], tag + "method"
        assert m.map.ravel().tolist() == st["map"], tag + "map"
        _same(m.dir, _h(st["dir"]), tag + "dir")
        _same(m.trial, _h(st["so"]), tag + "so")
        _same(m.ftrial, _h(st["fso"]), tag + "fso")
        _same(m.X, _h(st["X"]), tag + "X")
        _same(m.f, _h(st["f"]), tag + "f")
        _same(m.w, _h(st["w"]), tag + "w")
        _same(m.p, _h(st["p"]), tag + "p")
        assert (m.it, m.fev) == (st["it"], st["fev"]), tag
        assert m.converged() == bool(st["converged"]), tag


def test_fixture_covers_what_it_claims():
    steps = GOLD["steps"]
    assert {r["n"] for r in steps} <= set(range(1, 7)) and len({r["n"] for r in steps}) >= 5
    assert all(2 <= r["np"] <= 12 for r in steps) and any(r["np"] == 2 for r in steps)
    assert {r["adapt"] for r in steps} == {0, 1}
    assert all(len(r["states"]) == 4 for r in steps)
    methods, strategies = set(), set()
    for rec in steps:
        m = _model(rec)
        for st in rec["states"]:
            m.iterate_reference(jm.Words(st["words"]), st["imethd"])
            methods.add(m.imethd)
            strategies.add(m.strategy)
    assert methods == {0, 1, 2, 3} and strategies == {dm.RANDOM1, dm.DIFFERENTIAL, dm.RANDOM2}
    # the bandit's reset: an adaptive shape with nbatch = 2 whose weights fall back to 1 -- after
    # generation 3 (it = 2 on entry) only the method in use may differ from 1
    rec = next(r for r in steps if r["adapt"] and r["nbatch"] == 2)
    w2, w3 = _h(rec["states"][1]["w"]), _h(rec["states"][2]["w"])
    assert (w2 != 1.).sum() >= 1 and (w3 != 1.).sum() <= 1
    assert (np.delete(w3, rec["states"][2]["imethd"]) == 1.).all()
    rec = next(r for r in steps if r["adapt"] and r["nbatch"] == 100)
    assert (_h(rec["states"][3]["w"]) != 1.).sum() >= 2
    b = GOLD["bands"]
    assert len(b["sphere"]) == len(b["rosenbrock"]) == b["count"] == 256
    assert (b["n"], b["np"], b["mfev"], b["tol"], b["stol"], b["box"]) == (10, 40, 4000, 0., 0., 5.)
    assert [a["name"] for a in GOLD["signature"]] == ["mfev", "tol", "stol", "np", "adapt", "nbatch"]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "dsa_runs.json")) < 300 * 1024


def test_keyed_order_is_the_reference_order_given_the_same_decisions():
    """iterate_keyed fed draws that decide what the reference decided reproduces its generation:
    the raw uniforms are set so that the formulas give the recorded method, maps and repairs"""
    rec = next(r for r in GOLD["steps"] if r["name"].startswith("n5_np10"))
    n, np_ = rec["n"], rec["np"]
    ref, key = _model(rec), _model(rec)
    for st in rec["states"]:
        X0 = ref.X.copy()
        ref.iterate_reference(jm.Words(st["words"]), st["imethd"])
        mcap = 4
        md = np.zeros((np_, n + 2 + mcap))
        md[:, :n] = np.where(ref.map == 1, 0.25, 0.75)      # random-1 with rand = 0.5
        md[:, n] = 0.5
        dd = np.zeros((np_, 2))
        order = dm.ranked(key.f)
        dirrow = [int(np.flatnonzero((X0 == d).all(1))[0]) for d in ref.dir]
        if st["imethd"] == 0:
            dd[:, 0] = dirrow
        elif st["imethd"] == 1:         # ub = np, word -> the rank of the recorded row
            dd[:, 0] = 1. - 2. ** -53
            dd[:, 1] = [((order.index(r) << 32) + np_ - 1) // np_ for r in dirrow]
        elif st["imethd"] == 2:
            dd[0, 0] = (order.index(dirrow[0]) - 0.5) / np_ if order.index(dirrow[0]) < np_ - 1 else 0.999
        # the repairs: where the recorded trial sits on a bound the coin said "bound", else the
        # uniform is solved from the recorded value
        bd = np.zeros((np_, n, 2))
        so = _h(st["so"]).reshape(np_, n)
        lo, up = key.lo, key.up
        bd[..., 0] = ((so == lo) | (so == up)).astype(float)
        bd[..., 1] = (so - lo) / (up - lo)
        raw = [0., 0., (st["imethd"] + 0.5) / 4., 0.25, 0., 0.5]
        pre = key._trials(ref.R, ref.map.tolist(), dirrow)
        fixed = (pre < lo) | (pre > up)
        key.iterate_keyed(raw, ref.R, dd, md, bd, force_map=dm.RANDOM1)
        assert key.imethd == st["imethd"] and key.dirrow == dirrow
        assert key.map.tolist() == ref.map.tolist()
        # bit for bit, but for a coordinate redrawn inside the box: its uniform was solved from
        # the recorded value, one rounding away at most
        exact = ~fixed | (so == lo) | (so == up)
        _same(key.trial[exact], so[exact], "trial")
        assert np.all(np.abs(key.trial - so) <= 4 * np.spacing(up - lo))
        key.X, key.f = ref.X.copy(), ref.f.copy()
        assert (key.it, key.fev) == (ref.it, ref.fev)


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
def test_keyed_order_stays_inside_the_reference_bands(obj):
    """64 runs of Dsa.iterate_keyed, the code the device is held against, with NumPy draws in the
    device's recorded layouts -- like the device's 64 populations"""
    b = GOLD["bands"]
    n = b["n"]
    fobj = chol_model.objective(obj, n)
    lo, up = -b["box"] * np.ones(n), b["box"] * np.ones(n)
    got = [dm.run_keyed(np.random.default_rng(7000 + s), fobj, lo, up, b["np"], b["mfev"]) for s in range(64)]
    band(got, _h(b[obj]), obj + " keyed model")
