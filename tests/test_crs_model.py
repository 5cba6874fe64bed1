"""CPU: tests/crs_model.py against the recorded reference (tests/golden/crs_runs.json, written by
scripts/gen_crs_golden.py from the reference's own crs.cpp), and the model's own bounds.

Fed the raw mt19937 words an iteration of the reference consumed, the model's reference form reproduces
every point the reference handed to the objective, in order, with its value, and the sorted values, the
place of the new point, fev, _trial and _ftrial after the iteration, bit for bit.  Nothing here needs the
reference or oracle/_ref."""
import json
import os

import numpy as np
import pytest

import chol_model
import crs_model as cm
import jaya_model as jm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "crs_runs.json")
with open(PATH) as _fh:
    GOLD = json.load(_fh)
STEPS = {rec["name"]: rec for rec in GOLD["steps"]}
PATHS = ("B", "mut_acc", "M", "M_stale", "M_inner_mut", "popB_fail", "depth3")


def _h(v):
    if isinstance(v, str):
        return float.fromhex(v)
    return [float.fromhex(s) for s in v]


def _same(a, b, what):
    a, b = np.asarray(a, float).ravel(), np.asarray(b, float).ravel()
    assert a.shape == b.shape and a.tobytes() == b.tobytes(), (what, a[:4], b[:4])


def start_model(rec, f=None, **kw):
    """the model on the recorded initial pool, which the reference keeps sorted"""
    n, np_, box = rec["n"], rec["np"], rec["box"]
    f = chol_model.objective(rec["objective"], n) if f is None else f
    m = cm.Crs(f, n, np_, [-box] * n, [box] * n, rec["mfev"], 0., **kw)
    x0 = _h(rec["init"]["x"])
    return m, [x0[i * n:(i + 1) * n] for i in range(np_)]


def expand(st, n):
    """a recorded state as the harness wrote it (scripts/gen_crs_golden.py, compress()): "evals" flat, an
    index put back as the entry it names; "trial" and "ftrial" from the evaluation "trial_eval" names"""
    entries = []
    for e in st["evals"]:
        entries.append(entries[e] if isinstance(e, int) else _h(e))
    last = entries[st["trial_eval"]]
    return dict(st, evals=[v for e in entries for v in e], trial=last[:n], ftrial=last[n], count=len(entries))


def replay(rec):
    """yields (iteration, model, recorded state put back by expand()) after each recorded iteration"""
    n, np_ = rec["n"], rec["np"]
    m, x0 = start_model(rec)
    m.start(x0)
    _same(m.fs, _h(rec["init"]["f"]), rec["name"] + " init f")
    assert m.order == list(range(np_)) and m.fev == rec["init"]["fev"] == np_
    for k, st in enumerate(rec["states"]):
        w = jm.Words(st["words"])
        assert m.iterate(cm.WordsSource(w, n, np_))
        assert w.exhausted(), (rec["name"], k)
        yield k, m, expand(st, n)


@pytest.mark.parametrize("name", sorted(STEPS))
def test_the_model_reproduces_the_recorded_reference_bit_for_bit(name):
    rec = STEPS[name]
    n = rec["n"]
    assert len(rec["states"]) == 24
    paths = None
    deep, fev = 0, rec["np"]
    for k, m, st in replay(rec):
        tag = "%s iteration %d " % (name, k)
        _same([v for x, fx in m.evals for v in x + [fx]], st["evals"], tag + "evaluated points")
        _same(m.t, st["trial"], tag + "_trial")
        _same([m.ft], [st["ftrial"]], tag + "_ftrial")
        _same(m.x()[st["slot"]], st["trial"], tag + "the row that changed")
        assert (m.slot, m.fev) == (st["slot"], st["fev"]), tag
        fev += st["count"]
        assert m.fev == fev, tag
        deep += m.maxdepth >= 3
        paths = dict(m.paths)
    # the sorted values are kept for the last iteration: every one before it changed them by _ftrial at slot
    _same(m.fsorted(), _h(rec["states"][-1]["f"]), name + " f")
    paths["depth3"] = deep
    assert {k: paths[k] for k in PATHS} == {k: rec["paths"][k] for k in PATHS}
    assert m.stale == rec["paths"]["stale"]


def test_every_path_is_recorded_at_least_twice():
    total = {k: sum(rec["paths"][k] for rec in GOLD["steps"]) for k in PATHS}
    assert total == {k: GOLD["paths"][k] for k in PATHS}
    for k in PATHS:
        assert total[k] >= 2, (k, total)
    shapes = sorted((rec["n"], rec["np"]) for rec in GOLD["steps"])
    assert shapes == [(1, 3), (2, 5), (3, 7), (5, 20), (9, 20), (17, 40)]
    assert STEPS["n1_np3"]["objective"] == "sphere"
    assert len({rec["objective"] for rec in GOLD["steps"]}) >= 3


def test_no_tie_and_no_close_decision_where_the_objective_is_a_sum():
    """every pair of stored values and every trial value against the worst differ by more than 1e-6
    relative; the two shapes whose objective is ONE term (the sphere at n = 1, Rosenbrock at n = 2: the
    same bits on the device whatever the order of a sum) are recorded as they run, see
    scripts/gen_crs_golden.py"""
    def far(a, b):
        return abs(a - b) > 1e-6 * max(abs(a), abs(b))
    for rec in GOLD["steps"]:
        n = rec["n"]
        if (rec["objective"], n) in (("sphere", 1), ("rosenbrock", 2)):
            assert rec["np"] <= 16
            continue
        f = _h(rec["init"]["f"])
        for raw in rec["states"]:
            st = expand(raw, n)
            assert all(far(a, b) for a, b in zip(f, f[1:])), rec["name"]
            ev = st["evals"]
            assert all(far(ev[k * (n + 1) + n], f[-1]) for k in range(st["count"])), rec["name"]
            f = f[:-1]
            f.insert(st["slot"], st["ftrial"])
            assert f == sorted(f), rec["name"]
        assert f == _h(rec["states"][-1]["f"]) and all(far(a, b) for a, b in zip(f, f[1:])), rec["name"]


def test_the_fixture_is_small_and_holds_the_bands_and_the_signature():
    assert os.path.getsize(PATH) < 300 * 1024
    b = GOLD["bands"]
    assert (b["n"], b["np"], b["tol"], b["count"]) == (10, 110, 0., 256) and b["mfev"] <= 4000
    for obj in ("sphere", "rosenbrock"):
        f = _h(b[obj])
        assert len(f) == 256 and f == sorted(f)
        lo, hi, mean = _h(b[obj + "_stale_share"])
        assert 0. <= lo <= mean <= hi <= 1.
        assert _h(b[obj + "_fworst_min"]) > f[0]        # no pool collapsed
    assert GOLD["signature"] == [{"name": k, "required": True} for k in ("mfev", "np", "tol")]


def test_the_logged_records_replay_the_walk():
    """what the model logs while it reads the reference's words is the table of bbo_crs_inject_draws:
    read back through TableSource it gives the same iteration"""
    rec = STEPS["n3_np7"]
    n, np_ = rec["n"], rec["np"]
    other, x0 = start_model(rec)
    other.start(x0)
    for k, m, st in replay(rec):
        src = cm.TableSource(m.records, n, np_)
        assert other.iterate(src) and src.exhausted()
        _same(other.x(), m.x(), "x %d" % k)
        assert (other.fev, other.trials, other.muts, other.stale) == (m.fev, m.trials, m.muts, m.stale)
        for r in m.records:
            assert len(r) == 2 * n and all(-1. <= v < np_ for v in r[:n]) and all(0. <= v < 1. for v in r[n:])


@pytest.mark.parametrize("name", ["n2_np5", "n5_np20"])
def test_repair_never_replaces_the_worst_with_a_point_that_is_not_better(name):
    rec = STEPS[name]
    n, np_ = rec["n"], rec["np"]
    m, x0 = start_model(rec, repair=True)
    m.start(x0)
    rng = np.random.default_rng(5)
    for k in range(40):
        fworst = m.fsorted()[-1]
        fev = m.fev
        assert m.iterate(cm.RngSource(rng, n, np_))
        assert m.ft < fworst and m.maxdepth <= m.max_depth
        # the accepted point is evaluated once: the last evaluation is the point that went in
        assert m.fev - fev == len(m.evals) and m.evals[-1] == (m.t, m.ft)
        assert m.fsorted() == sorted(m.fsorted()) and m.x()[m.slot] == m.t
    assert m.stale == 0 and m.paths["M"] == 0 and m.paths["B"] == 0


@pytest.mark.parametrize("max_depth", [1, 8, 37])
def test_a_collapsed_box_stops_with_flag_3_at_the_count_the_recursion_implies(max_depth):
    """lower == upper == 0: every point is the box, every trial and every mutation is the point again
    (sums and products of zeros), so every trial is evaluated, mutated, evaluated again and rejected: M
    is pushed until the stack is full, two evaluations per frame and two more for the trial that finds
    it full"""
    n, np_ = 3, 4
    f = chol_model.objective("sphere", n)
    m = cm.Crs(f, n, np_, [0.] * n, [0.] * n, 10 ** 6, 0., max_depth=max_depth)
    m.start([[0.] * n] * np_)
    before = m.x()
    assert m.iterate(cm.RngSource(np.random.default_rng(1), n, np_)) is False
    assert m.flag == 3 and m.it == 0 and not m.converged()
    assert m.fev == np_ + 2 * (max_depth + 1) and m.trials == max_depth + 1
    assert m.x() == before and m.stale == 0
    # the loop of the paper redraws instead and ends on the budget
    r = cm.Crs(f, n, np_, [0.] * n, [0.] * n, 50, 0., max_depth=max_depth, repair=True)
    r.start([[0.] * n] * np_)
    assert r.iterate(cm.RngSource(np.random.default_rng(1), n, np_)) is False
    assert r.flag == 2 and r.fev == 50 and r.it == 0 and r.x() == before


def test_a_nan_value_counts_as_inf_and_a_new_point_goes_behind_its_equals():
    n, np_ = 2, 4
    f = lambda x: float("nan") if x[0] > 0.5 else x[0] * x[0] + x[1] * x[1]    # noqa: E731
    m = cm.Crs(f, n, np_, [-1.] * n, [1.] * n, 1000, 0.)
    m.start([[0.9, 0.], [0.25, 0.], [-0.25, 0.], [0., 0.]])
    assert m.order == [3, 1, 2, 0] and m.fsorted()[-1] == cm.INF       # (the tie keeps row order)
    # ranks 1 and 2 (the rows +-0.25): centroid (0 + 0.25) / 2, reflected through -0.25 gives (0.5, 0)
    src = cm.TableSource([[1., 2., 0.5, 0.5]], n, np_)
    assert m.iterate(src)
    assert m.t == [0.5, 0.] and m.slot == 3 and m.order == [3, 1, 2, 0]
    # a value equal to two stored ones goes behind both
    m.start([[0.9, 0.], [0.25, 0.], [-0.25, 0.], [0., 0.]])
    m.rows[0], m.fs[0] = [0.5, 0.], 0.25
    m.order = [3, 1, 2, 0]
    src = cm.TableSource([[0., 1., 0.5, 0.5]], n, np_)     # (0 + 0) / 2 reflected through 0.25: (-0.25, 0)
    assert m.iterate(src)
    assert m.t == [-0.25, 0.] and m.slot == 3 and m.order == [3, 1, 2, 0] and m.fsorted() == [0., 0.0625, 0.0625, 0.0625]
