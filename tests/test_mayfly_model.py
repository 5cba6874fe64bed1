"""CPU: tests/mayfly_model.py against the recorded reference (tests/golden/mayfly_runs.json, written by
scripts/gen_mayfly_golden.py from the reference's own MayflySearch).

The fixture stores a run as its seed and the number of mt19937 words each generation took: the words are
regenerated here (mayfly_model.mt19937_words) and decoded in the reference's program order.  Every value
handed back by the objective must be the recorded one bit for bit, and CRC-32 sums pin every bit of the
points handed to the objective and of the whole state after every generation."""
import json
import os
import random

import pytest

import chol_model
import jaya_model
import mayfly_model as mm

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mayfly_runs.json")
with open(PATH) as fh:
    GOLD = json.load(fh)
STEPS = {rec["name"]: rec for rec in GOLD["steps"]}
# one short record under bounds that differ in every coordinate (tests/_boxes.py): its "box" is "percoord"
with open(os.path.join(os.path.dirname(PATH), "mayfly_percoord.json")) as fh:
    PERCOORD = {rec["name"]: rec for rec in json.load(fh)["steps"]}
PATHS = ("f_attract", "f_random", "m_attract", "m_dance", "improve_not_last", "short_window", "aliased",
         "clamp_box", "clamp_vmax")


def _h(v):
    return [float.fromhex(s) for s in v]


def bounds_of(rec):
    if rec["box"] == "percoord":
        from _boxes import percoord_box
        return [list(v) for v in percoord_box(rec["n"])]
    return [rec["lower"]] * rec["n"], [rec["box"]] * rec["n"]


def reference_model(rec, **kw):
    """(model, source) at the recorded run's init()"""
    n, np_ = rec["n"], rec["np"]
    words = jaya_model.Words(mm.mt19937_words(rec["seed"], sum(rec["nwords"])))
    par = dict(rec["params"])
    par.update(kw)
    lo, up = bounds_of(rec)
    m = mm.Mayfly(chol_model.objective(rec["objective"], n), n, np_, lo, up, rec["mfev"], **par)
    m.init_words(words)
    assert words.i == rec["nwords"][0]
    return m, mm.WordsSource(words, n)


def walk(rec):
    """the recorded run generation by generation: (index, recorded generation, state before, model after)"""
    m, src = reference_model(rec)
    at = rec["nwords"][0]
    for g, st in enumerate(rec["states"]):
        before = m.state()
        m.iterate(src)
        at += rec["nwords"][g + 1]
        assert src.w.i == at, (rec["name"], g)
        yield g, st, before, m


def _check(m, st, tag):
    assert mm.crc(fx for _, fx in m.evals) == st["values_crc"], tag + "values"
    assert mm.crc(v for x, _ in m.evals for v in x) == st["points_crc"], tag + "points"
    assert mm.state_crc(m.state()) == st["state_crc"], tag + "state"
    assert m.fbest == float.fromhex(st["fbest"]), tag + "fbest"


@pytest.mark.parametrize("name", sorted(STEPS) + sorted(PERCOORD))
def test_the_model_replays_the_recorded_reference(name):
    rec = STEPS.get(name) or PERCOORD[name]
    m, _ = reference_model(rec)
    _check(m, rec["init"], name + " init ")
    assert m.nmut == rec["nmut"]
    np_ = rec["np"]
    for g, st, _, m in walk(rec):
        tag = "%s generation %d " % (name, g)
        _check(m, st, tag)
        assert len(m.evals) == 3 * np_ + m.nmut and m.fev == st["fev"] and m.took == st["took"], tag
        assert (m.duplicates(True), m.duplicates(False)) == (st["dup_m"], st["dup_f"]), tag
    assert m.fev == 2 * np_ + len(rec["states"]) * (3 * np_ + m.nmut)


def test_the_percoord_record_clamps_at_the_box_and_at_vmax():
    """the record that pins vmax = k (up[j] - lo[j]), the mutation's sigma and the clamps under bounds that differ
    in every coordinate: both clamps fire in generations the device can be held to, and every point the model
    evaluates on the way lies in its coordinate's interval"""
    (rec,) = PERCOORD.values()
    assert rec["n"] <= 12 and len(rec["states"]) <= 5 and rec["nmut"] >= 1
    assert rec["paths"]["clamp_box"] >= 3 and rec["paths"]["clamp_vmax"] >= 3
    lo, up = bounds_of(rec)
    for g, st, _, m in walk(rec):
        for x, _ in m.evals:
            assert all(a <= v <= b for a, v, b in zip(lo, x, up)), g
    percoord_witness(rec)


def percoord_witness(rec):
    """from the reference's recorded run alone (the model reproduces it bit for bit): over the generations,
    at least three coordinates of the flies on their lower bound, three on their upper bound, and three strictly
    inside in every fly"""
    import numpy as np
    from _boxes import binding_witness
    lo, up = (np.asarray(v, float) for v in bounds_of(rec))
    states = []
    for _, _, _, m in walk(rec):
        st = m.state()
        states += [np.asarray(st["males_x"], float), np.asarray(st["females_x"], float)]
    return binding_witness(states, lo, up)


def test_the_fixture_holds_the_shapes_the_paths_the_bands_and_the_signature():
    assert os.path.getsize(PATH) < 64 * 1024
    shapes = {(r["n"], r["np"], r["nmut"], bool(r["params"].get("pgb"))) for r in GOLD["steps"]}
    assert shapes == {(1, 2, 0, False), (2, 4, 0, False), (3, 6, 0, False), (17, 10, 0, False), (17, 10, 4, False),
                      (33, 40, 2, True), (65, 66, 4, False)}
    assert STEPS["n65_np66"]["params"] == {"pmutdim": 0.1}
    for k in PATHS:
        assert GOLD["paths"][k] >= 2, k
        assert GOLD["paths"][k] == sum(r["paths"][k] for r in GOLD["steps"])
    for rec in GOLD["steps"]:
        ok = sum(st["ok"] for st in rec["states"])
        assert ok >= 4 and all(st["ok"] or not st["stable"] for st in rec["states"]), rec["name"]
        # about half of each swarm is an exact duplicate after a generation of the reference
        if rec["np"] >= 10:
            assert max(st["dup_m"] for st in rec["states"]) >= rec["np"] // 4, rec["name"]
    b = GOLD["bands"]
    assert (b["n"], b["np"], b["count"]) == (10, 20, 256)
    for obj in ("sphere", "rosenbrock"):
        f = _h(b[obj])
        assert len(f) == 256 and f == sorted(f)
        lo, hi = b[obj + "_fev"]
        assert b["mfev"] <= lo <= hi < b["mfev"] + 3 * b["np"] + 2
    names = [s["name"] for s in GOLD["signature"]]
    assert names == ["np", "mfev", "a1", "a2", "a3", "beta", "dance", "ddamp", "fl", "fldamp", "gmin", "gmax",
                     "vdamp", "sigma", "pmutdim", "pmutnp", "l", "pgb"]
    assert [s["name"] for s in GOLD["signature"] if s["required"]] == ["np", "mfev"]
    for s in GOLD["signature"][2:]:
        assert s["default"] == mm.DEFAULTS[s["name"]], s


@pytest.mark.parametrize("name", sorted(STEPS))
def test_the_stable_order_and_the_logged_table_give_the_stable_generations(name):
    """what the GPU test relies on: from the state before a generation, the table the model logged while it
    read the reference's words and the STABLE order in every sort give the reference's state after it in
    every generation marked stable; there the chain over integers landed what the in-place loop landed"""
    rec = STEPS[name]
    n, np_ = rec["n"], rec["np"]
    for g, st, before, m in walk(rec):
        if not st["stable"]:
            continue
        assert m.chain_ok
        d = mm.Mayfly(m.fun, n, np_, m.lower, m.upper, rec["mfev"], **rec["params"])
        d.stable_sort = True
        d.start(before)
        d.iterate(mm.TableSource(m.table, n, np_, m.nmut, m.nmd))
        assert mm.state_crc(d.state()) == st["state_crc"], (name, g)
        assert d.table == m.table and d.src_m == m.src_m and d.src_f == m.src_f, (name, g)


@pytest.mark.parametrize("name", ["n17_np10_mut", "n33_np40_pgb"])
def test_repair_selects_from_untouched_copies(name):
    """repair=True: every slot takes the record the sort put at its rank, as it was before the selection
    wrote anything; the flies start at the points they drew"""
    rec = STEPS[name]
    m, src = reference_model(rec, repair=True)
    assert all(any(y.x) and not any(y.v) for y in m.males + m.females)
    m.stable_sort = True
    for g in range(6):
        m.iterate(src)
        assert m.src_m == m.sel_m[:rec["np"]] and m.src_f == m.sel_f[:rec["np"]]
        pool = ([m.moved_males[t] for t in m.rank_m] + [m.offspring[k] for k in m.perm_o[:rec["np"] // 2]]
                + [m.mutated[u] for u in m.perm_u[:m.nmut // 2]])
        for j, y in enumerate(m.males):
            assert y.fields(True) == pool[m.src_m[j]].fields(True), (g, j)


def test_std_sort_is_a_sort_and_stable_up_to_16_keys():
    rng = random.Random(5)
    for count in (1, 2, 7, 16, 17, 40, 99, 300):
        for _ in range(20):
            keys = [float(rng.randrange(6)) for _ in range(count)]
            order = mm.std_sort(keys)
            assert sorted(order) == list(range(count))
            assert all(keys[a] <= keys[b] for a, b in zip(order, order[1:]))
            if count <= 16:
                assert order == sorted(range(count), key=lambda t: keys[t])
