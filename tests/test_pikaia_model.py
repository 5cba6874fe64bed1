"""CPU: tests/pikaia_model.py against the recorded reference (tests/golden/pikaia_runs.json, written by
scripts/gen_pikaia_golden.py from the real PikaiaSearch).

The model replays every recorded run bit for bit over the words of std::mt19937(seed): the word count of every
generation, pmut, the elite decision, fev, and the CRC-32 sums of the new phenotypes, of the values handed back
by the objective, of the state after the generation and of the rank order (order="rqsort").  The fixture holds
the shapes the issue names, every path at least twice, at least 12 "ok" generations of 20 per shape, the bands
and the signature.  With the stable order and the logged table, an "ok" generation started from the reference's
state gives the recorded state."""
import json
import math
import os
import random

import pytest

import chol_model
import jaya_model
import mayfly_model
import pikaia_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "pikaia_runs.json")) as fh:
    GOLD = json.load(fh)
STEPS = {rec["name"]: rec for rec in GOLD["steps"]}
# (name, n, np, nd, imut, ielite, objective) as the issue lists them, then the two shapes it leaves open
WANT = [("n1_np8", 1, 8, 4, 1, 0, "sphere"), ("n2_np10", 2, 10, 6, 2, 1, "rosenbrock"),
        ("n3_np20", 3, 20, 5, 5, 0, "rosenbrock"), ("n17_np32", 17, 32, 6, 3, 1, "rosenbrock"),
        ("n33_np64_creep", 33, 64, 9, 4, 0, "rosenbrock"), ("n65_np66", 65, 66, 6, 6, 1, "rosenbrock")]


def params_of(rec):
    par = dict(pm.DEFAULTS)
    par.update(rec["params"])
    par["imut"], par["ielite"] = rec["imut"], rec["ielite"]
    return par


def model_of(rec, **kw):
    n = rec["n"]
    par = params_of(rec)
    par.update(kw)
    return pm.Pikaia(chol_model.objective(rec["objective"], n), n, rec["np"], 1 << 20, rec["nd"], [rec["lower"]] * n,
                     [rec["upper"]] * n, **par)


def walk(rec):
    """the reference's run of a shape, generation by generation: (k, the fixture's record of generation k, the
    state before it, the model after it -- its table, parents, ... are the generation's)"""
    m = model_of(rec)
    w = jaya_model.Words(mayfly_model.mt19937_words(rec["seed"], sum(rec["nwords"])))
    src = pm.WordsSource(w)
    m.init_words(w)
    assert w.i == rec["nwords"][0]
    assert pm.crc(fx for _, fx in m.evals) == rec["init"]["values_crc"]
    assert m.state_crc() == rec["init"]["state_crc"] and pm.crc(m.order) == rec["init"]["order_crc"]
    at = w.i
    for k, st in enumerate(rec["states"]):
        before = m.state()
        m.iterate(src)
        at += rec["nwords"][k + 1]
        assert w.i == at, (rec["name"], k, "words")
        yield k, st, before, m


@pytest.mark.parametrize("name", sorted(STEPS))
def test_model_replays_the_reference_bit_for_bit(name):
    rec = STEPS[name]
    ran = 0
    for k, st, before, m in walk(rec):
        tag = "%s generation %d" % (name, k)
        assert pm.crc(v for r in m.ph for v in r) == st["newph_crc"], tag
        assert pm.crc(fx for _, fx in m.evals) == st["values_crc"], tag
        assert m.state_crc() == st["state_crc"] and pm.crc(m.order) == st["order_crc"], tag
        assert (m.pmut.hex(), m.elite, m.fev, bool(m.ok())) == (st["pmut"], st["elite"], st["fev"], st["ok"]), tag
        assert m.fev == rec["np"] + (k + 1) * (rec["np"] + 1) and m.ig == k + 2, tag
        assert len(m.evals) == rec["np"] + rec["ielite"], tag
        ran += 1
    assert ran == 20 and m.paths == rec["paths"]


def test_fixture_holds_the_shapes_paths_bands_and_signature():
    for name, n, np_, nd, imut, ielite, obj in WANT:
        rec = STEPS[name]
        assert (rec["n"], rec["np"], rec["nd"], rec["imut"], rec["ielite"], rec["objective"]) == (n, np_, nd, imut, ielite, obj)
        assert rec["params"] == {}
    assert len(STEPS) == 8
    extra = [rec["params"] for name, rec in STEPS.items() if name not in [w[0] for w in WANT]]
    assert {"fdif": 0.5} in extra and {"pcross": 1., "pmut": 0.05} in extra
    for rec in STEPS.values():
        assert (rec["lower"], rec["upper"], len(rec["states"])) == (-3.25, 5., 20)
        assert sum(st["ok"] for st in rec["states"]) >= 12, rec["name"]
    assert set(GOLD["paths"]) == set(pm.PATHS)
    for k in pm.PATHS:
        assert GOLD["paths"][k] == sum(rec["paths"][k] for rec in STEPS.values()) >= 2, k
    b = GOLD["bands"]
    assert (b["n"], b["np"], b["nd"], b["ngen"], b["count"]) == (10, 50, 6, 60, 256)
    assert b["settings"] == [dict(imut=2, ielite=0), dict(imut=6, ielite=1)]
    assert [(r["imut"], r["ielite"], r["objective"]) for r in b["runs"]] == [
        (2, 0, "sphere"), (2, 0, "rosenbrock"), (6, 1, "sphere"), (6, 1, "rosenbrock")]
    for r in b["runs"]:
        f = r["fbest"]
        assert len(f) == 256 and f == sorted(f) and f[0] >= 0. and r["fev"] == 50 + 60 * 51
    sig = GOLD["signature"]
    assert [a["name"] for a in sig] == ["np", "ngen", "nd", "pcross", "imut", "pmut", "pmutmn", "pmutmx", "fdif", "irep", "ielite"]
    assert [a["required"] for a in sig] == [True] * 3 + [False] * 8
    assert {a["name"]: a["default"] for a in sig[3:]} == pm.DEFAULTS
    for nd in range(1, 10):
        assert GOLD["pow10"][str(nd)] == [math.pow(10., nd).hex(), math.pow(10., -nd).hex()]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "pikaia_runs.json")) < 44 * 1024


def test_rqsort_is_a_sort_and_the_stable_order_without_ties():
    rng = random.Random(5)
    for count in (1, 2, 3, 10, 11, 12, 13, 40, 257, 1000):
        a = [rng.random() for _ in range(count)]
        assert pm.rqsort(a) == pm.stable_order(a)
        t = [float(rng.randrange(4)) for _ in range(count)]     # many ties: a sort, not necessarily the stable one
        p = pm.rqsort(t)
        assert sorted(p) == list(range(count)) and all(t[p[i]] <= t[p[i + 1]] for i in range(count - 1))
    t = [0.] * 19 + [-1.]
    assert pm.rqsort(t) != pm.stable_order(t)       # the reference's order on the ties that init leaves


@pytest.mark.parametrize("name", sorted(STEPS))
def test_stable_order_and_logged_table_give_the_recorded_state(name):
    rec = STEPS[name]
    d = model_of(rec, order="stable")
    for k, st, before, m in walk(rec):
        if not st["ok"]:
            continue
        d.start(**before)
        d.iterate(pm.TableSource(m.table))
        tag = "%s generation %d" % (name, k)
        assert len(m.table) == pm.table_layout(rec["n"], rec["np"], rec["nd"])["len"]
        assert d.table == m.table and d.parents == m.parents and d.cross == m.cross and d.mode == m.mode, tag
        assert d.state_crc() == st["state_crc"] and (d.elite, d.fev) == (st["elite"], st["fev"]), tag
        assert pm.crc(v for r in d.ph for v in r) == st["newph_crc"], tag
        # ranks differ only among rows that are the same row
        assert all(a == b or (d.ph[a] == d.ph[b] and d.fitns[a] == d.fitns[b]) for a, b in zip(d.order, m.order)), tag


def test_repair_stores_every_initial_value_and_counts_np():
    rec = STEPS["n2_np10"]
    words = mayfly_model.mt19937_words(3, 100000)
    runs = {}
    for repair in (False, True):
        m = model_of(rec, repair=repair)
        w = jaya_model.Words(words)
        m.init_words(w)
        runs[repair] = (list(m.fitns), [fx for _, fx in m.evals])
        assert m.fev == 10
        m.iterate(pm.WordsSource(w))
        assert m.fev == (20 if repair else 21) and len(m.evals) == (10 if repair else 11)
    fit, vals = runs[False]
    assert fit[:-1] == [0.] * 9 and fit[-1] == -vals[-1]
    fit, vals = runs[True]
    assert fit == [-v for v in vals]


def test_raw_maximises_over_the_unit_cube():
    seen = []

    def f(u):
        seen.append(list(u))
        return -sum((v - 0.5) ** 2 for v in u)

    m = pm.Pikaia(f, 2, 10, 5, 4, [-7.] * 2, [9.] * 2, raw=True, ielite=1)
    w = jaya_model.Words(mayfly_model.mt19937_words(1, 100000))
    m.init_words(w)
    for _ in range(5):
        m.iterate(pm.WordsSource(w))
    assert all(0. <= v < 1. for u in seen for v in u)
    x, fx = m.best()
    assert fx == max(m.fitns) and x == m.ph[m.order[-1]]
