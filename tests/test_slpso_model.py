"""CPU: tests/slpso_model.py against the recorded reference (tests/golden/slpso_runs.json).

The model, fed the draws the reference made of its recorded mt19937 words in the reference's program
order, reproduces every recorded state bit for bit -- the integers and flags exactly -- and uses up the
words of every generation exactly.  The table of draws it writes on the way (the layout of
bbo_slpso_inject_draws) drives a second model to the same states: that table is what the GPU tests
inject.  The model's complete runs from the recorded seeds, over a live mt19937, reproduce the
recorded outcomes of optimize() exactly.  This pins the model the GPU tests lean on.

The fixture is compact (slpso_model.pack_states): the loader below restores it and checks, by count and
CRC-32, that the live mt19937 makes each generation's words; test_the_compact_form_loses_nothing packs
and unpacks again."""
import json
import os

import numpy as np
import pytest

import chol_model
import jaya_model as jm
import slpso_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "slpso_runs.json")) as fh:
    GOLD = json.load(fh)
# the fixture keeps the changed entries of a state's arrays and, of a generation's mt19937 words, their
# number and CRC-32: put whole arrays back, and the words from the record's seed
# one short record under bounds that differ in every coordinate (tests/_boxes.py), "box": "percoord"
with open(os.path.join(ROOT, "tests", "golden", "slpso_percoord.json")) as fh:
    PERCOORD = json.load(fh)
for _rec in GOLD["steps"] + PERCOORD["steps"]:
    sm.unpack_states([_rec["init"]] + _rec["states"])
    _live = sm.Mt19937Words(_rec["seed"])
    _live.take(_rec["init"]["words"])
    for _st in _rec["states"]:
        _w = _live.take(_st["words"]["count"])
        assert sm.words_crc(_w) == _st["words"]["crc32"], _rec["name"]
        _st["words"] = _w

FLOAT_KEYS = ("x", "v", "pb", "fx", "fpb", "fp", "s", "p", "Uf", "Pl", "abest", "vdavg")
INT_KEYS = ("g", "G", "m", "CF", "PF", "perm")
SCALAR_FLOAT = ("fabest", "alpha", "omega")
SCALAR_INT = ("mfes", "fev")
WANTED = {"op0", "op1", "op2", "op3", "forced", "op2_self", "op2_partner", "redraw_low", "redraw_high",
          "alg2_accept", "alg2_reject", "refresh", "cf_on", "cf_off"}


def _h(v):
    """a float array of the fixture: unpacked already, or a list of float.hex strings"""
    return np.array([float.fromhex(s) if isinstance(s, str) else float(s) for s in v])


def _same(a, b, what):
    a, b = np.asarray(a, float).ravel(), np.asarray(b, float).ravel()
    assert a.shape == b.shape, what
    assert a.tobytes() == b.tobytes(), (what, float(np.abs(a - b).max()))


def box_of(rec):
    if rec["box"] == "percoord":
        from _boxes import percoord_box
        return [list(v) for v in percoord_box(rec["n"])]
    return [-rec["box"]] * rec["n"], [rec["box"]] * rec["n"]


def model_of(rec):
    n, np_ = rec["n"], rec["np"]
    lo, up = box_of(rec)
    m = sm.Slpso(chol_model.objective(rec["objective"], n), lo, up, np_, rec["mfev"],
                 rec["stol"], Ufmax=rec["Ufmax"])
    return m.start(_h(rec["init"]["x"]).reshape(np_, n), rec["init"]["perm"])


def check_state(m, st, tag):
    got = m.state()
    for k in FLOAT_KEYS:
        _same(got[k], _h(st[k]), tag + k)
    for k in INT_KEYS:
        assert [int(v) for v in got[k]] == st[k], tag + k
    for k in SCALAR_FLOAT:
        assert float(got[k]).hex() == st[k], tag + k
    for k in SCALAR_INT:
        assert int(got[k]) == st[k], tag + k


def replay(rec, check=True):
    """the model over the record's words; returns the model and the tables of draws, one per generation"""
    n, np_ = rec["n"], rec["np"]
    m = model_of(rec)
    m.trace = True
    if check:
        check_state(m, rec["init"], rec["name"] + " init ")
    have, saved, tables = False, 0., []
    for g, st in enumerate(rec["states"], 1):
        w = jm.Words(st["words"])
        w.have, w.saved = have, saved       # (the cached second normal of the optimizer's distribution)
        src = sm.WordsSource(w, n, np_)
        m.iterate(src)
        have, saved = w.have, w.saved
        assert w.exhausted(), (rec["name"], g)
        tables.append(src.table)
        if check:
            check_state(m, st, "%s generation %d " % (rec["name"], g))
    return m, tables


@pytest.mark.parametrize("rec", GOLD["steps"] + PERCOORD["steps"],
                         ids=[r["name"] for r in GOLD["steps"] + PERCOORD["steps"]])
def test_model_reproduces_the_recorded_states_bit_for_bit(rec):
    m, tables = replay(rec)
    assert sorted(m.events) == rec["events"]
    assert min(m.gaps) >= 1e-9          # no recorded decision is close
    # the same generations from the tables alone
    t = model_of(rec)
    for g, (st, tab) in enumerate(zip(rec["states"], tables), 1):
        assert tab.size == sm.table_len(rec["n"], rec["np"])
        t.iterate(sm.TableSource(tab, rec["n"], rec["np"]))
        check_state(t, st, "%s table generation %d " % (rec["name"], g))


def test_the_records_cover_every_branch():
    seen, from_zero, to_np = set(), 0, 0
    for rec in GOLD["steps"]:
        seen |= set(rec["events"])
        assert 8 <= len(rec["states"]) <= 12 and rec["mfev"] == 40 * rec["np"]
        mfes = [st["mfes"] for st in rec["states"]]
        assert rec["init"]["mfes"] == 0 and mfes == sorted(mfes) and mfes[-1] >= 1, rec["name"]
        from_zero += mfes[0] == 0
        to_np += mfes[-1] == rec["np"]
    # mfes grows from 0 to np: the small shapes (few Algorithm 2 evaluations) show the start, the large
    # ones, whose first generation already spends a good part of the budget, the end
    assert from_zero >= 2 and to_np >= 3
    assert WANTED <= seen
    assert [(r["n"], r["np"]) for r in GOLD["steps"]] == [(2, 2), (5, 3), (12, 8), (33, 6), (65, 4)]
    assert GOLD["steps"][2]["Ufmax"] == 1.


def test_the_percoord_record_redraws_at_both_walls():
    """the record that pins the eq. 11 redraw (between the wall and the old position) and vmax under bounds that
    differ in every coordinate: at least three coordinates are redrawn at each wall, and every recorded position lies in its coordinate's interval"""
    (rec,) = PERCOORD["steps"]
    assert rec["n"] <= 12 and len(rec["states"]) <= 5
    assert {"redraw_low", "redraw_high"} <= set(rec["events"])
    # the witness that the box binds: coordinates the model redrew at each wall while it reproduced the record
    m, _ = replay(rec, check=False)
    assert m.repairs == rec["repairs"] and min(m.repairs.values()) >= 3, m.repairs
    lo, up = (np.asarray(v) for v in box_of(rec))
    for st in [rec["init"]] + rec["states"]:
        X = _h(st["x"]).reshape(rec["np"], rec["n"])
        assert (X >= lo).all() and (X <= up).all()


def test_the_live_mt19937_is_the_standard_one():
    w = sm.Mt19937Words(5489)
    assert w.next() == 3499211612       # the first output of std::mt19937 under its default seed
    for _ in range(9998):
        w.next()
    assert w.next() == 4123659995       # and the 10000th ([rand.predef])


@pytest.mark.parametrize("obj", ["sphere", "rosenbrock"])
def test_complete_runs_reproduce_the_recorded_outcomes(obj):
    R = GOLD["runs"]
    n, np_ = R["n"], R["np"]
    assert len(R[obj]) == 32 and (n, np_, R["mfev"], R["stol"], R["box"]) == (10, 20, 40000, 1e-6, 5.)
    for r in R[obj]:
        w = sm.Mt19937Words(r["seed"])
        m = sm.Slpso(chol_model.objective(obj, n), [-R["box"]] * n, [R["box"]] * n, np_, R["mfev"], R["stol"])
        m.start_words(w)
        src = sm.WordsSource(w, n, np_)
        fev, conv, fabest = m.optimize(lambda: src)
        assert (fev, int(conv), fabest.hex()) == (r["fev"], r["converged"], r["fabest"]), (obj, r["seed"])


def test_the_compact_form_loses_nothing():
    import copy
    for rec in GOLD["steps"]:
        states = [rec["init"]] + rec["states"]
        again = copy.deepcopy(states)
        sm.pack_states(again)
        assert any("rv" in st["x"] for st in again[1:]) and isinstance(again[0]["x"], str)
        sm.unpack_states(again)
        for a, b in zip(states, again):
            for k in sm.FLOAT_KEYS:
                _same(a[k], b[k], rec["name"] + " " + k)
