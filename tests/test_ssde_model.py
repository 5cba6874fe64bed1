"""tests/ssde_model.py against the reference's SSDE as recorded in tests/golden/ssde_runs.json
(scripts/gen_ssde_golden.py): the model replays every recorded generation bit for bit from the mt19937
words of the record's seed, reproduces the reference's init() from the same words, reproduces 64 complete
optimize() runs exactly, and shows that runs of seeds the "bands" never saw stay inside the recorded bands
as often as tests/test_ssde_gpu.py asks of the device.  No GPU."""
import json
import os

import numpy as np
import pytest

import chol_model
import jaya_model as jm
import ssde_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAND_RUNS, BAND_MAY_MISS = 32, 2          # the cap tests/test_ssde_gpu.py states for the device


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "ssde_runs.json")) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def steps(golden):
    return sm.load_steps(golden)


@pytest.fixture(scope="module")
def percoord():
    """one short record under bounds that differ in every coordinate (tests/_boxes.py): its "box" is "percoord" """
    with open(os.path.join(ROOT, "tests", "golden", "ssde_percoord.json")) as fh:
        return sm.load_steps(json.load(fh))


def same_bits(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def test_fixture_shapes(steps):
    got = [(r["n"], r["npinit"], r.get("usede", 0), r.get("h", 100), r.get("repaircr", 1)) for r in steps]
    assert got == [(1, 4, 0, 100, 1), (2, 5, 0, 100, 1), (3, 6, 0, 100, 1), (5, 20, 1, 3, 1), (17, 20, 1, 100, 0),
                   (66, 8, 0, 100, 1)]
    assert steps[1]["objective"] == "rosenbrock"
    assert all(len(r["states"]) == 6 for r in steps)
    # np shrinks inside the n = 17 record, the memory wraps inside the n = 5 record
    assert steps[4]["states"][-1]["np"] < steps[4]["init"]["np"]
    assert "wrap" in steps[3]["events"] and {"explore", "balance", "exploit"} <= set(steps[3]["events"])
    for r in steps:
        assert r["max_attempts"] <= 8 and (r["min_gap"] >= 1e-6 or r["n"] <= 2)


def test_the_percoord_record_starts_with_opposites_and_redraws(percoord):
    """the record that pins the model's box rule under bounds that differ in every coordinate: it starts with
    usede (points and their opposites lower + upper - x: test_model_reproduces_init_from_the_words holds the
    model's start to the record bit for bit), a redraw happens, and every evaluated point lies in its
    coordinate's interval"""
    (rec,) = percoord
    n, npinit = rec["n"], rec["npinit"]
    assert n <= 12 and len(rec["states"]) <= 5 and rec["usede"] == 1 and "de_redraw" in rec["events"]
    # the witness that the box binds: coordinates the model redrew past each bound while it replays the record
    m = sm.model_of(rec, chol_model.objective(rec["objective"], n))
    m.start(rec["init"]["x"].reshape(npinit, n), rec["init"]["f"], fev=rec["init"]["fev"])
    have, saved = False, 0.
    for st in rec["states"]:
        w = jm.Words(st["words"])
        w.have, w.saved = have, saved
        m.iterate(sm.WordsSource(w, n, npinit))
        have, saved = w.have, w.saved
    assert m.repairs == rec["repairs"] and min(m.repairs.values()) >= 3, m.repairs
    lo, up = (np.asarray(v) for v in sm.box_of(rec))
    X0 = rec["init"]["x"].reshape(-1, n)
    assert (X0 >= lo).all() and (X0 <= up).all()
    for st in rec["states"]:
        assert (st["pts"] >= lo).all() and (st["pts"] <= up).all()


def test_model_replays_the_recorded_generations_bit_for_bit(steps, percoord):
    for rec in steps + percoord:
        n, npinit = rec["n"], rec["npinit"]
        m = sm.model_of(rec, chol_model.objective(rec["objective"], n))
        m.trace = True
        m.start(rec["init"]["x"].reshape(npinit, n), rec["init"]["f"], fev=rec["init"]["fev"])
        have, saved = False, 0.
        for g, st in enumerate(rec["states"]):
            w = jm.Words(st["words"])
            w.have, w.saved = have, saved
            m.points = []
            m.iterate(sm.WordsSource(w, n, npinit))
            have, saved = w.have, w.saved
            assert w.exhausted(), (rec["name"], g)
            got = m.state()
            for k in sm.FLOAT_KEYS:
                assert same_bits(got[k], st[k]), (rec["name"], g, k)
            for k in sm.INT_KEYS:
                assert got[k] == st[k], (rec["name"], g, k)
            assert got["perm"] == st["perm"], (rec["name"], g)
            assert same_bits([p for p, _ in m.points], st["pts"]) and same_bits([v for _, v in m.points], st["vals"])


def test_model_reproduces_init_from_the_words(steps, percoord):
    for rec in steps + percoord:
        m = sm.model_of(rec, chol_model.objective(rec["objective"], rec["n"]))
        w = sm.Mt19937Words(rec["seed"])
        m.init_reference(w)
        assert w.count == rec["init"]["words"]
        got = m.state()
        for k in sm.FLOAT_KEYS:
            assert same_bits(got[k], rec["init"][k]), (rec["name"], k)
        for k in sm.INT_KEYS:
            assert got[k] == rec["init"][k], (rec["name"], k)


def run_reference(cfg, objective, usede, seed):
    """one optimize() of the reference through the model: (x*, fev, converged, best value)"""
    rec = dict(cfg, usede=usede)
    m = sm.model_of(rec, chol_model.objective(objective, cfg["n"]))
    w = sm.Mt19937Words(seed)
    m.init_reference(w)
    x, fev, conv = m.optimize(lambda: sm.WordsSource(w, cfg["n"], cfg["npinit"]))
    return x, fev, conv, m.fx[0]


def test_sixty_four_complete_runs_are_reproduced_exactly(golden):
    runs = golden["runs"]
    assert len(runs["cases"]) == 64
    for case in runs["cases"]:
        x, fev, conv, fbest = run_reference(runs, case["objective"], case["usede"], case["seed"])
        key = (case["objective"], case["usede"], case["seed"])
        assert fev == case["fev"] and int(conv) == case["converged"], key
        assert same_bits(x, [float.fromhex(v) for v in case["x"]]), key
        assert fbest.hex() == case["fbest"], key
    assert {c["converged"] for c in runs["cases"]} == {0, 1}


@pytest.mark.parametrize("objective", ["sphere", "rosenbrock"])
@pytest.mark.parametrize("usede", [0, 1])
def test_other_seeds_of_the_reference_stay_inside_the_bands(golden, objective, usede):
    """the cap the device is held to (at most BAND_MAY_MISS of BAND_RUNS runs outside the recorded
    min .. max of 256) holds for the reference's own runs of seeds the bands never saw"""
    bands = golden["bands"]
    band = [float.fromhex(v) for v in bands["%s_usede%d" % (objective, usede)]]
    assert len(band) == 256 and band == sorted(band)
    first = bands["seed0"] + bands["count"]
    vals = [run_reference(bands, objective, usede, first + s)[3] for s in range(BAND_RUNS)]
    outside = sum(1 for v in vals if not band[0] <= v <= band[-1])
    assert outside <= BAND_MAY_MISS, (outside, sorted(vals)[:3], sorted(vals)[-3:], band[0], band[-1])
