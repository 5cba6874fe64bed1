"""CPU: tests/nshs_model.py against the recorded reference (tests/golden/nshs_runs.json).

The reference form, fed the uniforms the reference made of its recorded mt19937 words, reproduces
every recorded state bit for bit and uses up the words exactly.  The device form (fstd in two passes
over a fixed-shape tree sum instead of Welford's recurrence) runs beside it: it differs in fstd
alone and takes the same wide / narrow branch in every state."""
import json
import os

import numpy as np
import pytest

import chol_model
import jaya_model as jm
import nshs_model as nm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "nshs_runs.json")) as fh:
    GOLD = json.load(fh)
# one short record under bounds that differ in every coordinate (tests/_boxes.py), "box": "percoord"
with open(os.path.join(ROOT, "tests", "golden", "nshs_percoord.json")) as fh:
    PERCOORD = json.load(fh)
for _rec in GOLD["steps"] + PERCOORD["steps"]:      # the fixture keeps the changed rows of a state: put the whole memory back
    _x, _f, _n = _rec["init"]["x"], _rec["init"]["f"], _rec["n"]
    for _st in _rec["states"]:
        _x, _f = list(_x), list(_f)
        for _i, _row in _st["x_rows"].items():
            _x[int(_i) * _n:(int(_i) + 1) * _n] = _row
        for _i, _v in _st["f_rows"].items():
            _f[int(_i)] = _v
        assert len(_st["x_rows"]) == len(_st["f_rows"]) <= 1
        _st["x"], _st["f"] = _x, _f

# the largest relative deviation of the device form's fstd from the reference form's over all
# recorded states is 3.1e-16 (test_device_form_differs_in_fstd_alone prints it); the bound is 100 x
FSTD_MEASURED = 3.1e-16
FSTD_BOUND = 100 * FSTD_MEASURED
MIN_GAP = 1e-6


def _h(v):
    return np.array([float.fromhex(s) for s in v])


def _same(a, b, what):
    a, b = np.asarray(a, float).ravel(), np.asarray(b, float).ravel()
    assert a.shape == b.shape, what
    assert a.tobytes() == b.tobytes(), (what, float(np.abs(a - b).max()))


def box_of(rec):
    if rec["box"] == "percoord":
        from _boxes import percoord_box
        return percoord_box(rec["n"])
    return [-rec["box"]] * rec["n"], [rec["box"]] * rec["n"]


def model_of(rec, form):
    n, hms = rec["n"], rec["hms"]
    lo, up = box_of(rec)
    m = nm.Nshs(chol_model.objective(rec["objective"], n), n, hms, lo, up, rec["mfev"],
                rec["fstdmin"], form=form)
    m.start(_h(rec["init"]["x"]).reshape(hms, n))
    return m


def uniforms_of(rec, st):
    w = jm.Words(st["words"])
    u = nm.uniforms_of(w, rec["n"], rec["hms"], 1.0 - 1.0 / (rec["n"] + 1))
    assert w.exhausted(), rec["name"]
    return u


def _check(m, st, tag, fstd=True):
    _same(m.x, _h(st["x"]), tag + "x")
    _same(m.fs, _h(st["f"]), tag + "f")
    if fstd:
        _same([m.fstd], [float.fromhex(st["fstd"])], tag + "fstd")
    assert (m.ibest, m.iworst, m.it, m.fev) == (st["ibest"], st["iworst"], st["it"], st["fev"]), tag


@pytest.mark.parametrize("rec", GOLD["steps"] + PERCOORD["steps"],
                         ids=[r["name"] for r in GOLD["steps"] + PERCOORD["steps"]])
def test_reference_form_reproduces_the_recorded_states_bit_for_bit(rec):
    m = model_of(rec, "reference")
    _check(m, rec["init"], rec["name"] + " init ")
    for g, st in enumerate(rec["states"], 1):
        m.iterate(uniforms_of(rec, st))
        tag = "%s iteration %d " % (rec["name"], g)
        _check(m, st, tag)
        _same(m.cand, _h(st["cand"]), tag + "cand")
        _same([m.fcand], [float.fromhex(st["fcand"])], tag + "fcand")
        assert m.wide == rec["wide"], tag


def test_the_percoord_record_binds_on_both_sides():
    """the record that pins nshs_coordinate under bounds that differ in every coordinate: the reference's own
    candidates reach a lower and an upper bound, its memory starts inside each coordinate's interval, and
    tunerange is half the largest width"""
    (rec,) = PERCOORD["steps"]
    lo, up = (np.asarray(v) for v in box_of(rec))
    assert rec["n"] <= 12 and len(rec["states"]) <= 5
    X0 = _h(rec["init"]["x"]).reshape(rec["hms"], rec["n"])
    assert (X0 >= lo).all() and (X0 <= up).all()
    cands = np.array([_h(st["cand"]) for st in rec["states"]])
    assert (cands >= lo).all() and (cands <= up).all()
    assert (cands == lo).any() and (cands == up).any()
    assert model_of(rec, "reference").tunerange == ((up - lo) / 2.).max()


def test_device_form_differs_in_fstd_alone():
    """Measured over the 10 recorded runs of 12 iterations: the device form's fstd deviates from the
    reference form's by 3.1e-16 relative at most; the bound is 100 times that, 3.1e-14.  Memory,
    values, candidates, rows and counters are the reference's bit for bit, and every state takes the
    reference's branch."""
    worst = 0.
    for rec in GOLD["steps"]:
        dev = model_of(rec, "device")
        for g, st in enumerate([rec["init"]] + rec["states"]):
            if g:
                dev.iterate(uniforms_of(rec, st))
                _same(dev.cand, _h(st["cand"]), rec["name"] + " cand")
                _same([dev.fcand], [float.fromhex(st["fcand"])], rec["name"] + " fcand")
            _check(dev, st, "%s state %d " % (rec["name"], g), fstd=False)
            ref = float.fromhex(st["fstd"])
            err = abs(dev.fstd - ref) / ref
            worst = max(worst, err)
            assert err <= FSTD_BOUND, (rec["name"], g, err)
            assert dev.wide == (ref > rec["fstdmin"]) == rec["wide"], (rec["name"], g)
    print("device form against reference form: largest relative deviation of fstd %.3e" % worst)
    assert worst <= FSTD_BOUND


def test_the_two_forms_of_fstd_on_their_edge_cases():
    assert nm.std_reference([3.]) == nm.std_device([3.]) == 0.
    assert nm.std_device([1., 1., 1.]) == 0.
    for form in (nm.std_reference, nm.std_device):      # an inf among the values: NaN, the narrow branch
        v = form([1., nm.INF, 2.])
        assert v != v and not v > 0.25
    # the tree's shape: 130 values, lane 0 adds rows 0, 64, 128 in this order
    f = [float(i) * 0.1 for i in range(130)]
    part = [0.] * 64
    for j, x in enumerate(f):
        part[j % 64] += x
    a = np.array(part)
    for off in (32, 16, 8, 4, 2, 1):
        a = a[:off] + a[off:2 * off]
    assert nm.tree_sum(f) == float(a[0])


def test_uniforms_of_pads_what_the_reference_did_not_draw():
    rec = GOLD["steps"][3]
    u = np.array(uniforms_of(rec, rec["states"][0]))
    hmcr = 1.0 - 1.0 / (rec["n"] + 1)
    fired = u[:, 0] < hmcr
    assert (u[fired, 2] == 0.5).all() and (u[~fired, 1] == 0.5).all()
    rows = np.floor(u[fired, 1] * rec["hms"])
    assert ((rows + 0.5) / rec["hms"] == u[fired, 1]).all() and ((u >= 0.) & (u < 1.)).all()


def test_the_fixture_keeps_its_gaps_its_branches_and_its_signature():
    def far(a, b):
        return abs(a - b) > MIN_GAP * max(abs(a), abs(b))

    shapes = []
    for rec in GOLD["steps"]:
        shapes.append((rec["n"], rec["hms"], rec["wide"]))
        assert len(rec["states"]) == 12 and rec["replacements"] > 0
        prev = rec["init"]
        for st in [rec["init"]] + rec["states"]:
            f = np.sort(_h(st["f"]))
            fstd = float.fromhex(st["fstd"])
            assert (fstd > rec["fstdmin"]) == rec["wide"] and far(fstd, rec["fstdmin"]), rec["name"]
            assert far(f[0], f[1]) and far(f[-1], f[-2]), rec["name"]
        for st in rec["states"]:
            fc, f = float.fromhex(st["fcand"]), _h(prev["f"])
            assert far(fc, f.max()) and far(fc, f.min()), rec["name"]
            prev = st
    assert sorted(s[:2] for s in shapes if s[2]) == [(1, 3), (2, 5), (3, 7), (5, 20), (9, 20), (17, 4)]
    assert sorted(s[:2] for s in shapes if not s[2]) == [(2, 5), (3, 7), (5, 20), (9, 20)]
    assert GOLD["signature"] == [{"name": "mfev", "required": True}, {"name": "hms", "required": True},
                                 {"name": "fstdmin", "required": False, "default": 0.0001}]
    b = GOLD["bands"]
    assert (b["n"], b["hms"], b["mfev"], b["box"]) == (10, 20, 4000, 5.)
    assert len(_h(b["sphere"])) == len(_h(b["rosenbrock"])) == 256
