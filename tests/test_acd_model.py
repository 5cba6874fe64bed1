"""tests/acd_model.py against the recorded runs of the reference's ACD (tests/golden/acd_runs.json): fed
the reference's own decompositions the model reproduces every point, value, sigma, m, p and C bit for bit.
Then the parts the recorded runs do not reach, by injection: the colmax form of the step rule, denom <= 0,
both repairs of the eigenvalues, the indices of the history rule."""
import json
import math
import os
import random

import numpy as np
import pytest

import acd_model as am
import chol_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "acd_runs.json")) as fh:
    GOLD = json.load(fh)
SHAPES = {r["name"]: am.unpack_run(r) for r in GOLD["steps"]}     # (the fixture keeps the compact, lossless form)


def hx(v):
    return [float.fromhex(s) for s in v]


def updates_of(rec):
    """the recorded updates that decomposed, as floats"""
    out = []
    for st in rec["steps"]:
        u = st.get("update")
        if u and u["itae"] > 1:
            out.append({k: hx(u[k]) for k in ("B", "invB", "diagd", "C", "p", "m")})
    return out


def reference_model(rec):
    n, box = rec["n"], rec["box"]
    m = am.Acd(chol_model.objective(rec["objective"], n), n, [-box] * n, [box] * n, 1 << 30, 0., 0.,
               decompose=am.recorded(updates_of(rec)))
    m.start(hx(rec["init"]["xbest"]))
    assert m.sigma == hx(rec["init"]["sigma"]) and m.period == rec["init"]["cp"]
    return m


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_the_model_replays_the_recorded_run_bit_for_bit(name):
    rec = SHAPES[name]
    n = rec["n"]
    m = reference_model(rec)
    paths = dict.fromkeys(("x1", "x2", "x1x2", "none"), 0)
    margin = math.inf
    for g, st in enumerate(rec["steps"]):
        ix = m.ix
        m.iterate()
        ev = hx(st["evals"])
        assert m.evals[0][0] + [m.evals[0][1]] + m.evals[1][0] + [m.evals[1][1]] == ev, (name, g)
        assert m.fbest == float.fromhex(st["fbest"]) and m.sigma[ix] == float.fromhex(st["sigma"])
        assert int(m.improved) == st["improved"] and m.fev == 2 * (g + 1)
        paths[m.path or "none"] += 1
        margin = min(margin, m.margin)
        assert m.updated == ("update" in st)
        if m.updated:
            u = st["update"]
            assert m.order == u["order"] and m.m == hx(u["m"]) and m.itae == u["itae"]
            if u["itae"] > 1:
                assert m.p == hx(u["p"])
                assert [v for row in m.C for v in row] == hx(u["C"])
                # the recorded decomposition against the model's own C, through the recorded residuals
                r1, r2 = am.residuals(m.B, m.invB, m.C)
                assert r1 <= 2. * float.fromhex(u["res_bbt"]) + n * 2. ** -52
                assert r2 <= 2. * float.fromhex(u["res_inv"]) + n * 2. ** -52
                d = hx(u["diagd"])
                assert all(a <= b for a, b in zip(d, d[1:]))
    assert {k: paths[k] for k in paths} == {k: rec["paths"][k] for k in paths}
    # the fixture's seed rule: no comparison closer than 1e-6 relative
    assert margin >= 1e-6 and margin == pytest.approx(float.fromhex(rec["margin"]), rel=1e-12)


def test_the_fixture_covers_the_paths_and_the_shapes():
    assert [(r["n"], r["objective"]) for r in GOLD["steps"]] == [
        (1, "sphere"), (2, "rosenbrock"), (3, "ellipsoid"), (5, "rosenbrock"), (9, "schwefel12"),
        (17, "ellipsoid"), (33, "schwefel12")]
    for k in ("x1", "x2", "x1x2", "none", "clamp"):
        assert GOLD["paths"][k] >= 2, k
    for r in GOLD["steps"]:
        assert r["sweeps"] == 4 and len(r["steps"]) == 4 * r["n"] and "note" not in r
        assert sum(1 for st in r["steps"] if st.get("update", {}).get("itae", 0) > 1) >= 1
        # the compact form leans on no exception: every dense point and every C is what the recorded
        # x_best, sigma, B, p and the C before give (and meets the checksum of the reference's own)
        assert all(not p.get("not") for st in r["steps"] for p in st["evals"])
        assert all(not st["update"].get("C_not") and not st["update"].get("V_not")
                   for st in r["steps"] if "update" in st)
    b = GOLD["bands"]
    for obj in b["objectives"]:
        assert len(b[obj]["n_evals"]) == len(b[obj]["fbest"]) == b["count"] == 256
        assert b[obj]["converged_share"] >= 0.9
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "acd_runs.json")) <= max(
        os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) for f in os.listdir(os.path.join(ROOT, "tests", "golden"))
        if f != "acd_runs.json")


def test_the_compact_form_of_a_run_is_lossless():
    for r in GOLD["steps"]:
        full = SHAPES[r["name"]]
        assert am.pack_run(full) == r and len(full["steps"][0]["evals"]) == 2 * (r["n"] + 1)
    # B and invB come back from V and diagd as the products the reference forms (:323-332)
    u = [st["update"] for st in SHAPES["n5_rosenbrock"]["steps"] if st.get("update", {}).get("itae", 0) > 1][0]
    n, d = 5, hx(u["diagd"])
    B, invB = hx(u["B"]), hx(u["invB"])
    assert all(abs(B[i * n + j] / d[j] - invB[j * n + i] * d[j]) <= 4 * 2. ** -52 * abs(B[i * n + j] / d[j])
               for i in range(n) for j in range(n))


def test_colmax_gives_the_step_rule_of_the_n_squared_loop():
    rng = random.Random(5)
    special = [0., 5e-324, 2.5e-310, math.inf, 1., 1e300, 1e-300]
    for trial in range(300):
        n = rng.choice((1, 2, 3, 5, 8))
        pick = lambda: rng.choice(special) if rng.random() < 0.3 else math.ldexp(rng.random(), rng.randint(-1070, 1000))
        sigma = [pick() for _ in range(n)]
        B = [[(pick() if rng.random() < 0.8 else 0.) * rng.choice((-1., 1.)) for _ in range(n)] for _ in range(n)]
        a, b = am.dxmax_full(sigma, B), am.dxmax_colmax(sigma, am.column_max(B))
        assert a == b and not math.isnan(a), (sigma, B)
    # inf times 0 is a NaN that std::max passes over in either form
    assert am.dxmax_full([math.inf, 1.], [[0., 2.], [0., -3.]]) == am.dxmax_colmax([math.inf, 1.], [0., 3.]) == 3.


def _fresh(n, decompose=am.eigh_decompose, f=None):
    m = am.Acd(f or chol_model.objective("sphere", n), n, [-5.] * n, [5.] * n, 1 << 30, 0., 0., decompose=decompose)
    return m.start([1.] * n)


def test_denom_not_positive_only_decays_the_path():
    n = 3
    m = _fresh(n)
    m.itae = 1
    m.p = [0.5, -0.25, 2.]
    m.X = [[0.125 * (i + 1)] * n for i in range(2 * n)]
    m.m = m.mean()                  # m - mold = 0: artmp = 0, denom = 0
    m.update_ae()
    assert m.denom == 0. and m.itae == 2
    cp = 1. / math.sqrt(3.)
    assert m.p == [0.5 * (1. - cp), -0.25 * (1. - cp), 2. * (1. - cp)]
    assert m.C[0][1] == 0. * (1. - m.c1) + m.c1 * m.p[0] * m.p[1]


def test_both_repairs_of_the_eigenvalues():
    # the spread: C = diag(1, 1, 1e15) -> shift = max / 1e14 - min
    C = [[1., 0., 0.], [0., 1., 0.], [0., 0., 1e15]]
    d = am.repair_and_root(C, [1., 1., 1e15])
    shift = 1e15 / 1e14 - 1.
    assert C[0][0] == 1. + shift and C[2][2] == 1e15 + shift
    assert d == [math.sqrt(1. + shift), math.sqrt(1. + shift), math.sqrt(1e15 + shift)]
    assert d[2] ** 2 <= 1e14 * d[0] ** 2 * (1 + 1e-12)
    # a negative eigenvalue: clamp at 0, shift by max / 1e14; the largest has grown by the shift, so the
    # spread repair behind it (:309) shifts once more, by (4 + s) / 1e14 - s
    C = [[2., 0., 0.], [0., -1., 0.], [0., 0., 4.]]
    d = am.repair_and_root(C, [-1., 2., 4.])
    s = 4. / 1e14
    s2 = (4. + s) / 1e14 - (0. + s)
    assert s2 > 0. and C[1][1] == (-1. + s) + s2
    assert d == [math.sqrt((0. + s) + s2), math.sqrt((2. + s) + s2), math.sqrt((4. + s) + s2)]
    # through an update: p = 0 and m = mold keep C, the decomposition repairs it
    m = _fresh(3)
    m.itae = 1
    m.C = [[1., 0., 0.], [0., 1., 0.], [0., 0., 1e15]]
    m.X = [[0.5] * 3 for _ in range(6)]
    m.m = m.mean()
    m.update_ae()
    c1 = m.c1
    lam = [(1. - c1) * 1., (1. - c1) * 1., (1. - c1) * 1e15]
    assert m.diagd == pytest.approx([math.sqrt(lam[2] / 1e14)] * 2 + [math.sqrt(lam[2] + lam[2] / 1e14 - lam[0])], rel=1e-12)
    r1, r2 = am.residuals(m.B, m.invB, m.C)
    assert r1 < 1e-14 and r2 < 1e-8


def test_history_rule_reads_oldest_against_newest():
    n = 1
    m = _fresh(n)
    cp = m.period
    assert cp == 30 == am.converge_period(1) and am.converge_period(128) == 10 + int(20 * 128 ** 1.5)
    m.ftol = 1e-3
    seen = {}
    for it in range(cp + 3):
        m.iterate(values=(100. - it, 200.))        # f_best falls by 1 per step: the rule must not fire
        ok, idx = m.history_rule()
        seen[m.it] = idx
        assert not ok
    assert seen[cp] is None                          # it == cp: not yet
    assert seen[cp + 1] == (0, 1)                    # it == cp + 1: newest at (it - 1) % cp = 0, oldest at 1
    assert seen[cp + 2] == (1, 2)
    # the newest entry is this step's f_best, the oldest the one written cp - 1 steps before
    i0, i1 = seen[cp + 3]
    assert m.fhist[i0] == m.fbest and m.fhist[i1] == m.fbest + (cp - 1)
    m.ftol = cp - 0.5
    assert m.history_rule()[0] and m.converged() == 1


def test_whole_runs_of_the_stand_in_stop_on_a_tolerance():
    b = GOLD["bands"]
    n = b["n"]
    rng = np.random.default_rng(3)
    m = am.Acd(chol_model.objective("sphere", n), n, [-b["box"]] * n, [b["box"]] * n, b["mfev"], b["ftol"], b["xtol"])
    flag = m.optimize(rng.uniform(-b["box"], b["box"], n))
    ref = b["sphere"]["n_evals"]
    assert flag == 1 and ref[0] // 2 <= m.fev <= 2 * ref[-1]
