"""CPU chain of evidence for CholeskyCMAES: recorded reference (tests/golden/chol_runs.json,
written by scripts/gen_chol_golden.py from the compiled reference) -> NumPy model
(tests/chol_model.py).  The GPU suites then hold the device against both.

1. fed the recorded normals, the model reproduces every recorded state;
2. on those states numpy.linalg.cholesky(C') IS the factor the rank-1 chain leaves (the premise
   of the device's factor update);
3. complete model runs under NumPy normals stop after as many generations as the reference's;
4. the fixture is what the generator writes today (where the reference and g++ exist)."""
import importlib.util
import os
import shutil

import numpy as np
import pytest

from _golden import load, unhex
from chol_model import CholModel, objective, objective_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = load("chol_runs.json")["steps"]
RUNS = load("chol_runs.json")["runs"]


def _rel(a, b):
    a, b = np.asarray(a, float).ravel(), np.asarray(b, float).ravel()
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _model(rec, **kw):
    n, box = rec["n"], rec["box"]
    m = CholModel(rec["mfev"], rec["tol"], rec["stol"], rec["lambda"], rec["sigma0"],
                  bool(rec["bound"]), **kw)
    m.init(objective(rec["objective"], n), -box * np.ones(n), box * np.ones(n), unhex(rec["guess"]))
    return m


def test_fixture_covers_the_shapes():
    assert {r["n"] for r in STEPS} == {2, 5, 10, 16}
    assert any(r["lambda"] < 2 * r["n"] for r in STEPS) and any(r["lambda"] >= 4 * r["n"] for r in STEPS)
    assert {r["bound"] for r in STEPS} == {0, 1}
    # the corner run's clamps bite: some recorded candidate sits on the box
    corner = [r for r in STEPS if "corner" in r["name"]][0]
    assert (np.abs(unhex(corner["states"][0]["arx"])) == corner["box"]).any()
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "chol_runs.json")) < 300 * 1024
    assert len(RUNS["results"]) == 16 and all(r["converged"] == 1 for r in RUNS["results"])


@pytest.mark.parametrize("idx", range(len(STEPS)))
def test_model_reproduces_the_recorded_reference(idx):
    rec = STEPS[idx]
    m = _model(rec)
    for st in rec["states"]:
        m.generation(unhex(st["normals"]))
        for key, got in (("arx", m.arx), ("fit_val", m.fit_val), ("xmean", m.xmean),
                         ("sigma", [m.sigma]), ("pc", m.pc), ("ps", m.ps), ("A", m.A)):
            err = _rel(got, unhex(st[key]))
            assert err <= 1e-13, "%s gen %d %s: %.3e" % (rec["name"], st["gen"], key, err)
        np.testing.assert_array_equal(m.fit_idx, unhex(st["fit_idx"]).astype(int))
        assert (m.it, m.fev, int(m.converged())) == (st["it"], st["fev"], st["converged"])
        assert (np.triu(unhex(st["A"]).reshape(rec["n"], rec["n"]), 1) == 0.).all()


def test_cholesky_of_cprime_is_the_chains_factor():
    worst = 0.
    for rec in STEPS:
        m = _model(rec, factor="both")
        for st in rec["states"]:
            m.generation(unhex(st["normals"]))
            worst = max(worst, _rel(np.linalg.cholesky(_cprime_of(rec, st)), unhex(st["A"])))
        worst = max(worst, m.max_factor_diff)
    print("largest relative difference cholesky(C') vs rank-1 chain: %.3e" % worst)
    assert worst <= 1e-12


def _cprime_of(rec, st):
    """C' rebuilt from the RECORDED reference state after the generation: the factor it must equal
    is the recorded A.  (pc, xmean are the new ones; A_old, sigma_old, xold come from the model,
    which test 1 ties to the reference at 1e-13.)"""
    prev = _model(rec)
    for s in rec["states"]:
        if s["gen"] == st["gen"]:
            break
        prev.generation(unhex(s["normals"]))
    n, lam = rec["n"], rec["lambda"]
    arx = unhex(st["arx"]).reshape(lam, n)
    a = 1. - prev.c1 - prev.cmu
    Cp = a * (prev.A @ prev.A.T) + prev.c1 * np.outer(unhex(st["pc"]), unhex(st["pc"]))
    for i in range(prev.mu):
        y = (arx[i] - unhex(st["xmean"])) / prev.sigma
        Cp += prev.cmu * prev.w[i] * np.outer(y, y)
    return Cp


def _generations_to_stop(m, f, seed):
    rng = np.random.default_rng(seed)
    n = RUNS["n"]
    _, fev, conv = m.optimize(f, -10. * np.ones(n), 10. * np.ones(n), rng.uniform(-3, 3, n), rng)
    return m.it, conv


def test_model_runs_stop_where_the_reference_runs_stop():
    ref = [r["generations"] for r in RUNS["results"]]
    f = objective(RUNS["objective"], RUNS["n"])
    gens = []
    for seed in range(32):
        m = CholModel(RUNS["mfev"], RUNS["tol"], RUNS["stol"], RUNS["lambda"], RUNS["sigma0"],
                      factor="cholesky")
        g, conv = _generations_to_stop(m, f, 1000 + seed)
        assert conv
        gens.append(g)
    med = float(np.median(gens))
    print("reference generations %d..%d, model median %.1f" % (min(ref), max(ref), med))
    assert min(ref) <= med <= max(ref)


@pytest.mark.parametrize("n,lam,gens", [(64, 256, 30), (128, 1024, 30), (130, 256, 30), (256, 512, 30),
                                        (128, 4096, 10)])
def test_chain_and_factorisation_agree_at_the_large_shapes(n, lam, gens):
    """The GPU suite holds the device at 1e-9 against the model whose factor update is
    numpy.linalg.cholesky(C') for n >= 64.  Here, at those shapes, that model runs beside the one
    that walks the reference's rank-1 chain under the same normals: the drift of the whole state
    after `gens` generations (and the per-step difference of the two factors) must stay below
    1e-10, a tenth of that bound.  Measured: at most 3e-14 (see the printed figures)."""
    lo, up = -5. * np.ones(n), 5. * np.ones(n)
    guess = np.random.default_rng(n + lam).uniform(-4.5, 4.5, n)
    a = CholModel(10 ** 8, 1e-12, 1e-12, lam, factor="both", fast=True)
    b = CholModel(10 ** 8, 1e-12, 1e-12, lam, factor="cholesky", fast=True)
    for m in (a, b):
        m.init(objective_rows("ellipsoid", n), lo, up, guess)
    rng = np.random.default_rng(7)
    worst = 0.
    for _ in range(gens):
        z = rng.standard_normal(lam * n)
        a.generation(z)
        b.generation(z)
        for key in ("arx", "xmean", "pc", "ps", "A"):
            worst = max(worst, _rel(getattr(b, key), getattr(a, key)))
        worst = max(worst, abs(a.sigma - b.sigma) / a.sigma)
    print("n %d lambda %d, %d generations: state drift chain vs cholesky %.3e, factor difference per step %.3e"
          % (n, lam, gens, worst, a.max_factor_diff))
    assert worst <= 1e-10 and a.max_factor_diff <= 1e-10


def test_ranked_switch_changes_only_the_rank_mu_vectors():
    rec = STEPS[1]
    a, b = _model(rec), _model(rec, ranked=True)
    z = unhex(rec["states"][0]["normals"])
    a.generation(z)
    b.generation(z)
    np.testing.assert_array_equal(a.xmean, b.xmean)
    np.testing.assert_array_equal(a.pc, b.pc)
    np.testing.assert_array_equal(a.ps, b.ps)
    assert not np.array_equal(a.A, b.A)


def test_fixture_is_current():
    if not os.path.isdir("/root/reference/src") or shutil.which("g++") is None:
        pytest.skip("the reference sources or g++ are not on this machine")
    spec = importlib.util.spec_from_file_location(
        "gen_chol_golden", os.path.join(ROOT, "scripts", "gen_chol_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(os.path.join(ROOT, "tests", "golden", "chol_runs.json")) as fh:
        assert mod.dumps(mod.generate()) == fh.read()
