"""CPU: tests/hees_model.py against the recorded reference (tests/golden/hees_runs.json, written by
scripts/gen_hees_golden.py from the real Hees).

Reference order: every recorded state of the first four generations of six shapes and both
restarted runs, BIT FOR BIT (the same IEEE operations in the same order; log, exp and sqrt go
through the same C library as the harness did -- no tolerance is needed or given), and every
generation consumes exactly the words the reference consumed.

Device form against reference form, the same normals, 30 generations, eight shapes: A, m, p_s and
sigma agree to 1e-10 relative to the largest entry (the low-rank update of A is the reference's
A G up to reduction order).

Bands: the median of log10 fbest inside the reference's inter-quartile band -- first on two fixed
halves of the reference's own 256 seeds, then on 64 runs of the device form with NumPy normals,
before tests/test_hees_gpu.py uses it on the device."""
import json
import os

import numpy as np
import pytest

import _tabular
import chol_model
import hees_model as hm
import jaya_model as jm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS_BOUND = 1e-10

with open(os.path.join(ROOT, "tests", "golden", "hees_runs.json")) as _fh:
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
    """median of log10 f inside the reference's inter-quartile band"""
    dev = np.log10(np.asarray(dev_f, float) + 1e-300)
    ref = np.log10(np.asarray(ref_f, float) + 1e-300)
    q1, q3 = np.percentile(ref, [25, 75])
    print("%s: median of log10 f %.3f, reference quartiles %.3f .. %.3f" % (what, np.median(dev), q1, q3))
    assert q1 <= np.median(dev) <= q3, (what, np.median(dev), q1, q3)


def _check_state(m, st, tag):
    sc = _h(st["scalars"])
    _same(m.A, _h(st["A"]), tag + "A")
    _same(m.m, _h(st["xmean"]), tag + "xmean")
    _same(m.ps, _h(st["ps"]), tag + "ps")
    _same(m.b, _h(st["b"]), tag + "b")
    _same(m.norms, _h(st["norms"]), tag + "norms")
    _same(m.x, _h(st["x"]), tag + "x")
    _same(m.f, _h(st["fit_val"]), tag + "fit_val")
    _same(m.hess, _h(st["hess"]), tag + "hess")
    _same(m.q, _h(st["q"]), tag + "q")
    _same(m.xbest, _h(st["xbest"]), tag + "xbest")
    _same(m.w, _h(st["weights"]), tag + "weights")
    _same([m.sigma, m.gs, m.fm, m.fbest, m.cs, m.ds, m.chi, m.mueff, m.mueffm], sc, tag + "scalars")
    assert m.rank == st["rank"], tag + "rank"
    assert (m.mu, m.B, m.fev) == (st["mu"], st["B"], st["fev"]), tag
    assert m.converged() == bool(st["converged"]), tag


@pytest.mark.parametrize("rec", GOLD["steps"], ids=[r["name"] for r in GOLD["steps"]])
def test_reference_order_reproduces_the_recorded_states_bit_for_bit(rec):
    n = rec["n"]
    m = hm.Hees(chol_model.objective(rec["objective"], n), n, rec["np"], rec["sigma0"], rec["tol"])
    m.init(_h(rec["guess"]))
    _check_state(m, rec["init"], rec["name"] + " init ")
    assert m.converged()        # the 2 mu values are still zeros (hees.cpp:117-121)
    have, saved = False, 0.
    for g, st in enumerate(rec["states"], 1):
        w = jm.Words(st["words"])
        w.have, w.saved = have, saved       # the spare normal of `_Z` outlives the generation
        m.iterate_reference(w)
        assert w.exhausted(), (g, w.i, len(w.w))
        have, saved = w.have, w.saved
        _check_state(m, st, "%s gen %d " % (rec["name"], g))


@pytest.mark.parametrize("rec", GOLD["runs"], ids=[r["name"] for r in GOLD["runs"]])
def test_reference_order_reproduces_the_restarted_runs_bit_for_bit(rec):
    n = rec["n"]
    lo, up = -rec["box"] * np.ones(n), rec["box"] * np.ones(n)
    w = jm.Words(rec["words"])
    x, fev, conv, rows = hm.run_reference(chol_model.objective(rec["objective"], n), n, lo, up,
                                          _h(rec["guess"]), w, rec["mfev"], rec["tol"], rec["mres"],
                                          rec["np"], rec["sigma0"])
    assert w.exhausted()
    _same(x, _h(rec["x"]), "x")
    assert (fev, conv) == (rec["n_evals"], bool(rec["converged"])) and conv is False
    widths = [5, 25, 10]
    want = [_tabular.fmt_row(["iter", "f*", "fev"], widths), _tabular.rule(widths)]
    want += [_tabular.fmt_row(list(r), widths) for r in rows]
    assert rec["table"] == want
    assert 2 <= len(rows) <= rec["mres"]
    assert fev >= rec["mfev"] or len(rows) == rec["mres"]


def test_fixture_covers_what_it_claims():
    steps = GOLD["steps"]
    assert [(r["n"], r["np"]) for r in steps] == [(1, 0), (2, 0), (3, 7), (5, 5), (6, 0), (8, 3)]
    assert all(len(r["states"]) == 4 for r in steps)
    by = {(r["n"], r["np"]): r["init"] for r in steps}
    assert (by[(1, 0)]["mu"], by[(1, 0)]["B"]) == (2, 2)            # B = 2 at n = 1
    assert (by[(3, 7)]["mu"], by[(3, 7)]["B"]) == (7, 3)            # a partial last batch
    assert (by[(5, 5)]["mu"], by[(5, 5)]["B"]) == (5, 1)            # mu = n
    assert (by[(8, 3)]["mu"], by[(8, 3)]["B"]) == (3, 1)            # mu < n
    # no generation leaves a tie for std::sort to settle
    for r in steps:
        for st in r["states"]:
            assert len(set(st["fit_val"])) == len(st["fit_val"]), r["name"]
    # one of the runs spends its budget in the second restart, the other makes all three
    for rec in GOLD["runs"]:
        assert rec["mres"] == 3 and rec["n"] == 4 and rec["converged"] == 0
    assert sorted(len(rec["table"]) - 2 for rec in GOLD["runs"]) == [2, 3]
    b = GOLD["bands"]
    assert len(b["sphere"]) == len(b["rosenbrock"]) == b["count"] == 256
    assert (b["n"], b["mfev"], b["tol"], b["box"], b["guess"]) == (10, 1500, 0., 5., 3.)
    assert [a["name"] for a in GOLD["signature"]] == ["mfev", "tol", "mres", "print", "np", "sigma0"]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "hees_runs.json")) < 300 * 1024


FORMS = [(4, 0), (5, 12), (16, 0), (16, 40), (33, 0), (64, 150), (128, 0), (128, 256)]


def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("n,np_", FORMS, ids=["n%d_np%d" % s for s in FORMS])
def test_device_form_is_the_reference_form_up_to_reduction_order(n, np_):
    """30 generations from the same normals: the reference's full B n rows, G and A G against the
    live rows and the low-rank update"""
    obj = ["sphere", "ellipsoid", "rosenbrock"][(n + np_) % 3]
    f = chol_model.objective_rows(obj, n)
    fobj = lambda x: float(f(np.asarray(x, float)[None, :])[0])     # noqa: E731
    rng = np.random.default_rng(100 * n + np_)
    guess = rng.uniform(-3., 3., n)
    ref = hm.Hees(fobj, n, np_, 1.).init(guess)
    dev = hm.Hees(fobj, n, np_, 1.).init(guess)
    worst = 0.
    for g in range(30):
        z = rng.standard_normal((ref.np, n))
        ref.iterate_reference(normals=z, fast=True)
        dev.iterate_device(z[:dev.mu])
        assert ref.rank == dev.rank or g > 3, g
        for a, b in ((dev.A, ref.A), (dev.m, ref.m), (dev.ps, ref.ps), ([dev.sigma], [ref.sigma])):
            worst = max(worst, _rel(a, b))
    print("n = %d, np = %d (mu = %d, B = %d, %s): worst relative difference of A, m, p_s, sigma "
          "over 30 generations %.3e" % (n, np_, ref.mu, ref.B, obj, worst))
    assert worst <= FORMS_BOUND


def test_fast_reference_form_is_the_serial_one():
    """the NumPy sums of `fast` against the serial loops the goldens pin, the same normals"""
    n, np_ = 5, 12
    fobj = chol_model.objective("rosenbrock", n)
    rng = np.random.default_rng(5)
    guess = rng.uniform(-2., 2., n)
    a, b = hm.Hees(fobj, n, np_, 1.).init(guess), hm.Hees(fobj, n, np_, 1.).init(guess)
    for _ in range(10):
        z = rng.standard_normal((a.np, n))
        a.iterate_reference(normals=z)
        b.iterate_reference(normals=z, fast=True)
    assert _rel(b.A, a.A) <= 1e-12 and _rel(b.m, a.m) <= 1e-12 and _rel([b.sigma], [a.sigma]) <= 1e-12


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
def test_device_form_stays_inside_the_reference_bands(obj):
    """64 runs of Hees.iterate_device, the code the device is held against, with NumPy normals --
    like the device's 64 populations"""
    b = GOLD["bands"]
    n = b["n"]
    f = chol_model.objective_rows(obj, n)
    fobj = lambda x: float(f(np.asarray(x, float)[None, :])[0])     # noqa: E731
    got = []
    for s in range(64):
        rng = np.random.default_rng(7000 + s)
        h = hm.run_device(fobj, n, b["guess"] * np.ones(n), lambda g, mu, nn: rng.standard_normal((mu, nn)),
                          b["mfev"], b["tol"])
        got.append(h.fbest)
    band(got, _h(b[obj]), obj + " device form")
