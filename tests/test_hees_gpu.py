"""GPU: the HEES kernels against tests/hees_model.py fed the device's own normals.

The device records the normals of a generation (`record_normals` / `zlast`); the model's device
form takes them and must hold the same state to 1e-9 relative to the largest entry -- the project's
constant for device against model (tests/test_chol_gpu.py), three orders above the reorder noise
tests/test_hees_model.py measures between the two forms of the model.  The ranking must be equal
in the first generations, `it`, `fev` and the stop flag throughout.  The reference ties in through
tests/test_hees_model.py (the model's reference order reproduces the recorded Hees bit for bit, its
device form is that order up to 6e-12) and tests/test_hees_golden_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import _tabular
import chol_model
import hees_model as hm
from test_hees_model import GOLD, band, _h

pytestmark = pytest.mark.gpu

RTOL = 1e-9
ORTHO_FACTOR = 16.
LDS_BYTES = 128 * 1024
STREAM_RESTART, STREAM_HEES_NORMAL = 7, 18

# (n, np): mu = n; B = 3 with a partial batch at odd n; full batches; below and off the tile sizes;
# the large shapes; n off the tiles with few rows (still in LDS unless forced) and, at (130, 140),
# past the LDS form
SHAPES = [(4, 0), (5, 12), (8, 16), (17, 0), (33, 7), (64, 150), (128, 0), (128, 256), (130, 9), (130, 140)]
# rows past one pass of a 256-thread workgroup, mu small and explicit: one live lane in the second pass
# (257), an odd n that is no multiple of 4 or 64 (301) and the cap (512); one population, six generations
WIDE_SHAPES = [(257, 5), (301, 7), (512, 6)]


def _bits(a, b, what):
    a, b = np.asarray(a, float).ravel(), np.asarray(b, float).ravel()
    assert a.shape == b.shape, what
    assert a.tobytes() == b.tobytes(), (what, np.flatnonzero(a != b)[:8], a[a != b][:4], b[a != b][:4])


def _rel(a, b):
    a, b = np.asarray(a, float).ravel(), np.asarray(b, float).ravel()
    assert a.shape == b.shape
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _fobj(obj, n):
    f = chol_model.objective_rows(obj, n)
    return lambda x: float(f(np.asarray(x, float)[None, :])[0])


def _lds_form_applies(n, mu):
    return min(n, mu) * ((n + 3) // 4 * 4) * 8 <= LDS_BYTES


def _cases():
    out = []
    for n, np_ in SHAPES:
        mu = np_ if np_ > 0 else hm.adaptive_mu(n)
        for P in (1, 5):
            for og in ((0, 1) if _lds_form_applies(n, mu) else (1,)):
                out.append((n, np_, P, og))
    for n, np_ in WIDE_SHAPES:
        for og in ((0, 1) if _lds_form_applies(n, np_) else (1,)):
            out.append((n, np_, 1, og))
    return out


STATE = ("A", "xmean", "ps", "sigma", "gs", "xbest")


def _snapshot(g, p=0, keys=STATE + ("fit_val", "fit_idx", "b", "y", "norms", "fm", "fbest", "it", "fev", "flag")):
    return {k: g.get_state(k, p).copy() for k in keys}


@pytest.mark.parametrize("n,np_,P,og", _cases(), ids=["n%d_np%d_P%d_global%d" % c for c in _cases()])
def test_thirty_generations_against_the_device_form_of_the_model(hip, n, np_, P, og):
    obj = ["sphere", "ellipsoid", "rosenbrock"][(n + np_) % 3]
    rng = np.random.default_rng(1000 * n + np_)
    guess = rng.uniform(-3., 3., (P, n))
    lo, up = -5. * np.ones(n), 5. * np.ones(n)
    g = hip.HEES(10 ** 9, 0., np=np_, sigma0=1., seed=31 * n + np_, populations=P)
    g.initialize(obj, lo, up, guess.ravel())
    g.set_state("record_normals", [1.])
    g.set_state("hees_ortho_global", [float(og)])
    assert int(g.get_state("hees_ortho_global")[0]) == og
    pops = list(range(P))
    models = {p: hm.Hees(_fobj(obj, n), n, np_, 1.).init(guess[p]) for p in pops}
    mu = models[pops[0]].mu
    assert int(g.get_state("mu")[0]) == mu and int(g.get_state("B")[0]) == models[pops[0]].B
    worst = 0.
    gens = 6 if n > 256 else 30
    for gen in range(1, gens + 1):
        g.iterate()
        for p in pops:
            m = models[p]
            z = g.get_state("zlast", p).reshape(mu, n)
            m.iterate_device(z)
            for key, val in (("A", m.A), ("xmean", m.m), ("ps", m.ps), ("sigma", [m.sigma]), ("gs", [m.gs]),
                             ("xbest", m.xbest), ("b", m.b), ("y", m.y), ("norms", m.norms), ("fit_val", m.f)):
                err = _rel(g.get_state(key, p), val)
                worst = max(worst, err)
                assert err <= RTOL, (key, gen, p, err)
            if gen <= 3:
                assert g.get_state("fit_idx", p).astype(int).tolist() == m.order, (gen, p)
            assert int(g.get_state("it", p)[0]) == gen == m.it
            assert int(g.get_state("fev", p)[0]) == m.fev == 1 + gen * (2 * mu + 1)
            assert int(g.get_state("flag", p)[0]) == 0 and not m.converged_device()
    print("n = %d, np = %d (mu = %d), P = %d, ortho in %s: worst relative deviation from the model over %d "
          "generations %.3e" % (n, np_, mu, P, "global memory" if og else "LDS", gens, worst))


@pytest.mark.parametrize("n,np_", [(10, 5), (260, 3)])
def test_the_recorded_normals_are_the_draws_their_counters_assign(hip, oracle_lib, n, np_):
    """zlast bit for bit from the host twin of the generator (bbo_normal_quad of oracle/philox.h):
    columns 4 q .. 4 q + 3 of row r are the four normals of the Philox call (r, q, generation,
    STREAM_HEES_NORMAL << 24 | population) under the handle's seed -- slow ziggurat paths included
    (0.43 % of the draws: some thirty at the larger shape).  A stream that repeated over rows,
    generations or populations, or a quad in the wrong columns, would not survive this."""
    P, seed = 3, 0xC0FFEE1234567
    g = hip.HEES(10 ** 9, 0., np=np_, seed=seed, populations=P)
    g.initialize("sphere", -np.ones(n), np.ones(n), np.zeros((P, n)).ravel())
    g.set_state("record_normals", [1.])
    quad = oracle_lib.f("normal_quad")
    out = np.zeros(4)
    seen = set()
    for gen in range(3):
        g.iterate()
        for p in range(P):
            z = g.get_state("zlast", p).reshape(np_, n)
            want = np.empty((np_, 4 * ((n + 3) // 4)))
            for r in range(np_):
                for q in range((n + 3) // 4):
                    quad(seed, r, q, gen, (STREAM_HEES_NORMAL << 24) | p, out)
                    want[r, 4 * q:4 * q + 4] = out
            _bits(z, want[:, :n], (gen, p))
            seen.add(z.tobytes())
    assert len(seen) == 3 * P


@pytest.mark.parametrize("n,np_,og", [(33, 7, 0), (8, 16, 0), (8, 16, 1), (64, 150, 0), (128, 256, 0),
                                      (128, 256, 1), (130, 140, 1)])
def test_the_rows_of_a_batch_are_orthonormal(hip, n, np_, og):
    """|b^ b^T - I|max per batch, device and model from the same normals; the factor covers a tree
    reduction against a sequential one"""
    g = hip.HEES(10 ** 9, 0., np=np_, seed=9 + n, populations=2)
    g.initialize("sphere", -np.ones(n), np.ones(n), np.ones((2, n)).ravel())
    g.set_state("record_normals", [1.])
    g.set_state("hees_ortho_global", [float(og)])
    g.phase(0)
    mu = int(g.get_state("mu", 1)[0])
    z = g.get_state("zlast", 1).reshape(mu, n)
    m = hm.Hees(lambda x: 0., n, np_).init(np.ones(n))
    unit_model, norms_model = m.ortho_device(z)
    b = g.get_state("b", 1).reshape(mu, n)
    norms = g.get_state("norms", 1)
    assert _rel(norms, norms_model) <= 1e-14
    # the device keeps the rows rescaled to |z_r|: both sides are taken back through the same division
    unit_dev = b / norms[:, None]
    unit_mod = (unit_model * norms_model[:, None]) / norms_model[:, None]

    def figure(u):
        worst = 0.
        for r0 in range(0, mu, n):
            blk = u[r0:min(r0 + n, mu)]
            worst = max(worst, float(np.abs(blk @ blk.T - np.eye(len(blk))).max()))
        return worst

    dev, mod = figure(unit_dev), figure(unit_mod)
    print("n = %d, mu = %d, ortho in %s: |b^ b^T - I|max device %.3e, model %.3e"
          % (n, mu, "global memory" if og else "LDS", dev, mod))
    assert dev <= ORTHO_FACTOR * mod


@pytest.mark.parametrize("n,np_", [(16, 8), (17, 9), (64, 150), (130, 140)])
def test_the_matrix_pipe_forms_are_the_plain_forms(hip, n, np_):
    """hees_points_mfma against hees_points and hees_adapt_mfma against hees_adapt, each pair from
    bit-identical inputs.  Both forms of a sum of K products lie within gamma_K sum |a b| of the exact
    value whatever their order (gamma_K ~ K eps; K + 2 covers the products' own roundings), so they
    differ by at most twice that; the update of A adds one rounding of A itself on either side."""
    eps = 2. ** -53
    rng = np.random.default_rng(n)
    lo, up, guess = -5. * np.ones(n), 5. * np.ones(n), rng.uniform(-3., 3., n)
    M = np.eye(n) + 0.3 * rng.standard_normal((n, n)) / np.sqrt(n)

    def handle(fma):
        g = hip.HEES(10 ** 9, 0., np=np_, sigma0=1., seed=77)
        g.initialize("ellipsoid", lo, up, guess)
        g.set_state("A", M.ravel())
        g.set_state("hees_force_fma", [fma])
        assert int(g.get_state("hees_mfma")[0]) == 1 - int(fma)
        g.phase(0)
        return g

    plain, pipe, mixed = handle(1.), handle(0.), handle(1.)
    b = plain.get_state("b").reshape(np_, n)
    _bits(pipe.get_state("b"), b, "b")
    y0, y1 = plain.get_state("y").reshape(np_, n), pipe.get_state("y").reshape(np_, n)
    bound = 2 * (n + 2) * eps * (np.abs(b) @ np.abs(M).T)
    ry = float((np.abs(y1 - y0) / bound).max())
    assert ry <= 1., ry
    assert _rel(pipe.get_state("fit_val"), plain.get_state("fit_val")) <= 1e-12
    # the update of A: `mixed` holds the plain form's Y and switches over for the update
    _bits(mixed.get_state("y"), y0, "y")
    mixed.set_state("hees_force_fma", [0.])
    for g in (plain, mixed):
        g.phase(1)
        g.phase(2)
    q, norms, B = plain.get_state("q"), plain.get_state("norms"), int(plain.get_state("B")[0])
    _bits(mixed.get_state("q"), q, "q")
    assert float(plain.get_state("maxh")[0]) > 0.
    coef = (q - 1.) / (norms * norms * B)
    T = np.abs(coef[:, None] * y0).T @ np.abs(b)
    A0, A1 = plain.get_state("A").reshape(n, n), mixed.get_state("A").reshape(n, n)
    assert not np.array_equal(A0, M)
    boundA = 2 * (np_ + 4) * eps * T + 2 * eps * np.abs(A0)
    ra = float((np.abs(A1 - A0) / boundA).max())
    print("n = %d, mu = %d: matrix-pipe forms against plain forms, worst difference over its bound: y %.3f, A %.3f"
          % (n, np_, ry, ra))
    assert ra <= 1., ra


def test_where_the_matrix_pipe_forms_begin(hip):
    for (n, np_), want in (((16, 8), 1), ((128, 0), 1), ((15, 8), 0), ((16, 7), 0), ((33, 0), 0)):
        g = hip.HEES(10 ** 9, 0., np=np_, seed=1)
        g.initialize("sphere", -np.ones(n), np.ones(n), np.zeros(n))
        assert int(g.get_state("hees_mfma")[0]) == want, (n, np_)


def test_a_concave_objective_leaves_A_the_identity_bit_for_bit(hip):
    n = 6
    g = hip.HEES(10 ** 9, 0., seed=3)
    g.initialize(lambda x: -float(x @ x), -5. * np.ones(n), 5. * np.ones(n), 0.5 + np.arange(n) / 4.)
    m0, s0 = g.get_state("xmean").copy(), float(g.get_state("sigma")[0])
    for _ in range(10):
        g.iterate()
        assert float(g.get_state("maxh")[0]) <= 0.
        _bits(g.get_state("A"), np.eye(n), "A")
    assert not np.array_equal(g.get_state("xmean"), m0) and float(g.get_state("sigma")[0]) != s0
    assert int(g.get_state("fev")[0]) == 1 + 10 * (2 * int(g.get_state("mu")[0]) + 1)


def _device_sphere(x):
    """the sphere as eval_row_group<64> adds it for n <= 64: one term per lane, xor butterfly"""
    a = np.zeros(64)
    a[:x.size] = x * x
    for off in (32, 16, 8, 4, 2, 1):
        a = a[:off] + a[off:2 * off]
    return float(a[0])


def test_arx_between_the_phases_is_what_was_evaluated(hip):
    """after the sampling phase of a later generation `arx` is rebuilt from the current mean and
    sigma, after the update from the ones the candidates were sampled with: both times the points
    the host objective was given"""
    n = 5
    seen = []

    def f(x):
        seen.append(x.copy())
        return float(x @ x)

    g = hip.HEES(10 ** 9, 0., np=3, seed=6)
    g.initialize(f, -5. * np.ones(n), 5. * np.ones(n), 0.5 + np.arange(n) / 4.)
    g.iterate()
    g.iterate()
    del seen[:]
    g.phase(0)
    pts = np.array(seen)
    assert pts.shape == (6, n)
    _bits(g.get_state("arx"), pts, "arx after the sampling phase")
    for ph in (1, 2, 3):
        g.phase(ph)
        _bits(g.get_state("arx"), pts, "arx after phase %d" % ph)


def test_phases_one_at_a_time_are_iterate(hip):
    n, np_ = 7, 10
    lo, up, guess = -5. * np.ones(n), 5. * np.ones(n), np.linspace(-2., 2., n)
    a, b = hip.HEES(10 ** 9, 0., np=np_, seed=21), hip.HEES(10 ** 9, 0., np=np_, seed=21)
    a.initialize("rosenbrock", lo, up, guess)
    b.initialize("rosenbrock", lo, up, guess)
    for _ in range(5):
        a.iterate()
        for ph in range(4):
            b.phase(ph)
    sa, sb = _snapshot(a), _snapshot(b)
    for k in sa:
        _bits(sa[k], sb[k], k)
    assert int(sa["it"][0]) == 5


def test_population_zero_of_a_batch_is_the_single_run(hip):
    n, np_, P = 9, 12, 3
    lo, up = -5. * np.ones(n), 5. * np.ones(n)
    guess = np.random.default_rng(4).uniform(-3., 3., (P, n))
    one = hip.HEES(10 ** 9, 0., np=np_, seed=77)
    many = hip.HEES(10 ** 9, 0., np=np_, seed=77, populations=P)
    one.initialize("ellipsoid", lo, up, guess[0])
    many.initialize("ellipsoid", lo, up, guess.ravel())
    for _ in range(6):
        one.iterate()
        many.iterate()
    sa, sb = _snapshot(one), _snapshot(many, 0)
    for k in sa:
        _bits(sa[k], sb[k], k)
    assert not np.array_equal(many.get_state("b", 1), many.get_state("b", 0))      # its own sub-stream


def test_callback_path_equals_the_builtin(hip):
    n = 5
    lo, up, guess = -5. * np.ones(n), 5. * np.ones(n), 0.5 + np.arange(n) / 4.
    runs, calls = [], []

    def counted(x):
        calls.append(1)
        return _device_sphere(x)

    for f in ("sphere", counted):
        g = hip.HEES(200, 0., seed=13)
        sol = g.optimize(f, lo, up, guess)
        runs.append((sol, _snapshot(g)))
    (a, sa), (b, sb) = runs
    mu = hm.adaptive_mu(n)
    gens = -(-199 // (2 * mu + 1))
    assert a.n_evals == b.n_evals == len(calls) == 1 + gens * (2 * mu + 1) and not a.converged and not b.converged
    _bits(a.x, b.x, "x*")
    for k in sa:
        _bits(sa[k], sb[k], k)
    assert int(sa["flag"][0]) == 2


def test_run_with_polling_is_iterate(hip):
    n, np_, P = 6, 0, 3
    lo, up = -5. * np.ones(n), 5. * np.ones(n)
    guess = np.random.default_rng(8).uniform(-3., 3., (P, n))
    a = hip.HEES(10 ** 9, 0., np=np_, seed=5, populations=P)
    b = hip.HEES(10 ** 9, 0., np=np_, seed=5, populations=P, poll_every=5)
    a.initialize("rosenbrock", lo, up, guess.ravel())
    b.initialize("rosenbrock", lo, up, guess.ravel())
    for _ in range(12):
        a.iterate()
    assert b.run(12) == 12
    for p in range(P):
        sa, sb = _snapshot(a, p), _snapshot(b, p)
        for k in sa:
            _bits(sa[k], sb[k], k)


def test_a_stopped_population_is_frozen(hip):
    """population 0 starts next to the optimum with a small sigma: the spread of its values is under
    the tolerance after one generation, while population 1 still travels"""
    n, P = 6, 2
    guess = np.vstack([1e-4 * np.ones(n), 3. * np.ones(n)])
    g = hip.HEES(10 ** 9, 1e-2, sigma0=0.01, seed=17, populations=P, poll_every=2)
    g.initialize("sphere", -5. * np.ones(n), 5. * np.ones(n), guess.ravel())
    assert g.run(1) == 1
    assert int(g.get_state("flag", 0)[0]) == 1 and int(g.get_state("flag", 1)[0]) == 0
    frozen = _snapshot(g, 0)
    g.run(6)
    after = _snapshot(g, 0)
    for k in frozen:
        _bits(frozen[k], after[k], k)
    assert int(after["it"][0]) == 1 and int(g.get_state("it", 1)[0]) > 1
    assert g.solution(0).converged and g.solution(0).n_evals == 1 + (2 * hm.adaptive_mu(n) + 1)


@pytest.mark.parametrize("side", ["below", "above"])
def test_the_stop_rule_at_its_threshold(hip, side):
    """count tol^2 = 4 * 0.25 = 1 against the spread of the crafted values (d, -d, d, -d): 4 d^2,
    a part in 10^9 under and over"""
    n, tol = 3, 0.5
    d = 0.5 * (1. - 1e-9 if side == "below" else 1. + 1e-9)
    calls = []

    def crafted(x):
        k = len(calls)
        calls.append(1)
        if k == 0 or k % 5 == 0:
            return 0.           # the means
        return d if (k % 5) % 2 == 1 else -d

    g = hip.HEES(10 ** 6, tol, np=2, seed=1)
    g.initialize(crafted, -np.ones(n), np.ones(n), np.zeros(n))
    assert g.solution().converged is True       # the 2 mu values are zeros before the first generation
    assert int(g.get_state("flag")[0]) == 0
    g.iterate()
    assert len(calls) == 6
    _bits(g.get_state("fit_val"), [d, -d, d, -d], "fit_val")
    want = side == "below"
    assert g.solution().converged is want and int(g.get_state("flag")[0]) == (1 if want else 0)
    assert (float(g.get_state("m2")[0]) <= 1.) is want


def test_the_budget_stop_overshoots_like_the_reference(hip):
    n = 3
    g = hip.HEES(20, 0., np=2, seed=2)
    sol = g.optimize("sphere", -5. * np.ones(n), 5. * np.ones(n), np.ones(n))
    assert sol.n_evals == 21 and sol.converged is False and int(g.get_state("flag")[0]) == 2
    assert g.run(5) == 0        # `while (fev < mfev)`: no generation once the budget is spent


def _u01(lo, hi):
    return float(((hi << 32) | lo) >> 11) * 2. ** -53


def test_restarts_double_mu_and_account_like_the_model(hip, capfd):
    n = 4
    _restarts_account_like_the_model(hip, capfd, -5. * np.ones(n), 5. * np.ones(n), 0.5 + np.arange(n) / 4.)


def test_restart_points_come_from_each_coordinates_own_interval(hip, capfd):
    """tests/_boxes.py's box: restart point j is u (upper[j] - lower[j]) + lower[j] (hees.cpp:194-196), another
    map in every coordinate.  The chain of runs is re-run one run at a time from the points the host twin of the
    generator maps into the box, as above: a run started anywhere else would not spend the evaluations or reach
    the value the chain reports.  Every such point lies in its own coordinate's interval, and in no case do two
    coordinates of it coincide (under a uniform box a shared u would show as equal coordinates)."""
    from _boxes import percoord_box, percoord_guess
    n = 7
    lo, up = percoord_box(n)
    starts = _restarts_account_like_the_model(hip, capfd, lo, up, percoord_guess(n))
    assert len(starts) >= 1
    for x0 in starts:
        assert ((x0 >= lo) & (x0 <= up)).all() and np.unique(x0).size == n


def _restarts_account_like_the_model(hip, capfd, lo, up, guess):
    """returns the restart points (the start points of the runs after the first)"""
    from bboptpy_amd.distributed import philox4x32_10
    n, np_, mfev, tol, sigma0, seed = len(lo), 6, 800, 1e-1, 1., 123
    g = hip.HEES(mfev, tol, mres=3, print=True, np=np_, sigma0=sigma0, seed=seed)
    sol = g.optimize("sphere", lo, up, guess)
    out = capfd.readouterr().out.splitlines()
    runs = g.get_state("runs").reshape(-1, 3)
    assert 2 <= len(runs) <= 3 and sol.converged is False
    assert runs[:, 0].astype(int).tolist() == [np_ << r for r in range(len(runs))]     # mu doubles
    widths = [5, 25, 10]
    want = [_tabular.fmt_row(["iter", "f*", "fev"], widths), _tabular.rule(widths)]
    best, fev = np.inf, 0
    for r, (mu, fe, fb) in enumerate(runs, 1):
        best, fev = min(best, fb), fev + int(fe)
        want.append(_tabular.fmt_row([r, float(best), fev], widths))
    assert out == want
    assert sol.n_evals == fev and (fev >= mfev or len(runs) == 3)
    # every run again as a single run of its own (seed + r, the remaining budget, the keyed start
    # point), its normals fed to the model: the model's fev and incumbent are the run's
    x0, spent, xbest, fbest, starts = guess, 0, None, np.inf, []
    for r, (mu, fe, fb) in enumerate(runs):
        one = hip.HEES(mfev - spent, tol, np=int(mu), sigma0=sigma0, seed=seed + r)
        one.initialize("sphere", lo, up, x0)
        one.set_state("record_normals", [1.])
        m = hm.Hees(_fobj("sphere", n), n, int(mu), sigma0, tol, mfev - spent).init(x0)
        while m.fev < mfev - spent:
            one.iterate()
            m.iterate_device(one.get_state("zlast").reshape(int(mu), n))
            if m.converged_device():
                break
        assert m.fev == int(fe) == int(one.get_state("fev")[0]), r
        assert _rel([m.fbest], [fb]) <= RTOL and _rel(one.get_state("fbest"), [fb]) == 0.
        if m.fbest < fbest:
            fbest, xbest = m.fbest, np.array(m.xbest)
        spent += int(fe)
        x0 = np.array([_u01(*philox4x32_10(seed, j, 0, r + 1, STREAM_RESTART << 24)[:2]) * (up[j] - lo[j]) + lo[j]
                       for j in range(n)])
        if r + 1 < len(runs):
            starts.append(x0)
    assert _rel(sol.x, xbest) <= RTOL
    return starts


def test_restarts_refuse_batches_and_open_boxes(hip):
    from bboptpy_amd import _ffi
    n = 4
    lo, up = -5. * np.ones(n), 5. * np.ones(n)
    with pytest.raises(ValueError, match="populations=1"):
        hip.HEES(1000, 1e-3, mres=3, populations=2)
    # the library says the same to a C caller
    g = hip.HEES(1000, 1e-3, populations=2, seed=1)
    g._hees.mres = 3
    with pytest.raises(_ffi.BboError) as ei:
        g.optimize("sphere", lo, up, np.ones((2, n)).ravel())
    assert ei.value.status == _ffi.ERR_ARG and "populations = 1" in str(ei.value)
    g = hip.HEES(1000, 1e-3, mres=3, seed=1)
    with pytest.raises(_ffi.BboError) as ei:
        g.optimize("sphere", lo, np.array([5., np.inf, 5., 5.]), np.ones(n))
    assert ei.value.status == _ffi.ERR_ARG and "finite" in str(ei.value)
    # initialize / iterate ignore mres, as in the reference
    g.initialize("sphere", lo, np.array([5., np.inf, 5., 5.]), np.ones(n))
    g.iterate()
    assert int(g.get_state("it")[0]) == 1


@pytest.mark.parametrize("obj", ["sphere", "rosenbrock"])
def test_outcome_bands_match_the_reference(hip, obj):
    b, P = GOLD["bands"], 64
    n = b["n"]
    g = hip.HEES(b["mfev"], b["tol"], seed=2024, populations=P)
    g.initialize(obj, -b["box"] * np.ones(n), b["box"] * np.ones(n), b["guess"] * np.ones((P, n)).ravel())
    g.run(10 ** 6)
    got = [float(g.get_state("fbest", p)[0]) for p in range(P)]
    mu = hm.adaptive_mu(n)
    gens = -(-(b["mfev"] - 1) // (2 * mu + 1))
    assert all(int(g.get_state("fev", p)[0]) == 1 + gens * (2 * mu + 1) for p in range(P))
    band(got, _h(b[obj]), obj + " device")


def test_configure_statuses_and_refusals(hip):
    from bboptpy_amd import _ffi
    L = _ffi.lib()
    d = _ffi.HeesParams()
    L.bbo_hees_params_default(C.byref(d))
    other = hip.DSA(1000, 1e-6, 1e-6, 12, seed=1)
    oh = other._ensure_handle()
    assert L.bbo_hees_configure(oh, C.byref(d)) == _ffi.ERR_ARG
    assert L.bbo_hees_phase(oh, 0) == _ffi.ERR_ARG and L.bbo_hees_inject_normals(oh, None, 0) == _ffi.ERR_ARG
    g = hip.HEES(1000, 1e-6, seed=1)
    h = g._ensure_handle()
    assert L.bbo_hees_configure(h, C.byref(d)) == 0
    assert L.bbo_hees_configure(h, None) == _ffi.ERR_ARG
    assert L.bbo_hees_phase(h, 0) == -2                         # BBO_ERR_STATE: before bbo_init
    n = 2
    lo, up = -np.ones(n), np.ones(n)
    # the limits, each named
    with pytest.raises(_ffi.BboError) as ei:
        hip.HEES(1000, 1e-6).initialize("sphere", -np.ones(513), np.ones(513), np.zeros(513))
    assert ei.value.status == _ffi.ERR_ARG and "512" in str(ei.value)
    with pytest.raises(_ffi.BboError) as ei:
        hip.HEES(1000, 1e-6, np=4097).initialize("sphere", lo, up, np.zeros(n))
    assert ei.value.status == _ffi.ERR_ARG and "4096" in str(ei.value)
    hip.HEES(1000, 1e-6).initialize("sphere", -np.ones(512), np.ones(512), np.zeros(512))
    # an objective program: refused by the class and by the library, naming who takes one
    prog = hip.DeviceObjective('extern "C" __device__ double bbo_user_objective(const double *x, int n, '
                               'const double *data) { return x[0] * x[0]; }')
    with pytest.raises(ValueError) as ei:
        g.initialize(prog, lo, up, np.zeros(n))
    assert "CMAES" in str(ei.value) and "JADE" in str(ei.value)
    ob = _ffi.Objective()
    ob.kind, ob.user = _ffi.OBJ_PROGRAM, prog._handle
    st = L.bbo_init(h, n, lo, up, np.zeros(n), C.byref(ob))
    msg = L.bbo_last_error(h).decode()
    assert st == -1 and "HEES" in msg and "CMAES" in msg and "SHADE" in msg, (st, msg)
    g.initialize("sphere", lo, up, np.zeros(n))
    assert L.bbo_hees_configure(h, C.byref(d)) == -2            # BBO_ERR_STATE
    assert L.bbo_hees_phase(h, 4) == _ffi.ERR_ARG
    with pytest.raises(_ffi.BboError):                          # one table per population, (B n) x n
        g.inject_normals(np.zeros(3))
    # a NaN value ranks last
    nan = hip.HEES(1000, 0., np=2, seed=4)
    nan.initialize(lambda x: float("nan") if x[0] > 0.5 else float(x @ x), lo, up, np.array([0.5, 0.]))
    nan.iterate()
    f = nan.get_state("fit_val")
    assert np.isinf(f).any() and not np.isnan(f).any()
    order = nan.get_state("fit_idx").astype(int)
    assert np.isinf(f[order[-1]]) and np.isfinite(f[order[0]])
