"""GPU: the DSA kernels against tests/dsa_model.py fed the device's own draws.

The model takes what the device recorded of a generation (`scalars`, `dirdraws`, `mapdraws`,
`bounddraws`, `ftrial`), recomputes every decision from the raw draws with the reference's
formulas and must then hold the same state BIT FOR BIT, signs of zeros included: dirrow, map,
trial, X, f, nsucc, fev, it, stop.  Three quantities pass through a transcendental function whose
device and host implementations differ (ocml / log_unit against libm):
  w, p  one exp at <= 1 ulp and fewer than ten operations: compared at relative WP_RTOL = 1e-14
        (a decade of margin); after each generation the model adopts the device's w and p;
  R     the recorded R against 1 / (-2 ln u) by libm at relative R_RTOL = 1e-12 (a correct
        evaluation errs by a few ulp, a wrong formula by O(1)); the model then uses the device's R.
Measured on an MI355X over the cases below: worst w 0, worst p 0 (ocml's exp returned libm's bits
every time), worst R 1.92e-16; each test prints the worst values so far.
The reference ties in through tests/test_dsa_model.py (the model's reference order reproduces the
recorded DSSearch bit for bit) and through the outcome bands of tests/golden/dsa_runs.json."""
import ctypes as C
import math

import numpy as np
import pytest

import dsa_model as dm
from slpso_model import device_objective
from test_dsa_model import GOLD, band, _h

pytestmark = pytest.mark.gpu

WP_RTOL = 1e-14
R_RTOL = 1e-12
STREAM_DSA_CTRL, STREAM_DSA_PERM, STREAM_DSA_DIR, STREAM_DSA_MAP, STREAM_DSA_R = 13, 14, 15, 16, 17
WORST = {"w": 0., "p": 0., "R": 0.}


def _bits(a, b, what):
    a, b = np.asarray(a, float).ravel(), np.asarray(b, float).ravel()
    assert a.shape == b.shape, what
    assert a.tobytes() == b.tobytes(), (what, np.flatnonzero(a != b)[:8], a[a != b][:4], b[a != b][:4])


def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b) / np.abs(b)))


def _perm(i, np_, seed, gen, p):
    """cso_perm of bbo_rng.hpp: the keyed bijection that stands in for std::shuffle"""
    from bboptpy_amd.distributed import philox4x32_10
    bits = 1
    while (1 << bits) < np_:
        bits += 1
    kb = (bits + 1) // 2
    mask = (1 << kb) - 1
    sw = (STREAM_DSA_PERM << 24) | p
    x = i
    while True:
        L, R = x >> kb, x & mask
        for r in range(4):
            t = L ^ (philox4x32_10(seed, R, 8 + r, gen, sw)[0] & mask)
            L, R = R, t
        x = (L << kb) | R
        if x < np_:
            return x


def _u01(lo, hi):
    return float(((hi << 32) | lo) >> 11) * 2. ** -53


def _check_keying(g, m, p, seed, gen):
    """The recorded draws are the Philox words the design assigns them (bbo_dsa_kernels.hpp): the
    counters (what, 0, generation) of the control stream, (row, 0 | 1 + q, generation) of the
    direction and map streams, (row, coordinate, generation) of the coordinate stream, each with
    (stream << 24 | population) -- recomputed here with the host twin of the generator.  A stream
    that repeated over generations, members, coordinates or populations, or two draws taken from
    the same words, would not survive this."""
    from bboptpy_amd.distributed import philox4x32_10 as ph
    np_, n = m.np, m.n
    sw = lambda stream: (stream << 24) | p
    sc = g.get_state("scalars", p)
    w0, w1, w2 = (ph(seed, what, 0, gen, sw(STREAM_DSA_CTRL)) for what in range(3))
    open0 = float((((w2[3] << 32) | w2[2]) >> 11) + 1) * 2. ** -53
    _bits(sc[:6], [_u01(w0[0], w0[1]), _u01(w0[2], w0[3]), _u01(w1[0], w1[1]), _u01(w1[2], w1[3]),
                   _u01(w2[0], w2[1]), open0], "the scalars' uniforms")
    dd = g.get_state("dirdraws", p).reshape(np_, 2)
    md = g.get_state("mapdraws", p).reshape(np_, -1)
    bd = g.get_state("bounddraws", p).reshape(np_, n, 2)
    rows = range(np_) if np_ * n <= 1000 else sorted({0, 1, np_ // 2, np_ - 1})
    if m.imethd == 2:
        w = ph(seed, 0, 1, gen, sw(STREAM_DSA_DIR))
        assert dd[0, 0] == _u01(w[0], w[1])
    for i in rows:
        if m.imethd == 1:
            w = ph(seed, i, 0, gen, sw(STREAM_DSA_DIR))
            assert (dd[i, 0], dd[i, 1]) == (_u01(w[0], w[1]), float(w[2])), ("dirdraws", i)
        w = ph(seed, i, 0, gen, sw(STREAM_DSA_MAP))
        assert (md[i, n], md[i, n + 1]) == (_u01(w[0], w[1]), float(w[2])), ("member draws", i)
        if m.strategy == dm.RANDOM2:
            for k in range(m.mapmax):
                assert md[i, n + 2 + k] == float(ph(seed, i, 1 + k // 4, gen, sw(STREAM_DSA_MAP))[k % 4]), (i, k)
        for j in range(n):
            w = ph(seed, i, j, gen, sw(STREAM_DSA_R))
            assert (md[i, j], bd[i, j, 0], bd[i, j, 1]) == (_u01(w[0], w[1]), float(w[2] & 1), _u01(w[2], w[3])), \
                ("coordinate draws", i, j)


def _plain_radius(x):
    s = 0.
    for v in x:
        s += float(v) * float(v)
    return math.sqrt(s)


def _model_of(g, p, lo, up, np_, adapt, nbatch=100, tol=0., stol=0.):
    m = dm.Dsa(None, lo, up, np_, adapt=adapt, nbatch=nbatch, tol=tol, stol=stol)
    m.start(g.get_state("X", p), g.get_state("f", p), int(g.get_state("fev", p)[0]))
    m.w, m.p = list(g.get_state("w", p)), list(g.get_state("p", p))
    m.it = int(g.get_state("it", p)[0])
    return m


def _step_model(g, m, p, seed=None, force_method=-1, force_map=-1, mfev=10 ** 9):
    """one device generation has just run: replay it in the model and compare"""
    np_, n = m.np, m.n
    sc = g.get_state("scalars", p)
    assert sc.size == 12
    raw, R = sc[:6], sc[11]
    assert all(0. <= u < 1. for u in raw[:5]) and 0. < raw[5] <= 1.
    want_R = 0. if raw[5] == 1. else 1. / (-2. * math.log(raw[5]))
    err = abs(R - want_R) / want_R if want_R else abs(R)
    WORST["R"] = max(WORST["R"], err)
    assert err <= R_RTOL, ("R", R, want_R)
    gen = int(g.get_state("gen", p)[0]) - 1
    m.iterate_keyed(raw, R, g.get_state("dirdraws", p), g.get_state("mapdraws", p),
                    g.get_state("bounddraws", p), ftrial=g.get_state("ftrial", p),
                    force_method=force_method, force_map=force_map)
    _bits(sc[6:8], [m.p1, m.p2], "p1, p2")
    assert (int(sc[8]), int(sc[9]), int(sc[10])) == (m.imethd, m.strategy, m.mapmax), (sc, m.imethd, m.strategy)
    dirrow = g.get_state("dirrow", p).astype(int)
    assert dirrow.tolist() == [int(r) for r in m.dirrow], "dirrow"
    if m.imethd == 0 and seed is not None:
        assert dirrow.tolist() == [_perm(i, np_, seed, gen, p) for i in range(np_)], "the keyed bijection"
    if seed is not None:
        _check_keying(g, m, p, seed, gen)
    assert g.get_state("map", p).astype(int).tolist() == m.map.ravel().tolist(), "map"
    _bits(g.get_state("trial", p), m.trial, "trial")
    _bits(g.get_state("X", p), m.X, "X")
    _bits(g.get_state("f", p), m.f, "f")
    fb, xb = m.best()
    _bits(g.get_state("fbest", p), [fb], "fbest")
    _bits(g.get_state("bestx", p), xb, "bestx")
    assert int(g.get_state("nsucc", p)[0]) == m.nsucc
    assert int(g.get_state("fev", p)[0]) == m.fev and int(g.get_state("it", p)[0]) == m.it
    stop = 1 if m.converged(_plain_radius) else 2 if m.fev >= mfev else 0
    assert int(g.get_state("stop", p)[0]) == stop
    w, pr = g.get_state("w", p), g.get_state("p", p)
    WORST["w"], WORST["p"] = max(WORST["w"], _rel(w, m.w)), max(WORST["p"], _rel(pr, m.p))
    assert _rel(w, m.w) <= WP_RTOL and _rel(pr, m.p) <= WP_RTOL, (w, m.w, pr, m.p)
    m.w, m.p = list(w), list(pr)


# (method, map, n, np, P, adapt, objective): every method x every map strategy, n in {1, 3, 64, 65,
# 130}, np in {2, 7, 70}, P in {1, 3}; the last three draw both decisions, two of them without `adapt`
CASES = [
    (0, 0, 1, 2, 1, 1, "sphere"),
    (0, 1, 3, 7, 3, 1, "rosenbrock"),
    (0, 2, 130, 70, 1, 1, "rastrigin"),
    (1, 0, 64, 70, 1, 1, "rosenbrock"),
    (1, 1, 65, 7, 1, 1, "ellipsoid"),
    (1, 2, 130, 70, 3, 1, "sphere"),
    (2, 0, 3, 7, 1, 1, "sphere"),
    (2, 1, 65, 70, 1, 1, "rosenbrock"),
    (2, 2, 3, 7, 3, 1, "sphere"),
    (3, 0, 130, 7, 1, 1, "sphere"),
    (3, 1, 1, 2, 1, 1, "sphere"),
    (3, 2, 64, 70, 1, 1, "sphere"),
    (-1, -1, 65, 70, 3, 0, "rosenbrock"),
    (-1, -1, 3, 7, 1, 1, "sphere"),
    (-1, -1, 130, 2, 1, 0, "sphere"),
    # rows past one pass of a 256-thread workgroup: one live lane in the second pass (257), in the
    # third (513), and the cap (1024: four full passes)
    (0, 0, 257, 7, 1, 1, "rosenbrock"),
    (1, 1, 513, 7, 1, 1, "ellipsoid"),
    (2, 2, 1024, 7, 1, 1, "rosenbrock"),
    (3, 1, 1024, 8, 1, 1, "ellipsoid"),
    (-1, -1, 513, 7, 3, 0, "rosenbrock"),
]


@pytest.mark.parametrize("method,mapst,n,np_,P,adapt,obj", CASES,
                         ids=["m%d-s%d-n%d-np%d-P%d-a%d" % c[:6] for c in CASES])
def test_three_generations_against_the_keyed_model(hip, method, mapst, n, np_, P, adapt, obj):
    lo, up = -3. * np.ones(n), 4. * np.ones(n)
    seed = 41 + n
    g = hip.DSA(10 ** 9, 0., 0., np_, bool(adapt), 2, seed=seed, populations=P)
    g.initialize(getattr(hip.objectives, obj), lo, up, np.zeros((P, n)))
    g.set_state("record_draws", [1.])
    g.set_state("force_method", [float(method)])
    g.set_state("force_map", [float(mapst)])
    assert float(g.get_state("gamma")[0]) == dm.gamma_of(2)
    models = [_model_of(g, p, lo, up, np_, adapt, nbatch=2) for p in range(P)]
    for p, m in enumerate(models):
        X = g.get_state("X", p).reshape(np_, n)
        assert ((X >= lo) & (X <= up)).all() and int(g.get_state("fev", p)[0]) == np_
        fb, xb = m.best()
        _bits(g.get_state("fbest", p), [fb], "init fbest")
        _bits(g.get_state("bestx", p), xb, "init bestx")
    fobj = getattr(hip.objectives, obj)
    for _ in range(3):
        g.iterate()
        for p, m in enumerate(models):
            _step_model(g, m, p, seed, method, mapst)
            T, ft = g.get_state("trial", p).reshape(np_, n), g.get_state("ftrial", p)
            want = np.array([fobj(t) for t in T])
            assert np.all(np.abs(ft - want) <= 1e-12 * np.abs(want) + 1e-300), (ft, want)
    print("worst deviations so far: w %.3e p %.3e R %.3e" % (WORST["w"], WORST["p"], WORST["R"]))
    if P > 1:       # the populations are independent streams
        assert not np.array_equal(g.get_state("X", 0), g.get_state("X", 1))
        assert not np.array_equal(g.get_state("scalars", 0)[:6], g.get_state("scalars", 1)[:6])


def _percoord_handle(hip, n, np_, P, seed, lo, up, pools):
    """a handle under tests/_boxes.py's box whose populations start from the given host-made pools"""
    f = device_objective("sphere", n)
    g = hip.DSA(10 ** 9, 0., 0., np_, True, 2, seed=seed, populations=P)
    g.initialize(hip.objectives.sphere, lo, up, np.zeros((P, n)))
    for p in range(P):
        X = g.get_state("X", p).reshape(np_, n)
        assert ((X >= lo) & (X <= up)).all()
        # the initial draw: every coordinate spread over its own interval, not a neighbour's
        assert ((X.max(0) - X.min(0)) > 0.25 * (up - lo)).sum() >= n // 2
        g.set_state("X", pools[p], p)
        g.set_state("f", [f(x) for x in pools[p]], p)
    g.set_state("record_draws", [1.])
    return g


@pytest.mark.parametrize("n,np_,P,gens", [(37, 7, 2, 15), (513, 7, 1, 10)])
def test_the_repair_coin_under_bounds_that_differ_in_every_coordinate(hip, n, np_, P, gens):
    """tests/_boxes.py's box: the initial draw u (up[j] - lo[j]) + lo[j] and the repair -- a redraw in
    [lo[j], up[j]] or the bound itself, by a coin -- read another pair of bounds in every coordinate.  DSA does
    not clamp, so the witness is the model's count of repaired coordinates (`paths`), three at each bound at
    least in every population.  It is established before anything is compared: a first handle only hands over
    the uniforms and words its generator drew (what _check_keying holds to the generator's host twin), and the
    model runs alone on them, from a pool made on the host, with its own objective and its own R, and counts.
    Then a second handle of the same seed walks beside a second model, as in
    test_three_generations_against_the_keyed_model, longer, with both decisions drawn: n = 37 is off every tile,
    513 puts one live lane into the third pass."""
    from _boxes import percoord_box
    lo, up = percoord_box(n)
    seed = 41 + n
    rng = np.random.default_rng(seed)
    pools = [lo + (up - lo) * rng.random((np_, n)) for _ in range(P)]
    fobj = device_objective("sphere", n)
    # ---- the witness: the model alone on the generator's draws
    a = _percoord_handle(hip, n, np_, P, seed, lo, up, pools)
    alone = []
    for p in range(P):
        w = dm.Dsa(fobj, lo, up, np_, adapt=True, nbatch=2)
        w.start(pools[p], [fobj(x) for x in pools[p]], np_)
        alone.append(w)
    for _ in range(gens):
        a.iterate()
        for p, w in enumerate(alone):
            raw = a.get_state("scalars", p)[:6]
            R = 0. if raw[5] == 1. else 1. / (-2. * math.log(raw[5]))
            w.iterate_keyed(raw, R, a.get_state("dirdraws", p), a.get_state("mapdraws", p),
                            a.get_state("bounddraws", p))
    for p, w in enumerate(alone):
        assert w.paths["repair_lo"] >= 3 and w.paths["repair_up"] >= 3, (p, w.paths)
    # ---- the walk
    g = _percoord_handle(hip, n, np_, P, seed, lo, up, pools)
    models = [_model_of(g, p, lo, up, np_, 1, nbatch=2) for p in range(P)]
    for _ in range(gens):
        g.iterate()
        for p, m in enumerate(models):
            _step_model(g, m, p, seed if n < 256 else None)
            T = g.get_state("trial", p).reshape(np_, n)
            assert ((T >= lo) & (T <= up)).all()
    for p, m in enumerate(models):
        assert m.paths["repair_lo"] >= 3 and m.paths["repair_up"] >= 3, (p, m.paths)


def test_a_pool_at_a_corner_is_repaired_into_the_box(hip):
    """the incumbent sits far outside the box (a crafted X), every other member at the upper
    corner, E2-DSA: every mapped coordinate of every trial leaves the box by a large step and
    comes back as a bound or as a fresh point inside"""
    n, np_ = 5, 7
    lo, up = -1. * np.ones(n), 2. * np.ones(n)
    g = hip.DSA(10 ** 9, 0., 0., np_, seed=3)
    g.initialize(hip.objectives.sphere, lo, up, np.zeros(n))
    X = np.tile(up, (np_, 1))
    X[2] = 1e6
    f = np.full(np_, 1e300)
    f[2] = 1e299
    g.set_state("X", X)
    g.set_state("f", f)
    g.set_state("record_draws", [1.])
    g.set_state("force_method", [3.])
    g.set_state("force_map", [0.])
    m = _model_of(g, 0, lo, up, np_, True)
    bound = fresh = 0
    for _ in range(3):
        g.iterate()
        _step_model(g, m, 0, force_method=3, force_map=0)
        T = g.get_state("trial").reshape(np_, n)
        assert (T >= lo).all() and (T <= up).all()
        bound += int((T == up).sum() + (T == lo).sum())
        fresh += int(((T > lo) & (T < up)).sum())
    assert bound > 0 and fresh > 0
    Xn = g.get_state("X").reshape(np_, n)
    assert (Xn >= lo).all() and (Xn <= up).all()        # every repaired trial beat 1e299


def test_a_nan_objective_is_never_accepted(hip):
    n, np_ = 4, 7
    lo, up = -2. * np.ones(n), 2. * np.ones(n)
    calls = []

    def f(x):
        calls.append(1)
        return float("nan") if len(calls) > np_ and len(calls) % 2 else float(np.sum(x * x))

    g = hip.DSA(10 ** 9, 0., 0., np_, seed=5)
    g.initialize(f, lo, up, np.zeros(n))
    assert len(calls) == np_
    g.set_state("record_draws", [1.])
    m = _model_of(g, 0, lo, up, np_, True)
    nan = 0
    for _ in range(3):
        before = g.get_state("f").copy()
        g.iterate()
        ft = g.get_state("ftrial")
        _step_model(g, m, 0)
        nan += int(np.isinf(ft).sum())
        after = g.get_state("f")
        assert (after[np.isinf(ft)] == before[np.isinf(ft)]).all()
    assert nan >= 9 and len(calls) == 4 * np_ and np.isfinite(g.get_state("f")).all()


def test_both_halves_of_the_stop_rule_and_the_budget(hip):
    n, np_ = 4, 7
    lo, up = -5. * np.ones(n), 5. * np.ones(n)
    row = np.array([1., 1.5, 2., 2.5])

    def crafted(X, f):
        g = hip.DSA(10 ** 6, 1e-3, 1e-3, np_, seed=6)
        g.initialize(hip.objectives.rosenbrock, lo, up, np.zeros(n))
        g.set_state("X", X)
        g.set_state("f", f)     # so low that no trial is accepted: the pool stays as crafted
        g.iterate()
        return g

    spread = np.random.default_rng(1).uniform(-4, 4, (np_, n))
    # equal fitness, equal radii: converged
    g = crafted(np.tile(row, (np_, 1)), np.full(np_, -1e300))
    assert int(g.get_state("stop")[0]) == 1 and int(g.get_state("conv")[0]) == 1 and g.solution().converged
    assert float(g.get_state("m2")[0]) < 1e-25 and g.run(5) == 0
    # equal fitness, spread radii: the second half says no
    g = crafted(spread, np.full(np_, -1e300))
    assert int(g.get_state("stop")[0]) == 0 and float(g.get_state("m2")[0]) > 6e-6
    # equal radii, spread fitness: the first half says no
    g = crafted(np.tile(row, (np_, 1)), -1e300 * (1. + np.arange(np_)))
    assert int(g.get_state("stop")[0]) == 0 and float(g.get_state("m2")[0]) < 1e-25
    assert not g.solution().converged
    # the budget: whole generations, so fev overshoots mfev like the reference's loop
    g = hip.DSA(100, 0., 0., np_, seed=6)
    g.initialize(hip.objectives.rosenbrock, lo, up, np.zeros(n))
    g.run(10 ** 6)
    assert int(g.get_state("stop")[0]) == 2 and int(g.get_state("fev")[0]) == 105
    assert int(g.get_state("it")[0]) == 14 and g.run(5) == 0 and not g.solution().converged


def test_the_weights_are_reset_every_nbatch_generations(hip):
    n, np_, nbatch = 3, 7, 5
    lo, up = -5. * np.ones(n), 5. * np.ones(n)
    for it, reset in ((5, True), (6, False), (0, True)):
        g = hip.DSA(10 ** 9, 0., 0., np_, True, nbatch, seed=8)
        g.initialize(hip.objectives.sphere, lo, up, np.zeros(n))
        g.set_state("record_draws", [1.])
        g.set_state("w", [2., 3., 4., 5.])
        g.set_state("p", [0.1, 0.2, 0.3, 0.4])
        g.set_state("it", [float(it)])
        m = _model_of(g, 0, lo, up, np_, True, nbatch=nbatch)
        assert m.w == [2., 3., 4., 5.] and m.it == it
        g.iterate()
        _step_model(g, m, 0)
        w, im = g.get_state("w"), int(g.get_state("scalars")[8])
        rest = np.delete(w, im)
        assert (rest == 1.).all() if reset else (rest == np.delete([2., 3., 4., 5.], im)).all()
        assert int(g.get_state("it")[0]) == it + 1


def _device_sphere3(x):
    """the built-in sphere at n = 3 in the device's order: one term per lane, then the butterfly"""
    return float((x[0] * x[0] + x[2] * x[2]) + x[1] * x[1])


def test_callback_path_equals_the_builtin(hip):
    n, np_ = 3, 70
    lo, up = -5. * np.ones(n), 5. * np.ones(n)
    runs, calls = [], []

    def counted(x):
        calls.append(1)
        return _device_sphere3(x)

    for f in (hip.objectives.sphere, counted):
        g = hip.DSA(500, 0., 0., np_, seed=77)
        sol = g.optimize(f, lo, up, np.zeros(n))
        runs.append((sol, {k: g.get_state(k).copy() for k in ("X", "f", "w", "p", "it", "fev", "stop", "bestx")}))
    (a, sa), (b, sb) = runs
    assert a.n_evals == b.n_evals == len(calls) == 560 and a.converged == b.converged is False
    _bits(a.x, b.x, "x*")
    for k, v in sa.items():
        _bits(v, sb[k], k)
    assert int(sa["stop"][0]) == 2
    g = hip.DSA(500, 0., 0., np_, seed=78)
    g.optimize(hip.objectives.sphere, lo, up, np.zeros(n))
    assert not np.array_equal(g.get_state("X"), sa["X"])        # another seed, another run


@pytest.mark.parametrize("obj", ["sphere", "rosenbrock"])
def test_outcome_bands_match_the_reference(hip, obj):
    b, P = GOLD["bands"], 64
    n = b["n"]
    g = hip.DSA(b["mfev"], b["tol"], b["stol"], b["np"], seed=2024, populations=P)
    g.initialize(getattr(hip.objectives, obj), -b["box"] * np.ones(n), b["box"] * np.ones(n), np.zeros((P, n)))
    g.run(10 ** 6)
    got = [float(g.get_state("fbest", p)[0]) for p in range(P)]
    assert all(int(g.get_state("fev", p)[0]) == 4000 for p in range(P))
    print("device %s: quartiles of log10 f" % obj, np.percentile(np.log10(got), [25, 50, 75]))
    band(got, _h(b[obj]), obj + " device")


def test_configure_statuses_and_refusals(hip):
    from bboptpy_amd import _ffi
    L = _ffi.lib()
    d = _ffi.DsaParams()
    L.bbo_dsa_params_default(C.byref(d))
    other = hip.JAYA(1000, 1e-6, 12, 3, seed=1)
    assert L.bbo_dsa_configure(other._ensure_handle(), C.byref(d)) == _ffi.ERR_ARG
    g = hip.DSA(1000, 1e-6, 1e-6, 12, seed=1)
    h = g._ensure_handle()
    assert L.bbo_dsa_configure(h, C.byref(d)) == 0
    assert L.bbo_dsa_configure(h, None) == _ffi.ERR_ARG
    bad = _ffi.DsaParams()
    bad.adapt, bad.nbatch = 1, 0
    assert L.bbo_dsa_configure(h, C.byref(bad)) == _ffi.ERR_ARG
    with pytest.raises(_ffi.BboError):
        hip.DSA(1000, 1e-6, 1e-6, 12, nbatch=0)._ensure_handle()
    with pytest.raises(_ffi.BboError) as e:
        hip.DSA(1000, 1e-6, 1e-6, 0)._ensure_handle()
    assert e.value.status == _ffi.ERR_ARG
    n = 2
    lo, up = -np.ones(n), np.ones(n)
    with pytest.raises(_ffi.BboError):                          # a finite box
        hip.DSA(1000, 1e-6, 1e-6, 12).initialize(hip.objectives.sphere, lo, np.array([1., np.inf]), np.zeros(n))
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
    assert st == -1 and "DSA" in msg and "CMAES" in msg and "SHADE" in msg, (st, msg)
    g.initialize(hip.objectives.sphere, lo, up, np.zeros(n))
    assert L.bbo_dsa_configure(h, C.byref(d)) == -2             # BBO_ERR_STATE
    # np = 1 is legal: best and worst are the one member, so converged() holds after a generation
    one = hip.DSA(20, 0., 0., 1, seed=2)
    sol = one.optimize(hip.objectives.sphere, lo, up, np.zeros(n))
    assert sol.n_evals == 2 and sol.converged and np.isfinite(sol.x).all()


def test_a_row_matrix_round_trips_at_odd_n_in_the_second_population(hip):
    """n = 3 (ld = 4), six rows, population 1: set_state -> get_state bit-equal, no padding column"""
    n, np_, P = 3, 6, 2
    g = hip.DSA(10 ** 6, 0., 0., np_, seed=4, populations=P)
    g.initialize(hip.objectives.sphere, -2. * np.ones(n), 2. * np.ones(n), np.zeros((P, n)))
    X = np.random.default_rng(9).uniform(-1., 1., (np_, n))
    g.set_state("X", X, population=1)
    got = g.get_state("X", 1)
    assert got.size == np_ * n and got.tobytes() == X.tobytes()
