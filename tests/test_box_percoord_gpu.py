"""GPU parity under bounds that differ in every coordinate and bind (tests/_boxes.py): the
oracle-backed engines -- CMAES / ActiveCMAES / SepCMAES with bound=True, SHADE, JADE, SaNSDE,
APSO, CSO, CCPSO and the restart drivers' starting points -- beside the CPU oracle, which
tests/test_oracle_vs_reference.py pins to the compiled reference under this same box.

Every other GPU file builds its box as c * ones(n), mostly symmetric around the optimum: a kernel
that reads lower[0], lower[t] for lower[col] or upper[j] for upper[j + 1], or that exchanges the
two bounds, passes all of them.  Here no two coordinates share a bound, lo != -up, and sphere's
optimum lies below the box in a third of the coordinates, above it in a third and inside in a third.

Each case first asserts, from a run of the ORACLE ALONE, that the box bound that run:
  engines that clamp    >= 3 coordinates on their lower bound, >= 3 on their upper bound and >= 3
                        strictly interior in every row of every walked generation;
  SHADE / JADE / SaNSDE (midpoint repair, never on a bound): >= 3 coordinates repaired at each
                        bound, counted by the oracle (`repairs_lo`, `repairs_up`);
  APSO with correct=False (positions are free; the box enters through vmax[j] alone):
                        >= 3 coordinates with v = -vmax[j] and >= 3 with v = +vmax[j];
  CCPSO                 the three-way split over all walked generations on `yhat`, the context vector
                        every evaluation goes through and every clamped draw ends in (the particles `x`
                        are Cauchy / Gaussian draws around it: within two generations every coordinate
                        of SOME particle has met a bound, so no coordinate of `x` stays interior in
                        every row); on `x`, three coordinates on each bound.
Then the device is walked beside the oracle with the keys and tolerances of the engine's own
parity file (test_cma_gpu.py, test_sep_gpu.py, tests/batch_oracle.py), none of them new or wider.
Seeds, sigma0 and generation counts were chosen on the CPU so that the oracle meets the witness.
"""
import numpy as np
import pytest

import batch_oracle as bo
import cma_route_cases as rc
import pyoracle as po
from _boxes import binding_witness, percoord_box, percoord_centre, percoord_guess

pytestmark = pytest.mark.gpu


def _close(a, b, rtol, what):
    """|a - b|_max <= rtol |b|_max: the `_close` of test_cma_gpu.py / test_sep_gpu.py"""
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    assert a.shape == b.shape, "%s: shape %s vs %s" % (what, a.shape, b.shape)
    err = np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)
    assert err <= rtol, "%s: rel err %.3e > %.1e" % (what, err, rtol)


# ---- CMA family, bound=True ---------------------------------------------------------------------------
def _cma_oracle(oracle_lib, variant, lam, sigma0, seed, obj, lo, up, guess):
    o = po.cma(oracle_lib, variant, 10 ** 9, 1e-12, lam, sigma0=sigma0, bound=True)
    o.set_rng(po.RNG_PHILOX, seed)
    o.init(obj, lo, up, guess)
    return o


def _cma_witness(oracle_lib, variant, n, lam, sigma0, seed, obj, gens):
    lo, up = percoord_box(n)
    o = _cma_oracle(oracle_lib, variant, lam, sigma0, seed, obj, lo, up, percoord_centre(n))
    states = []
    for _ in range(gens):
        o.iterate()
        states.append(o.get("arx").copy())
    o.destroy()
    return binding_witness(states, lo, up)


# (variant, n, lambda, sigma0, seed, objective, knobs, the sampler of tests/cma_route_cases.py it must take)
DENSE = [
    (24, 8, 0.5, 11, "sphere", {}, "cma_sample_eval64<1, 8>"),
    (37, 50, 0.5, 11, "sphere", {}, "cma_sample_eval64<1, 32>"),
    (100, 8, 0.5, 11, "sphere", {}, "cma_sample_eval64<2, 32>"),
    (132, 16, 0.5, 11, "sphere", {}, "cma_sample_eval<1, 16, false>"),
    (132, 528, 0.1, 11, "sphere", {}, "cma_sample_eval<4, 4, false>"),
    (260, 16, 0.5, 11, "sphere", {}, "cma_sample_eval<8, 4, false>"),
    # the whole-population kernel, whose lean build has no clamp: bound=True must keep it guarded
    (128, 16, 0.5, 11, "rosenbrock", dict(sample128_min=1), "cma_sample_eval128"),
]


@pytest.mark.parametrize("variant", ["cmaes", "active"])
@pytest.mark.parametrize("n,lam,sigma0,seed,obj,knobs,route", DENSE,
                         ids=["n%d-lam%d" % (c[0], c[1]) for c in DENSE])
def test_dense_cma_clamps_to_its_own_coordinates_bounds(hip, oracle_lib, variant, n, lam, sigma0, seed,
                                                        obj, knobs, route):
    """loc[t] / upc[t] of cma_sample_eval, the registers of cma_sample_eval64 and the guarded build
    of cma_sample_eval128: every phase of test_cma_gpu.py's walk, its tolerances"""
    from bboptpy_amd import _ffi
    gens = 6 if n <= 256 else 3
    _cma_witness(oracle_lib, variant, n, lam, sigma0, seed, obj, gens)
    lo, up = percoord_box(n)
    guess = percoord_centre(n)
    cls = hip.ActiveCMAES if variant == "active" else hip.CMAES
    g = cls(10 ** 9, 1e-12, lam, sigma0, True, seed=seed)
    g.initialize(getattr(hip.objectives, obj), lo, up, guess)
    for key, v in knobs.items():
        g.set_state(key, [float(v)])
    o = _cma_oracle(oracle_lib, variant, lam, sigma0, seed, obj, lo, up, guess)
    on_lo = on_up = 0
    for gen in range(gens):
        # (the device's eigenbasis goes to the oracle as in test_cma_gpu.py:64-69)
        o.set("B", g.get_state("B"))
        o.set("D", g.get_state("D"))
        o.set("invsqrtC", g.get_state("invsqrtC"))
        g.phase(_ffi.PHASE_SAMPLE_EVALUATE)
        assert rc.SAMPLE_NAMES[int(g.get_state("sample_route")[0])] == route
        assert int(g.get_state("sample_lean")[0]) == 0
        o.step("sample")
        o.step("evaluate_sort")
        X, Xo = g.get_state("arx").reshape(lam, n), o.get("arx").reshape(lam, n)
        _close(X, Xo, 1e-11, "arx gen %d" % gen)                                     # test_cma_gpu.py:76
        assert np.all(X >= lo) and np.all(X <= up)
        # a clamped coordinate is the bound itself, where the oracle's is
        np.testing.assert_array_equal(X == lo, Xo == lo)
        np.testing.assert_array_equal(X == up, Xo == up)
        on_lo, on_up = on_lo + int((Xo == lo).sum()), on_up + int((Xo == up).sum())
        g.phase(_ffi.PHASE_RANK)
        _close(g.get_state("fit_val"), o.get("fit_val"), 1e-10, "sorted fitness")    # :79
        np.testing.assert_array_equal(g.get_state("fit_idx").astype(int), o.get("fit_idx").astype(int))
        assert int(g.get_state("fev")[0]) == int(o.scalar("fev"))
        g.phase(_ffi.PHASE_UPDATE)
        g.phase(_ffi.PHASE_EIGEN)
        o.step("update_distribution")
        _close(g.get_state("xmean"), o.get("xmean"), 1e-11, "xmean")                  # :92
        _close(g.get_state("ps"), o.get("ps"), 1e-10, "ps")                           # :93
        _close(g.get_state("pc"), o.get("pc"), 1e-10, "pc")                           # :94
        _close(g.get_state("sigma"), o.get("sigma"), 1e-10, "sigma")                  # :95
        if variant == "active":
            _close(g.get_state("ycoeff"), o.get("ycoeff"), 1e-9, "ycoeff")            # :97
        _close(np.tril(g.get_state("C").reshape(n, n)), np.tril(o.get("C").reshape(n, n)), 1e-10,
               "C (lower)")                                                          # :99
        assert int(g.get_state("eigen_done")[0]) == int(o.scalar("eigen_done"))
        g.phase(_ffi.PHASE_HISTORY_STOP)
        o.step("update_history")
        assert int(g.get_state("flag")[0]) == o.converged()
    assert on_lo > 0 and on_up > 0
    o.destroy()


def test_whole_population_kernel_clamps_every_population(hip, oracle_lib):
    """n = 128, lambda = 4096, P = 8: cma_sample_eval128 by size; with bound=True its guarded build,
    every population clamped to the shared box from its own guess (test_cma_gpu.py's
    test_many_population_sampling_matches_oracle, its tolerances)"""
    from bboptpy_amd import _ffi
    n, lam, P, seed, sigma0 = 128, 4096, 8, 11, 0.25
    lo, up = percoord_box(n)
    _cma_witness(oracle_lib, "active", n, lam, sigma0, seed, "rosenbrock", 2)
    guess = np.vstack([percoord_centre(n)[None, :], percoord_guess(n, P - 1)])
    g = hip.ActiveCMAES(10 ** 9, 1e-12, lam, sigma0, True, seed=seed, populations=P)
    g.initialize(hip.objectives.rosenbrock, lo, up, guess)
    for ph in range(5):             # a non-trivial basis: one full generation first
        g.phase(ph)
    it = int(g.get_state("it")[0])
    z = np.zeros(lam * n)
    oracle_lib.f("philox_normals")(seed, it, lam, n, z)
    B, D = g.get_state("B").reshape(n, n), g.get_state("D")
    m, sigma = g.get_state("xmean"), g.get_state("sigma")[0]
    g.phase(_ffi.PHASE_SAMPLE_EVALUATE)
    assert rc.SAMPLE_NAMES[int(g.get_state("sample_route")[0])] == "cma_sample_eval128"
    assert int(g.get_state("sample_lean")[0]) == 0
    raw = m + sigma * (z.reshape(lam, n) * D) @ B.T
    want = np.clip(raw, lo, up)
    X = g.get_state("arx").reshape(lam, n)
    np.testing.assert_allclose(X, want, rtol=0, atol=1e-12)
    # clear of the bound by more than the tolerance: clamped exactly where the statement clamps
    sure = np.abs(raw - lo) > 1e-9
    np.testing.assert_array_equal((X == lo)[sure], (raw < lo)[sure])
    sure = np.abs(raw - up) > 1e-9
    np.testing.assert_array_equal((X == up)[sure], (raw > up)[sure])
    for p in range(P):
        X = g.get_state("arx", p).reshape(lam, n)
        f = g.get_state("fitness", p)
        assert np.all(X >= lo) and np.all(X <= up), p
        assert (X == lo).any() and (X == up).any(), p
        fo = np.array([oracle_lib.objective("rosenbrock", X[i]) for i in range(0, lam, 97)])
        np.testing.assert_allclose(f[::97], fo, rtol=1e-11, atol=1e-11)


# (n, lambda, sigma0, seed, generations, the sampler it must take)
SEP = [
    (8, 8, 0.7, 22, 6, "sep_sample_eval<16, 256, false>"),
    (260, 16, 0.5, 11, 6, rc.ROWS),
    (272, 16, 0.5, 11, 6, rc.ROWS),      # (lean without the clamp: sep_sample_sum<256, 0>)
    (1024, 16, 0.5, 11, 6, rc.ROWS),     # (lean without the clamp: sep_sample_sum<256, 4>)
    (2064, 8, 0.5, 11, 6, "sep_sample_eval<64, 256, false>"),
]


@pytest.mark.parametrize("n,lam,sigma0,seed,gens,route", SEP, ids=["n%d" % c[0] for c in SEP])
def test_sep_cma_clamps_to_its_own_coordinates_bounds(hip, oracle_lib, n, lam, sigma0, seed, gens, route):
    """every separable sampler with the clamp on: test_sep_gpu.py's walk, its tolerances"""
    from bboptpy_amd import _ffi
    _cma_witness(oracle_lib, "sep", n, lam, sigma0, seed, "sphere", gens)
    lo, up = percoord_box(n)
    guess = percoord_centre(n)
    g = hip.SepCMAES(10 ** 9, 1e-12, lam, sigma0, True, seed=seed)
    g.initialize(hip.objectives.sphere, lo, up, guess)
    o = _cma_oracle(oracle_lib, "sep", lam, sigma0, seed, "sphere", lo, up, guess)
    for key in ("mueff", "cc", "cs", "ccov", "damps", "chi"):
        assert g.get_state(key)[0] == o.scalar(key), key
    for gen in range(gens):
        g.phase(_ffi.PHASE_SAMPLE_EVALUATE)
        assert rc.SAMPLE_NAMES[int(g.get_state("sample_route")[0])] == route
        assert int(g.get_state("sample_lean")[0]) == 0
        o.step("sample")
        o.step("evaluate_sort")
        X, Xo = g.get_state("arx").reshape(lam, n), o.get("arx").reshape(lam, n)
        _close(X, Xo, 1e-14, "arx gen %d" % gen)                                      # test_sep_gpu.py:60
        assert np.all(X >= lo) and np.all(X <= up)
        np.testing.assert_array_equal(X == lo, Xo == lo)
        np.testing.assert_array_equal(X == up, Xo == up)
        g.phase(_ffi.PHASE_RANK)
        _close(g.get_state("fit_val"), o.get("fit_val"), 1e-11, "sorted fitness")     # :63
        np.testing.assert_array_equal(g.get_state("fit_idx").astype(int), o.get("fit_idx").astype(int))
        g.phase(_ffi.PHASE_UPDATE)
        g.phase(_ffi.PHASE_EIGEN)
        o.step("update_distribution")
        for key, tol in (("xmean", 1e-13), ("ps", 1e-11), ("pc", 1e-11), ("csep", 1e-11), ("D", 1e-11)):
            _close(g.get_state(key), o.get(key), tol, "%s gen %d" % (key, gen))      # :70-72
        _close(g.get_state("sigma"), [o.scalar("sigma")], 1e-11, "sigma")             # :73
        g.phase(_ffi.PHASE_HISTORY_STOP)
        o.step("update_history")
        assert int(g.get_state("flag")[0]) == o.converged()
        for key in ("xmean", "ps", "pc", "csep", "D", "sigma"):                       # :78-81
            o.set(key, g.get_state(key))
    o.destroy()


# ---- swarm engines: P populations of one handle, each beside its own oracle run ------------------------
def _swarm_oracle(oracle_lib, c, p, lo, up, guess):
    if c["engine"] == "apso":
        o = po.apso(oracle_lib, 10 ** 7, 1e-12, c["size"], c["correct"])
        o.set_mode(True, po.RNG_PHILOX, c["seed"])
        o.set_sub(p)
    else:
        o = bo.oracle_object(oracle_lib, c, p, init=False)
    o.init(c["obj"], lo, up, guess[p])
    if c["engine"] == "apso":
        o.set_chunk(c["chunk"])
    return o


def _swarm_witness(oracle_lib, c, lo, up, guess):
    """from the oracle alone, population by population"""
    e, n = c["engine"], c["n"]
    for p in range(c["P"]):
        o = _swarm_oracle(oracle_lib, c, p, lo, up, guess)
        xs, vs, yhats = [], [], []
        for _ in range(c["gens"]):
            o.iterate()
            xs.append(o.get("x").copy())
            if e == "ccpso":
                yhats.append(o.get("yhat").copy())
            if e == "apso":
                vs.append(o.get("v").reshape(-1, n).copy())
        if e in ("shade", "jade", "sansde"):
            rl, ru = o.repairs()
            assert rl >= 3 and ru >= 3, "population %d: %d / %d coordinates repaired" % (p, rl, ru)
        elif e == "apso" and not c["correct"]:
            vm = 0.2 * (up - lo)                       # vdamp (apso.cpp), oracle/bbo_oracle_pop.inc
            at_lo = np.any([(v == -vm).any(0) for v in vs], axis=0)
            at_up = np.any([(v == vm).any(0) for v in vs], axis=0)
            assert at_lo.sum() >= 3 and at_up.sum() >= 3, (p, at_lo.sum(), at_up.sum())
        elif e == "ccpso":
            binding_witness(yhats, lo, up)
            assert np.any([(x.reshape(-1, n) == lo).any(0) for x in xs], axis=0).sum() >= 3
            assert np.any([(x.reshape(-1, n) == up).any(0) for x in xs], axis=0).sum() >= 3
        else:
            binding_witness(xs, lo, up)
        o.destroy()


def _swarm_case(engine, n, size, gens, seed, kw=None, P=2, correct=True, chunk=None, set_chunk=None):
    c = bo.case(engine, n, size, "sphere", kw, P=P, gens=gens, seed=seed, chunk=chunk)
    c["correct"], c["set_chunk"] = correct, set_chunk
    c["id"] += "" if correct else "-free"
    c["id"] += "-ring" if c["kw"].get("ring") else ""
    c["id"] += "-pcauchy%g" % c["kw"]["pcauchy"] if "pcauchy" in c["kw"] else ""
    return c


SWARMS = [
    # the blo[u] / bup[u] lane units, the second 128-column pass, 8 rows per workgroup
    _swarm_case("shade", 33, 50, 10, 99), _swarm_case("shade", 201, 24, 10, 99),
    _swarm_case("shade", 600, 20, 10, 99),
    _swarm_case("jade", 33, 50, 10, 99), _swarm_case("jade", 201, 24, 10, 99),
    _swarm_case("jade", 600, 20, 10, 99),
    _swarm_case("sansde", 33, 50, 10, 123), _swarm_case("sansde", 201, 24, 10, 123),
    _swarm_case("sansde", 600, 20, 10, 123),
    # pso_update's coordinate pairs, pso_control's elitist coordinate, vmax; 16 < 48: three chunks
    _swarm_case("apso", 33, 48, 15, 4242, chunk=16, set_chunk=16),
    _swarm_case("apso", 33, 48, 15, 4242, chunk=16, set_chunk=16, correct=False),
    _swarm_case("apso", 513, 130, 15, 4242, chunk=48),
    _swarm_case("apso", 513, 130, 15, 4242, chunk=48, correct=False),
    _swarm_case("cso", 33, 50, 25, 321), _swarm_case("cso", 301, 30, 25, 321),
    _swarm_case("cso", 513, 30, 25, 321, dict(ring=True)),
    # the Gaussian and the Cauchy branch of the draw around the personal best: mostly the one, mostly
    # the other (a pcauchy outside (0, 1) is the adaptive rule, which starts at 0.5)
    _swarm_case("ccpso", 12, 8, 25, 7, dict(pps=[2, 3, 6], pcauchy=0.1)),
    _swarm_case("ccpso", 12, 8, 25, 48, dict(pps=[2, 3, 6], pcauchy=0.9)),
]


@pytest.mark.parametrize("c", SWARMS, ids=[c["id"] for c in SWARMS])
def test_swarms_under_the_percoord_box(hip, oracle_lib, c):
    e, n, P = c["engine"], c["n"], c["P"]
    lo, up = percoord_box(n)
    guess = percoord_guess(n, P)
    _swarm_witness(oracle_lib, c, lo, up, guess)
    if e == "apso":
        g = hip.APSO(mfev=10 ** 7, tol=1e-12, np=c["size"], correct=c["correct"], seed=c["seed"],
                     populations=P)
    else:
        g = bo.device_handle(hip, c)
    g.initialize(hip.objectives.sphere, lo, up, guess)
    if e == "apso":
        if c["set_chunk"]:
            g.set_state("chunk", [float(c["set_chunk"])])
        assert int(g.get_state("chunk")[0]) == c["chunk"] < c["size"]     # the swarm moves in several chunks
    objs = [_swarm_oracle(oracle_lib, c, p, lo, up, guess) for p in range(P)]
    worst = bo.Worst()
    for p, o in enumerate(objs):
        # the init kernel: the oracle's map u (up[j] - lo[j]) + lo[j] of the same uniforms, inside the box
        bo.compare_init(bo.Compare(g, o, p, "init", worst), c)
        X = g.get_state("x", p).reshape(-1, n)
        assert np.all(X >= lo) and np.all(X <= up), p
    for gen in range(c["gens"]):
        g.iterate()
        for p, o in enumerate(objs):
            o.iterate()
            bo.COMPARE[e](bo.Compare(g, o, p, "generation %d" % gen, worst), c)
            if c["correct"]:
                X = g.get_state("x", p).reshape(-1, n)
                assert np.all(X >= lo) and np.all(X <= up), (p, gen)
    print("%s, P = %d, %d generations: worst relative deviation from the oracle runs %s"
          % (c["id"], P, c["gens"], worst))
    for o in objs:
        o.destroy()


# ---- the restart drivers: every restart point is drawn coordinate by coordinate from the box ------------
@pytest.mark.parametrize("driver,seed", [("bipop", 21), ("ipop", 24)])
def test_restart_points_are_drawn_from_each_coordinates_own_interval(hip, oracle_lib, driver, seed):
    """tests/test_restart_gpu.py's per-decision comparison (the oracle takes over the device's
    bookkeeping before each restart; restart point and plan must be identical), here with a box in
    which u (up[i] - lo[i]) + lo[i] is a different map in every coordinate"""
    n, mfev = 7, 40000
    lo, up = percoord_box(n)
    guess = percoord_guess(n)
    base = hip.ActiveCMAES(mfev=1, tol=1e-6, np=4)
    ob = po.cma(oracle_lib, "active", 1, 1e-6, 4)
    if driver == "bipop":
        drv = hip.BiPopCMAES(base, mfev=mfev, seed=seed)
        o = po.bipop(oracle_lib, ob, mfev)
        book = ("fev", "it", "largelambda", "largebudget", "smallbudget", "largerestarts",
                "smallrestarts", "bestregime", "fxbest")
    else:
        drv = hip.IPopCMAES(base, mfev=mfev, seed=seed)
        o = po.ipop(oracle_lib, ob, mfev)
        book = ("fev", "it", "lambda", "sigma", "fxbest")
    drv.initialize(hip.objectives.rastrigin, lo, up, guess)
    o.set_mode(False, po.RNG_PHILOX, seed)
    o.init("rastrigin", lo, up, guess)
    gd = lambda k: drv.get_state(k)[0]
    plan = ("last_regime", "last_lambda", "last_sigma", "last_maxfev")
    assert [gd(k) for k in plan] == [o.scalar(k) for k in plan]
    rows, seen = 0, []
    for _ in range(8):
        if gd("fev") >= mfev or (driver == "bipop" and gd("largerestarts") >= 9):
            break
        for k in book:
            o.rset(k, gd(k))
        drv.iterate()
        o.iterate()
        x0 = drv.get_state("x0")
        np.testing.assert_array_equal(x0, o.get("x0"))
        assert np.all(x0 >= lo) and np.all(x0 <= up)
        assert [gd(k) for k in plan] == [o.scalar(k) for k in plan], "restart %d plan" % (rows + 1)
        seen.append(x0.copy())
        rows += 1
    assert rows >= 4
    # the draws do spread over each coordinate's own interval: no two restart points share a coordinate
    assert all(np.unique(np.array(seen)[:, j]).size == rows for j in range(n))


# ---- draw-only users of the box: the initial population is the map lo[j] + u (up[j] - lo[j]) of the
# generator's uniforms, recomputed here with the host twin of the generator ------------------------------
def _u01(lo, hi):
    return float(((hi << 32) | lo) >> 11) * 2. ** -53


STREAM_INIT, STREAM_AMALGAM_INIT = 2, 26        # bbo_rng.hpp


def _rows_equal(have, want, what):
    """the same rows, whatever their order"""
    have, want = np.asarray(have, float), np.asarray(want, float)
    assert have.shape == want.shape, what
    key = lambda M: M[np.lexsort(M.T[::-1])]
    assert key(have).tobytes() == key(want).tobytes(), what


@pytest.mark.parametrize("n", [37, 257])
def test_amalgam_draws_its_first_population_from_each_coordinates_own_interval(hip, n):
    """amalgam_init: coordinates 2 q and 2 q + 1 of row r share one Philox call (r, q); n = 37 ends in
    half a pair, 257 goes through the lane loop more than once"""
    from bboptpy_amd.distributed import philox4x32_10
    P, seed = 2, 50 + n
    lo, up = percoord_box(n)
    g = hip.AMALGAM(10 ** 9, 0., 0., 0, True, False, False, seed=seed, populations=P)
    g.initialize("sphere", lo, up, np.zeros(P * n))
    npop = int(g.get_state("np")[0])
    for p in range(P):
        want = np.empty((npop, n))
        for r in range(npop):
            for q in range((n + 1) // 2):
                w = philox4x32_10(seed, r, q, 0, (STREAM_AMALGAM_INIT << 24) | p)
                for t, u in enumerate((_u01(w[0], w[1]), _u01(w[2], w[3]))):
                    j = 2 * q + t
                    if j < n:
                        want[r, j] = lo[j] + u * (up[j] - lo[j])
        X = g.get_state("arx", p).reshape(npop, n)
        assert (X >= lo).all() and (X <= up).all(), p
        _rows_equal(X, want, "population %d" % p)


@pytest.mark.parametrize("n,np_", [(37, 20), (257, 5)])
def test_spiral_draws_its_first_points_from_each_coordinates_own_interval(hip, n, np_):
    """spiral_init: one Philox call per (point, coordinate)"""
    from bboptpy_amd.distributed import philox4x32_10
    P, seed = 2, 100 * n + np_
    lo, up = percoord_box(n)
    g = hip.SpiralSearch(10 ** 9, 0., np_, seed=seed, populations=P)
    g.initialize("sphere", lo, up, np.zeros(P * n))
    for p in range(P):
        want = np.empty((np_, n))
        for i in range(np_):
            for j in range(n):
                w = philox4x32_10(seed, i, j, 0, (STREAM_INIT << 24) | p)
                want[i, j] = _u01(w[0], w[1]) * (up[j] - lo[j]) + lo[j]
        X = g.get_state("x", p).reshape(np_, n)
        assert (X >= lo).all() and (X <= up).all(), p
        _rows_equal(X, want, "population %d" % p)


def test_concurrent_ipop_restarts_from_the_points_the_device_driver_draws(hip):
    """ConcurrentIPop with one slot per round draws its restart points on the host; the device's IPopCMAES
    (held to the oracle above) draws them in bbo_restart.hip: the same points bit for bit, each inside its
    coordinate's interval, and the same history (tests/test_distributed_gpu.py's comparison)"""
    from bboptpy_amd.distributed import ConcurrentIPop
    n, mfev, seed = 6, 30000, 46
    lo, up = percoord_box(n)
    guess = percoord_guess(n)
    d = ConcurrentIPop(mfev=mfev, tol=1e-8, seed=seed, world_size=1, rank=0)
    starts, run = [], d._device_run

    def spy(f, lam, sigma, maxfev, x0, s, slot=0):
        starts.append(np.array(x0, float))
        return run(f, lam, sigma, maxfev, x0, s, slot=slot)
    d._device_run = spy
    sol = d.optimize("rastrigin", lo, up, guess)
    got = [(h["lam"], h["sigma"], h["maxfev"], h["used"], h["fx"]) for h in d.state.history]
    base = hip.ActiveCMAES(mfev=1, tol=1e-8, np=4)
    c = hip.IPopCMAES(base, mfev=mfev, seed=seed)
    c.initialize(hip.objectives.rastrigin, lo, up, guess)
    gs = lambda k: c.get_state(k)[0]
    row = lambda: (int(gs("last_lambda")), gs("last_sigma"), int(gs("last_maxfev")), int(gs("last_inner_fev")),
                   gs("fx"))
    rows_c, x0s = [row()], [guess]
    while gs("fev") < mfev:
        c.iterate()
        rows_c.append(row())
        x0s.append(c.get_state("x0").copy())
    assert len(got) >= 3 and len(starts) == len(x0s)
    for k, (a, b) in enumerate(zip(starts, x0s)):
        np.testing.assert_array_equal(a, b, err_msg="restart %d" % k)
        assert (a >= lo).all() and (a <= up).all(), k
    assert got == rows_c
    assert sol.n_evals == int(gs("fev"))
    np.testing.assert_array_equal(sol.x, c.get_state("xbest"))
