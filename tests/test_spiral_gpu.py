"""GPU: the SpiralSearch kernels against tests/spiral_model.py, and the engine's behaviour at the C ABI.

The rotation is held bit for bit: the model's device form (the difference x_i - xbest rotated once,
in the reference's operation order) is fed the device's own cos, sin, r and xbest, and its new
points must be the device's.  The tile in LDS, split between LDS and global memory, and in global
memory whole, and every fusion depth K, give the same bits.  Against the recorded reference: tests/test_spiral_golden_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import spiral_model as sm
from slpso_model import device_objective
from test_hees_model import band
from test_spiral_model import GOLD, _h

pytestmark = pytest.mark.gpu

K = 8       # SPIRAL_DEFAULT_K: the stages spiral_rotate fuses in registers
STREAM_SPIRAL = 19
# two cosines or sines of one angle: the device library's bound is 2 units in the last place, the
# host libraries' 1, and a unit in the last place of a value up to 1 is 2^-53 at most
TRIG_ULPS = 3 * 2. ** -53
KEYS = ("x", "f", "r", "theta", "cos", "sin", "xbest", "fbest", "ibest", "fev", "it", "flag")


def _bits(a, b, what):
    a, b = np.asarray(a, float).ravel(), np.asarray(b, float).ravel()
    assert a.shape == b.shape, what
    assert a.tobytes() == b.tobytes(), (what, np.flatnonzero(a != b)[:8], a[a != b][:4], b[a != b][:4])


def _snapshot(g, p=0):
    return {k: g.get_state(k, p).copy() for k in KEYS}


def _box(n, w=5.):
    return -w * np.ones(n), w * np.ones(n), np.zeros(n)


def _start(hip, n, np_, obj="rosenbrock", seed=7, P=1, **kw):
    g = hip.SpiralSearch(10 ** 9, 0., np_, seed=seed, populations=P, **kw)
    lo, up, guess = _box(n)
    g.initialize(obj, lo, up, np.tile(guess, P))
    return g


def _rotation_is_the_model(g, n, np_, p=0, gens=2):
    """phase by phase: the rows spiral_rotate writes are step_device_rows of the state it read"""
    for _ in range(gens):
        g.phase(0)
        x = g.get_state("x", p).reshape(np_, n)
        want = sm.step_device_rows(x, g.get_state("xbest", p), g.get_state("r", p), g.get_state("cos", p),
                                   g.get_state("sin", p))
        g.phase(1)
        _bits(g.get_state("x", p), want, "rotated points")
        g.phase(2)
        g.phase(3)


# rows wider than one pass of a 256-thread workgroup: one live lane in the second pass (257), an
# odd n that is no multiple of 4 or 64 (301) and the cap (512), where most of the tile is in global memory
WIDE_SHAPES = [(257, 5), (301, 6), (512, 8)]
ROTATION_SHAPES = [(n, np_) for np_ in (1, 20, 63, 64, 65, 130) for n in (1, 2, 3, K, K + 1, 2 * K + 1, 33, 128)]


@pytest.mark.parametrize("n,np_", ROTATION_SHAPES + WIDE_SHAPES)
def test_the_rotation_is_the_device_form_of_the_model_bit_for_bit(hip, n, np_):
    wide = n > 256
    g = _start(hip, n, np_, obj="ellipsoid" if n == 301 else "rosenbrock", seed=100 * n + np_, taur=1.,
               tautheta=1.)                                                 # every point its own r and angle
    assert int(g.get_state("rot_k")[0]) == K
    assert int(g.get_state("rot_split")[0]) == max(n - int(g.get_state("rot_lds_coords")[0]), 0)
    if n == 512:
        assert int(g.get_state("rot_split")[0]) > 0        # the model against the tile in global memory
    _rotation_is_the_model(g, n, np_, gens=4 if wide else 2)
    if wide:        # the values of the rotated rows: the sum in the device's order (eval_row_group<64>), bit for bit
        fobj = device_objective("ellipsoid" if n == 301 else "rosenbrock", n)
        _bits(g.get_state("f"), [fobj(row) for row in g.get_state("x").reshape(np_, n)], "values")
    assert len(set(g.get_state("theta").tolist())) == np_


@pytest.mark.parametrize("over", [0, 1, 9])
def test_the_tile_in_global_memory_gives_the_bits_of_the_tile_in_lds(hip, over):
    """at the largest n whose tile lives in LDS whole, at the next n (one coordinate in global
    memory, the pivots of the first fused step on both sides) and where a fused step ends on the
    border: the dbg bit, which puts the whole tile into global memory, changes no bit, and the model
    agrees"""
    probe = _start(hip, 2, 3)
    n = int(probe.get_state("rot_lds_coords")[0]) + over
    np_ = 70
    runs = []
    for dbg in (0, 1):
        g = _start(hip, n, np_, seed=11, taur=0.5, tautheta=0.5)
        g.set_state("dbg", [float(dbg)])
        assert int(g.get_state("rot_split")[0]) == (n if dbg else over)
        for _ in range(2):
            g.iterate()
        runs.append(_snapshot(g))
        _rotation_is_the_model(g, n, np_, gens=1)
    for k in KEYS:
        _bits(runs[0][k], runs[1][k], k)


def test_a_grid_that_fills_the_device_keeps_the_bits(hip):
    """more wavefronts than the device holds at once (1088): the split tile, the tile in global
    memory whole and the model agree on the first and the last population"""
    n, np_, P = 90, 4096, 17
    runs = []
    for dbg in (0, 1):
        g = _start(hip, n, np_, seed=19, P=P, tautheta=0.5)
        g.set_state("dbg", [float(dbg)])
        assert int(g.get_state("rot_split")[0]) == (n if dbg else 10)
        g.phase(0)
        want = {p: sm.step_device_rows(g.get_state("x", p).reshape(np_, n), g.get_state("xbest", p), g.get_state("r", p),
                                       g.get_state("cos", p), g.get_state("sin", p)) for p in (0, P - 1)}
        g.phase(1)
        for p in (0, P - 1):
            _bits(g.get_state("x", p), want[p], "population %d, dbg %d" % (p, dbg))
        g.phase(2)
        g.phase(3)
        runs.append([_snapshot(g, p) for p in (0, P - 1)])
    for sa, sb in zip(*runs):
        for k in KEYS:
            _bits(sa[k], sb[k], k)


@pytest.mark.parametrize("k", [1, 2, 4])
def test_every_fusion_depth_gives_the_bits_of_the_default(hip, k):
    n, np_ = 37, 65
    runs = []
    for depth in (K, k):
        for dbg in (0, 1):
            g = _start(hip, n, np_, seed=21, taur=0.5, tautheta=0.5)
            g.set_state("rot_k", [float(depth)])
            g.set_state("dbg", [float(dbg)])
            assert int(g.get_state("rot_k")[0]) == depth
            for _ in range(2):
                g.iterate()
            runs.append(_snapshot(g))
    for other in runs[1:]:
        for key in KEYS:
            _bits(runs[0][key], other[key], key)


def test_population_zero_of_a_batch_is_the_single_run(hip):
    """np = 20: the points of three and a fifth populations share a wavefront"""
    n, np_, P = 7, 20, 5
    one, many = _start(hip, n, np_, seed=33), _start(hip, n, np_, seed=33, P=P)
    for _ in range(5):
        one.iterate()
        many.iterate()
    sa, sb = _snapshot(one), _snapshot(many)
    for k in KEYS:
        _bits(sa[k], sb[k], k)
    assert not np.array_equal(many.get_state("x", 1), many.get_state("x", 0))      # its own sub-stream
    for p in range(1, P):       # and a wavefront that straddles populations rotates each about its own xbest
        g = many
        x = g.get_state("x", p).reshape(np_, n)
        g.inject_uniforms(np.full((P, np_, 4), 0.75))      # no coin fires: phase 0 changes nothing
        g.phase(0)
        want = sm.step_device_rows(x, g.get_state("xbest", p), g.get_state("r", p), g.get_state("cos", p),
                                   g.get_state("sin", p))
        g.phase(1)
        _bits(g.get_state("x", p), want, "population %d" % p)
        g.phase(2)
        g.phase(3)


def test_joint_best_rows_tie_to_the_lower_row(hip):
    n, np_ = 4, 70
    g = _start(hip, n, np_, obj="sphere", seed=3)
    x = np.random.default_rng(5).uniform(1., 4., (np_, n))
    x[66] = x[9] = [0.5, -0.25, 0.125, 0.]
    x[40] = -x[9]                   # the same value from another point
    g.set_state("x", x)
    assert int(g.get_state("ibest")[0]) == 9 and int(g.get_state("fev")[0]) == np_
    _bits(g.get_state("xbest"), x[9], "xbest")
    _bits(g.get_state("f")[[9, 40, 66]], [x[9] @ x[9]] * 3, "the tied values")
    flat = _start(hip, n, np_, obj=lambda v: 1., seed=3)
    flat.iterate()
    assert int(flat.get_state("ibest")[0]) == 0


def test_xbest_is_the_best_of_the_generation_and_a_point_on_it_stays(hip):
    """the objective moves between generations and rises by 1e6 each time, so every generation's best
    value is worse than the one before: xbest still follows this generation's values (a best-so-far
    would keep the first), and the row that was the best does not move"""
    n, np_ = 6, 23
    centres = np.random.default_rng(9).uniform(-4., 4., (8, n))
    calls = []

    def moving(X):
        c = centres[len(calls)]
        calls.append(1)
        return ((X - c) ** 2).sum(axis=1) + 1e6 * (len(calls) - 1)

    moving._bbo_vectorized = True
    g = _start(hip, n, np_, obj=moving, seed=41, tautheta=1.)
    rose = 0
    for gen in range(1, 7):
        ib, xb, fb = int(g.get_state("ibest")[0]), g.get_state("xbest").copy(), float(g.get_state("fbest")[0])
        g.iterate()
        x, f = g.get_state("x").reshape(np_, n), g.get_state("f")
        _bits(x[ib], xb, "the point on xbest")
        _bits(f, ((x - centres[gen]) ** 2).sum(axis=1) + 1e6 * gen, "f")
        now = int(np.argmin(f))
        assert int(g.get_state("ibest")[0]) == now and float(g.get_state("fbest")[0]) == f[now]
        _bits(g.get_state("xbest"), x[now], "xbest")
        rose += f[now] > fb
    assert len(calls) == 7 and rose == 6


def test_phases_one_at_a_time_are_iterate(hip):
    n, np_, P = 9, 20, 3
    a, b = _start(hip, n, np_, seed=5, P=P, taur=0.3), _start(hip, n, np_, seed=5, P=P, taur=0.3)
    for _ in range(3):
        a.iterate()
        for ph in range(4):
            b.phase(ph)
    for p in range(P):
        sa, sb = _snapshot(a, p), _snapshot(b, p)
        for k in KEYS:
            _bits(sa[k], sb[k], k)


def test_run_with_polling_is_iterate(hip):
    n, np_, P = 9, 20, 3
    a = _start(hip, n, np_, seed=6, P=P)
    b = _start(hip, n, np_, seed=6, P=P, poll_every=5)
    for _ in range(12):
        a.iterate()
    assert b.run(12) == 12
    for p in range(P):
        sa, sb = _snapshot(a, p), _snapshot(b, p)
        for k in KEYS:
            _bits(sa[k], sb[k], k)


def _device_sum(terms):
    """a sum as eval_row_group<64> adds it for n <= 64: one term per lane, xor butterfly"""
    a = np.zeros(64)
    a[:len(terms)] = terms
    for off in (32, 16, 8, 4, 2, 1):
        a = a[:off] + a[off:2 * off]
    return float(a[0])


def test_callback_path_equals_the_builtin(hip):
    n = 5
    lo, up, guess = _box(n)
    calls = []

    def sphere(x):
        calls.append(1)
        return _device_sum(x * x)

    def rosenbrock(X):
        calls.extend([1] * len(X))
        return [_device_sum(100. * ((x[1:] - x[:-1] * x[:-1]) * (x[1:] - x[:-1] * x[:-1])) + (1. - x[:-1]) * (1. - x[:-1]))
                for x in X]

    rosenbrock._bbo_vectorized = True
    for name, f in (("sphere", sphere), ("rosenbrock", rosenbrock)):
        del calls[:]
        runs = []
        for obj in (name, f):
            g = hip.SpiralSearch(130, 0., seed=13)
            sol = g.optimize(obj, lo, up, guess)
            runs.append((sol, _snapshot(g)))
        (a, sa), (b, sb) = runs
        assert a.n_evals == b.n_evals == len(calls) == 140 and not a.converged and not b.converged
        _bits(a.x, b.x, "x*")
        for k in KEYS:
            _bits(sa[k], sb[k], k)
        assert int(sa["flag"][0]) == 2


def test_the_budget_stop_overshoots_like_the_reference(hip):
    n = 3
    lo, up, guess = _box(n)
    g = hip.SpiralSearch(50, 0., seed=2)
    sol = g.optimize("sphere", lo, up, guess)
    assert sol.n_evals == 60 and sol.converged is False and int(g.get_state("flag")[0]) == 2
    assert int(g.get_state("it")[0]) == 2 and g.solution().converged is False
    _bits(sol.x, g.get_state("xbest"), "x*")
    assert g.run(5) == 0        # `while (fev < mfev)`: no generation once the budget is spent
    g = hip.SpiralSearch(20, 0., seed=2)
    assert g.optimize("sphere", lo, up, guess).n_evals == 20      # the initial points spend it


def test_a_stopped_population_is_frozen(hip):
    n, np_, P = 5, 20, 3
    g = hip.SpiralSearch(200, 0., np_, seed=17, populations=P, poll_every=2)
    lo, up, guess = _box(n)
    g.initialize("sphere", lo, up, np.tile(guess, P))
    g.set_state("fev", [180.], 1)       # population 1 has one generation left
    assert g.run(1) == 1
    assert [int(g.get_state("flag", p)[0]) for p in range(P)] == [0, 2, 0]
    frozen = _snapshot(g, 1)
    g.run(100)
    after = _snapshot(g, 1)
    for k in KEYS:
        _bits(frozen[k], after[k], k)
    assert [int(g.get_state("fev", p)[0]) for p in range(P)] == [200, 200, 200]
    assert [int(g.get_state("it", p)[0]) for p in range(P)] == [9, 1, 9]
    assert all(int(g.get_state("flag", p)[0]) == 2 and not g.solution(p).converged for p in range(P))


def _u01(lo, hi):
    return float(((hi << 32) | lo) >> 11) * 2. ** -53


def test_the_recorded_draws_are_the_uniforms_their_counters_assign(hip):
    from bboptpy_amd.distributed import philox4x32_10
    n, np_, P, seed = 4, 67, 2, 77
    kw = dict(taur=0.4, tautheta=0.6, rlow=0.8, rhigh=0.99, thetalow=0.5, thetahigh=2.5)
    g = _start(hip, n, np_, seed=seed, P=P, **kw)
    with pytest.raises(Exception):
        g.get_state("draws")
    g.set_state("record_draws", [1.])
    for gen in range(3):
        before = [(g.get_state("r", p).copy(), g.get_state("theta", p).copy()) for p in range(P)]
        g.iterate()
        for p in range(P):
            d = g.get_state("draws", p).reshape(np_, 4)
            want = np.empty((np_, 4))
            for i in range(np_):
                w0 = philox4x32_10(seed, i, 0, gen, (STREAM_SPIRAL << 24) | p)
                w1 = philox4x32_10(seed, i, 1, gen, (STREAM_SPIRAL << 24) | p)
                want[i] = [_u01(w0[0], w0[1]), _u01(w0[2], w0[3]), _u01(w1[0], w1[1]), _u01(w1[2], w1[3])]
            _bits(d, want, "draws")
            m = sm.Spiral(None, np_, **kw)
            m.rs, m.thetas = list(before[p][0]), list(before[p][1])
            m.draw(d)
            _bits(g.get_state("r", p), m.rs, "r")
            _bits(g.get_state("theta", p), m.thetas, "theta")
            assert 0 < (d[:, 0] < 0.4).sum() < np_ and 0 < (d[:, 2] < 0.6).sum() < np_
    # cos and sin follow theta: the device library's (2 ulp) against the host's (1 ulp)
    th = g.get_state("theta")
    assert np.abs(g.get_state("cos") - np.cos(th)).max() <= TRIG_ULPS
    assert np.abs(g.get_state("sin") - np.sin(th)).max() <= TRIG_ULPS


def test_r_and_theta_are_settable_and_cos_and_sin_follow(hip):
    n, np_ = 3, 5
    g = _start(hip, n, np_, seed=8, tautheta=0.)
    th = np.array([0., 0.5, 1., 2., 4.])
    g.set_state("theta", th)
    g.set_state("r", 0.5 * np.ones(np_))
    _bits(g.get_state("theta"), th, "theta")
    assert np.abs(g.get_state("cos") - np.cos(th)).max() <= TRIG_ULPS
    assert np.abs(g.get_state("sin") - np.sin(th)).max() <= TRIG_ULPS
    _rotation_is_the_model(g, n, np_, gens=1)
    _bits(g.get_state("r"), 0.5 * np.ones(np_), "r")


@pytest.mark.parametrize("obj", ["sphere", "rosenbrock"])
def test_outcome_bands_match_the_reference(hip, obj):
    b, P = GOLD["bands"], 64
    n = b["n"]
    g = hip.SpiralSearch(b["mfev"], b["tol"], seed=2024, populations=P)
    g.initialize(obj, -b["box"] * np.ones(n), b["box"] * np.ones(n), np.zeros(P * n))
    g.run(10 ** 6)
    got = [float(g.get_state("fbest", p)[0]) for p in range(P)]
    assert all(int(g.get_state("fev", p)[0]) == b["mfev"] for p in range(P))
    band(got, _h(b[obj]), obj + " device")


def test_configure_statuses_and_refusals(hip):
    from bboptpy_amd import _ffi
    L = _ffi.lib()
    d = _ffi.SpiralParams()
    L.bbo_spiral_params_default(C.byref(d))
    other = hip.DSA(1000, 1e-6, 1e-6, 12, seed=1)
    oh = other._ensure_handle()
    assert L.bbo_spiral_configure(oh, C.byref(d)) == _ffi.ERR_ARG
    assert "not a SpiralSearch handle" in L.bbo_last_error(oh).decode()
    assert L.bbo_spiral_phase(oh, 0) == _ffi.ERR_ARG and L.bbo_spiral_inject_uniforms(oh, None, 0) == _ffi.ERR_ARG
    g = hip.SpiralSearch(1000, 1e-6, seed=1)
    h = g._ensure_handle()
    assert L.bbo_spiral_configure(h, C.byref(d)) == 0
    assert L.bbo_spiral_configure(h, None) == _ffi.ERR_ARG
    bad = _ffi.SpiralParams()
    L.bbo_spiral_params_default(C.byref(bad))
    bad.theta = float("nan")
    assert L.bbo_spiral_configure(h, C.byref(bad)) == _ffi.ERR_ARG and "finite" in L.bbo_last_error(h).decode()
    assert L.bbo_spiral_phase(h, 0) == -2                       # BBO_ERR_STATE: before bbo_init
    n = 2
    lo, up = -np.ones(n), np.ones(n)
    # the limits, each named
    with pytest.raises(_ffi.BboError) as ei:
        hip.SpiralSearch(1000, 1e-6).initialize("sphere", -np.ones(513), np.ones(513), np.zeros(513))
    assert ei.value.status == _ffi.ERR_ARG and "512" in str(ei.value)
    for np_ in (0, 65537):
        with pytest.raises(_ffi.BboError) as ei:
            hip.SpiralSearch(1000, 1e-6, np_).initialize("sphere", lo, up, np.zeros(n))
        assert ei.value.status == _ffi.ERR_ARG and "65536" in str(ei.value)
    with pytest.raises(_ffi.BboError) as ei:
        hip.SpiralSearch(1000, 1e-6).initialize("sphere", lo, np.array([1., np.inf]), np.zeros(n))
    assert ei.value.status == _ffi.ERR_ARG and "finite" in str(ei.value)
    hip.SpiralSearch(1000, 1e-6, 3).initialize("sphere", -np.ones(512), np.ones(512), np.zeros(512))
    # an objective program: refused by the class and by the library, naming who takes one
    prog = hip.DeviceObjective('extern "C" __device__ double bbo_user_objective(const double *x, int n, '
                               'const double *data) { return x[0] * x[0]; }')
    with pytest.raises(ValueError) as ei:
        g.initialize(prog, lo, up, np.zeros(n))
    assert "SpiralSearch does not take a DeviceObjective" in str(ei.value) and "JADE" in str(ei.value)
    ob = _ffi.Objective()
    ob.kind, ob.user = _ffi.OBJ_PROGRAM, prog._handle
    st = L.bbo_init(h, n, lo, up, np.zeros(n), C.byref(ob))
    msg = L.bbo_last_error(h).decode()
    assert st == -1 and "SpiralSearch" in msg and "CMAES" in msg and "SHADE" in msg, (st, msg)
    g.initialize("sphere", lo, up, np.zeros(n))
    assert L.bbo_spiral_configure(h, C.byref(d)) == -2          # BBO_ERR_STATE
    assert "after bbo_init" in L.bbo_last_error(h).decode()
    assert L.bbo_spiral_phase(h, 4) == _ffi.ERR_ARG and L.bbo_spiral_phase(h, -1) == _ffi.ERR_ARG
    with pytest.raises(_ffi.BboError):                          # one table per population, np x 4
        g.inject_uniforms(np.zeros(3))
    with pytest.raises(_ffi.BboError):                          # [0, 1)
        g.inject_uniforms(np.ones((20, 4)))
    for key, val in (("rot_k", 3.), ("dbg", 2.), ("x", np.zeros(3)), ("fev", -1.), ("ibest", 0.)):
        with pytest.raises(_ffi.BboError):
            g.set_state(key, val)
    with pytest.raises(_ffi.BboError) as ei:
        g.get_state("draws")
    assert ei.value.status == -2
    with pytest.raises(_ffi.BboError) as ei:
        g.get_state("sigma")
    assert ei.value.status == -6
    # a NaN value ranks last
    nan = hip.SpiralSearch(1000, 0., 20, seed=4)
    nan.initialize(lambda x: float("nan") if x[0] > 0. else float(x @ x), lo, up, np.zeros(n))
    f = nan.get_state("f")
    assert np.isinf(f).any() and not np.isnan(f).any() and np.isfinite(f[int(nan.get_state("ibest")[0])])
