"""GPU: the CRS kernels against tests/crs_model.py, and the engine's behaviour at the C ABI.

The walk is held bit for bit: the model's device form is fed the device's own recorded draws and the
pool the kernel read, and every state key must be the device's after every iteration -- walked one
evaluation at a time through bbo_crs_phase, fused through bbo_iterate and bbo_run, and cut after every
single step (launch_evals = 1), which is the smallest setting at which a launch ends inside a recursion.
Against the recorded reference: tests/test_crs_golden_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import crs_model as cm
from slpso_model import device_objective
from test_crs_model import GOLD, _h
from test_hees_model import band

pytestmark = pytest.mark.gpu

CHUNK = 256             # CRS_DEFAULT_CHUNK: the iterations of one chunk of run()
KEYS = ("x", "f", "order", "cand", "fcand", "cand2", "fcand2", "fbest", "fworst", "fev", "it", "trials", "muts",
        "depth", "maxdepth", "stage", "pending", "flag", "stale")
DEPTH = 32              # the cap of the grid tests: a collapsed pool of 2 ends there, not 4096 frames later
RECORDS = 1024


def _bits(a, b, what):
    a, b = np.asarray(a, float).ravel(), np.asarray(b, float).ravel()
    assert a.shape == b.shape, what
    assert a.tobytes() == b.tobytes(), (what, np.flatnonzero(a != b)[:8], a[a != b][:4], b[a != b][:4])


def _snapshot(g, p=0):
    return {k: g.get_state(k, p).copy() for k in KEYS}


def _same_state(sa, sb, tag=""):
    for k in KEYS:
        _bits(sa[k], sb[k], tag + k)


def _start(hip, n, np_, obj="rosenbrock", seed=7, P=1, mfev=10 ** 6, tol=0., box=5., lower=None, inner=0.84, **kw):
    """At n >= 63 a pool that fills the box reflects out of it in all but one trial in thousands (every
    coordinate has to stay inside), and the walk would be one run of B pushes into the depth cap: there
    the pool is set to points of the inner 84 % of the box, from which about every second or third
    trial stays inside (`inner`: another share, for the rows past n = 256)."""
    g = hip.CRS(mfev, np_, tol, seed=seed, populations=P, **kw)
    lo = -box * np.ones(n) if lower is None else lower * np.ones(n)
    g.initialize(obj, lo, box * np.ones(n) if lower is None else lo.copy(), np.zeros(P * n))
    if n >= 63 and lower is None:
        rng = np.random.default_rng(seed)
        for p in range(P):
            g.set_state("x", rng.uniform(-inner * box, inner * box, (np_, n)), p)
    return g


def _model_of(g, n, np_, obj, box, p=0, mfev=10 ** 6, tol=0., f=None, lower=None, **kw):
    """the model's device form in the state the device holds"""
    lo = [-box] * n if lower is None else [lower] * n
    up = [box] * n if lower is None else [lower] * n
    m = cm.Crs(device_objective(obj, n) if f is None else f, n, np_, lo, up, mfev, tol, **kw)
    order = [int(v) for v in g.get_state("order", p)]
    fs = np.empty(np_)
    fs[order] = g.get_state("f", p)
    m.start(g.get_state("rows", p).reshape(np_, n), fs=fs)
    assert m.order == order, "the stable ranking"
    for k in ("fev", "it", "trials", "muts", "stale"):
        setattr(m, k, int(g.get_state(k, p)[0]))
    return m


def _device_is_model(g, m, tag, p=0):
    _bits(g.get_state("x", p), m.x(), tag + "x")
    _bits(g.get_state("f", p), m.fsorted(), tag + "f")
    assert [int(v) for v in g.get_state("order", p)] == m.order, tag + "order"
    _bits(g.get_state("cand", p), m.t, tag + "cand")
    _bits(g.get_state("cand2", p), m.t2, tag + "cand2")
    _bits(g.get_state("fcand", p), [m.ft], tag + "fcand")
    _bits(g.get_state("fcand2", p), [m.ft2], tag + "fcand2")
    _bits(g.get_state("fbest", p), [m.fsorted()[0]], tag + "fbest")
    _bits(g.get_state("fworst", p), [m.fsorted()[-1]], tag + "fworst")
    got = {k: int(g.get_state(k, p)[0]) for k in ("fev", "it", "trials", "muts", "depth", "maxdepth", "stage",
                                                  "pending", "flag", "stale")}
    want = dict(fev=m.fev, it=m.it, trials=m.trials, muts=m.muts, depth=0, maxdepth=m.maxdepth, stage=0, pending=0,
                flag=m.flag, stale=m.stale)
    assert got == want, (tag, got, want)


def _walk(g):
    """one iteration one evaluation at a time"""
    pending = g.phase(0)
    while pending:
        g.phase(1)
        pending = g.phase(2)


def _records(g, n, p=0):
    nrec = int(g.get_state("nrec", p)[0])
    assert 1 <= nrec <= RECORDS, nrec
    return g.get_state("draws", p).reshape(nrec, 2 * n)


# rows past one pass of a 256-thread workgroup: one live lane in the second pass (257), an odd n that
# is no multiple of 4 or 64 (301, ld = 302) and the cap; rosenbrock, ellipsoid, ellipsoid by the rule below
# (rosenbrock at n = 512 with np = 8 runs into the depth cap in the very first iteration under one set of
# draws in four: its first worst point is hard to beat; the ellipsoid with np = 12 walked all 20 iterations
# under every one of 12 generators tried with the model)
WIDE_SHAPES = [(257, 5), (301, 7), (512, 12)]
WALK_SHAPES = [(n, np_) for np_ in (2, 5, 70) for n in (1, 2, 63, 64, 65, 130)]


@pytest.mark.parametrize("n,np_", WALK_SHAPES + WIDE_SHAPES)
def test_the_walk_is_the_model_bit_for_bit(hip, n, np_):
    """40 iterations (20 past n = 256): the odd ones through bbo_crs_phase, the even ones fused
    (bbo_iterate and bbo_run in turn).  The model reads the records the device logged.  A pool that
    collapses (np = 2 does) ends at the depth cap, in the model at the same evaluation.  Past n = 256
    the pool starts in the inner 60 % of the box: with np <= 8 the centroid of n drawn rows is close to
    the pool's mean, and from there the model with a generator of its own takes every path of the
    recursion (B, M, an accepted mutation, a stale replacement) within 16 iterations."""
    wide = n > 256
    obj = ("sphere", "rosenbrock", "ellipsoid")[(n + np_) % 3] if n > 1 else "sphere"
    g = _start(hip, n, np_, obj=obj, seed=100 * n + np_, max_depth=DEPTH, **({"inner": 0.6} if wide else {}))
    # a lane per coordinate up to 256: the walk runs the configuration its n is meant to reach
    assert int(g.get_state("wg")[0]) == (64 if n <= 128 else 128 if n <= 256 else 256)
    g.set_state("record_draws", [float(RECORDS)])
    m = _model_of(g, n, np_, obj, 5., max_depth=DEPTH)
    tag0 = "n %d np %d " % (n, np_)
    for it in range(20 if wide else 40):
        tag = tag0 + "iteration %d " % it
        if it % 2:
            _walk(g)
        elif it % 4:
            assert g.run(1) == 1
        else:
            g.iterate()
        rec = _records(g, n)
        src = cm.TableSource(rec, n, np_)
        done = m.iterate(src)
        assert src.exhausted(), tag
        _device_is_model(g, m, tag)
        # the log is the table the model writes from the same draws
        _bits(rec, m.records, tag + "records")
        if not done:
            assert m.flag == 3 and m.maxdepth == DEPTH, tag
            break
    print(tag0, obj, "iterations", m.it, "fev", m.fev, "paths", m.paths, "flag", m.flag)
    if wide:
        assert m.it >= 10 and m.fev > np_ + m.it, "the wide walk ended early or never mutated: choose another pool"


@pytest.mark.parametrize("n,np_", [(5, 20), (65, 5), (130, 70)])
def test_a_fused_run_of_k_iterations_is_k_single_iterations(hip, n, np_):
    k = 37
    runs = []
    for how in ("run", "chunks", "iterate", "walk"):
        g = _start(hip, n, np_, seed=5, max_depth=DEPTH, **({"poll_every": 7} if how == "chunks" else {}))
        if how in ("run", "chunks"):
            g.run(k)
        else:
            for _ in range(k):
                if int(g.get_state("flag")[0]) == 3:
                    break
                g.iterate() if how == "iterate" else _walk(g)
        runs.append(_snapshot(g))
    for s in runs[1:]:
        _same_state(runs[0], s)
    assert int(runs[0]["it"][0]) == k or int(runs[0]["flag"][0]) == 3


@pytest.mark.parametrize("np_", [5, 70])
@pytest.mark.parametrize("n", [2, 65, 130])
def test_a_launch_cut_after_every_step_gives_the_bits_of_the_default(hip, n, np_):
    """launch_evals = 1: every launch ends after one drawn trial or one evaluation, inside the recursion
    wherever it stands, and the next one resumes from the saved stage, stack, t, t2, ft and ft2"""
    runs = []
    for steps in (0., 1., 3.):
        g = _start(hip, n, np_, seed=11 * n + np_, max_depth=DEPTH)
        assert g.get_state("launch_evals")[0] == 0.
        g.set_state("launch_evals", [steps])
        g.run(40)
        runs.append(_snapshot(g))
    _same_state(runs[0], runs[1], "one step per launch: ")
    _same_state(runs[0], runs[2], "three steps per launch: ")
    assert int(runs[0]["it"][0]) == 40 or int(runs[0]["flag"][0]) == 3
    assert int(runs[0]["fev"][0]) > np_ + 40 or int(runs[0]["flag"][0]) == 3    # (some iteration took more than one)


def test_a_new_point_goes_behind_equal_values(hip):
    """set_state("x") with duplicated rows: the ranking keeps their row order, and a point whose value
    equals stored ones is ranked behind them"""
    n, np_ = 2, 4
    g = _start(hip, n, np_, obj="sphere", box=1.)
    x = np.array([[0.5, 0.], [0.25, 0.], [-0.25, 0.], [0., 0.]])
    g.set_state("x", x)
    assert [int(v) for v in g.get_state("order")] == [3, 1, 2, 0] and int(g.get_state("fev")[0]) == np_
    _bits(g.get_state("f"), [0., 0.0625, 0.0625, 0.25], "f in rank order")
    _bits(g.get_state("x"), x[[3, 1, 2, 0]], "x in rank order")
    m = _model_of(g, n, np_, "sphere", 1.)
    table = [[0., 1., 0.5, 0.5]]        # (0 + 0) / 2 reflected through rank 1, (0.25, 0): (-0.25, 0)
    g.inject_draws(table)
    g.iterate()
    assert m.iterate(cm.TableSource(table, n, np_))
    _device_is_model(g, m, "tie ")
    _bits(g.get_state("cand"), [-0.25, 0.], "the trial")
    assert [int(v) for v in g.get_state("order")] == [3, 1, 2, 0]       # the new row 0 behind rows 1 and 2
    _bits(g.get_state("f"), [0., 0.0625, 0.0625, 0.0625], "f")
    # the table is spent: the next iteration waits for another one
    g.iterate()
    assert int(g.get_state("starved")[0]) == 1 and int(g.get_state("it")[0]) == 1
    from bboptpy_amd import _ffi
    with pytest.raises(_ffi.BboError):
        g.run(1)
    g.inject_draws(None)
    g.iterate()
    assert int(g.get_state("starved")[0]) == 0 and int(g.get_state("it")[0]) == 2


def test_population_0_of_a_batch_is_the_single_run(hip):
    n, np_ = 9, 12
    single = _start(hip, n, np_, seed=21)
    batch = _start(hip, n, np_, seed=21, P=3)
    single.run(30)
    batch.run(30)
    _same_state(_snapshot(single), _snapshot(batch, 0))
    assert _snapshot(batch, 1)["x"].tobytes() != _snapshot(batch, 0)["x"].tobytes()


def test_more_workgroups_than_the_device_holds_at_once(hip):
    n, np_, P = 2, 5, 4096
    g = _start(hip, n, np_, seed=3, P=P, max_depth=64)
    g.run(20)
    single = _start(hip, n, np_, seed=3, max_depth=64)
    single.run(20)
    _same_state(_snapshot(single), _snapshot(g, 0))
    for p in (1, 63, 64, 2047, 4095):
        it, flag, fev = (int(g.get_state(k, p)[0]) for k in ("it", "flag", "fev"))
        assert (it == 20 and flag == 0 and fev >= np_ + 20) or flag == 3, (p, it, flag, fev)
        f = g.get_state("f", p)
        assert (np.diff(f) >= 0.).all() and sorted(int(v) for v in g.get_state("order", p)) == list(range(np_))


def test_a_host_callable_is_the_builtin_and_is_called_fev_times(hip):
    """n = 1 sphere: x * x is exact on both sides, so the runs agree bit for bit"""
    lo, up, guess = -3. * np.ones(1), 3. * np.ones(1), np.zeros(1)
    calls = []

    def sphere(x):
        calls.append(1)
        return float(x[0] * x[0])

    runs = []
    for obj in ("sphere", sphere):
        g = hip.CRS(10 ** 6, 6, 0., seed=13, max_depth=64)
        g.initialize(obj, lo, up, guess)
        g.run(30)
        runs.append(_snapshot(g))
    _same_state(runs[0], runs[1])
    assert len(calls) == int(runs[1]["fev"][0]) > 36
    del calls[:]
    sol = hip.CRS(40, 6, 0., seed=13, max_depth=64).optimize(sphere, lo, up, guess)
    assert sol.n_evals == len(calls) >= 40 and not sol.converged


def test_the_budget_ends_the_run_at_the_first_iteration_boundary_at_or_past_mfev(hip):
    n, np_, mfev = 5, 20, 60
    g = _start(hip, n, np_, seed=9, mfev=mfev)
    fev = [np_]
    while int(g.get_state("flag")[0]) == 0:
        assert g.run(1) == 1
        fev.append(int(g.get_state("fev")[0]))
    assert int(g.get_state("flag")[0]) == 2 and fev[-2] < mfev <= fev[-1]
    assert g.run(10) == 0 and int(g.get_state("fev")[0]) == fev[-1]
    fused = _start(hip, n, np_, seed=9, mfev=mfev)
    fused.run(10 ** 6)
    _same_state(_snapshot(g), _snapshot(fused))
    sol = hip.CRS(mfev, np_, 0., seed=9).optimize("rosenbrock", -5. * np.ones(n), 5. * np.ones(n), np.zeros(n))
    assert sol.n_evals == fev[-1] and not sol.converged
    _bits(sol.x, g.get_state("x")[:n], "the best point")


def test_a_tolerance_ends_the_run_with_flag_1_and_converged(hip):
    n, np_ = 4, 10
    g = _start(hip, n, np_, obj="sphere", seed=2, tol=1e-3, box=1.)
    g.run(10 ** 6)
    f = g.get_state("f")
    assert int(g.get_state("flag")[0]) == 1 and abs(f[0] - f[-1]) < 1e-3 and int(g.get_state("conv")[0]) == 1
    assert int(g.get_state("fev")[0]) < 10 ** 6
    sol = g.solution()
    assert sol.converged and sol.n_evals == int(g.get_state("fev")[0])
    # one iteration earlier the spread was not under the tolerance
    h = _start(hip, n, np_, obj="sphere", seed=2, tol=1e-3, box=1.)
    h.run(int(g.get_state("it")[0]) - 1)
    fh = h.get_state("f")
    assert int(h.get_state("flag")[0]) == 0 and not abs(fh[0] - fh[-1]) < 1e-3 and not h.solution().converged


@pytest.mark.parametrize("P", [1, 64])
def test_the_depth_cap_ends_a_collapsed_pool_with_flag_3(hip, P):
    """lower == upper == 0: every trial and every mutation is the one point of the box, evaluated and
    rejected: M is pushed until the stack is full.  A designed stop of a bounded loop: 2 evaluations per
    frame and 2 for the trial that finds the stack full."""
    n, np_, depth = 3, 4, 8
    g = _start(hip, n, np_, obj="sphere", P=P, lower=0., box=0., max_depth=depth)
    m = _model_of(g, n, np_, "sphere", 0., lower=0., max_depth=depth)
    before = [g.get_state("x", p).copy() for p in range(P)]
    g.run(5)
    assert m.iterate(cm.RngSource(np.random.default_rng(0), n, np_)) is False
    assert m.fev == np_ + 2 * (depth + 1)
    for p in range(P):
        got = [int(g.get_state(k, p)[0]) for k in ("flag", "fev", "it", "trials", "stage", "depth", "pending", "stale")]
        assert got == [3, m.fev, 0, depth + 1, 0, 0, 0, 0], (p, got)
        _bits(g.get_state("x", p), before[p], "the pool is untouched")
        assert not g.solution(p).converged
    assert g.run(5) == 0        # sticky
    # the loop of the paper redraws instead, and ends on the budget
    r = _start(hip, n, np_, obj="sphere", P=P, lower=0., box=0., max_depth=depth, repair=True, mfev=50)
    r.run(5)
    for p in range(P):
        got = [int(r.get_state(k, p)[0]) for k in ("flag", "fev", "it", "stage", "pending", "stale")]
        assert got == [2, 50, 0, 0, 0, 0], (p, got)


def _percoord_handle(hip, n, np_, seed, lo, up, pool, repair):
    g = hip.CRS(10 ** 6, np_, 0., seed=seed, max_depth=DEPTH, repair=repair)
    g.initialize("sphere", lo, up, np.zeros(n))
    X = g.get_state("rows").reshape(np_, n)
    assert ((X >= lo) & (X <= up)).all()            # the initial draw, coordinate by coordinate
    assert ((X.max(0) - X.min(0)) > 0.25 * (up - lo)).sum() >= n // 2
    g.set_state("x", pool)
    g.set_state("record_draws", [float(RECORDS)])
    return g


@pytest.mark.parametrize("n,np_,repair,inner", [(37, 20, False, 0.84), (37, 20, True, 0.84), (257, 7, False, 0.72)])
def test_the_box_test_under_bounds_that_differ_in_every_coordinate(hip, n, np_, repair, inner):
    """tests/_boxes.py's box: CRS rejects a reflected point with a coordinate outside [lo[i], up[i]] (and draws
    again under `repair`); the kernel stages lo[i] / up[i], another pair in every coordinate.  CRS never clamps,
    so the witness is the model's count of coordinates that put a trial point out (`paths`: out_lo, out_up),
    three on each side at least.  It is established before anything is compared: a first handle only hands over
    the records of what its generator drew, and the model runs alone on them from the pool made here, with its
    own objective.  Then a second handle of the same seed walks beside a second model, as in
    test_the_walk_is_the_model_bit_for_bit.  The pool fills the inner share of every coordinate's own interval
    (see _start); n = 37 is off every tile, 257 puts one live lane into the second pass."""
    from _boxes import percoord_box
    lo, up = percoord_box(n)
    seed, its = 100 * n + np_, 12
    pool = 0.5 * (lo + up) + inner * 0.5 * (up - lo) * np.random.default_rng(seed).uniform(-1., 1., (np_, n))
    # ---- the witness: the model alone on the generator's draws
    a = _percoord_handle(hip, n, np_, seed, lo, up, pool, repair)
    w = cm.Crs(device_objective("sphere", n), n, np_, list(lo), list(up), 10 ** 6, 0., max_depth=DEPTH, repair=repair)
    w.start(pool)
    for it in range(its):
        a.iterate()
        assert w.iterate(cm.TableSource(_records(a, n), n, np_)), "the pool collapsed: choose another"
    assert w.paths["out_lo"] >= 3 and w.paths["out_up"] >= 3, w.paths
    # ---- the walk
    g = _percoord_handle(hip, n, np_, seed, lo, up, pool, repair)
    order = [int(v) for v in g.get_state("order")]
    fs = np.empty(np_)
    fs[order] = g.get_state("f")
    m = cm.Crs(device_objective("sphere", n), n, np_, list(lo), list(up), 10 ** 6, 0., max_depth=DEPTH, repair=repair)
    m.start(g.get_state("rows").reshape(np_, n), fs=fs)
    assert m.order == order, "the stable ranking"
    for k in ("fev", "it", "trials", "muts", "stale"):
        setattr(m, k, int(g.get_state(k)[0]))
    for it in range(its):
        tag = "n %d np %d iteration %d " % (n, np_, it)
        if it % 2:
            _walk(g)
        elif it % 4:
            assert g.run(1) == 1
        else:
            g.iterate()
        rec = _records(g, n)
        src = cm.TableSource(rec, n, np_)
        assert m.iterate(src) and src.exhausted(), tag
        _device_is_model(g, m, tag)
        _bits(rec, m.records, tag + "records")
        # (no containment is asserted: the reflected point is tested against the box, the mutated one that may
        # take its place is not, in the reference either -- crs.cpp:176 tests the reflection alone)
    assert m.paths["out_lo"] >= 3 and m.paths["out_up"] >= 3, m.paths


def test_repair_is_the_model_and_only_better_points_go_in(hip):
    n, np_ = 5, 8
    g = _start(hip, n, np_, seed=4, repair=True, box=2.)
    g.set_state("record_draws", [float(RECORDS)])
    m = _model_of(g, n, np_, "rosenbrock", 2., repair=True)
    for it in range(30):
        fworst = g.get_state("fworst")[0]
        if it % 2:
            _walk(g)
        else:
            g.run(1)
        assert m.iterate(cm.TableSource(_records(g, n), n, np_))
        _device_is_model(g, m, "repair %d " % it)
        assert g.get_state("fcand")[0] < fworst
    assert int(g.get_state("stale")[0]) == 0


def test_a_nan_value_counts_as_inf(hip):
    n, np_ = 2, 12
    g = hip.CRS(10 ** 6, np_, 0., seed=4)
    g.initialize(lambda v: float("nan") if v[0] > 0. else float(v @ v), -np.ones(n), np.ones(n), np.zeros(n))
    f = g.get_state("f")
    assert np.isinf(f).any() and not np.isnan(f).any() and np.isfinite(f[0]) and (np.diff(f[np.isfinite(f)]) >= 0.).all()
    assert np.isinf(g.get_state("fworst")[0]) and not g.solution().converged
    g.run(15)
    f = g.get_state("f")
    assert not np.isnan(f).any() and int(g.get_state("it")[0]) == 15
    for k in ("fcand", "fcand2"):
        assert not np.isnan(g.get_state(k)[0])


def test_configure_statuses_and_refusals(hip):
    from bboptpy_amd import _ffi
    L = _ffi.lib()
    d = _ffi.CrsParams()
    L.bbo_crs_params_default(C.byref(d))
    other = hip.NSHS(1000, 12, seed=1)
    oh = other._ensure_handle()
    assert L.bbo_crs_configure(oh, C.byref(d)) == _ffi.ERR_ARG
    assert "not a CRS handle" in L.bbo_last_error(oh).decode()
    assert L.bbo_crs_phase(oh, 0) == _ffi.ERR_ARG and L.bbo_crs_inject_draws(oh, None, 0) == _ffi.ERR_ARG
    g = hip.CRS(1000, 20, 0., seed=1)
    h = g._ensure_handle()
    assert L.bbo_crs_configure(h, C.byref(d)) == 0
    assert L.bbo_crs_configure(h, None) == _ffi.ERR_ARG
    for depth, repair, word in ((0, 0, "max_depth"), ((1 << 20) + 1, 0, "max_depth"), (8, 2, "repair")):
        bad = _ffi.CrsParams()
        bad.max_depth, bad.repair = depth, repair
        assert L.bbo_crs_configure(h, C.byref(bad)) == _ffi.ERR_ARG and word in L.bbo_last_error(h).decode()
    assert L.bbo_crs_phase(h, 0) == -2                          # BBO_ERR_STATE: before bbo_init
    n = 2
    lo, up = -np.ones(n), np.ones(n)
    # the limits, each named
    ob = _ffi.Objective()
    ob.kind, ob.builtin = _ffi.OBJ_BUILTIN, 0
    st = L.bbo_init(h, 513, -np.ones(513), np.ones(513), np.zeros(513), C.byref(ob))
    assert st == _ffi.ERR_ARG and "512" in L.bbo_last_error(h).decode()
    with pytest.raises(ValueError, match="512"):
        hip.CRS(1000, 5, 0.).initialize("sphere", -np.ones(513), np.ones(513), np.zeros(513))
    for np_ in (1, 65537):
        p = _ffi.default_params(_ffi.ALGO_CRS)
        p.mfev, p.np = 1000, np_
        out = C.c_void_p()
        assert L.bbo_create(C.byref(p), C.byref(out)) == _ffi.ERR_ARG and "65536" in L.bbo_last_error(None).decode()
    st = L.bbo_init(h, n, lo, np.array([1., np.inf]), np.zeros(n), C.byref(ob))
    assert st == _ffi.ERR_ARG and "finite" in L.bbo_last_error(h).decode()
    # an objective program: refused by the class and by the library, naming who takes one
    prog = hip.DeviceObjective('extern "C" __device__ double bbo_user_objective(const double *x, int n, '
                               'const double *data) { return x[0] * x[0]; }')
    with pytest.raises(ValueError) as ei:
        g.initialize(prog, lo, up, np.zeros(n))
    assert "CRS does not take a DeviceObjective" in str(ei.value) and "JADE" in str(ei.value)
    ob = _ffi.Objective()
    ob.kind, ob.user = _ffi.OBJ_PROGRAM, prog._handle
    st = L.bbo_init(h, n, lo, up, np.zeros(n), C.byref(ob))
    msg = L.bbo_last_error(h).decode()
    assert st == -1 and "CRS" in msg and "CMAES" in msg and "SHADE" in msg, (st, msg)
    g.initialize("sphere", lo, up, np.zeros(n))
    assert L.bbo_crs_configure(h, C.byref(d)) == -2             # BBO_ERR_STATE
    assert "after bbo_init" in L.bbo_last_error(h).decode()
    assert L.bbo_crs_phase(h, 3) == _ffi.ERR_ARG and L.bbo_crs_phase(h, -1) == _ffi.ERR_ARG
    with pytest.raises(_ffi.BboError):                          # whole records of 2 n per population
        g.inject_draws(np.zeros(3))
    with pytest.raises(_ffi.BboError):                          # uniforms in [0, 1)
        g.inject_draws([[0., 1., 1., 0.5]])
    with pytest.raises(_ffi.BboError):                          # indices below np
        g.inject_draws([[0., 20., 0.5, 0.5]])
    for key, val in (("max_depth", 0.), ("max_depth", 4097.), ("launch_evals", -1.), ("record_draws", 0.5),
                     ("x", np.zeros(3)), ("f", np.zeros(3)), ("fev", -1.), ("order", 0.)):
        with pytest.raises(_ffi.BboError):
            g.set_state(key, val)
    with pytest.raises(_ffi.BboError) as ei:
        g.get_state("draws")
    assert ei.value.status == -2
    with pytest.raises(_ffi.BboError) as ei:
        g.get_state("sigma")
    assert ei.value.status == -6
    assert g.get_state("max_depth")[0] == 4096 and g.get_state("repair")[0] == 0 and g.get_state("chunk")[0] == CHUNK
    assert g.get_state("wg")[0] == 64
    g.set_state("max_depth", [100.])
    assert g.get_state("max_depth")[0] == 100
    # one profile slot per kernel: init, rank, steps, eval (ms, calls each)
    g.set_state("profile", [1.])
    g.iterate()
    g.run(3)
    prof = g.get_state("profile")
    assert prof.size == 8 and prof[1] == 0. and prof[3] == 0. and prof[5] >= 2. and prof[7] == 0. and prof[4] > 0.
    # CRS is no base of a restart driver
    p = _ffi.default_params(_ffi.ALGO_IPOP)
    p.mfev, p.np = 1000, 8
    out = C.c_void_p()
    fn = C.CDLL(_ffi.LIB_PATH).bbo_create_restart
    fn.argtypes, fn.restype = [C.c_void_p, C.c_void_p, C.c_void_p], C.c_int
    assert fn(C.byref(p), h, C.byref(out)) == _ffi.ERR_ARG and not out.value
    assert "CMA-ES handle" in L.bbo_last_error(None).decode()
    big = hip.CRS(10 ** 6, 65536, 0., seed=3)                   # the largest pool
    big.initialize("sphere", -np.ones(4), np.ones(4), np.zeros(4))
    f = big.get_state("f")
    assert (np.diff(f) >= 0.).all() and big.run(3) == 3 and int(big.get_state("it")[0]) == 3
    assert (np.diff(big.get_state("f")) >= 0.).all()


@pytest.mark.parametrize("obj", ["sphere", "rosenbrock"])
def test_outcome_bands_match_the_reference(hip, obj):
    """64 populations at the recorded budget: the median of log10 f(best) inside the reference's
    inter-quartile band (the comparison of the NSHS and SLPSO tests), and the mean share of stale
    replacements within the min .. max of the reference's 256 runs"""
    b, P = GOLD["bands"], 64
    n = b["n"]
    g = hip.CRS(b["mfev"], b["np"], b["tol"], seed=2024, populations=P)
    g.initialize(obj, -b["box"] * np.ones(n), b["box"] * np.ones(n), np.zeros(P * n))
    g.run(10 ** 6)
    got = [float(g.get_state("fbest", p)[0]) for p in range(P)]
    assert all(int(g.get_state("flag", p)[0]) == 2 and int(g.get_state("fev", p)[0]) >= b["mfev"] for p in range(P))
    band(got, _h(b[obj]), obj + " device")
    share = np.mean([g.get_state("stale", p)[0] / g.get_state("it", p)[0] for p in range(P)])
    lo, hi, mean = _h(b[obj + "_stale_share"])
    print("%s: mean stale share %.4f, reference %.4f .. %.4f (mean %.4f)" % (obj, share, lo, hi, mean))
    assert lo <= share <= hi
