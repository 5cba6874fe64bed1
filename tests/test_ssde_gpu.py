"""GPU: the SSDE engine on its own generator against tests/ssde_model.py.

The device records the outcomes of its draws ("record_draws"); the model is fed that table and sums its
objective in the device's order (ssde_model.device_objective), so every key is bit-exact: the pool and its
values in rank order, the three memories, every counter.  Further: the fused kernel against the phase path,
seeds and sub-streams, a Python callable against the built-in, the stop rules, the invariants, the outcome
bands of the reference, and what bbo_init refuses."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import ssde_model as sm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = sm.FLOAT_KEYS + sm.INT_KEYS
# n, npinit, objective, mfev, options: the shapes of the fixture, and n = 130 (256 threads, three wavefronts at work)
SHAPES = [
    (1, 4, "sphere", 400, {}),
    (2, 5, "rosenbrock", 500, {}),
    (3, 6, "sphere", 240, {}),
    (5, 20, "rosenbrock", 190, {"usede": True, "h": 3}),
    (17, 20, "ellipsoid", 400, {"usede": True, "repaircr": False}),
    (66, 8, "rosenbrock", 640, {}),
    (130, 6, "rosenbrock", 120, {}),
    (130, 6, "ellipsoid", 120, {"usede": True}),
    # rows past one pass of the 256-thread workgroup: one live lane in the second pass (257), an odd n
    # that is no multiple of 4 or 64 (301) and the cap (512), with and without the DE step
    (257, 6, "rosenbrock", 120, {}),
    (301, 6, "ellipsoid", 120, {"usede": True}),
    (512, 6, "rosenbrock", 120, {}),
    (512, 6, "ellipsoid", 120, {"usede": True}),
]
BAND_RUNS, BAND_MAY_MISS = 32, 2     # tests/test_ssde_model.py holds the reference's own other seeds to this


def ident(shape):
    n, npinit, obj, _, opts = shape
    return "n%d_np%d_%s%s" % (n, npinit, obj, "_de" if opts.get("usede") else "")


def box(n):
    return -3. * np.ones(n), 5. * np.ones(n)


def make(hip, shape, f=None, bounds=None, **ext):
    """`bounds`: (lower, upper) in place of box(n)"""
    n, npinit, obj, mfev, opts = shape
    ext.setdefault("seed", 77)
    g = hip.SSDE(mfev, npinit, 1e-12, **opts, **ext)
    lo, up = bounds or box(n)
    g.initialize(obj if f is None else f, lo, up, np.zeros(n * ext.get("populations", 1)))
    return g


def model_from(g, shape, population=0, bounds=None):
    """the model started from the device's pool and values"""
    n, npinit, obj, mfev, opts = shape
    lo, up = bounds or box(n)
    m = sm.Ssde(sm.device_objective(obj, n), lo, up, mfev, npinit, 1e-12, min_np=4, **opts)
    x = g.get_state("x", population).reshape(-1, n)
    m.start(x, g.get_state("f", population), fev=int(g.get_state("fev", population)[0]))
    return m


def same(g, m, tag, population=0):
    want = m.state()
    for k in sm.FLOAT_KEYS:
        a, b = g.get_state(k, population), np.asarray(want[k], float)
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (tag, k, np.flatnonzero(a != b)[:6])
    for k in sm.INT_KEYS:
        assert int(g.get_state(k, population)[0]) == want[k], (tag, k)
    assert [int(v) for v in g.get_state("perm", population)] == want["perm"], tag


def snapshot(g, population=0):
    return {k: g.get_state(k, population).copy() for k in KEYS + ("perm", "order")}


def same_snapshots(a, b, tag):
    for k in a:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (tag, k)


def phase_generation(g):
    evals = 0
    while g.phase(0):
        g.phase(1)
        g.phase(2)
        evals += 1
    return evals


@pytest.mark.parametrize("shape", SHAPES, ids=[ident(s) for s in SHAPES])
def test_device_draws_against_the_model(hip, shape):
    n, npinit, obj, mfev, opts = shape
    g = make(hip, shape, record_draws=True)
    f = sm.device_objective(obj, n)
    x0, f0 = g.get_state("x").reshape(-1, n), g.get_state("f")
    lo, up = box(n)
    assert len(f0) == npinit and (np.diff(f0) >= 0).all() and (x0 >= lo).all() and (x0 <= up).all()
    assert int(g.get_state("fev")[0]) == (2 if opts.get("usede") else 1) * npinit
    assert [f(r) for r in x0] == list(f0)
    m = model_from(g, shape)
    same(g, m, "init")
    for it in range(1, 6):
        g.iterate()
        table = g.get_state("draws")
        perm = table[:n]
        assert sorted(int(v) for v in perm) == list(range(n))
        m.iterate(sm.TableSource(table, n, npinit))
        same(g, m, "generation %d" % it)
        assert int(g.get_state("np")[0]) >= 4
    assert int(g.get_state("gen")[0]) == 5
    if opts.get("usede"):
        assert {"de_success", "de_failure"} & m.events


# (n, npinit, seed): the seed is one under which the model's own run meets the witness below
PERCOORD = [(37, 12, 77), (257, 12, 77)]


@pytest.mark.parametrize("n,npinit,seed", PERCOORD, ids=["n%d" % c[0] for c in PERCOORD])
def test_the_redraw_under_bounds_that_differ_in_every_coordinate(hip, n, npinit, seed):
    """tests/_boxes.py's box with the DE step: the start holds every point beside its opposite
    lower + upper - x, and a coordinate of a DE trial outside [lo[d], up[d]] is drawn again inside it -- another
    pair of bounds in every coordinate (the kernels stage them as lo[i] / up[i]).  SSDE never sits on a bound,
    so the witness is the model's count of coordinates redrawn past each bound (`repairs`), three at least.  It
    is established before anything is compared: a first handle only hands over its starting pool and the tables
    of what its generator drew, and the model runs alone on them with its own objective.  Then a second handle
    of the same seed walks as in test_device_draws_against_the_model, twice as long.  n = 37 is off every tile,
    257 puts one live lane into the second pass."""
    from _boxes import percoord_box
    bounds = percoord_box(n)
    lo, up = bounds
    shape, gens = (n, npinit, "sphere", 100 * npinit, {"usede": True}), 10
    # ---- the witness: the model alone on the generator's draws
    a = make(hip, shape, bounds=bounds, seed=seed, record_draws=True)
    x0 = a.get_state("x").reshape(-1, n)
    assert (x0 >= lo).all() and (x0 <= up).all()
    w = model_from(a, shape, bounds=bounds)
    for _ in range(gens):
        a.iterate()
        w.iterate(sm.TableSource(a.get_state("draws"), n, npinit))
    assert min(w.repairs.values()) >= 3, w.repairs
    # ---- the walk
    g = make(hip, shape, bounds=bounds, seed=seed, record_draws=True)
    m = model_from(g, shape, bounds=bounds)
    same(g, m, "init")
    for it in range(1, gens + 1):
        g.iterate()
        m.iterate(sm.TableSource(g.get_state("draws"), n, npinit))
        same(g, m, "generation %d" % it)
        x = g.get_state("x").reshape(-1, n)
        assert (x >= lo).all() and (x <= up).all()
    assert m.repairs == w.repairs


def test_the_fused_kernel_and_the_phase_path_agree(hip):
    for shape in (SHAPES[3], SHAPES[7], SHAPES[5]):
        a = make(hip, shape, populations=3)
        b = make(hip, shape, populations=3)
        for it in range(3):
            a.iterate()
            evals = phase_generation(b)
            assert evals > 0 and int(b.get_state("pending")[0]) == 0
            for p in range(3):
                same_snapshots(snapshot(a, p), snapshot(b, p), "%s generation %d population %d" % (ident(shape), it, p))
        # the populations are different runs
        assert a.get_state("x", 0).tobytes() != a.get_state("x", 1).tobytes()


def test_seeds_and_substreams(hip):
    shape = SHAPES[3]
    a, b, c = make(hip, shape, seed=5), make(hip, shape, seed=5), make(hip, shape, seed=6)
    for g in (a, b, c):
        g.iterate()
        g.iterate()
    same_snapshots(snapshot(a), snapshot(b), "same seed")
    assert snapshot(a)["x"].tobytes() != snapshot(c)["x"].tobytes()
    batch = make(hip, shape, seed=5, populations=3)
    batch.iterate()
    batch.iterate()
    same_snapshots(snapshot(a), snapshot(batch, 0), "population 0")
    for p in (1, 2):
        single = make(hip, shape, seed=5)
        single.set_state("substream", [p])
        single.iterate()
        single.iterate()
        same_snapshots(snapshot(single), snapshot(batch, p), "population %d" % p)


@pytest.mark.parametrize("shape", [SHAPES[3], SHAPES[6]], ids=[ident(SHAPES[3]), ident(SHAPES[6])])
def test_python_callable_gives_the_states_of_the_builtin(hip, shape):
    n, npinit, obj, mfev, opts = shape
    f = sm.device_objective(obj, n)
    calls = []

    def counted(x):
        calls.append(np.array(x))
        return f(x)

    a = make(hip, shape)
    b = make(hip, shape, f=counted, record_draws=True)
    same_snapshots(snapshot(a), snapshot(b), "init")
    # the pool was evaluated in the reference's order: the npinit points, then their opposites
    lo, up = box(n)
    if opts.get("usede"):
        assert len(calls) == 2 * npinit
        for k in range(npinit):
            assert (calls[npinit + k] == lo + up - calls[k]).all()
    m = model_from(b, shape)
    m.trace = True
    for it in range(3):
        before = len(calls)
        a.iterate()
        b.iterate()
        same_snapshots(snapshot(a), snapshot(b), "generation %d" % it)
        m.points = []
        m.iterate(sm.TableSource(b.get_state("draws"), n, npinit))
        assert len(calls) - before == len(m.points)
        for got, (want, _) in zip(calls[before:], m.points):
            assert got.tobytes() == np.asarray(want, float).tobytes()
    assert len(calls) == int(b.get_state("fev")[0])


def test_budget_stop_with_the_overshoot_the_model_predicts(hip):
    shape = (5, 20, "rosenbrock", 150, {"usede": True})
    n, npinit = shape[0], shape[1]
    a = make(hip, shape, record_draws=True)
    m = model_from(a, shape)
    gens = 0
    while m.fev < m.mfev:
        a.iterate()
        m.iterate(sm.TableSource(a.get_state("draws"), n, npinit))
        gens += 1
        assert not m.converged()
    assert m.fev >= 150                    # (the budget is tested between generations)
    b = make(hip, shape)
    b.run(10 ** 6)
    assert int(b.get_state("gen")[0]) == gens
    assert int(b.get_state("fev")[0]) == m.fev and int(b.get_state("stop")[0]) == 2
    assert b.run(10) == 0
    sol = make(hip, shape).optimize(shape[2], *box(n), np.zeros(n))
    assert sol.n_evals == m.fev and not sol.converged
    assert sol.x.tobytes() == np.asarray(m.x[0]).tobytes()


def test_a_tiny_box_meets_the_tolerance(hip):
    n = 6
    g = hip.SSDE(10000, 10, 1e-3, seed=3)
    g.initialize("sphere", np.ones(n), (1. + 1e-9) * np.ones(n), np.zeros(n))
    g.run(100)
    assert int(g.get_state("gen")[0]) == 1
    assert int(g.get_state("stop")[0]) == 1 and g.solution().converged
    sol = hip.SSDE(10000, 10, 1e-3, seed=3).optimize("sphere", np.ones(n), (1. + 1e-9) * np.ones(n), np.zeros(n))
    assert sol.converged and sol.n_evals == 20


def test_patience_stops_a_run_that_no_longer_improves(hip):
    n, npinit = 4, 8
    lo, up = box(n)
    m = sm.Ssde(lambda x: 0., lo, up, 10 ** 6, npinit, 0., patience=2, min_np=4)
    w = sm.Mt19937Words(1)
    m.init_reference(w)
    gens = 0
    while not m.converged():
        m.iterate(sm.WordsSource(w, n, npinit))
        gens += 1
    assert gens == 3 and m.convcount == 3
    g = hip.SSDE(10 ** 6, npinit, 0., patience=2, seed=4)
    g.initialize(lambda x: 0., lo, up, np.zeros(n))
    g.run(100)
    assert int(g.get_state("gen")[0]) == gens
    assert int(g.get_state("stop")[0]) == 1 and int(g.get_state("convcount")[0]) == 3
    # (the linear shrink truncates: np is npinit - 1 from the first generation on)
    assert g.solution().converged and g.solution().n_evals == m.fev == 30


def test_np_never_falls_under_four_and_points_stay_inside_the_box(hip):
    shape = (7, 12, "rosenbrock", 60, {"usede": True})
    n = shape[0]
    lo, up = box(n)
    g = make(hip, shape, populations=2)
    sizes = []
    for _ in range(8):              # iterate() ignores the budget: fev runs to several times mfev
        g.iterate()
        for p in range(2):
            x = g.get_state("x", p).reshape(-1, n)
            sizes.append(len(x))
            assert len(x) == int(g.get_state("np", p)[0]) >= 4
            assert (x >= lo).all() and (x <= up).all() and np.isfinite(g.get_state("f", p)).all()
    assert int(g.get_state("fev")[0]) > 60 and sizes[-1] == 4


@pytest.mark.parametrize("objective", ["sphere", "rosenbrock"])
@pytest.mark.parametrize("usede", [False, True])
def test_outcome_bands(hip, objective, usede):
    """32 device runs at the "bands" configuration against the reference's recorded min .. max of 256 runs:
    at most BAND_MAY_MISS may fall outside"""
    with open(os.path.join(ROOT, "tests", "golden", "ssde_runs.json")) as fh:
        bands = json.load(fh)["bands"]
    band = [float.fromhex(v) for v in bands["%s_usede%d" % (objective, int(usede))]]
    n = bands["n"]
    g = hip.SSDE(bands["mfev"], bands["npinit"], bands["tol"], usede=usede, seed=2024, populations=BAND_RUNS)
    g.initialize(objective, bands["box"][0] * np.ones(n), bands["box"][1] * np.ones(n), np.zeros(n * BAND_RUNS))
    g.run(10 ** 6)
    vals = [float(g.get_state("f", p)[0]) for p in range(BAND_RUNS)]
    assert all(int(g.get_state("stop", p)[0]) == 2 for p in range(BAND_RUNS))
    outside = sum(1 for v in vals if not band[0] <= v <= band[-1])
    print("%s usede=%d: device %.3e .. %.3e, reference %.3e .. %.3e, %d outside"
          % (objective, usede, min(vals), max(vals), band[0], band[-1], outside))
    assert outside <= BAND_MAY_MISS


def test_bbo_init_refuses_what_the_header_says(hip):
    from bboptpy_amd import _ffi
    L = _ffi.lib()
    n = 3
    lo, up, x0 = -np.ones(n), np.ones(n), np.zeros(n)
    ob = _ffi.Objective()
    ob.kind, ob.builtin = _ffi.OBJ_BUILTIN, 0

    def refused(alg, n_=n, lo_=lo, up_=up, obj=ob):
        h = alg._create()
        st = L.bbo_init(h, n_, lo_, up_, np.zeros(n_), C.byref(obj))
        msg = L.bbo_last_error(h).decode()
        L.bbo_destroy(h)
        return st, msg

    ok = dict(mfev=100, npinit=6, tol=1e-6)
    for kw, word in ((dict(ok, npinit=3), "npinit"), (dict(ok, npinit=4097), "npinit"), (dict(ok, npmin=3), "npmin"),
                     (dict(ok, npmin=7), "npmin"), (dict(ok, h=0), "h must"), (dict(ok, ptop=0.), "ptop"),
                     (dict(ok, ptop=1.), "ptop"), (dict(ok, patience=-1), "patience")):
        st, msg = refused(hip.SSDE(**kw))
        assert st == _ffi.ERR_ARG and word in msg, (kw, st, msg)
    st, msg = refused(hip.SSDE(**ok), up_=np.array([1., np.inf, 1.]))
    assert st == _ffi.ERR_ARG and "finite" in msg
    st, msg = refused(hip.SSDE(**ok), n_=513, lo_=-np.ones(513), up_=np.ones(513))
    assert st == _ffi.ERR_ARG and "[1, 512]" in msg
    prog = hip.DeviceObjective('extern "C" __device__ double bbo_user_objective(const double *x, int n, '
                               'const double *data) { return x[0] * x[0]; }')
    with pytest.raises(ValueError) as ei:
        hip.SSDE(**ok).initialize(prog, lo, up, x0)
    assert "SSDE does not take a DeviceObjective" in str(ei.value) and "JADE" in str(ei.value)
    pob = _ffi.Objective()
    pob.kind, pob.user = _ffi.OBJ_PROGRAM, prog._handle
    st, msg = refused(hip.SSDE(**ok), obj=pob)
    assert st == _ffi.ERR_ARG and "SSDE" in msg and "CMAES" in msg and "SHADE" in msg, (st, msg)
    # the handle's own calls: configure after init, a table of the wrong size, keys
    g = hip.SSDE(**ok)
    g.initialize("sphere", lo, up, x0)
    assert L.bbo_ssde_configure(g._handle, C.byref(g._ssde)) == -2      # BBO_ERR_STATE
    with pytest.raises(_ffi.BboError):
        g.inject_draws(np.zeros(5))
    with pytest.raises(_ffi.BboError):
        g.set_state("x", np.zeros(3 * n))       # fewer than four rows
    with pytest.raises(_ffi.BboError):
        g.get_state("draws")                    # needs record_draws
    other = hip.CRS(100, 6, 1e-6)
    other.initialize("sphere", lo, up, x0)
    assert L.bbo_ssde_phase(other._handle, 0) == _ffi.ERR_ARG
