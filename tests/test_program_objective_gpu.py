"""Objective programs (bbo_program_create, bboptpy_amd.DeviceObjective) on the device.

The yardstick is the host scalar-callback path that existed before: a program and a pure-Python
function that compute the same expression in the same order with + - * only must give runs that
agree BIT FOR BIT under one seed (the library compiles programs without contraction, and both
paths use the same OBJ_HOST kernels around the evaluation).  Shapes are the smallest at which the
evaluation kernels can go wrong: n and row counts that are no multiples of 16 / 64, more than one
wavefront of rows, both forms (prog_stage 0 / 1), and the automatic boundary between them.
No program here reads out of bounds or loops without end."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROSEN_SRC = r"""
extern "C" __device__ double bbo_user_objective(const double *x, int n, const double *data)
{
    double s = 0.;
    for (int j = 0; j + 1 < n; j++) {
        const double t = x[j + 1] - x[j] * x[j], u = 1. - x[j];
        s += 100. * (t * t) + u * u;
    }
    return s;
}
"""

WSPHERE_SRC = r"""
extern "C" __device__ double bbo_user_objective(const double *x, int n, const double *data)
{
    double s = 0.;
    for (int j = 0; j < n; j++) s += data[j] * (x[j] * x[j]);
    return s;
}
"""

NAN_SRC = r"""
extern "C" __device__ double bbo_user_objective(const double *x, int n, const double *data)
{
    double s = 0.;
    for (int j = 0; j < n; j++) s += x[j] * x[j];
    return x[0] > 0. ? __builtin_nan("") : s;
}
"""

WEIGHTS = 1. + np.arange(64) / 64.          # exactly representable, in [1, 2)


def rosen_py(x):
    s = 0.
    for j in range(len(x) - 1):
        xj = float(x[j])
        t = float(x[j + 1]) - xj * xj
        u = 1. - xj
        s += 100. * (t * t) + u * u
    return s


def wsphere_py(x):
    s = 0.
    for j in range(len(x)):
        xj = float(x[j])
        s += float(WEIGHTS[j]) * (xj * xj)
    return s


def nan_py(x):
    s = 0.
    for j in range(len(x)):
        xj = float(x[j])
        s += xj * xj
    return float("nan") if x[0] > 0. else s


@pytest.fixture(scope="module")
def programs(hip):
    """each test program compiled once (for the device's own architecture: arch=None)"""
    return {"rosen": (hip.DeviceObjective(ROSEN_SRC), rosen_py),
            "wsphere": (hip.DeviceObjective(WSPHERE_SRC, data=WEIGHTS), wsphere_py),
            "nan": (hip.DeviceObjective(NAN_SRC), nan_py)}


# ---- the engines and the smallest shapes ---------------------------------------------------------
CMA_KEYS = ("arx", "fitness", "xmean", "sigma", "fev", "it", "flag")
DE_KEYS = ("x", "f", "fev", "np", "gen", "stop")
SHAPES = {
    "CMAES": (5, lambda hip, **k: hip.CMAES(100000, 1e-30, 8, **k), CMA_KEYS),
    "ActiveCMAES": (17, lambda hip, **k: hip.ActiveCMAES(100000, 1e-30, 70, **k), CMA_KEYS),
    "SepCMAES": (33, lambda hip, **k: hip.SepCMAES(100000, 1e-30, 12, **k), CMA_KEYS),
    "CholeskyCMAES": (20, lambda hip, **k: hip.CholeskyCMAES(100000, 1e-30, 1e-30, 10, **k), CMA_KEYS),
    "JADE": (7, lambda hip, **k: hip.JADE(100000, 20, 1e-30, **k), DE_KEYS),
    "SANSDE": (7, lambda hip, **k: hip.SANSDE(100000, 20, 1e-30, **k), DE_KEYS),
    # mfev = 400: np shrinks from the first generation on (shade.cpp:218-225)
    "SHADE": (7, lambda hip, **k: hip.SHADE(400, 40, 1e-30, npmin=4, **k), DE_KEYS),
}
GENS = 5


def _box(n):
    return -5. * np.ones(n), 5. * np.ones(n)


def _guess(n, pops=1):
    return np.random.default_rng(100 + n).uniform(-3., 3., n * pops)


def _state(g, keys, pops=1):
    return {(k, p): g.get_state(k, p).copy() for p in range(pops) for k in keys}


def _assert_same(got, want, skip=()):
    for key in want:
        if key in skip:
            continue
        a, b = got[key], want[key]
        assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)), \
            "%s of population %d differs from the host-callback run" % key


_callback_runs = {}


def _callback_run(hip, name, obj, fpy):
    """the yardstick run of (class, objective): computed once, shared by both forms"""
    if (name, obj) not in _callback_runs:
        n, make, keys = SHAPES[name]
        g = make(hip, seed=4242)
        g.initialize(fpy, *_box(n), _guess(n))
        for _ in range(GENS):
            g.iterate()
        _callback_runs[(name, obj)] = _state(g, keys)
    return _callback_runs[(name, obj)]


@pytest.mark.parametrize("stage", [0, 1], ids=["direct", "staged"])
@pytest.mark.parametrize("obj", ["rosen", "wsphere"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_program_run_equals_callback_run(hip, programs, name, obj, stage):
    prog, fpy = programs[obj]
    n, make, keys = SHAPES[name]
    want = _callback_run(hip, name, obj, fpy)
    g = make(hip, seed=4242)
    g.initialize(prog, *_box(n), _guess(n))
    g.set_state("prog_stage", [stage])
    if name in ("JADE", "SANSDE", "SHADE"):
        # (the initial population was evaluated by the automatic form; again by the forced one)
        g.initialize(prog, *_box(n), _guess(n))
        assert g.get_state("prog_stage")[0] == stage
    assert g.get_state("prog_staged")[0] == stage
    for _ in range(GENS):
        g.iterate()
    _assert_same(_state(g, keys), want)
    if name == "SHADE":
        assert g.get_state("np")[0] < 40, "the test is meant to cross a shrinking population"


def test_automatic_boundary(hip, programs):
    """n at the default staged / direct boundary and on either side: the form taken is the
    documented one, and each computes the callback's run"""
    prog, fpy = programs["rosen"]
    probe = hip.SepCMAES(1000, 1e-30, 12, seed=1)
    probe.initialize(prog, *_box(4), np.zeros(4))
    nb = int(probe.get_state("prog_stage_max_n")[0])
    assert 16 <= nb <= 319       # (64 staged rows of n > 319 do not fit a compute unit's LDS)
    for n in (nb - 1, nb, nb + 1):
        runs = []
        for f in (fpy, prog):
            g = hip.SepCMAES(100000, 1e-30, 12, seed=77)
            g.initialize(f, *_box(n), _guess(n))
            if f is prog:
                assert g.get_state("prog_stage")[0] == -1
                assert g.get_state("prog_staged")[0] == (1 if n <= nb else 0)
            for _ in range(3):
                g.iterate()
            runs.append(_state(g, CMA_KEYS))
        _assert_same(runs[1], runs[0])


def test_stopped_population_freezes_and_the_others_go_on(hip, programs):
    """populations=3, population 0 starts at the optimum with a small step: its history range falls
    under tol (flag 2) after hlen = 29 generations while the others are still descending"""
    prog, fpy = programs["wsphere"]
    n = 5
    guess = np.concatenate([np.zeros(n), _guess(n, 2)])
    runs = []
    for f in (fpy, prog):
        g = hip.CMAES(100000, 1e-2, 8, sigma0=0.01, seed=99, populations=3, poll_every=4)
        g.initialize(f, *_box(n), guess)
        assert g.run(40) == 40
        mid = _state(g, CMA_KEYS, 3)
        assert g.run(8) == 8
        runs.append((mid, _state(g, CMA_KEYS, 3)))
    (cb_mid, cb_end), (pr_mid, pr_end) = runs
    assert pr_mid[("flag", 0)][0] != 0 and pr_mid[("it", 0)][0] < 40
    assert pr_end[("flag", 1)][0] == 0 and pr_end[("flag", 2)][0] == 0
    assert pr_end[("it", 1)][0] == 48 and pr_end[("it", 2)][0] == 48
    # frozen: nothing of population 0 moved in the eight further generations, its fitness included
    for k in CMA_KEYS:
        assert np.array_equal(pr_mid[(k, 0)], pr_end[(k, 0)]), k
    # (the callback path overwrites a frozen population's fitness with +inf: not compared)
    _assert_same(pr_end, cb_end, skip={("fitness", 0)})
    _assert_same(pr_mid, cb_mid, skip={("fitness", 0)})


def test_run_with_polling_equals_iterate(hip, programs):
    prog, _ = programs["rosen"]
    n = 5
    a = hip.CMAES(100000, 1e-30, 8, seed=5, poll_every=8)
    a.initialize(prog, *_box(n), _guess(n))
    assert a.run(64) == 64
    b = hip.CMAES(100000, 1e-30, 8, seed=5)
    b.initialize(prog, *_box(n), _guess(n))
    for _ in range(64):
        b.iterate()
    assert a.get_state("it")[0] == 64
    _assert_same(_state(a, CMA_KEYS), _state(b, CMA_KEYS))


@pytest.mark.parametrize("name", ["CMAES", "JADE"])
def test_nan_ranks_last_like_the_callback(hip, programs, name):
    prog, fpy = programs["nan"]
    n, make, keys = SHAPES[name]
    runs = []
    for f in (fpy, prog):
        g = make(hip, seed=31)
        g.initialize(f, *_box(n), _guess(n))
        for _ in range(GENS):
            g.iterate()
        runs.append(_state(g, keys))
    _assert_same(runs[1], runs[0])
    fkey = "fitness" if name == "CMAES" else "f"
    assert not np.isnan(runs[1][(fkey, 0)]).any()


def test_ipop_over_a_program_base(hip, programs):
    prog, fpy = programs["rosen"]
    n = 4
    sols = []
    for f in (fpy, prog):
        base = hip.CMAES(600, 1e-8, 6, seed=8)
        drv = hip.IPopCMAES(base, 2500, seed=9)
        sols.append(drv.optimize(f, *_box(n), _guess(n)))
    assert np.array_equal(sols[0].x.view(np.uint64), sols[1].x.view(np.uint64))
    assert sols[0].n_evals == sols[1].n_evals and sols[0].converged == sols[1].converged


def test_evaluate_returns_the_programs_value(hip, programs):
    for obj, n in (("rosen", 5), ("wsphere", 17)):
        prog, fpy = programs[obj]
        g = hip.ActiveCMAES(1000, 1e-8, 8, seed=3)
        g.initialize(prog, *_box(n), _guess(n))
        x = np.random.default_rng(12).uniform(-2., 2., n)
        assert g.evaluate(x) == fpy(x)


def test_other_families_refuse_a_program(hip, programs):
    from bboptpy_amd import _ffi
    prog, _ = programs["rosen"]
    n = 4
    lo, up = _box(n)
    for alg in (hip.APSO(100, 1e-4, 8, seed=1), hip.CSO(100, 1e-4, 9, seed=1),
                hip.CCPSO(100, 1e-4, 8, [2, 4], seed=1)):
        with pytest.raises(ValueError) as ei:
            alg.initialize(prog, lo, up, np.zeros(n))
        assert "CMAES" in str(ei.value) and "JADE" in str(ei.value)
        # and the library itself, for a C caller
        h = alg._ensure_handle()
        ob = _ffi.Objective()
        ob.kind, ob.user = _ffi.OBJ_PROGRAM, prog._handle
        st = _ffi.lib().bbo_init(h, n, lo, up, np.zeros(n), C.byref(ob))
        msg = _ffi.lib().bbo_last_error(h).decode()
        assert st == -1 and "CMAES" in msg and "SHADE" in msg, (st, msg)


def test_one_program_serves_several_handles(hip, programs):
    prog, fpy = programs["wsphere"]
    n = 7

    def run(g, f):
        g.initialize(f, *_box(n), _guess(n))
        for _ in range(3):
            g.iterate()
        return _state(g, CMA_KEYS)

    a, b = hip.CMAES(10000, 1e-30, 8, seed=21), hip.SepCMAES(10000, 1e-30, 8, seed=22)
    first = run(a, prog)
    second = run(b, prog)
    _assert_same(first, run(hip.CMAES(10000, 1e-30, 8, seed=21), fpy))
    _assert_same(second, run(hip.SepCMAES(10000, 1e-30, 8, seed=22), fpy))
    a.reseed(23)                          # the handle is re-created; the program is the same object
    third = run(a, prog)
    _assert_same(third, run(hip.CMAES(10000, 1e-30, 8, seed=23), fpy))
    _assert_same(run(b, prog), second)    # and the first user of it still works
