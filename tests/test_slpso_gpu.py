"""GPU: the SLPSO engine under its own generator, against tests/slpso_model.py (pinned to the reference
by tests/test_slpso_model.py), against itself along its three routes, and in its outcomes against the
reference's recorded complete runs (tests/golden/slpso_runs.json, "runs")."""
import math

import numpy as np
import pytest

import slpso_model as sm
from test_slpso_golden_gpu import bits, close, compare, phase_generation
from test_slpso_model import GOLD

pytestmark = pytest.mark.gpu

ALL_KEYS = ("x", "v", "pb", "fx", "fpb", "fp", "s", "p", "g", "G", "m", "CF", "PF", "Uf", "Pl", "perm", "abest",
            "fabest", "vdavg", "alpha", "omega", "mfes", "fev", "it", "flag", "conv")


def same_states(a, b, tag, pa=0, pb=0, keys=ALL_KEYS):
    for k in keys:
        bits(a.get_state(k, pa), b.get_state(k, pb), tag + k)


def box(n, w=3.):
    return -w * np.ones(n), w * np.ones(n)


def model_beside(g, obj, n, np_, mfev, stol, w, population=0, **kw):
    """the model started from the device's initial swarm and permutation, its objective summed in the
    device's order (slpso_model.device_objective): the values, and with them p and the selection ratios
    a refresh forms from p / sum(p), are then the device's bit for bit and not only to 1e-10"""
    m = sm.Slpso(sm.device_objective(obj, n), [-w] * n, [w] * n, np_, mfev, stol, **kw)
    m.trace = True
    return m.start(g.get_state("x", population).reshape(np_, n), [int(v) for v in g.get_state("perm", population)])


# (a) ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,np_,obj,ufmax", [(2, 2, "rosenbrock", 10.), (5, 3, "rosenbrock", 10.),
                                             (33, 6, "rosenbrock", 10.), (65, 4, "rosenbrock", 10.),
                                             (130, 5, "rosenbrock", 10.), (12, 8, "ellipsoid", 1.),
                                             # rows past one pass of the 256-thread workgroup: one live lane in
                                             # the second pass, an odd n off every tile, and the cap (rosenbrock
                                             # throughout: on the ellipsoid past n = 256 a step of Algorithm 2
                                             # along a light coordinate moves the value by 1e-12 of it, under the
                                             # gap asserted below, whatever the seed or np)
                                             (257, 5, "rosenbrock", 10.), (301, 6, "rosenbrock", 1.),
                                             (512, 5, "rosenbrock", 10.)])
def test_device_generator_against_the_model_fed_its_recorded_draws(hip, n, np_, obj, ufmax):
    """10 generations with mfev = 40 np under the device's generator; the recorded draws of every
    generation drive the model: the states agree as in tests/test_slpso_golden_gpu.py.  The seed is one
    whose fitness comparisons all have a relative gap of 1e-9 or more in the model (asserted), so that the
    objective's summation order cannot turn a decision."""
    lo, up = box(n)
    g = hip.SLPSO(40 * np_, 1e-12, np_, Ufmax=ufmax, seed=1000 + n, record_draws=True)
    g.initialize(obj, lo, up, np.zeros(n))
    assert int(g.get_state("wg")[0]) == (64 if n <= 64 else 128 if n <= 128 else 256)
    m = model_beside(g, obj, n, np_, 40 * np_, 1e-12, 3., Ufmax=ufmax)
    worst = {"f": 0., "p": 0., "s": 0.}
    compare(g, m.state(), "init ", worst)
    for it in range(1, 11):
        if it % 2:
            g.iterate()
        else:
            phase_generation(g)
        tab = g.get_state("draws")
        assert tab.size == g.table_len() == sm.table_len(n, np_)
        m.iterate(sm.TableSource(tab, n, np_))
        assert min(m.gaps) >= 1e-9, "a close decision: choose another seed"
        compare(g, m.state(), "n = %d generation %d " % (n, it), worst)
    print("n = %d, np = %d: worst relative deviation from the model: f %.3e, p %.3e, s %.3e; events %s"
          % (n, np_, worst["f"], worst["p"], worst["s"], " ".join(sorted(m.events))))

def _percoord_pair(hip, n, np_, seed):
    """a handle under tests/_boxes.py's box (rosenbrock, as above) and the model started from its initial swarm"""
    from _boxes import percoord_box
    lo, up = percoord_box(n)
    g = hip.SLPSO(40 * np_, 1e-12, np_, seed=seed, record_draws=True)
    g.initialize("rosenbrock", lo, up, np.zeros(n))
    X = g.get_state("x").reshape(np_, n)
    assert ((X >= lo) & (X <= up)).all()            # the initial draw, coordinate by coordinate
    m = sm.Slpso(sm.device_objective("rosenbrock", n), list(lo), list(up), np_, 40 * np_, 1e-12)
    m.trace = True
    return g, m.start(X, [int(v) for v in g.get_state("perm")]), lo, up


# (the seeds: ones under which the model's own run redraws at both walls and meets no close decision)
@pytest.mark.parametrize("n,np_,seed", [(37, 6, 1037), (257, 5, 1257)])
def test_the_redraw_under_bounds_that_differ_in_every_coordinate(hip, n, np_, seed):
    """tests/_boxes.py's box: the eq. 11 redraw between a wall and the old position, and vmax, read another pair
    of bounds in every coordinate (the kernels stage them as lo[i] / up[i]).  SLPSO never sits on a bound, so the
    witness is the model's count of coordinates redrawn at each wall (`repairs`), three at least.  It is
    established before anything is compared: a first handle only hands over its initial swarm and the tables of
    what its generator drew, and the model runs alone on them: it must redraw at both walls and meet no decision
    closer than 1e-9.  Then a second handle of the same seed walks
    as in test_device_generator_against_the_model_fed_its_recorded_draws.  n = 37 is off every tile, 257 puts
    one live lane into the second pass."""
    gens = 10
    a, w, lo, up = _percoord_pair(hip, n, np_, seed)
    for _ in range(gens):
        a.iterate()
        w.iterate(sm.TableSource(a.get_state("draws"), n, np_))
    assert min(w.repairs.values()) >= 3, w.repairs
    assert min(w.gaps) >= 1e-9, "a close decision: choose another seed"
    g, m, lo, up = _percoord_pair(hip, n, np_, seed)
    worst = {"f": 0., "p": 0., "s": 0.}
    compare(g, m.state(), "init ", worst)
    for it in range(1, gens + 1):
        if it % 2:
            g.iterate()
        else:
            phase_generation(g)
        m.iterate(sm.TableSource(g.get_state("draws"), n, np_))
        compare(g, m.state(), "n = %d generation %d " % (n, it), worst)
        X = g.get_state("x").reshape(np_, n)
        assert ((X >= lo) & (X <= up)).all()
    assert m.repairs == w.repairs and min(m.gaps) >= 1e-9


# (b) ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 130])
def test_fused_phase_and_sequential_algorithm_2_agree_bit_for_bit(hip, n):
    np_, gens = 5, 8
    lo, up = box(n)
    hs = [hip.SLPSO(100000, 1e-12, np_, seed=77) for _ in range(3)]
    for h in hs:
        h.initialize("rosenbrock", lo, up, np.zeros(n))
    fused, phased, seq = hs
    seq.set_state("dbg", [1.])
    assert int(fused.get_state("speculative")[0]) == 1 and int(seq.get_state("speculative")[0]) == 0
    same_states(fused, phased, "init ")
    walked = 0
    for it in range(1, gens + 1):
        fev = int(fused.get_state("fev")[0])
        fused.iterate()
        seq.iterate()
        evals = phase_generation(phased)
        assert evals == int(fused.get_state("fev")[0]) - fev
        walked += evals - np_
        same_states(fused, phased, "phase path, generation %d " % it)
        same_states(fused, seq, "sequential Algorithm 2, generation %d " % it)
    assert walked > gens        # Algorithm 2 ran


def test_phase_path_of_several_populations_is_the_fused_generation(hip):
    """the populations of a handle need different numbers of evaluations per generation: one that has
    completed its generation waits for the others, and phase 0 reports 0 only when all have"""
    n, np_, P = 20, 4, 3
    lo, up = box(n)
    a = hip.SLPSO(100000, 1e-12, np_, seed=6, populations=P)
    b = hip.SLPSO(100000, 1e-12, np_, seed=6, populations=P)
    for h in (a, b):
        h.initialize("rosenbrock", lo, up, np.zeros(n * P))
    for it in range(1, 5):
        a.iterate()
        rounds = phase_generation(b)
        spent = [int(a.get_state("fev", p)[0]) for p in range(P)]
        for p in range(P):
            same_states(a, b, "generation %d population %d " % (it, p), pa=p, pb=p)
        assert [int(b.get_state("it", p)[0]) for p in range(P)] == [it] * P
    assert len(set(spent)) > 1 and rounds >= np_


# (c) ---------------------------------------------------------------------------------------------
def test_same_seed_same_run(hip):
    n, np_ = 33, 7
    lo, up = box(n)
    hs = [hip.SLPSO(100000, 1e-12, np_, seed=s) for s in (31, 31, 32)]
    for h in hs:
        h.initialize("rosenbrock", lo, up, np.zeros(n))
        assert h.run(12) == 12
    same_states(hs[0], hs[1], "")
    assert not np.array_equal(hs[0].get_state("x"), hs[2].get_state("x"))


# (d) ---------------------------------------------------------------------------------------------
def test_population_p_is_the_single_handle_on_its_sub_stream(hip):
    n, np_, P = 9, 6, 5
    lo, up = box(n)
    many = hip.SLPSO(100000, 1e-12, np_, seed=5, populations=P)
    many.initialize("rosenbrock", lo, up, np.zeros(n * P))
    assert many.run(9) == 9
    for p in range(P):
        one = hip.SLPSO(100000, 1e-12, np_, seed=5)
        one.initialize("rosenbrock", lo, up, np.zeros(n))
        one.set_state("substream", [float(p)])
        assert one.run(9) == 9
        same_states(many, one, "population %d " % p, pa=p)
    assert not np.array_equal(many.get_state("x", 0), many.get_state("x", 1))


# (e) ---------------------------------------------------------------------------------------------
def test_python_callable_gives_the_states_of_the_builtin(hip):
    n, np_, P, gens = 7, 5, 2, 5
    lo, up = box(n)
    calls = []

    def sphere(x):
        calls.append(1)
        return float(np.dot(x, x))

    a = hip.SLPSO(100000, 1e-12, np_, seed=19, populations=P)
    b = hip.SLPSO(100000, 1e-12, np_, seed=19, populations=P)
    a.initialize("sphere", lo, up, np.zeros(n * P))
    b.initialize(sphere, lo, up, np.zeros(n * P))
    for _ in range(gens):
        a.iterate()
        b.iterate()
    fev = 0
    for p in range(P):
        for k in ALL_KEYS:
            close(b.get_state(k, p), a.get_state(k, p), "population %d %s" % (p, k))
        fev += int(b.get_state("fev", p)[0])
    assert len(calls) == fev        # the callable is called once per counted evaluation


# (f) ---------------------------------------------------------------------------------------------
def test_budget_stop_with_the_overshoot_the_model_predicts(hip):
    n, np_, mfev = 5, 6, 300
    lo, up = box(n)
    g = hip.SLPSO(mfev, 1e-12, np_, seed=3, record_draws=True)
    g.initialize("rosenbrock", lo, up, np.zeros(n))
    m = model_beside(g, "rosenbrock", n, np_, mfev, 1e-12, 3.)
    gens = 0
    while m.fev < m.mfev:
        assert g.run(1) == 1
        m.iterate(sm.TableSource(g.get_state("draws"), n, np_))
        assert not m.converged()
        gens += 1
        assert int(g.get_state("fev")[0]) == m.fev
        assert int(g.get_state("flag")[0]) == (2 if m.fev >= mfev else 0)
    assert min(m.gaps) >= 1e-9
    assert g.run(5) == 0 and int(g.get_state("it")[0]) == gens
    sol = g.solution()
    assert sol.n_evals == m.fev >= mfev and sol.converged is False
    assert m.fev - mfev < np_ * (n + 1)


def test_a_tiny_box_meets_the_stol_test(hip):
    n, np_ = 4, 5
    g = hip.SLPSO(10000, 1e-3, np_, seed=8)
    sol = g.optimize("sphere", -1e-6 * np.ones(n), 1e-6 * np.ones(n), np.zeros(n))
    assert sol.converged is True and sol.n_evals < 10000
    assert int(g.get_state("flag")[0]) == 1 and int(g.get_state("it")[0]) == 1


# (g) ---------------------------------------------------------------------------------------------
def test_positions_stay_inside_the_box(hip):
    n, np_ = 37, 9
    lo, up = -np.arange(1., n + 1.), 0.5 * np.arange(1., n + 1.)
    g = hip.SLPSO(10 ** 7, 1e-12, np_, vmax=1., seed=4, populations=3)
    g.initialize("rosenbrock", lo, up, np.zeros(3 * n))
    assert g.run(50) == 50
    for p in range(3):
        for k in ("x", "pb"):
            X = g.get_state(k, p).reshape(np_, n)
            assert (X >= lo).all() and (X <= up).all(), (p, k)
        a = g.get_state("abest", p)
        assert (a >= lo).all() and (a <= up).all()
        assert (np.abs(g.get_state("v", p).reshape(np_, n)) <= (up - lo)).all()


# (h) ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("obj", ["sphere", "rosenbrock"])
def test_outcomes_lie_in_the_reference_ranges(hip, obj):
    """32 device runs (the populations of one handle) at the shape of the reference's 32 recorded complete
    runs: n = 10, box +-5, np = 20, stol = 1e-6, mfev = 40000.  The device's median log10 fabest lies
    inside the min .. max of the reference's runs, and its converged count inside the range the two halves
    of the reference's runs span (each half's rate over 32 runs), widened by the binomial 2 sigma of 32 runs
    at the pooled rate.  tests/slpso_model.py under its own generator over 32 other seeds passes the same
    bounds (sphere: median -19.63 in [-21.15, -17.91], 32 converged in [32, 32]; Rosenbrock: median -7.21 in
    [-8.40, -6.06], 12 converged in [0.63, 21.37]), so they stand as the reference gives them."""
    R = GOLD["runs"]
    n, np_, P = R["n"], R["np"], 32
    ref = R[obj]
    logf = [math.log10(float.fromhex(r["fabest"])) for r in ref]
    c = [r["converged"] for r in ref]
    c1, c2 = sum(c[:16]), sum(c[16:])
    rate = sum(c) / 32.
    sigma = math.sqrt(32 * rate * (1. - rate))
    lo_c, hi_c = 2 * min(c1, c2) - 2 * sigma, 2 * max(c1, c2) + 2 * sigma
    g = hip.SLPSO(R["mfev"], R["stol"], np_, seed=2024, populations=P, poll_every=64)
    g.initialize(obj, -R["box"] * np.ones(n), R["box"] * np.ones(n), np.zeros(n * P))
    g.run(10 ** 6)
    sols = [g.solution(p) for p in range(P)]
    flags = [int(g.get_state("flag", p)[0]) for p in range(P)]
    assert all(f in (1, 2) for f in flags)
    med = float(np.median([math.log10(max(float(g.get_state("fabest", p)[0]), 1e-300)) for p in range(P)]))
    conv = sum(s.converged for s in sols)
    print("%s: device median log10 fabest %.3f (reference %.3f .. %.3f), converged %d of 32 (bounds %.2f .. %.2f)"
          % (obj, med, min(logf), max(logf), conv, lo_c, hi_c))
    assert conv == sum(f == 1 for f in flags)
    assert min(logf) <= med <= max(logf)
    assert lo_c <= conv <= hi_c
    assert all(s.n_evals < R["mfev"] + np_ * (n + 1) for s in sols)


# the statuses of bbo_init that need a device ----------------------------------------------------------
def test_bbo_init_refuses_what_the_header_says(hip):
    import ctypes as C
    from bboptpy_amd import _ffi
    L = _ffi.lib()

    def init(n, lower, upper):
        p = _ffi.default_params(_ffi.ALGO_SLPSO)
        p.mfev, p.np = 100, 5
        h = C.c_void_p()
        assert L.bbo_create(C.byref(p), C.byref(h)) == 0
        o = _ffi.Objective()
        o.kind, o.builtin = _ffi.OBJ_BUILTIN, 0
        st = L.bbo_init(h, n, np.ascontiguousarray(lower), np.ascontiguousarray(upper), np.zeros(n), C.byref(o))
        msg = L.bbo_last_error(h)
        d = _ffi.SlpsoParams()
        L.bbo_slpso_params_default(C.byref(d))
        late = L.bbo_slpso_configure(h, C.byref(d))
        L.bbo_destroy(h)
        return st, msg, late

    st, msg, late = init(3, -np.ones(3), np.ones(3))
    assert st == 0 and late == -2       # bbo_slpso_configure after bbo_init: BBO_ERR_STATE
    st, msg, _ = init(513, -np.ones(513), np.ones(513))
    assert st == _ffi.ERR_ARG and b"dimension must be in [1, 512]" in msg
    st, msg, _ = init(3, np.array([-1., -np.inf, -1.]), np.ones(3))
    assert st == _ffi.ERR_ARG and b"the bounds must be finite" in msg
    # (an objective program reaches reject_program, the refusal every engine without a program path
    # shares; the class refuses it before that: tests/test_slpso_abi.py)
