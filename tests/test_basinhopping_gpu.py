"""GPU: BasinHopping's device-resident hops held to themselves and to the model.

  * the Python-driven path (native=False), a second implementation of the chain, gives the engine's log
  * the re-arm: every hop's minimisation is what a fresh minimiser handle started at log_start[k] returns
  * scheduling does not show: asynchronous / lockstep, poll_every, the minimiser's chunk, batched / one population
  * the log's invariants, recomputed on the host from the log and the Philox draws
  * the edges: mit = 0, temp = 0, a NaN objective, Rosenbrock's zero vector on a budget exit, print, the handles' lives
  * a global method: Rastrigin's global basin is reached more often than by the first minimisations alone

Shapes: n in {1, 2, 17, 65, 128} (one lane, the padded odd ld, the first size past one wavefront, the cap),
populations in {1, 3, 300} (more workgroups than the device has CUs); mit <= 8, the minimisers' mfev <= 4000."""
import numpy as np
import pytest

import _tabular
import basinhopping_model as bm
import objective_reference as R
import rosenbrock_model as rm
from test_basinhopping_model import GOLDEN

pytestmark = pytest.mark.gpu

KEYS = ("log", "log_start", "log_sol", "log_fev")
SHAPES = {17: ("rastrigin", 5.12), 65: ("rosenbrock", 5.)}


def minimizer(hip, kind, P=1, mfev=1500, **kw):
    if kind == "nm":
        return hip.NelderMead(mfev, 1e-8, 0.5, populations=P, seed=5, **kw)
    return hip.Rosenbrock(mfev, 1e-6, 0.5, populations=P, seed=5, **kw)


def adapt(hip):
    return hip.BasinHopping_AdaptStrategy(0.25, 0.5, 2, 0.9)


def starts(P, n, box, seed=1):
    return np.random.default_rng(seed).uniform(-0.9 * box, 0.9 * box, (P, n))


def logs(b, pops):
    return {p: [b.get_state(k, p) for k in KEYS] for p in pops}


def same_logs(a, b, tag):
    assert a.keys() == b.keys()
    for p in a:
        for k, u, v in zip(KEYS, a[p], b[p]):
            assert u.shape == v.shape and u.tobytes() == v.tobytes(), (tag, "population %d" % p, k)


# ---- the Python-driven path ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["nm", "rosen"])
def test_the_python_driven_path_gives_the_engines_log(hip, kind):
    n, mit, seed = 2, 8, 21
    fobj = rm.objective("rosenbrock", n)

    def f(x):
        return fobj(x.tolist())

    lo, up, guess = -5. * np.ones(n), 5. * np.ones(n), np.array([-1.25, 1.5])
    out = []
    for native in (True, False):
        b = hip.BasinHopping(minimizer(hip, kind, mfev=400), adapt(hip), False, mit, 1., seed=seed, native=native)
        sol = b.optimize(f, lo, up, guess)
        out.append((logs(b, [0]), sol.x.tobytes(), sol.n_evals, sol.converged))
        assert b._native is native and sol.converged is False
    same_logs(out[0][0], out[1][0], kind)
    assert out[0][1:] == out[1][1:]


# ---- the re-arm ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 17, 65, 128])
@pytest.mark.parametrize("kind,form", [("nm", dict(lds=True)), ("nm", dict(lds=False)), ("rosen", dict(wide=True)),
                                       ("rosen", dict(wide=False))], ids=["nm-lds", "nm-hbm", "rosen-wide", "rosen-narrow"])
def test_every_hop_is_a_fresh_minimisation_from_its_start(hip, kind, form, n):
    P, mit, mfev = 3, 4, 1500 if n <= 17 else 4000
    obj, box = ("rastrigin", 5.12) if n == 17 else ("rosenbrock", 5.)
    f = getattr(hip.objectives, obj)
    lo, up = -box * np.ones(n), box * np.ones(n)
    b = hip.BasinHopping(minimizer(hip, kind, P, mfev), adapt(hip), False, mit, 1., seed=4)
    b.initialize(f, lo, up, starts(P, n, box))
    b.run(mit)
    hops = 0
    for p in range(P):
        start, sol = b.get_state("log_start", p).reshape(-1, n), b.get_state("log_sol", p).reshape(-1, n)
        fev, conv = b.get_state("log_fev", p), b.get_state("log", p).reshape(-1, 7)[:, 2]
        assert start.shape == (mit + 1, n)
        # one fresh handle whose populations are the hops of this chain
        fresh = minimizer(hip, kind, mit + 1, mfev, **form)
        fresh.initialize(f, lo, up, start)
        fresh.run(1 << 30)
        for k in range(mit + 1):
            s = fresh.solution(k)
            want = fresh.get_state("xmin", k) if kind == "nm" else s.x
            tag = (kind, form, n, "population %d hop %d" % (p, k - 1))
            assert want.tobytes() == sol[k].tobytes(), tag
            assert int(fresh.get_state("fev", k)[0]) == int(fev[k]), tag
            assert int(fresh.get_state("flag", k)[0] == 1) == int(conv[k]), tag
            hops += 1
    assert hops == P * (mit + 1)


# ---- scheduling does not show ----------------------------------------------------------------------------------
_BASE = {}


def base_run(hip, kind, n, P=300, mit=4, seed=8, **ext):
    """a built-in run of P chains; the default (asynchronous) one is computed once and shared"""
    key = (kind, n) if not ext else None
    if key in _BASE:
        return _BASE[key]
    obj, box = SHAPES[n]
    mkw = {"poll_every": ext.pop("chunk")} if "chunk" in ext else {}
    b = hip.BasinHopping(minimizer(hip, kind, P, 1500, **mkw), adapt(hip), False, mit, 1., seed=seed, **ext)
    b.initialize(getattr(hip.objectives, obj), -box * np.ones(n), box * np.ones(n), starts(P, n, box))
    b.run(mit)
    out = (b, logs(b, range(P)))
    if key:
        _BASE[key] = out
    return out


@pytest.mark.parametrize("n", [17, 65])
@pytest.mark.parametrize("kind", ["nm", "rosen"])
def test_scheduling_does_not_show(hip, kind, n):
    P, mit, seed = 300, 4, 8
    b, base = base_run(hip, kind, n)
    assert int(b.get_state("lockstep")[0]) == int(n > 64)       # the default: lockstep past one wavefront from 256 chains on
    its = {int(b.get_state("it", p)[0]) for p in range(P)}
    assert its == {mit} and all(v[0].size == (mit + 1) * 7 for v in base.values())
    for lockstep in (True, False):
        other, got = base_run(hip, kind, n, lockstep=lockstep)
        assert int(other.get_state("lockstep")[0]) == int(lockstep)
        same_logs(base, got, "lockstep %s" % lockstep)
    same_logs(base, base_run(hip, kind, n, poll_every=1)[1], "poll_every 1")
    same_logs(base, base_run(hip, kind, n, chunk=1)[1], "the minimiser's chunk 1")
    # population p of the batch against a handle of its own on sub-stream p
    obj, box = SHAPES[n]
    x0 = starts(P, n, box)
    for p in (0, 7, 299):
        one = hip.BasinHopping(minimizer(hip, kind, 1, 1500), adapt(hip), False, mit, 1., seed=seed, substream=p)
        one.initialize(getattr(hip.objectives, obj), -box * np.ones(n), box * np.ones(n), x0[p])
        one.run(mit)
        same_logs({p: base[p]}, {p: logs(one, [0])[0]}, "one population on sub-stream %d" % p)
    # run(g) in pieces and iterate() are the same chain
    piece = hip.BasinHopping(minimizer(hip, kind, 3, 1500), adapt(hip), False, mit, 1., seed=seed)
    piece.initialize(getattr(hip.objectives, obj), -box * np.ones(n), box * np.ones(n), x0[:3])
    assert piece.run(1) == 1
    piece.iterate()
    assert piece.run(100) == mit - 2 and int(piece.get_state("flag", 2)[0]) == 2
    same_logs({p: base[p] for p in range(3)}, logs(piece, range(3)), "run in pieces")


# ---- the log's invariants ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [17, 65])
@pytest.mark.parametrize("kind", ["nm", "rosen"])
def test_log_invariants_on_builtin_runs(hip, kind, n):
    P, mit, seed = 300, 4, 8
    obj, box = SHAPES[n]
    b, base = base_run(hip, kind, n)
    margin = 0.05 * (box + box)
    hi, lw = box - margin, -box + margin
    decided = close = 0
    worst = 0.
    for p in range(P):
        log, start, sol, ifev = (v.reshape(mit + 1, -1) for v in base[p])
        assert log[:, 0].tolist() == list(range(-1, mit)) and log[0, 4] == 1.
        assert log[:, 6].tolist() == np.cumsum(ifev[:, 0] + 1).tolist(), p          # fev: the running sum
        assert log[:, 5].tolist() == np.minimum.accumulate(log[:, 1]).tolist(), p   # f*: the running minimum
        step, nstep, nacc, energy, x = 0.25, 0, 0, log[0, 1], sol[0]
        for k in range(mit):
            u = hip.BasinHopping.draws(seed, p, k, n)
            nstep += 1
            if nstep % 2 == 0:
                step = step / 0.9 if (1. * nacc) / nstep > 0.5 else step * 0.9
            assert log[k + 1, 3] == step, (p, k)
            want = []
            for i in range(n):      # takeStep() on the Philox draws, clamped as std::max(lw, std::min(v, hi))
                v = float(x[i]) + step * float(u[i]) * (box + box)
                t = hi if hi < v else v
                want.append(t if lw < t else lw)
            assert start[k + 1].tolist() == want, (p, k)
            gap = bm.metropolis_w(log[k + 1, 1], energy, 1.) - u[n]
            if abs(gap) < bm.CLOSE:
                close += 1
            else:
                decided += 1
                assert log[k + 1, 4] == float(gap >= 0.), (p, k, gap)
            if log[k + 1, 4]:
                energy, x = log[k + 1, 1], sol[k + 1]
                nacc += 1
        assert (int(b.get_state("nstep", p)[0]), int(b.get_state("naccept", p)[0])) == (nstep, nacc)
        assert b.get_state("stepsize", p)[0] == step and b.get_state("energy", p)[0] == energy
        assert b.get_state("x", p).tobytes() == np.asarray(x).tobytes()
        if p < 4:       # each row's energy is the objective at log_sol, within the bound of every built-in form
            for k in range(mit + 1):
                worst = max(worst, R.ratio(log[k, 1], *R.reference_at(obj, sol[k])))
    assert worst <= 1., "%.4g bounds" % worst
    assert decided >= P * mit - 2 and close <= 2
    print("RATIO BasinHopping %s n = %d: %.3f; %d decisions, %d close" % (kind, n, worst, decided, close))


# ---- edges ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 3])
def test_mit_zero_is_the_init_row_only(hip, P):
    n = 1
    b = hip.BasinHopping(minimizer(hip, "nm", P, 400), hip.BasinHopping_StepStrategy(0.1), False, 0, seed=2)
    sol = b.optimize(hip.objectives.sphere, -2. * np.ones(n), 2. * np.ones(n), np.linspace(0.5, 1.5, P * n))
    for p in range(P):
        log = b.get_state("log", p).reshape(-1, 7)
        assert log.shape == (1, 7) and log[0, 0] == -1. and log[0, 4] == 1. and log[0, 6] == b.get_state("log_fev", p)[0] + 1
        assert int(b.get_state("flag", p)[0]) == 2 and int(b.get_state("it", p)[0]) == 0
    assert sol.n_evals == int(b.get_state("fev")[0]) and sol.converged is False
    assert b.run(5) == 0
    b.iterate()
    assert b.get_state("log").size == 7


def test_temperature_zero_accepts_only_what_is_not_worse(hip):
    n, P, mit = 2, 300, 8
    b = hip.BasinHopping(minimizer(hip, "nm", P, 400), adapt(hip), False, mit, 0., seed=6)
    b.initialize(hip.objectives.rastrigin, -5.12 * np.ones(n), 5.12 * np.ones(n), starts(P, n, 5.12))
    b.run(mit)
    seen = set()
    for p in range(P):
        log = b.get_state("log", p).reshape(-1, 7)
        energy = log[0, 1]
        for k in range(1, mit + 1):
            assert log[k, 4] == float(log[k, 1] <= energy), (p, k)
            seen.add(log[k, 4])
            energy = log[k, 1] if log[k, 4] else energy
        assert b.get_state("energy", p)[0] == energy == log[-1, 5]      # greedy: the incumbent is the best
    assert seen == {0., 1.}


def test_a_nan_objective_counts_as_infinity(hip):
    n, mit = 2, 3
    b = hip.BasinHopping(minimizer(hip, "nm", 1, 60), hip.BasinHopping_StepStrategy(0.1), False, mit, seed=2)
    sol = b.optimize(lambda x: float("nan"), -np.ones(n), np.ones(n), np.zeros(n))
    log = b.get_state("log").reshape(-1, 7)
    assert np.isposinf(log[:, 1]).all() and np.isposinf(log[:, 5]).all()
    assert log[:, 4].tolist() == [1.] * (mit + 1)       # inf - inf is NaN, which std::min(0., v) passes on as 0
    assert sol.n_evals == int(log[-1, 6]) and np.isfinite(sol.x).all()


@pytest.mark.parametrize("n", [2, 65])
def test_rosenbrock_on_its_budget_hops_from_the_zero_vector(hip, n):
    P, mit, box = 3, 3, 5.
    f, lo, up, x0 = hip.objectives.rosenbrock, -box * np.ones(n), box * np.ones(n), starts(3, n, box)
    b = hip.BasinHopping(minimizer(hip, "rosen", P, 40), hip.BasinHopping_StepStrategy(0.1), False, mit, seed=2)
    b.initialize(f, lo, up, x0)
    b.run(mit)
    for p in range(P):
        log, sol = b.get_state("log", p).reshape(-1, 7), b.get_state("log_sol", p).reshape(-1, n)
        start = b.get_state("log_start", p).reshape(-1, n)
        assert (log[:, 2] == 0.).all() and (sol == 0.).all() and (log[:, 1] == float(n - 1)).all()
        assert (log[:, 4] == 1.).all()      # equal energies: exp(0) = 1 >= u
        for k in range(mit):                # every hop starts a step away from the zero vector
            u = hip.BasinHopping.draws(2, p, k, n)[:n]
            assert start[k + 1].tolist() == [0. + 0.1 * float(v) * (box + box) for v in u]
    r = hip.BasinHopping(minimizer(hip, "rosen", P, 40, repair=True), hip.BasinHopping_StepStrategy(0.1), False, mit, seed=2)
    r.initialize(f, lo, up, x0)
    r.run(mit)
    for p in range(P):
        sol = r.get_state("log_sol", p).reshape(-1, n)
        assert (np.abs(sol).sum(axis=1) > 0.).all() and (r.get_state("log", p).reshape(-1, 7)[:, 2] == 0.).all()


@pytest.mark.parametrize("P", [1, 3])
def test_print_is_the_references_table_for_population_zero(hip, capfd, P):
    n, mit = 2, 5
    b = hip.BasinHopping(minimizer(hip, "nm", P, 400), adapt(hip), True, mit, seed=12)
    b.optimize(hip.objectives.rosenbrock, -5. * np.ones(n), 5. * np.ones(n), starts(P, n, 5.))
    out = capfd.readouterr().out.splitlines()
    W = [5, 25, 5, 25, 6, 25, 10]
    want = [_tabular.fmt_row(["it", "f", "conv", "step", "accept", "f*", "fev"], W), _tabular.rule(W)]
    for r in b.get_state("log", 0).reshape(-1, 7):
        want.append(_tabular.fmt_row([int(r[0]), float(r[1]), int(r[2]), float(r[3]), int(r[4]), float(r[5]), int(r[6])], W))
    assert out == want and len(out) == mit + 3


def test_the_minimizer_handle_is_borrowed(hip):
    n, mit = 2, 3
    f, lo, up, x0 = hip.objectives.rosenbrock, -5. * np.ones(n), 5. * np.ones(n), np.array([-1.25, 1.5])
    nm = minimizer(hip, "nm", 1, 400)
    alone = nm.optimize(f, lo, up, x0)
    b = hip.BasinHopping(nm, adapt(hip), False, mit, seed=3)
    b.optimize(f, lo, up, x0)
    first = logs(b, [0])
    # the first minimisation is the minimiser's own run from the guess
    assert b.get_state("log_sol").reshape(-1, n)[0].tobytes() == alone.x.tobytes()
    assert int(b.get_state("log_fev")[0]) == alone.n_evals
    # the minimiser outlives the chain and is its own again
    del b
    again = nm.optimize(f, lo, up, x0)
    assert again.x.tobytes() == alone.x.tobytes() and again.n_evals == alone.n_evals
    # a second chain over the same handle, and the same chain again: the same bits
    st = adapt(hip)
    c = hip.BasinHopping(nm, st, False, mit, seed=3)
    c.optimize(f, lo, up, x0)
    same_logs(first, logs(c, [0]), "a second chain over the same minimiser")
    # a minimiser that ran on its own since leaves the chain stale: refused until the chain is initialised again
    from bboptpy_amd import _ffi
    nm.optimize(f, lo, up, x0)
    for call in (c.iterate, lambda: c.run(1), lambda: c.get_state("log")):
        with pytest.raises(_ffi.BboError, match="the minimizer was initialised again") as ei:
            call()
        assert ei.value.status == -2
    st.stepsize, st.nstep, st.naccept = 0.25, 0, 0
    c.optimize(f, lo, up, x0)
    same_logs(first, logs(c, [0]), "after the minimiser's own run")
    # a minimiser that re-created its handle leaves the chain stale until it is initialised again
    nm.reseed(77)
    with pytest.raises(RuntimeError, match="the minimizer was re-created"):
        c.iterate()
    assert (st.nstep, st.stepsize != 0.25) == (mit, True)       # the caller's strategy object carries the history
    st.stepsize, st.nstep, st.naccept = 0.25, 0, 0
    c.optimize(f, lo, up, x0)
    same_logs(first, logs(c, [0]), "after the minimiser's reseed")


def test_the_c_abi_refuses_what_the_classes_refuse_first(hip):
    """bbo_create_basin, bbo_bh_configure and bbo_init through the binding alone: BBO_ERR_ARG and its message"""
    import ctypes as C
    from bboptpy_amd import _ffi
    L, n = _ffi.lib(), 3

    def create(inner, P=1):
        p, h = _ffi.default_params(_ffi.ALGO_BASIN_HOPPING), C.c_void_p()
        p.populations = P
        status = L.bbo_create_basin(C.byref(p), inner._ensure_handle(), C.byref(h))
        return status, h, L.bbo_last_error(None).decode()

    for inner, P, text in ((hip.CRS(1000, 20, 1e-8), 1, "must be a NelderMead or a Rosenbrock handle of this library"),
                           (hip.NelderMead(400, 1e-8, 0.5, populations=2), 1, "as many populations as there are chains"),
                           (hip.Rosenbrock(400, 1e-6, 0.5), 3, "as many populations as there are chains"),
                           (hip.NelderMead(400, 1e-8, 0.5, hip.NelderMead.random), 1, "draws its simplex by the restart count alone")):
        status, h, msg = create(inner, P)
        assert status == _ffi.ERR_ARG and not h.value and text in msg, (msg, text)
    nm = hip.NelderMead(400, 1e-8, 0.5)
    status, h, _ = create(nm)
    assert status == 0 and h.value
    for field, bad, text in (("interval", 0, "interval must be >= 1"), ("factor", 0., "factor must be finite and positive"),
                             ("factor", float("inf"), "factor must be finite and positive"),
                             ("temp", -1., "temp must be >= 0"), ("mit", -1, "mit must be >= 0")):
        s = _ffi.BhParams()
        L.bbo_bh_params_default(C.byref(s))
        setattr(s, field, bad)
        assert L.bbo_bh_configure(h, C.byref(s)) == _ffi.ERR_ARG and text in L.bbo_last_error(h).decode(), field
    obj = _ffi.Objective()
    obj.kind, obj.builtin = _ffi.OBJ_BUILTIN, 0
    lo, up, x0 = -np.ones(n), np.ones(n), np.zeros(n)
    assert L.bbo_iterate(h) == -2                                       # before bbo_init
    assert L.bbo_init(h, n, np.array([-1., -np.inf, -1.]), up, x0, C.byref(obj)) == _ffi.ERR_ARG
    assert "the bounds must be finite" in L.bbo_last_error(h).decode()
    assert L.bbo_init(h, 129, -np.ones(129), np.ones(129), np.zeros(129), C.byref(obj)) == _ffi.ERR_ARG
    prog = hip.DeviceObjective('extern "C" __device__ double bbo_user_objective(const double *x, int n, const double *d)'
                               " { return x[0] * x[0]; }")
    pobj = _ffi.Objective()
    pobj.kind, pobj.user = _ffi.OBJ_PROGRAM, prog._handle
    assert L.bbo_init(h, n, lo, up, x0, C.byref(pobj)) == _ffi.ERR_ARG
    assert "objective programs are not supported" in L.bbo_last_error(h).decode()
    s = _ffi.BhParams()
    L.bbo_bh_params_default(C.byref(s))
    s.mit, s.print = 2, 0
    assert L.bbo_bh_configure(h, C.byref(s)) == 0 and L.bbo_init(h, n, lo, up, x0, C.byref(obj)) == 0
    done = C.c_int()
    assert L.bbo_run(h, 5, C.byref(done)) == 0 and done.value == 2
    assert L.bbo_destroy(h) == 0


# ---- a global method --------------------------------------------------------------------------------------------
def test_hops_reach_the_global_basin_more_often_than_multi_start(hip):
    g = GOLDEN["global"]
    n, box, mit = g["n"], g["box"], g["mit"]
    lo, up = -box * np.ones(n), box * np.ones(n)

    def chains(P, f, seed):
        b = hip.BasinHopping(hip.NelderMead(g["mfev"], g["tol"], g["rad0"], populations=P, seed=5),
                             hip.BasinHopping_StepStrategy(g["stepsize"]), False, mit, g["temp"], seed=seed)
        b.initialize(f, lo, up, np.random.default_rng(seed).uniform(-box, box, (P, n)))
        b.run(mit)
        first = sum(b.get_state("log", p)[1] < 0.5 for p in range(P))
        best = sum(b.get_state("fbest", p)[0] < 0.5 for p in range(P))
        return int(first), int(best)

    # 300 chains, the built-in: no fewer than the first minimisations alone, and more
    first, best = chains(300, hip.objectives.rastrigin, g["seed"])
    print("GLOBAL 300 chains: %d first minimisations in the global basin, %d chains after %d hops" % (first, best, mit))
    assert best >= first and best > first
    # the model's chains with a callable: the same chains bit for bit, so the model's counts
    fobj = rm.objective("rastrigin", n)
    first, best = chains(g["chains"], lambda x: fobj(x.tolist()), g["seed"])
    assert (first, best) == (g["first_in_global_basin"], g["best_in_global_basin"])
