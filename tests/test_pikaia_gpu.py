"""GPU: the behaviour of the PIKAIA engine at the C ABI: determinism, run() against iterate(), a batch against
single runs on its sub-streams, a Python callable against the built-in objective and the order of its calls,
recorded draws injected again, a stopped population, the stop after ngen generations, raw, repair, an objective
program against the same function as a callable, a NaN from either in both modes, the library's own refusals
(bbo_pikaia_configure, a table that leaves out a draw) and the statistics of the device's own generator.  Against the
recorded reference: tests/test_pikaia_golden_gpu.py."""
import math

import numpy as np
import pytest

import pikaia_model as pm
from slpso_model import device_objective

pytestmark = pytest.mark.gpu

KEYS = ("ph", "x", "fitns", "order", "rank", "cum", "pmut", "ig", "fev", "flag", "fbest", "xbest", "parents", "cross",
        "mode", "new_ph", "new_x", "new_f", "elite", "rdif")
STATE = ("ph", "fitns", "order", "pmut", "ig", "fev", "fbest", "xbest")
LO, UP = -3.25, 5.


def _start(hip, n=17, np_=32, nd=6, obj="rosenbrock", seed=7, P=1, ngen=10 ** 5, box=None, **kw):
    """`box`: (lower, upper) arrays in place of LO, UP"""
    g = hip.PIKAIA(np_, ngen, nd, seed=seed, populations=P, **kw)
    lo, up = (LO * np.ones(n), UP * np.ones(n)) if box is None else box
    g.initialize(obj, lo, up, np.zeros(P * n))
    return g


def _snapshot(g, p=0):
    return {k: g.get_state(k, p).copy() for k in KEYS}


def _same(sa, sb, tag="", skip=()):
    for k in KEYS:
        if k in skip:
            continue
        a, b = sa[k], sb[k]
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (tag + k, np.flatnonzero(a != b)[:6])


def test_same_seed_same_bits_and_run_equals_iterate(hip):
    # n = 65: a lane owns two coordinates; np = 66: more than one wavefront of ranks, no power of two
    a, b, c = (_start(hip, 65, 66, imut=6, ielite=1, seed=s) for s in (11, 11, 12))
    _same(_snapshot(a), _snapshot(b), "init ")
    assert int(a.get_state("fev")[0]) == 66 and int(a.get_state("ig")[0]) == 1
    f0 = a.get_state("fitns")
    assert (f0[:-1] == 0.).all() and f0[-1] < 0.       # the single stored value of init
    for _ in range(6):
        a.iterate()
    assert b.run(6) == 6
    _same(_snapshot(a), _snapshot(b), "6 generations ")
    c.run(6)
    assert _snapshot(c)["ph"].tobytes() != _snapshot(a)["ph"].tobytes()
    assert int(a.get_state("fev")[0]) == 66 + 6 * 67 and int(a.get_state("ig")[0]) == 7
    ph = a.get_state("ph")
    assert (ph >= 0.).all() and (ph < 1.).all()
    assert a.get_state("x").tobytes() == (LO + ph * (UP - LO)).tobytes()
    order = a.get_state("order").astype(int)
    fit = a.get_state("fitns")
    assert sorted(order) == list(range(66)) and (np.diff(fit[order]) >= 0.).all()
    assert a.get_state("fitns").tobytes() == (-a.get_state("new_f")).tobytes()


def test_populations_equal_single_runs_on_their_substreams(hip):
    P = 5
    batch = _start(hip, 17, 32, P=P, imut=5, ielite=1, seed=3)
    batch.run(5)
    for p in (0, 2, 4):
        one = _start(hip, 17, 32, imut=5, ielite=1, seed=3, substream=p)
        one.run(5)
        _same(_snapshot(batch, p), _snapshot(one), "population %d " % p)


@pytest.mark.parametrize("ielite,repair", [(0, False), (1, False), (1, True)])
def test_a_python_callable_equals_the_builtin_bit_for_bit(hip, ielite, repair):
    """Rosenbrock in +, - and * alone, summed as the device sums it: the same bits.  The callable is called in
    the reference's order: new row 1 first when ielite = 1, then rows 1 .. np (np under repair)"""
    n, np_, gens = 17, 20, 5
    f = device_objective("rosenbrock", n)
    calls = []

    def counted(x):
        calls.append(np.array(x))
        return f(x)

    a = _start(hip, n, np_, imut=5, ielite=ielite, repair=repair, seed=5)
    b = hip.PIKAIA(np_, 10 ** 5, 6, imut=5, ielite=ielite, repair=repair, seed=5)
    b.initialize(counted, LO * np.ones(n), UP * np.ones(n), np.zeros(n))
    _same(_snapshot(a), _snapshot(b), "init ")
    assert len(calls) == np_
    per = np_ if repair else np_ + ielite
    taken = 0
    for k in range(gens):
        a.iterate()
        before = len(calls)
        b.iterate()
        _same(_snapshot(a), _snapshot(b), "generation %d " % k)
        seen = np.array(calls[before:])
        assert len(seen) == per, k
        rows = b.get_state("new_x").reshape(np_, n)
        elite = int(b.get_state("elite")[0])
        taken += elite
        if repair:
            # every bred row once; where the elite replaced row 1, that row keeps its stored value
            assert seen[1:].tobytes() == rows[1:].tobytes() and (elite or seen[0].tobytes() == rows[0].tobytes())
        else:
            assert seen[ielite:].tobytes() == rows.tobytes(), "generation %d: the order of the calls" % k
            if ielite and not elite:
                assert seen[0].tobytes() == rows[0].tobytes()
    assert ielite == 0 or taken > 0
    want = np_ + gens * (np_ if repair else np_ + 1)       # the reference's counter
    assert b.solution().n_evals == want and len(calls) == np_ + gens * per


# (n, np, objective, options): a shape of the other tests, then rows past one pass of a 256-thread
# workgroup: one live lane in the second pass (257), an odd n that is no multiple of 4 or 64 (301), the cap
WALK_SHAPES = [(17, 6, "rosenbrock", dict(imut=5, ielite=1)),
               (257, 6, "rosenbrock", dict(imut=5, ielite=1)),
               (301, 6, "ellipsoid", dict(imut=6, ielite=1, repair=True)),
               (512, 8, "rosenbrock", dict(imut=2, ielite=0)),
               (512, 6, "ellipsoid", dict(imut=5, ielite=1))]


@pytest.mark.parametrize("n,np_,obj,kw", WALK_SHAPES,
                         ids=["n%d_np%d_%s_imut%d" % (s[0], s[1], s[2], s[3]["imut"]) for s in WALK_SHAPES])
def test_generations_under_the_devices_draws_are_the_model(hip, n, np_, obj, kw):
    """Five generations under the device's own generator.  Each is replayed by the model (in the stable order,
    the objective summed in the device's order) from the state the device held before it, with the draws the
    device recorded: parents, crossover windows, kinds of mutation, phenotypes, points, values, the elite
    decision, the rank order, pmut and the counters are the device's, the floats bit for bit.  A generation
    with a decision too close to call (pikaia_model.Pikaia.ok) asks for another seed."""
    _walk_under_the_devices_draws(hip, n, np_, obj, kw, [LO] * n, [UP] * n)


@pytest.mark.parametrize("n", [37, 257])
def test_the_phenotype_is_scaled_by_each_coordinates_own_bounds(hip, n):
    """tests/_boxes.py's box: x[i] = lower[i] + u[i] (upper[i] - lower[i]) is another map in every coordinate
    (PIKAIA only scales by the box: the search runs in the unit cube and nothing is repaired into the box, so
    there is no bound to sit on).  The walk above, bit for bit; n = 37 is off every tile, 257 puts one live lane
    into the second pass."""
    from _boxes import percoord_box
    lo, up = percoord_box(n)
    g = _walk_under_the_devices_draws(hip, n, 6, "sphere", dict(imut=5, ielite=1), list(lo), list(up))
    X, U = g.get_state("x").reshape(6, n), g.get_state("ph").reshape(6, n)
    assert ((X >= lo) & (X <= up)).all()
    assert X.tobytes() == (lo + U * (up - lo)).tobytes()


def _walk_under_the_devices_draws(hip, n, np_, obj, kw, lo, up):
    nd = 6
    g = _start(hip, n, np_, nd, obj=obj, seed=200 + n, record_draws=True, box=(np.asarray(lo), np.asarray(up)), **kw)
    assert g.table_len() == pm.table_layout(n, np_, nd)["len"]
    d = pm.Pikaia(device_objective(obj, n), n, np_, 10 ** 5, nd, lo, up, order="stable", **kw)
    for k in range(5):
        tag = "n %d generation %d " % (n, k)
        before = {key: g.get_state(key).copy() for key in ("ph", "fitns", "order", "pmut", "ig", "fev")}
        g.iterate()
        d.start(before["ph"].reshape(np_, n), before["fitns"], before["order"], before["pmut"][0], before["ig"][0],
                before["fev"][0])
        d.iterate(pm.TableSource(g.get_state("draws")))
        # (close values are no obstacle here: the model's sums are the device's own; only rdif, which goes
        # through pow and sqrt, may fall on the other side of a threshold)
        assert not d.rdif_close, tag + "rdif too close to a threshold: choose another seed"
        ints = lambda key: [int(v) for v in g.get_state(key)]
        assert ints("parents") == [v for pr in d.parents for v in pr], tag + "parents"
        assert ints("cross") == [v for cr in d.cross for v in cr], tag + "crossover windows"
        assert ints("mode") == d.mode, tag + "kinds of mutation"
        ph = np.asarray(d.ph, float)
        assert g.get_state("new_ph").tobytes() == ph.tobytes(), tag + "new phenotypes"
        assert g.get_state("ph").tobytes() == ph.tobytes(), tag + "the population"
        x = np.asarray([d.map(r) for r in d.ph], float)
        assert g.get_state("new_x").tobytes() == x.tobytes() and g.get_state("x").tobytes() == x.tobytes(), tag + "points"
        assert int(g.get_state("elite")[0]) == d.elite, tag + "elite"
        fit = np.asarray(d.fitns, float)
        assert g.get_state("fitns").tobytes() == fit.tobytes(), (tag + "values", g.get_state("fitns"), fit)
        assert ints("order") == d.order, tag + "rank order"
        assert g.get_state("pmut")[0] == d.pmut, tag + "pmut"
        got = [int(g.get_state(key)[0]) for key in ("fev", "ig", "flag")]
        assert got == [d.fev, d.ig, 0], (tag, got)
    print("n %d np %d %s: paths %s" % (n, np_, obj, {p: c for p, c in d.paths.items() if c}))
    return g


def test_recorded_draws_injected_again_reproduce_the_run(hip):
    n, np_, nd = 5, 12, 6
    kw = dict(imut=5, ielite=1, pmut=0.05)
    a = _start(hip, n, np_, nd, seed=31, record_draws=True, **kw)
    b = _start(hip, n, np_, nd, seed=32, **kw)
    for key in STATE:
        b.set_state(key, a.get_state(key))
    lay = pm.table_layout(n, np_, nd)
    assert a.table_len() == lay["len"] == 6 * (69 + 2 * (1 + 2 * 30))
    for k in range(5):
        a.iterate()
        table = a.get_state("draws")
        assert table.size == a.table_len()
        t = table.reshape(np_ // 2, -1)
        assert (t[:, 0] >= 0.).all() and (t[:, lay["x"]] >= 0.).all() and (t[:, lay["child"]] >= 0.).all()
        assert ((t == -1.) | ((t >= 0.) & (t < 1.))).all() and (t[:, lay["p2"] + 8:lay["x"]] == -1.).all()
        b.inject_draws(table)
        b.iterate()
        _same(_snapshot(a), _snapshot(b), "generation %d " % k)
    b.inject_draws(None)                    # back to the generator: another seed, another run
    a.iterate()
    b.iterate()
    assert a.get_state("ph").tobytes() != b.get_state("ph").tobytes()
    with pytest.raises(Exception, match=r"uniforms lie in \[0, 1\)"):
        bad = table.copy()
        bad[3] = 1.5
        b.inject_draws(bad)
    with pytest.raises(Exception, match="populations \\*"):
        b.inject_draws(table[:-1])
    with pytest.raises(Exception, match="needs record_draws"):
        b.get_state("draws")


def test_a_stopped_population_freezes_while_the_others_go_on(hip):
    P, ngen = 3, 8
    g = _start(hip, 17, 32, P=P, ngen=ngen, ielite=1, seed=13)
    g.run(2)
    g.set_state("ig", [float(ngen + 1)], 1)         # population 1 has had its generations
    frozen = _snapshot(g, 1)
    others = [_snapshot(g, p) for p in (0, 2)]
    assert g.run(3) == 3
    _same(frozen, _snapshot(g, 1), "the stopped population ", skip=("flag",))
    assert int(g.get_state("flag", 1)[0]) != 0
    for p, was in zip((0, 2), others):
        assert int(g.get_state("ig", p)[0]) == 6 and g.get_state("ph", p).tobytes() != was["ph"].tobytes()
    # iterate() is the reference's: it advances every population, stopped or not
    g.iterate()
    assert int(g.get_state("ig", 1)[0]) == ngen + 2


def test_it_stops_after_exactly_ngen_generations_converged(hip):
    n, np_, ngen = 10, 20, 7
    g = hip.PIKAIA(np_, ngen, 6, seed=4)
    sol = g.optimize("sphere", LO * np.ones(n), UP * np.ones(n), np.zeros(n))
    assert sol.n_evals == np_ + ngen * (np_ + 1) and sol.converged is True
    assert int(g.get_state("flag")[0]) == 1 and int(g.get_state("ig")[0]) == ngen + 1
    assert g.run(5) == 0 and g.solution().n_evals == sol.n_evals       # no generation beyond ngen
    best = int(g.get_state("order")[-1])
    assert np.array_equal(sol.x, g.get_state("x").reshape(np_, n)[best]) and g.solution().converged is True
    h = hip.PIKAIA(np_, ngen, 6, seed=4)
    h.initialize("sphere", LO * np.ones(n), UP * np.ones(n), np.zeros(n))
    assert h.run(ngen - 1) == ngen - 1 and int(h.get_state("flag")[0]) == 0
    h.run(100)          # (returns the generations launched, a whole poll interval; one of them runs)
    assert int(h.get_state("flag")[0]) == 1 and int(h.get_state("ig")[0]) == ngen + 1
    assert h.solution().n_evals == sol.n_evals and h.get_state("ph").tobytes() == g.get_state("ph").tobytes()
    # the best ever, on the objective's scale, is never worse than the best of the population
    assert h.get_state("fbest")[0] <= -np.max(h.get_state("fitns")) and h.get_state("fbest")[0] >= 0.


def test_raw_maximises_over_the_unit_cube_and_never_reads_the_box(hip):
    n, np_ = 4, 20
    bad = np.array([np.inf, np.nan, -np.inf, 0.])
    g = hip.PIKAIA(np_, 40, 6, ielite=1, raw=True, seed=8)
    g.initialize("sphere", bad, bad, np.zeros(n))
    first = float(np.max(g.get_state("new_f")))
    assert g.get_state("x").tobytes() == g.get_state("ph").tobytes()
    g.run(40)
    x, fit = g.get_state("x").reshape(np_, n), g.get_state("fitns")
    assert (x >= 0.).all() and (x < 1.).all() and g.get_state("x").tobytes() == g.get_state("ph").tobytes()
    assert fit.tobytes() == g.get_state("new_f").tobytes()             # the fitness is +f
    sol = g.solution()
    assert fit.max() > first and np.array_equal(sol.x, x[int(g.get_state("order")[-1])])
    assert g.get_state("fbest")[0] >= fit.max()
    seen = []

    def f(u):
        seen.append(np.array(u))
        return float(np.sum(u * u))

    c = hip.PIKAIA(np_, 3, 6, raw=True, seed=8)
    c.optimize(f, bad, bad, np.zeros(n))
    seen = np.array(seen)
    assert len(seen) == np_ + 3 * np_ and (seen >= 0.).all() and (seen < 1.).all()
    with pytest.raises(ValueError, match="finite"):
        hip.PIKAIA(np_, 3, 6).initialize("sphere", bad, bad, np.zeros(n))


def test_repair_lets_pmut_fall_and_the_default_only_raises_it(hip):
    """sphere >= 0: the fitness is <= 0 and the signed denominator of imut 2 makes rdif negative"""
    seqs = {}
    for repair in (False, True):
        g = _start(hip, 2, 20, 4, obj="sphere", imut=2, ielite=1, repair=repair, seed=17)
        if repair:
            f0 = g.get_state("fitns")
            assert (f0 < 0.).all() and f0.tobytes() == (-g.get_state("new_f")).tobytes()    # every initial value
        seq = [g.get_state("pmut")[0]]
        for _ in range(60):
            g.iterate()
            seq.append(g.get_state("pmut")[0])
            assert repair or g.get_state("rdif")[0] <= 0.
        seqs[repair] = np.diff(seq)
        assert int(g.get_state("fev")[0]) == 20 + 60 * (20 if repair else 21)
    assert (seqs[False] >= 0.).all() and (seqs[False] > 0.).sum() == 10       # 0.005 1.5^10 > 0.25: ten rises, then held
    assert (seqs[True] < 0.).any() and (seqs[True] > 0.).any()


PROG = '''
extern "C" __device__ double bbo_user_objective(const double *x, int n, const double *data)
{
    double m = 0.;
    for (int j = 0; j < n; j++) {
        const double d = fabs(x[j] - data[j]);
        m = d > m ? d : m;
    }
    return m;
}
'''


def test_a_device_objective_equals_the_same_function_as_a_callable(hip):
    """max_j |x_j - data_j|: no accumulated rounding, so the two runs are the same bits"""
    n, np_, P, gens = 5, 16, 3, 10
    data = np.array([0.5, -1.25, 2., 3.5, -0.75])
    prog = hip.DeviceObjective(PROG, data=data)
    runs = []
    for f in (prog, lambda x: float(np.max(np.abs(x - data)))):
        g = hip.PIKAIA(np_, 100, 6, imut=6, ielite=1, seed=23, populations=P)
        g.initialize(f, LO * np.ones(n), UP * np.ones(n), np.zeros(P * n))
        taken = 0
        for _ in range(gens):
            g.iterate()
            taken += sum(int(g.get_state("elite", p)[0]) for p in range(P))
        assert taken > 0        # the elite path ran: the one-row launch and the copy
        runs.append([_snapshot(g, p) for p in range(P)])
        assert int(g.get_state("fev", P - 1)[0]) == np_ + gens * (np_ + 1)
    for p in range(P):
        _same(runs[0][p], runs[1][p], "population %d " % p)
    assert runs[0][0]["ph"].tobytes() != runs[0][1]["ph"].tobytes()


NAN_PROG = '''
extern "C" __device__ double bbo_user_objective(const double *x, int n, const double *data)
{
    double m = 0.;
    for (int j = 0; j < n; j++) {
        const double d = fabs(x[j] - data[j]);
        m = d > m ? d : m;
    }
    return x[0] > data[n] ? __builtin_nan("") : m;
}
'''


@pytest.mark.parametrize("raw", [False, True])
def test_a_nan_ranks_worst_from_a_program_and_from_a_callable(hip, raw):
    """the objective is undefined (NaN) on the part of the domain where x_0 exceeds a threshold; minimised by
    default, maximised under raw.  The program's NaN is stored as +inf, the callable's stays a NaN: the same run"""
    n, np_, gens = 4, 20, 12
    data = np.array([0.25, 0.5, 0.75, 0.125, 0.5]) if raw else np.array([0.5, -1.25, 2., 3.5, 1.])
    cut = data[n]

    def f(x):
        return float("nan") if x[0] > cut else float(np.max(np.abs(x - data[:n])))

    keys = ("ph", "x", "fitns", "order", "rank", "pmut", "fbest", "xbest", "parents", "cross", "mode", "elite", "fev")
    runs = []
    for obj in (hip.DeviceObjective(NAN_PROG, data=data), f):
        g = hip.PIKAIA(np_, 100, 6, imut=6, ielite=1, raw=raw, seed=29)
        g.initialize(obj, LO * np.ones(n), UP * np.ones(n), np.zeros(n))
        undefined = 0
        for _ in range(gens):
            g.iterate()
            x, fit, order = g.get_state("x").reshape(np_, n), g.get_state("fitns"), g.get_state("order").astype(int)
            bad = x[:, 0] > cut
            undefined += int(bad.sum())
            assert (fit[bad] == -np.inf).all() and np.isfinite(fit[~bad]).all()
            assert (~np.isfinite(g.get_state("new_f"))[bad]).all()
            assert not bad[order[np_ - 1]] and list(order[:bad.sum()]) == sorted(np.flatnonzero(bad))   # worst, by row
        assert undefined > 0
        best = g.get_state("xbest")
        assert best[0] <= cut and np.isfinite(g.get_state("fbest")[0]) and g.solution().x[0] <= cut
        assert g.get_state("fbest")[0] == f(best)
        runs.append({k: g.get_state(k).copy() for k in keys})
    for k in keys:
        assert runs[0][k].tobytes() == runs[1][k].tobytes(), k


def test_the_library_refuses_what_the_class_refuses(hip):
    """bbo_pikaia_configure through the C ABI: every refusal with its reason, and BBO_ERR_STATE after bbo_init"""
    import ctypes as C
    from bboptpy_amd import _ffi
    L = _ffi.lib()
    g = hip.PIKAIA(10, 5, 6, seed=1)
    h = g._ensure_handle()
    for field, value, why in (("irep", 2, "steady-state"), ("irep", 3, "sequential walk"), ("imut", 0, "imut must be in"),
                              ("imut", 7, "imut must be in"), ("ielite", 2, "ielite is 0 or 1"),
                              ("pcross", 1.5, "pcross must lie in"), ("pmut", -0.1, "pmut must lie in"),
                              ("pmutmn", 2., "pmutmn must lie in"), ("pmutmx", -1., "pmutmx must lie in"),
                              ("pmutmn", 0.3, "pmutmn must not exceed pmutmx"), ("fdif", 1.5, "fdif must lie in"),
                              ("fdif", -0.5, "fdif must lie in"), ("repair", 2, "repair is 0 or 1"),
                              ("raw", -1, "raw is 0 or 1"), ("substream", -1, "substream must be in")):
        d = _ffi.PikaiaParams()
        L.bbo_pikaia_params_default(C.byref(d))
        setattr(d, field, value)
        assert L.bbo_pikaia_configure(h, C.byref(d)) == _ffi.ERR_ARG, field
        assert why in L.bbo_last_error(h).decode(), (field, L.bbo_last_error(h).decode())
    assert L.bbo_pikaia_configure(h, None) == _ffi.ERR_ARG
    d = _ffi.PikaiaParams()
    L.bbo_pikaia_params_default(C.byref(d))
    assert L.bbo_pikaia_configure(h, C.byref(d)) == 0
    assert L.bbo_pikaia_inject_draws(h, None, 0) == -2 and "before initialize" in L.bbo_last_error(h).decode()
    lo, up = LO * np.ones(3), UP * np.ones(3)
    with pytest.raises(_ffi.BboError, match="finite"):
        ob = _ffi.Objective(kind=_ffi.OBJ_BUILTIN, builtin=0)
        _ffi.check(L.bbo_init(h, 3, lo, np.array([1., np.inf, 1.]), np.zeros(3), C.byref(ob)), h)
    g.initialize("sphere", lo, up, np.zeros(3))
    assert L.bbo_pikaia_configure(h, C.byref(d)) == -2 and "after bbo_init" in L.bbo_last_error(h).decode()
    other = hip.Mayfly(10, 1000, seed=1)
    assert L.bbo_pikaia_configure(other._ensure_handle(), C.byref(d)) == _ffi.ERR_ARG
    assert "not a PIKAIA handle" in L.bbo_last_error(other._handle).decode()


def test_a_table_that_leaves_out_a_draw_is_refused(hip):
    n, np_, nd = 3, 8, 4
    g = _start(hip, n, np_, nd, imut=4, pmut=0.3, seed=2, record_draws=True)     # imut 4: pmut stays
    g.iterate()
    table = g.get_state("draws")
    g.inject_draws(table)
    lay = pm.table_layout(n, np_, nd)
    t = table.reshape(np_ // 2, -1)
    crossed = int(np.flatnonzero(t[:, lay["x"]] < 0.85)[0])
    two = np.flatnonzero((t[:, lay["x"]] < 0.85) & (t[:, lay["x"] + 2] >= 0.5))
    child = lay["child"]
    hit = int(np.flatnonzero(t[0, child + 1:child + 1 + lay["loci"]] < 0.3)[0])
    cases = [(0, 0, "first parent"), (0, lay["p2"], "first parent"), (0, lay["x"], "crossover coin"),
             (crossed, lay["x"] + 1, "draws ispl"), (crossed, lay["x"] + 2, "draws ispl"),
             (0, child, "coin of every child"), (0, child + lay["per_child"], "coin of every child"),
             (0, child + 2, "every locus draws"), (0, child + 1 + lay["loci"] + hit, "its value where")]
    if two.size:
        cases.append((int(two[0]), lay["x"] + 3, "ispl2"))
    for row, col, why in cases:
        bad = t.copy()
        bad[row, col] = -1.
        with pytest.raises(Exception, match=why):
            g.inject_draws(bad)
    g.iterate()         # the table that stood is still the one in use (another state reads other optional slots)
    now = g.get_state("draws")
    both = (now != -1.) & (table != -1.)
    assert (now[both] == table[both]).all() and both.sum() > np_ // 2 * (3 + 2 * lay["loci"])


def test_statistics_of_the_device_generator(hip):
    """4096 populations x one generation at n = 2, np = 16, nd = 6: the share of matings with a crossover
    against pcross, the share of mutated loci against pmut, the first parents' ranks against the roulette's
    weights and the second parents' against the same weights without the first parent's row.  Each bound is 5 sigma of the binomial / multinomial counts themselves."""
    n, np_, nd, P, pcross, pmut = 2, 16, 6, 4096, 0.85, 0.005
    g = _start(hip, n, np_, nd, P=P, imut=1, repair=True, seed=41, record_draws=True)
    jfit = np.array([np_ - g.get_state("rank", p) for p in range(P)]).astype(int)       # 1 = best
    g.iterate()
    lay = pm.table_layout(n, np_, nd)
    crossed = loci = mutated = 0
    counts, counts2, expect2 = np.zeros(np_ + 1), np.zeros(np_ + 1), np.zeros(np_ + 1)
    weight = np.array([(np_ + 1) + 1. * (np_ + 1 - 2 * j) for j in range(1, np_ + 1)])
    for p in range(P):
        t = g.get_state("draws", p).reshape(np_ // 2, -1)
        cross = g.get_state("cross", p).reshape(-1, 2)
        assert ((cross[:, 0] > 0) == (t[:, lay["x"]] < pcross)).all()
        crossed += int((cross[:, 0] > 0).sum())
        for ch in range(2):
            u = t[:, lay["child"] + ch * lay["per_child"] + 1:][:, :lay["loci"]]
            v = t[:, lay["child"] + ch * lay["per_child"] + 1 + lay["loci"]:][:, :lay["loci"]]
            assert ((u >= 0.) & (u < 1.)).all() and ((v >= 0.) == (u < pmut)).all()
            loci += u.size
            mutated += int((u < pmut).sum())
        par = g.get_state("parents", p).reshape(-1, 2).astype(int)
        assert (par[:, 0] != par[:, 1]).all()
        np.add.at(counts, jfit[p][par[:, 0]], 1)
        np.add.at(counts2, jfit[p][par[:, 1]], 1)
        # the second parent given the first: the weights without the first parent's row, renormalised
        for a in jfit[p][par[:, 0]]:
            q = weight.copy()
            q[a - 1] = 0.
            expect2[1:] += q / q.sum()
    matings = P * np_ // 2
    for what, k, N, q in (("crossover", crossed, matings, pcross), ("mutated loci", mutated, loci, pmut)):
        sigma = math.sqrt(N * q * (1. - q))
        print("%s: %d of %d, expected %.1f +- %.1f" % (what, k, N, N * q, sigma))
        assert abs(k - N * q) <= 5. * sigma, what
    np1 = np_ + 1
    prob = np.array([(np1 + 1. * (np1 - 2 * j)) / (np_ * np1) for j in range(1, np_ + 1)])
    assert abs(prob.sum() - 1.) < 1e-12
    chi2 = float(((counts[1:] - matings * prob) ** 2 / (matings * prob)).sum())
    dof = np_ - 1
    print("ranks of the first parents: chi^2 %.1f at %d degrees of freedom" % (chi2, dof))
    assert chi2 <= dof + 5. * math.sqrt(2. * dof)
    chi2 = float(((counts2[1:] - expect2[1:]) ** 2 / expect2[1:]).sum())
    print("ranks of the second parents given the first: chi^2 %.1f at %d degrees of freedom" % (chi2, dof))
    assert counts2.sum() == matings and chi2 <= dof + 5. * math.sqrt(2. * dof)
