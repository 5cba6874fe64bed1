"""GPU: the behaviour of the Mayfly engine at the C ABI: determinism, run() against iterate(), a batch against
single runs on its sub-streams, the male loop's window (1, the default, all remaining males: the same bits),
a Python callable against the built-in objective, the budget, `repair`, a stopped population, and recorded
draws injected again.  Against the recorded reference: tests/test_mayfly_golden_gpu.py."""
import numpy as np
import pytest

import mayfly_model as mm
from slpso_model import device_objective
from test_mayfly_golden_gpu import FTOL, XTOL, Worst, _ints

pytestmark = pytest.mark.gpu

KEYS = ("males_x", "males_v", "males_bx", "males_f", "males_bf", "females_x", "females_v", "females_f", "xbest",
        "fbest", "g", "dance", "fl", "it", "fev", "took", "flag", "src_m", "src_f", "branch_m", "branch_f")
STATE = ("males_x", "males_v", "males_bx", "males_f", "males_bf", "females_x", "females_v", "females_f", "xbest",
         "fbest", "g", "dance", "fl", "it", "itmax", "fev")


def _start(hip, n=17, np_=10, obj="rosenbrock", seed=7, P=1, mfev=10 ** 6, box=5., **kw):
    g = hip.Mayfly(np_, mfev, seed=seed, populations=P, **kw)
    g.initialize(obj, -box * np.ones(n), box * np.ones(n), np.zeros(P * n))
    return g


def _snapshot(g, p=0):
    return {k: g.get_state(k, p).copy() for k in KEYS}


def _same(sa, sb, tag=""):
    for k in KEYS:
        a, b = sa[k], sb[k]
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (tag + k, np.flatnonzero(a != b)[:6])


def test_same_seed_same_bits_and_run_equals_iterate(hip):
    a, b, c = (_start(hip, 33, 40, pmutnp=0.3, seed=s) for s in (11, 11, 12))
    _same(_snapshot(a), _snapshot(b), "init ")
    for _ in range(6):
        a.iterate()
    assert b.run(6) == 6
    _same(_snapshot(a), _snapshot(b), "6 generations ")
    c.run(6)
    assert _snapshot(c)["males_x"].tobytes() != _snapshot(a)["males_x"].tobytes()
    assert int(a.get_state("fev")[0]) == 2 * 40 + 6 * (3 * 40 + 12) and int(a.get_state("nmut")[0]) == 12


def test_populations_equal_single_runs_on_their_substreams(hip):
    P = 5
    batch = _start(hip, 17, 10, P=P, pmutnp=0.3, pgb=True, seed=3)
    batch.run(5)
    for p in (0, 2, 4):
        one = _start(hip, 17, 10, pmutnp=0.3, pgb=True, seed=3, substream=p)
        one.run(5)
        _same(_snapshot(batch, p), _snapshot(one), "population %d " % p)


@pytest.mark.parametrize("pgb", [False, True])
def test_the_window_of_the_male_loop_does_not_change_a_bit(hip, pgb):
    """np = 66 is no multiple of the default window; W = 1 is the sequential loop itself"""
    runs = {}
    for w in (1, 4, 0):
        g = _start(hip, 65, 66, pgb=pgb, pmutdim=0.1, seed=21)
        g.set_state("window", [float(w)])
        assert int(g.get_state("window")[0]) == w
        for _ in range(5):
            g.iterate()
        runs[w] = (_snapshot(g), int(g.get_state("dropped")[0]), int(g.get_state("rounds")[0]))
    _same(runs[1][0], runs[4][0], "window 1 against 4 ")
    _same(runs[1][0], runs[0][0], "window 1 against all ")
    assert runs[1][1] == 0 and runs[1][2] == 5 * 66            # one male per round, nothing dropped
    assert runs[4][2] < runs[1][2] and runs[0][2] < runs[4][2]
    assert runs[0][1] >= runs[4][1] > 0                          # the improvements inside a round cost redone males
    print("pgb %d: rounds / dropped of 5 generations: window 1 %s, 4 %s, all %s"
          % (pgb, runs[1][1:], runs[4][1:], runs[0][1:]))


@pytest.mark.parametrize("pgb,pmutnp", [(False, 0.05), (True, 0.3)])
def test_a_python_callable_equals_the_builtin_bit_for_bit(hip, pgb, pmutnp):
    """Rosenbrock in +, - and * alone, summed as the device sums it: the same bits.  The callable is called
    exactly n_evals times, in the reference's order: male j and female j at init, then per generation the
    females, the males, the offspring and the mutated flies"""
    n, np_, gens = 17, 10, 4
    f = device_objective("rosenbrock", n)
    calls = []

    def counted(x):
        calls.append(np.array(x))
        return f(x)

    a = _start(hip, n, np_, pgb=pgb, pmutnp=pmutnp, seed=5)
    b = hip.Mayfly(np_, 10 ** 6, seed=5, pgb=pgb, pmutnp=pmutnp)
    b.initialize(counted, -5. * np.ones(n), 5. * np.ones(n), np.zeros(n))
    _same(_snapshot(a), _snapshot(b), "init ")
    assert len(calls) == 2 * np_
    nmut = int(a.get_state("nmut")[0])
    for k in range(gens):
        a.iterate()
        before = len(calls)
        b.iterate()
        _same(_snapshot(a), _snapshot(b), "generation %d " % k)
        seen = np.array(calls[before:])
        assert len(seen) == 3 * np_ + nmut
        want = np.concatenate([b.get_state("moved_females_x").reshape(np_, n), b.get_state("moved_males_x").reshape(np_, n),
                               b.get_state("off_x").reshape(np_, n), b.get_state("mut_x").reshape(nmut, n)])
        assert seen.tobytes() == want.tobytes(), "generation %d: the order of the calls" % k
    assert b.solution().n_evals == len(calls) == 2 * np_ + gens * (3 * np_ + nmut)


# (n, np, objective, pgb): a shape of the other tests, then rows past one pass of a 256-thread workgroup:
# one live lane in the second pass (257), an odd n that is no multiple of 4 or 64 (301) and the cap (512)
WALK_SHAPES = [(33, 6, "rosenbrock", False), (257, 6, "rosenbrock", False), (301, 6, "ellipsoid", True),
               (512, 8, "rosenbrock", True)]


@pytest.mark.parametrize("n,np_,obj,pgb", WALK_SHAPES, ids=["n%d_np%d_%s_pgb%d" % s for s in WALK_SHAPES])
def test_generations_under_the_devices_draws_are_the_model(hip, n, np_, obj, pgb):
    """Four generations under the device's own generator.  Each is replayed by the model from the state the
    device held before it, with the draws the device recorded and the objective summed in the device's
    order, and compared by the rules of tests/test_mayfly_golden_gpu.py: every branch, rank, shuffle,
    selection and counter equal; positions and velocities bit for bit, except the descendants of an exp()
    form, which are held to XTOL of the box width; values to FTOL.  Two flies the mutation touches
    (pmutnp = 0.3), a tenth of their coordinates each."""
    _walk_under_the_devices_draws(hip, n, np_, obj, pgb, [-5.] * n, [5.] * n, 100 + n)


PAR = dict(pmutnp=0.3, pmutdim=0.1)
# (n, np, pgb, seed): the seed is one under which the model's own run meets the witness below
PERCOORD = [(37, 6, False, 137), (257, 6, True, 357)]


def _percoord_handle(hip, n, np_, pgb, seed, lo, up):
    g = hip.Mayfly(np_, 10 ** 6, seed=seed, record_draws=True, pgb=pgb, **PAR)
    g.initialize("sphere", np.asarray(lo), np.asarray(up), np.zeros(n))
    return g


@pytest.mark.parametrize("n,np_,pgb,seed", PERCOORD, ids=["n%d" % c[0] for c in PERCOORD])
def test_generations_under_bounds_that_differ_in_every_coordinate(hip, n, np_, pgb, seed):
    """tests/_boxes.py's box: the initial draw, vmax = k (up[j] - lo[j]), the mutation's sigma and both clamps
    read another pair of bounds in every coordinate.  The witness is established before anything is compared: a
    first handle only hands over its starting state and the tables of what its generator drew, and the model
    runs alone on them with its own objective; over its generations at least three coordinates of a fly sit on
    their lower bound, three on their upper bound, and three stay strictly inside in every fly.  Then a second
    handle of the same seed walks as above.  n = 37 is off every tile, 257 puts one live lane into the second
    pass."""
    from _boxes import binding_witness, percoord_box
    lo, up = percoord_box(n)
    gens = 4
    a = _percoord_handle(hip, n, np_, pgb, seed, lo, up)
    w = mm.Mayfly(device_objective("sphere", n), n, np_, list(lo), list(up), 10 ** 6, pgb=pgb, **PAR)
    w.stable_sort = True
    w.start({key: a.get_state(key).copy() for key in STATE})
    # the initial draw, coordinate by coordinate (the reference, and so the engine, stores the drawn point as
    # the fly's velocity and starts every fly at the origin: mayfly_model.Mayfly.init_words)
    for key in ("males_v", "females_v"):
        V = a.get_state(key).reshape(np_, n)
        assert ((V >= lo) & (V <= up)).all()
        assert ((V.max(0) - V.min(0)) > 0.1 * (up - lo)).sum() >= n // 2
    flies = []
    for _ in range(gens):
        a.iterate()
        w.iterate(mm.TableSource(a.get_state("draws"), n, np_, w.nmut, w.nmd))
        flies += [np.array([y.x for y in w.males]), np.array([y.x for y in w.females])]
    binding_witness(flies, lo, up)
    _walk_under_the_devices_draws(hip, n, np_, "sphere", pgb, list(lo), list(up), seed, gens)


def _walk_under_the_devices_draws(hip, n, np_, obj, pgb, lo, up, seed, gens=4):
    f = device_objective(obj, n)
    width = np.asarray(up, float) - np.asarray(lo, float)
    par = dict(pgb=pgb, **PAR)
    g = hip.Mayfly(np_, 10 ** 6, seed=seed, record_draws=True, **par)
    g.initialize(obj, np.asarray(lo, float), np.asarray(up, float), np.zeros(n))
    worst = Worst()
    for k in range(gens):
        tag = "n %d generation %d " % (n, k)
        before = {key: g.get_state(key).copy() for key in STATE}
        g.iterate()
        d = mm.Mayfly(f, n, np_, lo, up, 10 ** 6, **par)
        d.stable_sort = True
        d.start(before)
        assert d.nmut == 2 == int(g.get_state("nmut")[0])
        table = g.get_state("draws")
        assert table.size == g.table_len()
        d.iterate(mm.TableSource(table, n, np_, d.nmut, d.nmd))
        # (no guard against close values, as the golden test needs one: the model's sums are the device's
        # own, so two close values are the same two values on both sides and rank the same way)
        assert _ints(g, "branch_f") == d.branch_f and _ints(g, "branch_m") == d.branch_m, tag + "branches"
        for sex, flies in (("females", d.moved_females), ("males", d.moved_males)):
            taint = [y.taint for y in flies]
            worst.rows(g.get_state("moved_%s_x" % sex), [y.x for y in flies], taint, width, tag + sex + " x")
            worst.rows(g.get_state("moved_%s_v" % sex), [y.v for y in flies], taint, width, tag + sex + " v")
            worst.vals(g.get_state("moved_%s_f" % sex), [y.f for y in flies], tag + sex + " f")
        assert _ints(g, "rank_m") == d.rank_m and _ints(g, "rank_f") == d.rank_f, tag + "ranks"
        worst.rows(g.get_state("off_x"), [y.x for y in d.offspring], [y.taint for y in d.offspring], width, tag + "off x")
        worst.vals(g.get_state("off_f"), [y.f for y in d.offspring], tag + "off f")
        assert _ints(g, "perm_o") == d.perm_o and _ints(g, "perm_u") == d.perm_u, tag + "shuffles"
        worst.rows(g.get_state("mut_x"), [y.x for y in d.mutated], [y.taint for y in d.mutated], width, tag + "mut x")
        worst.vals(g.get_state("mut_f"), [y.f for y in d.mutated], tag + "mut f")
        got = [int(g.get_state(key)[0]) for key in ("took", "fev", "nmut", "it", "flag")]
        assert got == [d.took, d.fev, d.nmut, d.it, 0], (tag, got)
        worst.vals(g.get_state("fbest"), [d.fbest], tag + "fbest")
        worst.rows(g.get_state("xbest"), [d.best], [d.best_taint], width, tag + "xbest")
        assert g.get_state("g")[0] == d.g and g.get_state("dance")[0] == d.dance_now and g.get_state("fl")[0] == d.fl_now
        assert _ints(g, "sel_m") == d.sel_m and _ints(g, "sel_f") == d.sel_f, tag + "selection ranks"
        assert _ints(g, "src_m") == d.src_m and _ints(g, "src_f") == d.src_f, tag + "selection sources"
        tm, tf = [y.taint for y in d.males], [y.taint for y in d.females]
        worst.rows(g.get_state("males_x"), [y.x for y in d.males], tm, width, tag + "males_x")
        worst.rows(g.get_state("males_v"), [y.v for y in d.males], tm, width, tag + "males_v")
        worst.rows(g.get_state("males_bx"), [y.bx for y in d.males], tm, width, tag + "males_bx")
        worst.rows(g.get_state("females_x"), [y.x for y in d.females], tf, width, tag + "females_x")
        worst.rows(g.get_state("females_v"), [y.v for y in d.females], tf, width, tag + "females_v")
        worst.vals(g.get_state("males_f"), [y.f for y in d.males], tag + "males_f")
        worst.vals(g.get_state("males_bf"), [y.bf for y in d.males], tag + "males_bf")
        worst.vals(g.get_state("females_f"), [y.f for y in d.females], tag + "females_f")
        print(tag + "worst exp() descendant %.3e of the box width (%s), worst value %.3e relative"
              % (worst.x, worst.at, worst.f))
        assert worst.x <= XTOL and worst.f <= FTOL, (tag, worst.x, worst.at, worst.f)


def test_the_budget_passes_by_less_than_a_generation_and_nothing_converges(hip):
    n, np_, mfev = 10, 20, 1000
    g = hip.Mayfly(np_, mfev, seed=4)
    sol = g.optimize("sphere", -5. * np.ones(n), 5. * np.ones(n), np.zeros(n))
    per = 3 * np_ + 2
    assert mfev <= sol.n_evals < mfev + per and (sol.n_evals - 2 * np_) % per == 0 and sol.converged is False
    assert int(g.get_state("flag")[0]) == 2 and int(g.get_state("itmax")[0]) == int(np.ceil((mfev - 2 * np_) / per))
    assert g.run(5) == 0 and g.solution().n_evals == sol.n_evals       # the budget is spent: no generation
    assert np.array_equal(sol.x, g.get_state("xbest"))


def test_repair_leaves_no_aliased_slot_and_the_default_the_duplicates_the_model_predicts(hip):
    n, np_ = 33, 40
    f = device_objective("rosenbrock", n)
    for repair in (False, True):
        g = _start(hip, n, np_, seed=9, repair=repair, record_draws=True)
        x0 = g.get_state("males_x").reshape(np_, n)
        assert (x0 != 0.).all() if repair else (x0 == 0.).all()     # (the reference starts every fly at the origin)
        for k in range(4):
            before = {key: g.get_state(key).copy() for key in STATE}
            g.iterate()
            m = mm.Mayfly(f, n, np_, [-5.] * n, [5.] * n, 10 ** 6, repair=repair)
            m.stable_sort = True
            m.start(before)
            m.iterate(mm.TableSource(g.get_state("draws"), n, np_, m.nmut, m.nmd))
            src_m, src_f = [int(v) for v in g.get_state("src_m")], [int(v) for v in g.get_state("src_f")]
            assert src_m == m.src_m and src_f == m.src_f, (repair, k)
            rows = np.concatenate([g.get_state(key).reshape(np_, -1) for key in
                                   ("males_x", "males_v", "males_bx", "males_f", "males_bf")], 1)
            dup = np_ - len({r.tobytes() for r in rows})
            if repair:
                assert src_m == [int(v) for v in g.get_state("sel_m")][:np_] and len(set(src_m)) == np_
                assert src_f == [int(v) for v in g.get_state("sel_f")][:np_] and len(set(src_f)) == np_
            else:
                assert dup == m.duplicates(True) >= np_ - len(set(src_m)), (k, dup)
                assert k == 0 or dup >= np_ // 4


def test_a_stopped_population_freezes_while_the_others_go_on(hip):
    P = 3
    g = _start(hip, 17, 10, P=P, mfev=10 ** 4, seed=13)
    g.run(2)
    g.set_state("fev", [1e4], 1)            # population 1 has spent its budget
    frozen = _snapshot(g, 1)
    others = [_snapshot(g, p) for p in (0, 2)]
    assert g.run(3) == 3
    now = _snapshot(g, 1)
    now["flag"] = frozen["flag"]            # (run() marked it: flag 2)
    _same(frozen, now, "the stopped population ")
    assert int(g.get_state("flag", 1)[0]) == 2
    for p, was in zip((0, 2), others):
        assert int(g.get_state("it", p)[0]) == 5 and g.get_state("males_x", p).tobytes() != was["males_x"].tobytes()
    # iterate() is the reference's: it advances every population, stopped or not
    g.iterate()
    assert int(g.get_state("it", 1)[0]) == 3


def test_recorded_draws_injected_again_reproduce_the_run(hip):
    n, np_ = 17, 10
    a = _start(hip, n, np_, pmutnp=0.3, pmutdim=0.2, seed=31, record_draws=True)
    b = _start(hip, n, np_, pmutnp=0.3, pmutdim=0.2, seed=32)
    for key in STATE:
        b.set_state(key, a.get_state(key))
    assert a.table_len() == 2 * np_ * n + np_ + 4 + 2 * 4 * 4
    for k in range(5):
        a.iterate()
        table = a.get_state("draws")
        assert table.size == a.table_len()
        b.inject_draws(table)
        b.iterate()
        _same(_snapshot(a), _snapshot(b), "generation %d " % k)
    b.inject_draws(None)                    # back to the generator: another seed, another run
    a.iterate()
    b.iterate()
    assert a.get_state("males_x").tobytes() != b.get_state("males_x").tobytes()
    with pytest.raises(Exception, match="permutation"):
        bad = table.copy()
        bad[2 * np_ * n] = bad[2 * np_ * n + 1]
        b.inject_draws(bad)
    with pytest.raises(Exception, match="needs record_draws"):
        b.get_state("draws")
