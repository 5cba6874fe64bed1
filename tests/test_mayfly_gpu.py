"""GPU: the behaviour of the Mayfly engine at the C ABI: determinism, run() against iterate(), a batch against
single runs on its sub-streams, the male loop's window (1, the default, all remaining males: the same bits),
a Python callable against the built-in objective, the budget, `repair`, a stopped population, and recorded
draws injected again.  Against the recorded reference: tests/test_mayfly_golden_gpu.py."""
import numpy as np
import pytest

import mayfly_model as mm
from slpso_model import device_objective

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
