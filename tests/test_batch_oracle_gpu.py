"""GPU parity of EVERY population of a batched swarm handle: population p of a handle made with
`populations=P` against its own run of the CPU oracle on Philox sub-stream p (Handle.set_sub).

The single-population parity files (test_de_gpu.py, test_sansde_gpu.py, test_cso_gpu.py,
test_pso_gpu.py, test_ccpso_gpu.py) hold sub-stream 0; tests/test_batch_gpu.py holds population 0
of a batch to the single run.  Here the populations p > 0 -- whose archive fill, success-memory
slot, fuzzy state, swarm count and shuffle key go their own way from generation 0 on -- are held,
after initialize and after every generation, to the same keys at the same tolerances as those files
(tests/batch_oracle.py cites each line).  tests/test_oracle_substreams.py shows on the CPU that an
oracle object on sub-stream p draws what it says and that the cases below are runs in which the
populations do differ.

SepCMAES records its normals like the dense variants (`zlast`), so both are held.

Measured on an MI355X -- worst relative deviation over all populations and generations of a case,
with the key, population and generation that held it (every test prints its own line):
  SHADE  n 8 np 64 LPSR     2.5e-15  x, population 3, generation 24
  SHADE  n 33 np 50         8.7e-16  MCR, population 0, generation 0
  SHADE  n 12 np 20 h 3     1.7e-15  x, population 1, generation 8
  SHADE  n 150 np 24        4.4e-16  x, population 0, generation 8
  JADE   n 8 np 16          9.1e-16  f, population 3, generation 9
  JADE   n 21 np 40         7.3e-16  x, population 2, generation 8
  SaNSDE n 8 np 16          8.4e-16  crrec, population 2, generation 0
  SaNSDE n 12 np 20         1.5e-15  crrec, population 0, generation 8
  CSO    n 8 np 12          4.5e-16  f, population 2, generation 6
  CSO    n 7 np 31 ring     2.3e-16  f, population 1, generation 2
  CSO    n 12 np 202 ring   1.3e-15  f, population 3, generation 7
  APSO   n 8 np 12          2.0e-12  evof, population 4, generation 7
  APSO   n 33 np 70         3.5e-13  evof, population 1, generation 7
  APSO   n 12 np 150        3.1e-12  evof, population 2, generation 0
  CCPSO  n 12 np 8          4.2e-15  fyhat, population 0, generation 29
  CCPSO  n 16 np 6          9.6e-15  yhat, population 4, generation 29
  CCPSO  n 300 np 24        5.6e-15  x, population 1, generation 1
  frozen neighbour: SHADE 9.2e-16 (f, population 3), CCPSO 8.9e-16 (fyhat, population 0)
  host callable against the built-in: SHADE 4.5e-16, CSO 2.2e-16, APSO 2.0e-16, CCPSO 2.0e-16
  CMA normals: equal bits in all 5 populations, both variants
All integer keys equal; every population matched its own oracle run."""
import numpy as np
import pytest

import batch_oracle as bo

pytestmark = pytest.mark.gpu


def _pair(hip, oracle_lib, c, sub_shift=0):
    """one device handle with P populations and P oracle objects, object p on sub-stream p + shift"""
    n, P = c["n"], c["P"]
    lo, up = bo.box(n)
    guess = np.random.default_rng(4).uniform(-4., 4., (P, n))       # (ignored by these engines, like the reference)
    g = bo.device_handle(hip, c)
    g.initialize(getattr(hip.objectives, c["obj"]), lo, up, guess)
    if c["engine"] == "apso":
        assert int(g.get_state("chunk")[0]) == c["chunk"]           # what the oracle objects are told
    objs = [bo.oracle_object(oracle_lib, c, p + sub_shift) for p in range(P)]
    return g, objs


def _compare_all(g, objs, c, tag, worst, skip=()):
    for p, o in enumerate(objs):
        if p in skip:
            continue
        bo.COMPARE[c["engine"]](bo.Compare(g, o, p, tag, worst), c)


@pytest.mark.parametrize("c", bo.CASES, ids=[c["id"] for c in bo.CASES])
def test_every_population_matches_its_own_oracle_run(hip, oracle_lib, c):
    g, objs = _pair(hip, oracle_lib, c)
    worst = bo.Worst()
    for p, o in enumerate(objs):
        bo.compare_init(bo.Compare(g, o, p, "init", worst), c)
    for gen in range(c["gens"]):
        g.iterate()
        for o in objs:
            o.iterate()
        _compare_all(g, objs, c, "generation %d" % gen, worst)
    print("%s, P = %d, %d generations (%s): worst relative deviation from the oracle runs %s"
          % (c["id"], c["P"], c["gens"], c["note"], worst))
    if c["engine"] == "shade" and "npmin" in c["kw"]:
        assert int(g.get_state("np", c["P"] - 1)[0]) < c["size"]    # the population reduction did run
    for o in objs:
        o.destroy()


@pytest.mark.parametrize("engine", ["shade", "jade", "sansde", "cso", "apso", "ccpso"])
def test_the_comparison_tells_sub_streams_apart(hip, oracle_lib, engine):
    """negative control: oracle object p on sub-stream p + 1 does NOT start where population p does
    -- it starts where population p + 1 does, whose stream it is"""
    c = bo.FIRST[engine]
    g, shifted = _pair(hip, oracle_lib, c, sub_shift=1)
    for p, o in enumerate(shifted):
        have, want = np.sort(g.get_state("x", p), axis=None), np.sort(o.get("x"), axis=None)
        assert have.shape == want.shape
        assert not np.array_equal(have, want), (engine, p)
        if p + 1 < c["P"]:
            np.testing.assert_array_equal(np.sort(g.get_state("x", p + 1), axis=None), want)
        o.destroy()


@pytest.mark.parametrize("which", [("shade", 8, 64), ("ccpso", 12, 8)], ids=["shade", "ccpso"])
def test_a_frozen_neighbour_disturbs_nobody(hip, oracle_lib, which):
    """population 2 is stopped after 3 generations; run(7) takes the others to generation 10, where
    they still match their oracle runs, and leaves population 2 bit for bit where it stood.  (SHADE:
    the host's one np schedule for all populations still covers the live ones while LPSR shrinks
    them.)"""
    c = bo.find(*which)
    frozen = 2
    g, objs = _pair(hip, oracle_lib, c)
    worst = bo.Worst()
    for gen in range(3):
        g.iterate()
        for o in objs:
            o.iterate()
        _compare_all(g, objs, c, "generation %d" % gen, worst)
    g.set_state("stop", [1.], population=frozen)
    before = bo.device_state(g, c, frozen)
    assert g.run(7) == 7
    for p, o in enumerate(objs):
        if p != frozen:
            for _ in range(7):
                o.iterate()
    _compare_all(g, objs, c, "generation 9", worst, skip=(frozen,))
    after = bo.device_state(g, c, frozen)
    for k in bo.keys_of(c):
        assert before[k].tobytes() == after[k].tobytes(), (k, "the stopped population moved")
    assert int(g.get_state("stop", frozen)[0]) == 1
    # the stopped population is where its oracle run was after generation 2, the others moved on
    bo.COMPARE[c["engine"]](bo.Compare(g, objs[frozen], frozen, "frozen at generation 2", worst), c)
    for p in range(c["P"]):
        assert int(g.get_state("stop", p)[0]) == (1 if p == frozen else 0)
    print("%s, population %d frozen after 3 of 10 generations: worst relative deviation of the others %s"
          % (c["id"], frozen, worst))
    for o in objs:
        o.destroy()


def _host_case(hip, engine, seed=3):
    ext = dict(seed=seed, populations=3)
    if engine == "shade":
        return hip.SHADE(mfev=10 ** 7, npinit=18, tol=1e-12, **ext), ("x", "f")
    if engine == "cso":
        return hip.CSO(mfev=10 ** 7, stol=1e-12, np=12, **ext), ("x", "f", "xbest")
    if engine == "apso":
        return hip.APSO(mfev=10 ** 7, tol=1e-12, np=70, **ext), ("x", "f", "xbest")     # two chunks of 48 and 22
    return hip.CCPSO(mfev=10 ** 7, sigmatol=1e-12, np=6, pps=[2, 3], **ext), ("x", "yhat", "fyhat")


@pytest.mark.parametrize("engine", ["shade", "cso", "apso", "ccpso"])
def test_python_objective_in_every_population(hip, engine):
    """the host-callback path (host_evaluate_rows: rows p np ld of every population) against the
    built-in objective of the same function: the same swarms after every generation in all three
    populations, at the tolerance of test_pso_gpu.py:146-148 (1e-12, equal fev), and exactly the
    summed fev calls of the callable"""
    n, P, gens = 6, 3, 8
    lo, up = bo.box(n)
    calls = [0]

    def sphere(x):
        calls[0] += 1
        return float(np.sum(np.asarray(x) ** 2))

    a, keys = _host_case(hip, engine)
    b, _ = _host_case(hip, engine)
    a.initialize(hip.objectives.sphere, lo, up, np.zeros((P, n)))
    b.initialize(sphere, lo, up, np.zeros((P, n)))
    worst = bo.Worst()
    for gen in range(gens):
        a.iterate()
        b.iterate()
        for p in range(P):
            for k in keys:
                u, v = a.get_state(k, p), b.get_state(k, p)
                assert u.shape == v.shape and u.size > 0
                err = np.abs(u - v).max() / max(np.abs(v).max(), 1e-300)
                worst.see(err, "generation %d population %d %s" % (gen, p, k))
                assert err <= 1e-12, (gen, p, k, err)
            assert int(a.get_state("fev", p)[0]) == int(b.get_state("fev", p)[0]), (gen, p)
    fev = sum(int(b.get_state("fev", p)[0]) for p in range(P))
    assert calls[0] == fev, (calls[0], fev)
    # three different runs, or the comparison above says nothing about p > 0
    assert not np.array_equal(b.get_state("x", 0), b.get_state("x", 1))
    assert not np.array_equal(b.get_state("x", 1), b.get_state("x", 2))
    print("%s, host callable against the built-in, 3 populations, %d generations, %d calls: worst relative "
          "deviation %s" % (engine, gens, calls[0], worst))


@pytest.mark.parametrize("algo", ["ActiveCMAES", "SepCMAES"])
def test_cma_normals_of_every_population(hip, oracle_lib, algo):
    """the recorded sampling normals of population p are the oracle's statement of sub-stream p
    (philox_normals_sub), bit for bit, in two generations"""
    from bboptpy_amd import _ffi
    n, lam, P, seed = 12, 24, 5, 987654321
    lo, up = bo.box(n)
    g = getattr(hip, algo)(mfev=10 ** 7, tol=1e-12, np=lam, seed=seed, populations=P)
    g.initialize(hip.objectives.sphere, lo, up, np.random.default_rng(2).uniform(-4., 4., (P, n)))
    g.set_state("record_normals", [1.0])
    for gen in range(2):
        it = int(g.get_state("it")[0])
        g.phase(_ffi.PHASE_SAMPLE_EVALUATE)
        seen = []
        for p in range(P):
            z = g.get_state("zlast", p)
            want = np.zeros(lam * n)
            oracle_lib.f("philox_normals_sub")(seed, p, it, lam, n, want)
            assert z.size == want.size
            assert z.tobytes() == want.tobytes(), (algo, gen, p)
            seen.append(z.copy())
        for p in range(1, P):
            assert not np.array_equal(seen[p], seen[p - 1])
        for ph in (_ffi.PHASE_RANK, _ffi.PHASE_UPDATE, _ffi.PHASE_EIGEN, _ffi.PHASE_HISTORY_STOP):
            g.phase(ph)
