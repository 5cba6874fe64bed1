"""The covariance update formed by the fixed-shape batch eigensolver of n = ld = 128 on its load
(cma_eigen_fx128) against the unfused pair it replaces in a generation -- cma_cov, then the same
eigensolver without the prologue, cma_eigen_fx128u -- which diagnostic bit 32 keeps.  The element's
expression and the order of the Gram slabs are the same, so everything is compared bit for bit: two
handles with the same seed, one with the bit, after every generation.  33 and 40 populations: the
smallest batches above eig_split_maxp = 32; lambda = 16, 64, 512 give 1, 2 and 16 (P = 33) or 8 (P = 40)
Gram slabs, BBO_GRAM_WANT 3, 6 and 5, so the slab loop's steps of four, two and one are taken in every
combination.  The split form of at most 32 populations (cma_eigen_r1_fx128) is not fused -- one workgroup
summing one population's slabs was slower than cma_cov's 33 -- and is held to exactly that."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 128
UNFUSED = 32
GENS = 6
KEYS = ("C", "B", "D", "BD", "xmean", "sigma", "pc", "ps", "fitness", "it", "fev", "flag")


def _handle(hip, lam, pops, dbg=0, seed=5, algo="ActiveCMAES", **kw):
    g = getattr(hip, algo)(mfev=10 ** 9, tol=1e-14, np=lam, seed=seed, populations=pops, **kw)
    rng = np.random.default_rng(pops * 1000 + lam)
    g.initialize(hip.objectives.rosenbrock, -5. * np.ones(N), 5. * np.ones(N), rng.uniform(-2., 2., (pops, N)))
    if dbg:
        g.set_state("dbg", [float(dbg)])
    return g


def _pair(hip, lam, pops, seed=5, **kw):
    return _handle(hip, lam, pops, 0, seed, **kw), _handle(hip, lam, pops, UNFUSED, seed, **kw)


def _state(g, pops, keys=KEYS):
    return {k: np.stack([g.get_state(k, p) for p in range(pops)]) for k in keys}


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _assert_same(a, b, what, pops=None):
    for k in a:
        for p in (range(a[k].shape[0]) if pops is None else pops):
            assert _bits_equal(a[k][p], b[k][p]), (what, k, p)


def _step(g, mode):
    if mode == "run":
        assert g.run(1) == 1
    else:
        g.iterate()


def _forms(f, u):
    assert int(f.get_state("cov_fused")[0]) == 1 and int(u.get_state("cov_fused")[0]) == 0
    assert int(f.get_state("eig_fixed128")[0]) == 1 and int(u.get_state("eig_fixed128")[0]) == 1


@pytest.mark.parametrize("mode", ["run", "iterate"])
@pytest.mark.parametrize("pops", [33, 40])
@pytest.mark.parametrize("lam", [16, 64, 512])
def test_fused_equals_unfused_after_every_generation(hip, lam, pops, mode):
    f, u = _pair(hip, lam, pops)
    if pops == 33:
        # the slab loop: its single step alone, its step of two alone, four steps of four
        assert int(f.get_state("splits")[0]) == {16: 1, 64: 2, 512: 16}[lam]
    before = _state(f, pops, ("C",))
    for gen in range(GENS):
        _step(f, mode)
        _step(u, mode)
        _forms(f, u)
        sf, su = _state(f, pops), _state(u, pops)
        _assert_same(sf, su, "lambda %d, %d populations, %s, generation %d" % (lam, pops, mode, gen))
    assert not np.array_equal(before["C"], sf["C"])


@pytest.mark.parametrize("lam,want,slabs", [(512, 3, 3), (512, 7, 6), (160, 5, 5)])
def test_other_slab_counts(hip, monkeypatch, lam, want, slabs):
    """three slabs: a step of two, then the single step; six: four and two; five: four and one"""
    monkeypatch.setenv("BBO_GRAM_WANT", str(want))
    f, u = _pair(hip, lam, 33)
    assert int(f.get_state("splits")[0]) == slabs and int(u.get_state("splits")[0]) == slabs
    for gen in range(3):
        f.iterate()
        u.iterate()
        _forms(f, u)
        _assert_same(_state(f, 33), _state(u, 33), "%d slabs, generation %d" % (slabs, gen))


@pytest.mark.parametrize("algo,kw", [("ActiveCMAES", {"eigenrate": 10.}), ("CMAES", {})])
def test_generation_without_decomposition_still_updates_c(hip, algo, kw):
    """lambda = 16: the decomposition is not due every generation (cmaes.cpp:233: every fifth with the
    plain variant's constants, which also take the other branch of `decay`; every fourth or so with
    the active variant at eigenrate = 10), and population 2 is held back for good; C moves all the
    same, to the bits of cma_cov"""
    pops = 33
    f, u = _pair(hip, 16, pops, algo=algo, **kw)
    assert float(f.get_state("eigenfreq")[0]) > 16.
    skipped = 0
    for gen in range(GENS):
        if gen == 2:
            for g in (f, u):
                g.set_state("eigenlastev", [10 ** 8], 2)
        bf = _state(f, pops, ("C", "B"))
        f.iterate()
        u.iterate()
        _forms(f, u)
        sf, su = _state(f, pops, KEYS + ("eigen_done",)), _state(u, pops, KEYS + ("eigen_done",))
        _assert_same(sf, su, "generation %d" % gen)
        for p in range(pops):
            if int(sf["eigen_done"][p][0]) == 0:
                skipped += 1
                assert _bits_equal(bf["B"][p], sf["B"][p]), (gen, p)
                assert not np.array_equal(bf["C"][p], sf["C"][p]), (gen, p)
                assert _bits_equal(sf["C"][p], su["C"][p]), (gen, p)
        if gen >= 2:
            assert int(sf["eigen_done"][2][0]) == 0
    # (beside population 2 from generation 2 on: every population on the generations between two
    # decompositions)
    assert skipped > GENS - 2


def test_stopped_population_is_left_alone(hip):
    """run() honours the stop flag: the stopped population keeps C, B and D in both forms"""
    pops, frozen = 33, 7
    f, u = _pair(hip, 16, pops)
    out = []
    for g in (f, u):
        assert g.run(2) == 2
        g.set_state("stop", [1], frozen)
        g.set_state("eigenlastev", [0], frozen)        # (its decomposition would be due)
        before = _state(g, pops, ("C", "B", "D"))
        assert g.run(3) == 3
        after = _state(g, pops)
        for k in before:
            assert _bits_equal(before[k][frozen], after[k][frozen]), k
            assert not np.array_equal(before[k][0], after[k][0]), k
        out.append(after)
    _forms(f, u)
    _assert_same(out[0], out[1], "beside a stopped population")


def test_both_values_of_hsig(hip):
    """a path ps far too long for its generation count: hsig = 0 and the c2 term enters"""
    pops, long_ps = 33, 4
    f, u = _pair(hip, 64, pops)
    for g in (f, u):
        g.iterate()
        g.set_state("ps", 1e3 * np.ones(N), long_ps)
    for gen in range(2):
        f.iterate()
        u.iterate()
        sf, su = _state(f, pops, KEYS + ("hsig",)), _state(u, pops, KEYS + ("hsig",))
        assert int(sf["hsig"][long_ps][0]) == 0
        assert (np.delete(sf["hsig"][:, 0], long_ps) == 1).any()
        _assert_same(sf, su, "generation %d" % gen)
    _forms(f, u)


def test_nan_entry_gives_the_same_bits_in_both_forms(hip):
    """a NaN in C reaches the update, the decomposition (its guards apply), the sampler and with the
    next generation the Gram slabs"""
    pops, bad = 33, 3
    f, u = _pair(hip, 64, pops)
    for g in (f, u):
        g.iterate()
        c = g.get_state("C", bad).reshape(N, N).copy()
        c[17, 5] = c[5, 17] = np.nan
        g.set_state("C", c, bad)
        g.set_state("eigenlastev", [0], bad)
    for gen in range(3):
        f.iterate()
        u.iterate()
        sf, su = _state(f, pops), _state(u, pops)
        assert np.isnan(sf["C"][bad]).any()
        assert np.isfinite(sf["C"][0]).all()
        _assert_same(sf, su, "generation %d" % gen)
    _forms(f, u)


@pytest.mark.parametrize("pops", [1, 3])
def test_split_form_keeps_cma_cov(hip, pops):
    f = _handle(hip, 64, pops)
    before = f.get_state("C", 0)
    for mode in ("run", "iterate"):
        _step(f, mode)
        assert int(f.get_state("cov_fused")[0]) == 0 and int(f.get_state("eig_fixed128")[0]) == 1
    assert not np.array_equal(before, f.get_state("C", 0))


def test_phase_by_phase_ends_a_generation_like_iterate(hip, pops=33):
    """phase() launches cma_cov and the unfused eigensolver; iterate() the fused one"""
    from bboptpy_amd import _ffi
    f, ph = _handle(hip, 64, pops), _handle(hip, 64, pops)
    for gen in range(3):
        f.iterate()
        for which in (_ffi.PHASE_SAMPLE_EVALUATE, _ffi.PHASE_RANK, _ffi.PHASE_UPDATE):
            ph.phase(which)
        # (C after the cov phase is C after the fused prologue)
        sf = _state(f, pops, ("C",))
        idle = [p for p in range(pops) if int(f.get_state("eigen_done", p)[0]) == 0]
        _assert_same(sf, _state(ph, pops, ("C",)), "C after the cov phase, generation %d" % gen, idle)
        ph.phase(_ffi.PHASE_EIGEN)
        ph.phase(_ffi.PHASE_HISTORY_STOP)
        assert int(f.get_state("cov_fused")[0]) == 1 and int(ph.get_state("cov_fused")[0]) == 0
        _assert_same(_state(f, pops), _state(ph, pops), "generation %d" % gen)
