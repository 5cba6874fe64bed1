"""Every fitness-ranking form against its one contract (bbo_rank.hpp) on TIED keys:

    rank[i] = #{ j : f_j < f_i  or  (f_j == f_i and j < i) },   order[rank[i]] = i

-- a total order, stable in the index, the same for every form.  The reference is numpy's stable argsort
of the fitness the handle holds; every comparison is exact.  The forms (enum RankKernel, read back through
the key `rank_route`) are reached at the smallest lengths that reach them and their seams: lane, thread,
wavefront, merge run, the 2048-key tile of the counting rank, the power-of-two padding of the sorts (whose
padding key (+inf, INT_MAX) meets real +inf here).  The expected routes below were written down from the
launch conditions as they read before the route function existed (CmaEngine::launch_rank,
DeEngine::launch_rank), not by calling that function.

The two tests without the `gpu` mark check the tables themselves on the host."""
import numpy as np
import pytest

# the key families and the reference, shared with test_select_ties_gpu.py
from _tie_families import FAMILIES, EDGES, family, groups, bits, reference

gpu = pytest.mark.gpu

# enum RankKernel (bbo_rank.hpp), in its order: the contract of the key `rank_route`
ROUTES = ("wave", "sort_bitonic256", "sort_bitonic_e1", "sort_bitonic_e2", "sort_bitonic_e4", "sort_bitonic_e8",
          "sort_merge2", "sort_merge4", "count8", "count32", "count64")
DBG_RANK_COUNT32, DBG_RANK_COUNT_NO64, DBG_RANK_BITONIC, DBG_NO_SMALL_FUSED = 128, 4096, 262144, 64

# ---- the case tables -------------------------------------------------------------------------------------
# CMA: (expected route, populations, lambda, dbg)
CMA_CASES = (
    [("wave", 7, L, 0) for L in (4, 5, 63, 64)]
    + [("sort_bitonic256", 7, L, 0) for L in (65, 255, 256)]
    + [("sort_bitonic_e1", 7, L, 0) for L in (257, 1000, 1024)]
    + [("sort_merge2", 7, L, 0) for L in (1025, 2047, 2048)]
    + [("sort_bitonic_e2", 7, L, DBG_RANK_BITONIC) for L in (1025, 2047, 2048)]
    + [("sort_merge4", 7, L, 0) for L in (2049, 4095, 4096)]
    + [("sort_bitonic_e4", 7, L, DBG_RANK_BITONIC) for L in (2049, 4095, 4096)]
    + [("sort_bitonic_e8", 7, L, 0) for L in (4097, 8191, 8192)]
    + [("count8", P, L, 0) for P in (1, 3) for L in (4, 33, 500)]
    + [("count8", 7, 8193, 0)]                                        # past SORT_LDS_MAX
    + [("count32", 1, L, 0) for L in (512, 2047)]
    + [("count8", 1, L, DBG_RANK_COUNT32) for L in (512, 2047)]
    + [("count64", 1, L, 0) for L in (2048, 2049, 4097)]              # the tile seam of 2048
    + [("count32", 1, L, DBG_RANK_COUNT_NO64) for L in (2048, 2049, 4097)]
)
# DE: (expected route, populations, npinit); the key count of a population is `rows`, below
DE_CASES = [("wave", 4, 64), ("sort_bitonic256", 4, 256), ("sort_bitonic_e1", 4, 1024), ("sort_merge2", 4, 2048),
            ("sort_merge4", 4, 4096), ("sort_bitonic_e8", 4, 8192), ("count8", 1, 40), ("count8", 1, 2049)]


def de_rows(npinit):
    return (npinit, npinit - 1, npinit // 2 + 1, 5)


HEES_NP = (2, 17, 1024, 1025, 4096)      # 2 mu keys: 2048 is one tile exactly, 2050 puts two into a second, 8192 is four
DSA_NP = (5, 33, 2049)
NORM_CASES = [(64, "wave", "count8"), (1000, "sort_bitonic_e1", "count32"), (2048, "sort_merge2", "count64")]


def all_lengths():
    Ls = {c[2] for c in CMA_CASES} | {r for c in DE_CASES for r in de_rows(c[2])}
    return sorted(Ls | {2 * m for m in HEES_NP} | set(DSA_NP) | {c[0] for c in NORM_CASES})


def test_every_route_is_the_expected_route_of_a_case():
    seen = {c[0] for c in CMA_CASES} | {c[0] for c in DE_CASES}
    assert seen == set(ROUTES)
    assert {c[0] for c in CMA_CASES} == set(ROUTES)          # (CMA alone reaches all of them)
    for P in (1, 2, 3, 4, 7):
        g = groups(P)
        assert all(len(h) == P for h in g) and {k for h in g for k in h} == set(range(7))


@pytest.mark.parametrize("L", all_lengths())
def test_families_hold_the_ties_they_claim(L):
    f = [family(k, L) for k in range(7)]
    for k in range(7):
        assert f[k].shape == (L,) and f[k].dtype == np.float64 and not np.isnan(f[k]).any()
        np.testing.assert_array_equal(bits(f[k]), bits(family(k, L)))      # a function of (k, L) alone
    const, parity, halves, few, desc, edges, distinct = f
    assert np.unique(bits(const)).size == 1
    assert (parity[0::2] == 0.).all() and (parity[1::2] == 1.).all() and L >= 4
    assert (halves[:L // 2] == 1.).all() and (halves[L // 2:] == 0.).all()
    assert np.isin(few, np.arange(8.)).all() and np.unique(few).size < L and few[0] == few[L - 1]
    assert (np.diff(desc) < 0).all()
    assert np.isin(bits(edges), bits(EDGES)).all()
    assert (edges == np.inf).sum() >= 2 and edges[0] == np.inf and edges[L - 1] == np.inf
    zero = edges == 0.
    assert (zero & np.signbit(edges)).sum() >= 1 and (zero & ~np.signbit(edges)).sum() >= 1
    if L >= 64:                             # every value is there, +inf in about a third of the entries
        assert np.unique(bits(edges)).size == 7 and 0.2 < (edges == np.inf).mean() < 0.5
    assert np.unique(distinct).size == L
    # the stable order is not the identity and not the reverse wherever there is a choice to get wrong
    for k in (1, 2, 3, 5):
        order, _ = reference(f[k])
        assert not np.array_equal(order, np.arange(L)) and not np.array_equal(order, np.arange(L)[::-1])


# ---- CMA --------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("variant", ["active", "cmaes"])
@pytest.mark.parametrize("route,P,lam,dbg", CMA_CASES,
                         ids=["%s-P%d-L%d%s" % (r, P, L, "-dbg" if d else "") for r, P, L, d in CMA_CASES])
def test_cma_ranking_is_the_stable_order(hip, variant, route, P, lam, dbg):
    """sample, replace the fitness by a family per population, rank: order, rank, the sorted values, the four
    extremes handed to the stop tests (`ybw`, `ibw`) and the evaluation count, in every population"""
    from bboptpy_amd import _ffi
    n = 2
    cls = hip.ActiveCMAES if variant == "active" else hip.CMAES
    for fams in groups(P):
        g = cls(mfev=10 ** 9, tol=1e-12, np=lam, seed=5, populations=P)
        g.initialize(hip.objectives.sphere, -5. * np.ones(n), 5. * np.ones(n), np.zeros((P, n)))
        if dbg:
            g.set_state("dbg", [float(dbg)])
        g.phase(_ffi.PHASE_SAMPLE_EVALUATE)
        fev0 = [int(g.get_state("fev", p)[0]) for p in range(P)]
        for p, k in enumerate(fams):
            g.set_state("fitness", family(k, lam), p)
        g.phase(_ffi.PHASE_RANK)
        assert ROUTES[int(g.get_state("rank_route")[0])] == route
        for p, k in enumerate(fams):
            msg = "%s, lambda = %d, %s, population %d" % (FAMILIES[k], lam, route, p)
            f = g.get_state("fitness", p)
            np.testing.assert_array_equal(bits(f), bits(family(k, lam)), err_msg=msg)
            order, rank = reference(f)
            np.testing.assert_array_equal(g.get_state("fit_idx", p), order, err_msg=msg)
            np.testing.assert_array_equal(g.get_state("rank", p), rank, err_msg=msg)
            np.testing.assert_array_equal(bits(g.get_state("fit_val", p)), bits(f[order]), err_msg=msg)
            assert int(g.get_state("ibest", p)[0]) == order[0], msg
            ends = order[[0, 1, lam - 2, lam - 1]]
            np.testing.assert_array_equal(g.get_state("ibw", p), ends, err_msg=msg)
            np.testing.assert_array_equal(bits(g.get_state("ybw", p)), bits(f[ends]), err_msg=msg)
            assert int(g.get_state("fev", p)[0]) == fev0[p] + lam, msg


@gpu
def test_cma_set_fitness_takes_nan_as_inf(hip):
    """no NaN reaches a ranking: set_state("fitness") stores +inf for it, like every evaluation path, and the
    entry ranks by its index among the other +inf"""
    from bboptpy_amd import _ffi
    lam = 9
    f = np.array([np.inf, 1., np.nan, -np.inf, np.inf, np.nan, 0., np.inf, 1.])
    for cls in (hip.CMAES, hip.ActiveCMAES, hip.SepCMAES):
        g = cls(mfev=10 ** 9, tol=1e-12, np=lam, seed=1)
        g.initialize(hip.objectives.sphere, -np.ones(2), np.ones(2), np.zeros(2))
        g.phase(_ffi.PHASE_SAMPLE_EVALUATE)
        g.set_state("fitness", f)
        g.phase(_ffi.PHASE_RANK)
        np.testing.assert_array_equal(bits(g.get_state("fitness")), bits(np.where(np.isnan(f), np.inf, f)))
        np.testing.assert_array_equal(g.get_state("fit_idx"), [3, 6, 1, 8, 0, 2, 4, 5, 7])


# ---- DE ---------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("which", range(4), ids=["all", "all-1", "half+1", "5"])
@pytest.mark.parametrize("route,P,npinit", DE_CASES, ids=["%s-P%d-np%d" % c for c in DE_CASES])
def test_de_ranking_is_the_stable_order(hip, route, P, npinit, which):
    """SHADE: the sort is sized by npinit, the keys of a population are its first `rows` <= npinit.  Rows
    tagged x[i, 0] = i come back from get_state("x") in ranked order."""
    n = 2
    for rows in (de_rows(npinit)[which],):
        for fams in groups(P):
            g = hip.SHADE(mfev=10 ** 9, npinit=npinit, tol=1e-12, seed=3, populations=P)
            g.initialize(hip.objectives.sphere, -5. * np.ones(n), 5. * np.ones(n), np.zeros((P, n)))
            X = np.zeros((rows, n))
            X[:, 0] = np.arange(rows)
            for p in range(P):
                g.set_state("x", X, p)
            for p, k in enumerate(fams):
                g.set_state("f", family(k, rows), p)
            assert ROUTES[int(g.get_state("rank_route")[0])] == route
            for p, k in enumerate(fams):
                msg = "%s, %d of %d rows, %s, population %d" % (FAMILIES[k], rows, npinit, route, p)
                f = family(k, rows)
                order, _ = reference(f)
                assert int(g.get_state("np", p)[0]) == rows, msg
                np.testing.assert_array_equal(g.get_state("x", p).reshape(rows, n)[:, 0], order, err_msg=msg)
                np.testing.assert_array_equal(bits(g.get_state("f", p)), bits(f[order]), err_msg=msg)


# ---- HEES ---------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("P", [1, 2])
@pytest.mark.parametrize("mu", HEES_NP)
def test_hees_ranking_is_the_stable_order(hip, mu, P):
    """a callback objective that returns the next value of the family; the first value of every population
    is NaN, which must be stored as +inf and rank first among the +inf (it has the lowest index).
    At most 4 handles x 2 x 8192 + a few calls of the callback."""
    from bboptpy_amd import _ffi
    n, L = 2, 2 * mu
    for fams in groups(P):
        queue = []

        def f_next(x):
            return queue.pop() if queue else 0.         # (the mean's evaluations outside the sampling: 0)

        g = hip.HEES(10 ** 9, 0., np=mu, seed=2, populations=P)
        g.initialize(f_next, -5. * np.ones(n), 5. * np.ones(n), np.zeros((P, n)))
        want = []
        for k in fams:
            v = family(k, L)
            v[0] = np.nan
            queue.extend(v)
            v[0] = np.inf
            want.append(v)
        queue.reverse()
        g.phase(_ffi.HEES_PHASE_SAMPLE)
        assert not queue                                 # every value was handed out, population by population
        g.phase(_ffi.HEES_PHASE_RANK)
        for p, k in enumerate(fams):
            msg = "%s, 2 mu = %d, population %d" % (FAMILIES[k], L, p)
            f = g.get_state("fit_val", p)
            np.testing.assert_array_equal(bits(f), bits(want[p]), err_msg=msg)
            order, rank = reference(f)
            np.testing.assert_array_equal(g.get_state("fit_idx", p), order, err_msg=msg)
            np.testing.assert_array_equal(g.get_state("fit_rank", p), rank, err_msg=msg)
            assert int(g.get_state("fit_rank", p)[0]) == L - int((f == np.inf).sum()), msg


# ---- DSA ----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("P", [1, 2])
@pytest.mark.parametrize("npop_size", DSA_NP)
def test_dsa_ranking_is_the_stable_order(hip, npop_size, P):
    """the pool's order of the generation that follows set_state("f") (method 1 is one of the two that sort)"""
    n, L = 2, npop_size
    for fams in groups(P):
        g = hip.DSA(10 ** 9, 0., 0., L, seed=4, populations=P)
        g.initialize(hip.objectives.sphere, -5. * np.ones(n), 5. * np.ones(n), np.zeros((P, n)))
        g.set_state("force_method", [1.])
        for p, k in enumerate(fams):
            g.set_state("f", family(k, L), p)
        held = [g.get_state("f", p).copy() for p in range(P)]
        g.iterate()
        for p, k in enumerate(fams):
            msg = "%s, np = %d, population %d" % (FAMILIES[k], L, p)
            np.testing.assert_array_equal(bits(held[p]), bits(family(k, L)), err_msg=msg)
            np.testing.assert_array_equal(g.get_state("fit_idx", p), reference(held[p])[0], err_msg=msg)


# ---- the norms handed down with the ranking ---------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("lam,batch_route,single_route", NORM_CASES, ids=["L%d" % c[0] for c in NORM_CASES])
def test_whitened_norms_follow_the_ranking_on_ties(hip, lam, batch_route, single_route):
    """ActiveCMAES, no box, initial state (C = I): the whitened norms of the worst mu are the sampler's
    sigma^2 ||z||^2 gathered THROUGH the ranking (cma_rank_body, cma_rank_sort; behind the one-wavefront
    form, which does not write them, cma_whiten gathers them through `order` in the update phase -- there
    ycoeff is read after PHASE_UPDATE, everything else before it).  With C = I, sigma^2 ||z||^2 =
    ||x - xmean||^2, so from arx, xmean and the stable order:
        S_ref[r] = ||arx[order_ref[lambda - mu + r]] - xmean||^2,  ycoeff_ref[i] = S_ref[i] / max(S_ref[mu-1-i], 1e-8)
    to 1e-12 relative: a three-term sum and a quotient round to a few ulp (the mean is 0, so x - xmean is
    exact), a wrong choice among tied candidates changes the value by order one (the rows are distinct
    draws).  n = 3 has ld = 16 and takes cma_sample_eval64, which writes zn2 (use_zn = 1 without a box); were
    that not so, S would still hold the zeros of init() behind the counting and sorting forms and the
    comparison would fail.  Population 0 of the batch and the single run of the same seed: the same bits."""
    from bboptpy_amd import _ffi
    n, seed = 3, 11
    got = {}
    for P, route in ((4, batch_route), (1, single_route)):
        g = hip.ActiveCMAES(mfev=10 ** 9, tol=1e-12, np=lam, seed=seed, populations=P)
        g.initialize(hip.objectives.sphere, -5. * np.ones(n), 5. * np.ones(n), np.zeros((P, n)))
        g.phase(_ffi.PHASE_SAMPLE_EVALUATE)
        for p in range(P):
            g.set_state("fitness", family((3, 1, 2, 0)[p], lam), p)          # few, parity, halves, constant
        g.phase(_ffi.PHASE_RANK)
        assert ROUTES[int(g.get_state("rank_route")[0])] == route
        mu = int(g.get_state("mu")[0])
        state = [(g.get_state("arx", p).reshape(lam, n), g.get_state("xmean", p), g.get_state("fitness", p))
                 for p in range(P)]
        if route == "wave":
            g.phase(_ffi.PHASE_UPDATE)
        for p, (arx, xmean, f) in enumerate(state):
            order, _ = reference(f)
            np.testing.assert_array_equal(g.get_state("fit_idx", p), order)
            S = ((arx[order[lam - mu:]] - xmean) ** 2).sum(axis=1)
            assert S.min() > 1e-6 and np.unique(S).size == mu        # distinct rows, far above the floor
            y = g.get_state("ycoeff", p)
            np.testing.assert_allclose(y, S / np.maximum(S[::-1], 1e-8), rtol=1e-12, atol=0,
                                       err_msg="lambda = %d, %s, population %d" % (lam, route, p))
            if p == 0:
                got[P] = y.copy()
    np.testing.assert_array_equal(bits(got[4]), bits(got[1]))


# ---- ties the device produces itself, the fused small-generation kernel included -------------------------------------
TIE_SEED = 277


@gpu
@pytest.mark.parametrize("variant", ["active", "cmaes"])
@pytest.mark.parametrize("P", [1, 5])
@pytest.mark.parametrize("lam", [6, 33, 64])
def test_clamped_candidates_tie_and_both_generation_forms_agree(hip, variant, lam, P):
    """Sphere on the box [1, 3]^2 from the mean (1.5, 1.5): the optimum lies outside, candidates clamp onto
    the corner (1, 1) with f = 2.0 exactly and tie at the best ranks.  Five generations, one iterate() each,
    by cma_small_generations (the default) and by the nine-kernel sequence (dbg = 64): after each, every key
    that test_fused_small_generations_equal_the_kernel_sequence compares is bit-equal between the two, and
    both hold fit_idx = the stable argsort of their fitness.

    Seed 277 was picked with the CPU oracle (oracle/pyoracle.py, Philox normals, this seed, bound = True),
    whose population 0 alone meets the condition "at least two bit-equal fitness values in each of the five
    generations".  Its counts per generation, values that share their bits with another / values equal to 2.0:
        lambda =  6: 5/2, 2/2, 3/3, 3/3, 2/2                (both variants)
        lambda = 33: 17/7, 8/8, 10/10, 12/12, 11/11         (CMAES: 12/12 in the fifth)
        lambda = 64: 30/13, 23/23, 28/28, 36/36, 31/31      (both variants)
    The test asserts the condition on the device's own fitness."""
    n = 2
    cls = hip.ActiveCMAES if variant == "active" else hip.CMAES
    keys = ("xmean", "sigma", "pc", "ps", "C", "B", "D", "invsqrtC", "arx", "fitness", "fit_idx", "it", "fev", "flag",
            "best_hist", "kth_hist", "fbest", "fworst")

    def make(dbg):
        g = cls(mfev=10 ** 7, tol=1e-12, np=lam, seed=TIE_SEED, populations=P, bound=True)
        g.initialize(hip.objectives.sphere, np.ones(n), 3. * np.ones(n), 1.5 * np.ones((P, n)))
        if dbg:
            g.set_state("dbg", [float(dbg)])
        return g

    a, b = make(0), make(DBG_NO_SMALL_FUSED)
    for gen in range(5):
        a.iterate()
        b.iterate()
        for p in range(P):
            for key in keys:
                np.testing.assert_array_equal(bits(a.get_state(key, p)), bits(b.get_state(key, p)),
                                              err_msg="%s, generation %d, population %d" % (key, gen, p))
            for g in (a, b):
                f = g.get_state("fitness", p)
                np.testing.assert_array_equal(g.get_state("fit_idx", p), reference(f)[0],
                                              err_msg="generation %d, population %d" % (gen, p))
        f0 = a.get_state("fitness", 0)
        assert np.unique(bits(f0)).size <= lam - 1, "generation %d: no two fitness values tie" % gen
        assert (f0 == 2.0).sum() >= 2, "generation %d: fewer than two candidates on the corner" % gen
    assert int(a.get_state("it")[0]) == 5
