"""cma_gram128s takes its per-row coefficients from the table cma_rank_sort leaves with the ranking
 where that ranking vouches for it, and looks them up itself otherwise.  Both
forms, and the LDS-staged cma_gram128 (diagnostic bit 512), form the same products in the same order:
after four generations every population's state is bit-identical.  The shapes are the smallest that
reach each branch; `gram_coef_stamp` says which one a run took.

With the default slab geometry these small shapes are cut into slabs of ONE 32-row chunk (512
workgroups are aimed at), so the chunk loop's look-ahead never carries a value into a sweep.  The
first two shapes therefore run a second time as one slab per population (BBO_GRAM_WANT=1, the
tuning variable CmaEngine::init reads): 8 and 32 chunks, the look-ahead wraps, the last chunk of
lambda = 1000 is ragged inside a long slab."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GRAM128_LDS = 512             # CmaDbg: DBG_GRAM128_LDS
GRAM_LOOKUP = 1073741824      # CmaDbg: DBG_GRAM_LOOKUP
GENS = 4

CASES = [
    # algo, n, lambda, P, box, table path expected, slabs wanted (None: the default geometry)
    pytest.param("ActiveCMAES", 128, 256, 4, False, True, None, id="sort"),
    pytest.param("ActiveCMAES", 128, 256, 4, False, True, 1, id="sort-one-slab-8-chunks"),
    pytest.param("ActiveCMAES", 128, 1000, 4, False, True, None, id="ragged-last-chunk"),    # lambda_pad = 1008
    pytest.param("ActiveCMAES", 128, 1000, 4, False, True, 1, id="ragged-one-slab-32-chunks"),
    pytest.param("CMAES", 120, 300, 4, False, True, None, id="n-below-ld-no-negative"),
    pytest.param("ActiveCMAES", 128, 256, 4, True, False, None, id="box-norms-from-whiten"),
    pytest.param("ActiveCMAES", 128, 256, 4, True, False, 1, id="box-one-slab-8-chunks"),
    pytest.param("ActiveCMAES", 128, 256, 2, False, False, None, id="counting-rank"),
    pytest.param("ActiveCMAES", 128, 64, 8, False, False, None, id="wave-rank"),
]


def _handle(hip, algo, n, lam, pops, box, dbg):
    g = getattr(hip, algo)(mfev=10 ** 9, tol=1e-14, np=lam, seed=11, populations=pops, bound=box)
    rng = np.random.default_rng(pops * 1000 + lam)
    # (a box the clamp bites into: sigma0 = 2 around points within a unit of its faces)
    half = 2.5 if box else 5.
    g.initialize(hip.objectives.rosenbrock, -half * np.ones(n), half * np.ones(n), rng.uniform(-2., 2., (pops, n)))
    if dbg:
        g.set_state("dbg", [float(dbg)])
    return g


def _state(g, pops):
    return {(key, p): g.get_state(key, p).copy() for key in ("C", "xmean", "sigma", "arx") for p in (0, pops - 1)}


@pytest.mark.parametrize("algo,n,lam,pops,box,table,want", CASES)
def test_table_lookup_and_lds_forms_agree_bit_for_bit(hip, monkeypatch, algo, n, lam, pops, box, table, want):
    if want is not None:
        monkeypatch.setenv("BBO_GRAM_WANT", str(want))
    else:
        monkeypatch.delenv("BBO_GRAM_WANT", raising=False)
    runs = {}
    for name, dbg in (("default", 0), ("lds", GRAM128_LDS), ("lookup", GRAM_LOOKUP)):
        g = _handle(hip, algo, n, lam, pops, box, dbg)
        assert g.run(GENS) == GENS
        runs[name] = (_state(g, pops), [int(g.get_state("gram_coef_stamp", p)[0]) for p in range(pops)],
                      [int(g.get_state("it", p)[0]) for p in range(pops)], int(g.get_state("splits")[0]))
    state, stamps, its, splits = runs["default"]
    assert its == [GENS] * pops
    # the branch this case is here for: the last generation's ranking stamped its table, or no ranking ever did
    assert stamps == ([GENS] * pops if table else [0] * pops), stamps
    assert runs["lookup"][1] == [0] * pops, runs["lookup"][1]
    if want is not None:
        assert splits == want and lam >= 3 * 32 * want, splits      # at least three chunks a slab
    for name in ("lds", "lookup"):
        for key, ref in state.items():
            assert np.isfinite(ref).all(), key
            np.testing.assert_array_equal(runs[name][0][key], ref, err_msg="%s: %s of population %d" % ((name,) + key))
