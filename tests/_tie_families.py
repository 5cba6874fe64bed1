"""The key families of the tie tests (test_rank_ties_gpu.py, test_select_ties_gpu.py): functions of the
length, a seeded generator, and nothing else; and the reference they are held to, numpy's stable argsort.
A plain module: no fixture, no pytest setting."""
import numpy as np

FAMILIES = ("constant", "parity", "halves", "few", "descending", "edges", "distinct")
EDGES = np.array([-np.inf, -1.797e308, -0.0, 0.0, 5e-324, 1.797e308, np.inf])


def family(k, L):
    """family k at length L >= 4"""
    name, rng = FAMILIES[k], np.random.default_rng([k, L])
    i = np.arange(L)
    if name == "constant":
        return np.full(L, 3.25)
    if name == "parity":
        return (i % 2).astype(np.float64)
    if name == "halves":
        return np.where(i < L // 2, 1., 0.)
    if name == "few":                       # long runs of ties across every seam; the ends tie whatever was drawn
        f = rng.integers(0, 8, L).astype(np.float64)
        f[L - 1] = f[0]
        return f
    if name == "descending":
        return (L - i).astype(np.float64)
    if name == "edges":                     # +inf in about a third of the entries: real +inf ties the padding key
        f = EDGES[rng.choice(7, size=L, p=[1 / 9.] * 6 + [1 / 3.])]
        f[0], f[1], f[2], f[L - 1] = np.inf, -0.0, 0.0, np.inf
        return f
    return rng.standard_normal(L)           # the control


def groups(P):
    """the seven families over handles of P populations (population p of a handle gets the p-th of its group;
    the last group wraps round to fill its handle)"""
    return [[(i + k) % 7 for k in range(P)] for i in range(0, 7, P)]


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def reference(f):
    order = np.argsort(f, kind="stable")
    rank = np.empty_like(order)
    rank[order] = np.arange(f.size)
    return order, rank


def check_family_claims(L):
    """what the families claim at length L: the ties, the edge values, and a stable order that is neither the
    identity nor the reverse wherever there is a choice to get wrong"""
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
    for k in (1, 2, 3, 5):
        order, _ = reference(f[k])
        assert not np.array_equal(order, np.arange(L)) and not np.array_equal(order, np.arange(L)[::-1])
