"""No device: the order in which the TRANSPOSED tile of cma_sample_eval128 adds an objective's terms
(eval_frag_cols, bbo_objectives.hpp), restated in NumPy and held to the bit to the row layout's order
(eval_frag_rows; the model of tests/test_frag_objectives_gpu.py, restated here, not imported).

Row layout: the 16 lanes of a DPP row share a candidate, lane c holds the coordinates 16 t + c, adds
their terms in ascending t into a_c, and the 16 sums meet as v += ror8; ror4; ror2; ror1.
Transposed: lane group fk = lane >> 4 holds the coordinates 16 t + 4 fk + r, r = 0..3, of ONE
candidate.  a[r], ascending in t, is a_c of class c = 4 fk + r.  Then
    s[r] = a[r] + (a[r] of the lanes 32 away)          group fk ^ 2
    q[r] = s[r] + (s[r] of the lanes 16 away)          group fk ^ 1
    F    = (q[0] + q[2]) + (q[1] + q[3])
and group 0 stores F.  Rosenbrock's right-hand neighbour is in the lane for r < 3; for r = 3 it is
the value the lanes 16 higher (group (fk + 1) mod 4) OFFER: their first coordinate of the tile, but
group 0 offers its first coordinate of the NEXT tile (the last tile: anything, the term adds 0.).
Every product and sum is an operation of its own (-ffp-contract=off), as in NumPy."""
import math

import numpy as np
import pytest

N, NT, ROWS = 128, 8, 2000
OBJECTIVES = ("sphere", "rosenbrock", "ellipsoid", "cigar", "discus")


def _aux_ellipsoid(n):
    return np.array([math.pow(10., 6. * (i / (n - 1))) for i in range(n)])


# ---- the row layout (eval_frag_rows) ----------------------------------------------------------
def _ror(v, k):
    return np.roll(v, k, axis=-1)            # row_ror:k -- lane i reads lane (i - k) mod 16


def _row_sum(v):
    for k in (8, 4, 2, 1):
        v = v + _ror(v, k)
    return v


def _rows_model(obj, X):
    rows, n = X.shape
    Xp = np.zeros((rows, n + 1))
    Xp[:, :n] = X
    c0 = np.arange(16)
    a = np.zeros((rows, 16))
    aux = _aux_ellipsoid(n)
    for t in range(n // 16):
        j = 16 * t + c0
        x = Xp[:, j]
        if obj == "sphere":
            a = a + x * x
        elif obj == "rosenbrock":
            tt = Xp[:, j + 1] - x * x
            u = 1. - x
            a = a + np.where((j + 1 < n)[None, :], 100. * (tt * tt) + u * u, 0.)
        elif obj == "ellipsoid":
            a = a + aux[j][None, :] * (x * x)
        else:
            a = a + np.where((j > 0)[None, :], x * x, 0.)
    a = _row_sum(a)
    if obj in ("cigar", "discus"):
        x0 = _row_sum(np.where((c0 == 0)[None, :], Xp[:, :16], 0.))
        a = x0 * x0 + 1.0e6 * a if obj == "cigar" else 1.0e6 * (x0 * x0) + a
    return a[:, 0].copy()


# ---- the transposed tile (eval_frag_cols) -----------------------------------------------------
def _cols_model(obj, X):
    rows = X.shape[0]
    x = X.reshape(rows, NT, 4, 4)            # x[row, t, fk, r] = coordinate 16 t + 4 fk + r
    aux = _aux_ellipsoid(N).reshape(NT, 4, 4)
    a = np.zeros((rows, 4, 4))               # a[row, fk, r]
    for t in range(NT):
        xt = x[:, t]
        if obj == "sphere":
            a = a + xt * xt
        elif obj == "rosenbrock":
            offer = xt[:, :, 0].copy()                       # what each group offers the lanes 16 below it
            offer[:, 0] = x[:, min(t + 1, NT - 1), 0, 0]
            xn = np.empty_like(xt)
            xn[:, :, :3] = xt[:, :, 1:]
            xn[:, :, 3] = np.roll(offer, -1, axis=1)         # group fk reads group (fk + 1) mod 4
            tt = xn - xt * xt
            u = 1. - xt
            term = 100. * (tt * tt) + u * u
            if t == NT - 1:
                term[:, 3, 3] = 0.                           # coordinate 127 has no neighbour
            a = a + term
        elif obj == "ellipsoid":
            a = a + aux[t][None] * (xt * xt)
        else:
            sq = xt * xt
            if t == 0:
                sq[:, 0, 0] = 0.                             # coordinate 0 enters as x0 below
            a = a + sq
    s = a + a[:, [2, 3, 0, 1]]               # the lanes 32 away
    q = s + s[:, [1, 0, 3, 2]]               # the lanes 16 away
    f = (q[:, :, 0] + q[:, :, 2]) + (q[:, :, 1] + q[:, :, 3])
    if obj in ("cigar", "discus"):
        x0 = x[:, 0, 0, 0]
        f0 = f[:, 0]
        return x0 * x0 + 1.0e6 * f0 if obj == "cigar" else 1.0e6 * (x0 * x0) + f0
    # every group ends with the same bits (a + b = b + a at both exchanges)
    assert all(np.array_equal(f[:, 0].view(np.uint64), f[:, g].view(np.uint64)) for g in (1, 2, 3))
    return f[:, 0].copy()


def _rows():
    """2000 candidates whose coordinates spread over 16 decades, both signs: no two orders of a sum
    of their terms agree by accident"""
    rng = np.random.default_rng(11)
    X = rng.uniform(-1., 1., (ROWS, N)) * 10. ** rng.uniform(-8., 8., (ROWS, N))
    X[0] = 0.                                # all-zero row: the signs of the zero sums
    X[1, 0] = -0.
    return X


@pytest.mark.parametrize("obj", OBJECTIVES)
def test_transposed_order_gives_the_row_order_bits(obj):
    X = _rows()
    want = _rows_model(obj, X)
    got = _cols_model(obj, X)
    assert np.isfinite(want).all()
    bad = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]
    print("%s: %d of %d rows differ" % (obj, bad.size, ROWS))
    assert bad.size == 0, (obj, bad[:4], got[bad[:4]], want[bad[:4]])


def test_the_models_are_the_objectives():
    """(up to the order of the sums: both restatements against the package's plain formulas)"""
    import bboptpy_amd as bb
    X = np.random.default_rng(1).uniform(-3, 3, (5, N))
    for obj in OBJECTIVES:
        want = np.array([getattr(bb.objectives, obj)(x) for x in X])
        np.testing.assert_allclose(_rows_model(obj, X), want, rtol=1e-12)
        np.testing.assert_allclose(_cols_model(obj, X), want, rtol=1e-12)


def test_lds_copy_permutation_is_a_transpose_of_the_index():
    """position m of a run of 16 takes source position 4 (m & 3) + (m >> 2): an involution, and operand
    row fk + 4 r of a block is then coordinate 4 fk + r of it"""
    m = np.arange(16)
    src = 4 * (m & 3) + (m >> 2)
    assert np.array_equal(src[src], m)
    for fk in range(4):
        for r in range(4):
            assert src[fk + 4 * r] == 4 * fk + r
