"""One per-coordinate box shared by every test that holds an engine's box handling to bounds
that bind (plain helper module, no tests of its own).

Three coordinate classes by j % 3; every value is a multiple of 1/1024 and so exact in fp64, no
two coordinates share a bound, the widths differ per coordinate and lo != -up everywhere:

    j % 3 == 0   lo = 0.5 + j/1024   up = 3 + j/512      0 lies below the box
    j % 3 == 1   lo = -4 + j/1024    up = -0.5 + j/512   0 lies above the box
    j % 3 == 2   lo = -3 + j/1024    up = 2 + j/512      0 lies inside

so on sphere a third of the coordinates is driven onto its lower bound, a third onto its upper
bound and a third stays free: a kernel that reads lower[0], lower[t] for lower[col], upper[j] for
upper[j + 1] or exchanges the two bounds computes something else.
"""
import numpy as np

_LO = (0.5, -4., -3.)
_UP = (3., -0.5, 2.)


def percoord_box(n):
    j = np.arange(n)
    lo = np.choose(j % 3, _LO) + j / 1024.
    up = np.choose(j % 3, _UP) + j / 512.
    return lo, up


def percoord_guess(n, P=None):
    """off-centre and strictly inside; P rows, every one different (P=None: one vector)"""
    lo, up = percoord_box(n)
    j = np.arange(n)
    rows = [lo + (up - lo) * (0.2 + 0.6 * ((7 * j + 3 * p + 1) % 11) / 10.) for p in range(P or 1)]
    return rows[0] if P is None else np.array(rows)


def percoord_centre(n):
    lo, up = percoord_box(n)
    return 0.5 * (lo + up)


def binding_witness(states, lo, up, need=3):
    """the box bound the reference's run: over the given states (each rows x n, from the
    oracle or a model, never the device) at least `need` coordinates sat exactly on their lower
    bound, `need` on their upper bound, and `need` were strictly interior in every row"""
    n = lo.size
    on_lo, on_up, inner = np.zeros(n, bool), np.zeros(n, bool), np.ones(n, bool)
    for s in states:
        s = np.asarray(s, dtype=float).reshape(-1, n)
        on_lo |= (s == lo).any(axis=0)
        on_up |= (s == up).any(axis=0)
        inner &= ((s > lo) & (s < up)).all(axis=0)
    got = int(on_lo.sum()), int(on_up.sum()), int(inner.sum())
    assert min(got) >= need, "the box does not bind: %d on lower / %d on upper / %d interior" % got
    return got
