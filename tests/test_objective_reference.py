"""CPU: the host statements of the ten built-in objectives against the extended-precision reference
of objective_reference.py, and the reference's own footing.

    the oracle's bbo_cos_2pi (oracle/objectives.h, the restatement of the device's cos_2pi) against
        the exactly reduced mpmath cosine: within 2^-52 absolute at every octant seam m + k/8 and one
        ulp beside it, at 2^52 +- 0.5, 2^53, +-1e300 and 45 000 points in between; exact where the
        cosine is; never beyond 1; even
    oracle_lib.objective (bbo_objective_eval), every objective, family and n: inside the bound
    bboptpy_amd.objectives (numpy), the same without `large`.  numpy forms cos(fl(2 pi x)): 2 pi x is
        rounded BEFORE the cosine sees it, which costs up to 2 u |2 pi x| of the cosine -- the bound is
        taken with cos_arg_rounded=True -- and all of it at 1e30 and beyond, which is why `large` is
        left out.  These functions are a convenience for looking at results; no optimizer's values
        come from them.
The GPU side of the same reference is test_objective_forms_gpu.py."""
import math
from fractions import Fraction

import mpmath
import numpy as np
import pytest

import objective_reference as R

NS = (1, 2, 3, 16, 17, 64, 65, 130)


# ---- the reference's own footing ---------------------------------------------------------------------
def test_unreduced_mpmath_cosine_is_wrong_at_1e300_and_the_reduced_one_is_not():
    """1e300 is an even integer: cos(2 pi 1e300) = 1.  At 200 and at 500 bits 2 pi 1e300 is known to
    far fewer digits than it has in front of the point, so mp.cos of the product is noise"""
    for prec in (200, 500):
        with mpmath.workprec(prec):
            naive = mpmath.cos(2 * mpmath.pi * mpmath.mpf(1e300))
            assert abs(naive - 1) > 1e-3
            assert R.cos_2pi_ref(1e300) == 1
            assert R.cos_2pi_ref(-1e300) == 1
            assert R.cos_2pi_ref(2.0 ** 52 - 0.5) == -1


def test_the_tables_are_the_checkers(oracle_lib):
    """aux_table restates fill_objective_aux; held here to the oracle's copy through an objective that
    multiplies by it: ellipsoid and diffpow at unit vectors return one entry each"""
    n = 17
    for i in range(n):
        e = np.zeros(n)
        e[i] = 1.
        assert oracle_lib.objective("ellipsoid", e) == R.aux_table("ellipsoid", n)[i]
        e[i] = 2.
        assert oracle_lib.objective("diffpow", e) == math.pow(2., R.aux_table("diffpow", n)[i])


@pytest.mark.parametrize("n", [1, 2, 17, 130])
def test_every_family_is_what_it_is_named_for(n):
    for seed in range(3):
        for name in R.FAMILIES:
            a, b = R.family(name, n, seed), R.family(name, n, seed)
            assert a.shape == (n,) and a.dtype == np.float64 and np.array_equal(a, b), name
        x = R.family("control", n, seed)
        assert (np.abs(x) <= 5.).all()
        assert not R.family("zeros", n, seed).any() and (R.family("ones", n, seed) == 1.).all()
        x = R.family("tiny", n, seed)
        assert (np.abs(x) <= 1e-9).all() and x.all()
        x = R.family("large", n, seed)
        assert (np.abs(x) >= 1e30).all() and (np.abs(x) <= 1e45).all()
        # seams: every coordinate is m + k/8 or a neighbour of it
        x = R.family("seams", n, seed)
        near = np.round(x * 8.) / 8.
        assert ((x == near) | (np.nextafter(near, np.inf) == x) | (np.nextafter(near, -np.inf) == x)).all()
        assert (np.abs(near) <= 6.).all()
        # parabola: the mathematical t = x[j+1] - x[j]^2 is the rounding of a square
        x = R.family("parabola", n, seed)
        for j in range(n - 1):
            if x[j] > 1e3:
                assert 1.01 <= x[j + 1] <= 1.2
                continue
            t = Fraction(x[j + 1]) - Fraction(x[j]) ** 2
            assert abs(t) <= Fraction(2) ** -52 * Fraction(x[j]) ** 2
        # alternating: the exact prefix sums return to 0 after every pair
        x = R.family("alternating", n, seed)
        run = Fraction(0)
        for j in range(n):
            run += Fraction(x[j])
            assert (run == 0) == (j % 2 == 1)
            assert 1. <= abs(x[j]) <= 5.
    # over the seeds and sizes the tests use: exact seams, both neighbours, and a parabola that is not
    # exactly on the curve (a square of a 53-bit number seldom fits 53 bits)
    x = np.concatenate([R.family("seams", 130, s) for s in range(8)])
    near = np.round(x * 8.) / 8.
    assert (x == near).sum() > 100 and (x > near).sum() > 100 and (x < near).sum() > 100
    assert {int(v) for v in np.round((near % 1.) * 8.)} == set(range(8))
    x = R.family("parabola", 130, 0)
    assert any(Fraction(x[j + 1]) != Fraction(x[j]) ** 2 for j in range(129) if x[j] <= 1e3)


# ---- the oracle's cos_2pi ----------------------------------------------------------------------------
def cos_2pi_points():
    """the seams m + k/8 and their neighbours for m = -6..6, the ends of the double grid, and 45 000
    points: U(-6, 6), 1e-9 U(-1, 1), +-10^U(0, 45), +-10^U(45, 300), halves and quarters up to 2^53"""
    seams = np.array([m + k / 8. for m in range(-6, 7) for k in range(8)])
    edge = np.array([2.0 ** 52 - 0.5, 2.0 ** 52, 2.0 ** 52 + 0.5, 2.0 ** 53, 1e300, -1e300,
                     2.0 ** 51 + 0.25, 2.0 ** 51 + 0.125, 2.0 ** 50 + 0.375, 0.5, -0.5, 0.25, 0.75])
    rng = np.random.default_rng(2718)
    sign = lambda k: rng.choice([-1., 1.], k)
    rnd = np.concatenate([
        rng.uniform(-6., 6., 25000), 1e-9 * rng.uniform(-1., 1., 2000),
        sign(8000) * 10. ** rng.uniform(0., 45., 8000), sign(4000) * 10. ** rng.uniform(45., 300., 4000),
        sign(6000) * (rng.integers(0, 2 ** 40, 6000) + rng.integers(0, 8, 6000) / 8.)])
    return np.concatenate([seams, np.nextafter(seams, np.inf), np.nextafter(seams, -np.inf), edge, rnd])


def test_oracle_cos_2pi_against_the_reduced_cosine(oracle_lib):
    cos_2pi = oracle_lib.f("cos_2pi")
    pts = cos_2pi_points()
    assert pts.size >= 45000
    worst, at = 0., None
    with mpmath.workprec(200):
        for x in pts:
            got = cos_2pi(x)
            assert abs(got) <= 1., x
            assert cos_2pi(-x) == got, x
            err = float(abs(mpmath.mpf(got) - R.cos_2pi_ref(x)))
            if err > worst:
                worst, at = err, x
    print("bbo_cos_2pi: largest |error| %.3f * 2^-53 at x = %r over %d points"
          % (worst * 2.0 ** 53, at, pts.size))
    assert worst <= 2.0 ** -52, "bbo_cos_2pi(%r) errs by %.3e" % (at, worst)


def test_oracle_cos_2pi_exact_values(oracle_lib):
    cos_2pi = oracle_lib.f("cos_2pi")
    assert cos_2pi(0.) == 1. and cos_2pi(-0.) == 1.
    assert cos_2pi(0.5) == -1. and cos_2pi(-0.5) == -1. and cos_2pi(2.0 ** 52 - 0.5) == -1.
    for m in list(range(-6, 7)) + [2.0 ** 40, 2.0 ** 52, 2.0 ** 53, 1e300, -1e300]:
        assert cos_2pi(float(m)) == 1., m
        if abs(m) < 2.0 ** 51:
            assert cos_2pi(m + 0.5) == -1., m
    # the quarter turns: the cosine is 0, the code returns sin(fl(pi/4) * 0) = 0 from the odd octant
    for m in range(-6, 7):
        assert cos_2pi(m + 0.25) == 0. and cos_2pi(m + 0.75) == 0., m


# ---- the two host statements of the objectives -------------------------------------------------------
def _hold(evaluate, families, n, cos_arg_rounded, what):
    worst = {}
    for obj in R.OBJECTIVES:
        for name in families:
            for seed in range(2):
                x = R.family(name, n, seed)
                f_ref, bound = R.reference_at(obj, x, cos_arg_rounded)
                got = evaluate(obj, x)
                r = R.ratio(got, f_ref, bound)
                worst[obj] = max(worst.get(obj, 0.), r)
                assert r <= 1., "%s %s on %s, n = %d, seed %d: %r against %s, %.3g bounds (bound %.3e)" % (
                    what, obj, name, n, seed, got, mpmath.nstr(f_ref, 20), r, bound)
    print("%s n = %d: largest error / bound  %s" % (
        what, n, "  ".join("%s %.3f" % (o, worst[o]) for o in R.OBJECTIVES)))


@pytest.mark.parametrize("n", NS)
def test_oracle_objectives_inside_the_bound(oracle_lib, n):
    _hold(oracle_lib.objective, R.FAMILIES, n, False, "oracle")


@pytest.mark.parametrize("n", NS)
def test_numpy_objectives_inside_the_bound(n):
    import bboptpy_amd as bb
    _hold(lambda obj, x: getattr(bb.objectives, obj)(x), [f for f in R.FAMILIES if f != "large"], n, True,
          "numpy")


def test_exact_values_at_the_optimum(oracle_lib):
    for n in (1, 3, 17, 130):
        z, o = np.zeros(n), np.ones(n)
        for obj in ("sphere", "ellipsoid", "cigar", "discus", "diffpow", "schwefel12", "rastrigin",
                    "griewank"):
            assert oracle_lib.objective(obj, z) == 0., (obj, n)
        assert oracle_lib.objective("rosenbrock", z) == n - 1.
        assert oracle_lib.objective("rosenbrock", o) == 0.


def test_the_bound_separates_a_wrong_term_from_a_rounding():
    """what the bound is for: one column dropped, one column doubled, a neighbour one off or a cosine
    from the wrong octant moves f by thousands of bounds on every family where the term is not zero"""
    n = 17
    for name in ("control", "seams", "parabola", "alternating"):
        x = R.family(name, n, 0)
        for obj in R.OBJECTIVES:
            f_ref, bound = R.reference_at(obj, x)
            dropped, _ = R.reference(obj, x[:-1])
            if obj in ("ellipsoid", "diffpow", "ackley"):
                continue            # their tables / means change with n: not a dropped term
            if abs(dropped - f_ref) == 0:
                continue            # (alternating: the last prefix sum of Schwefel 1.2 is 0 at even n)
            assert abs(dropped - f_ref) > 1000 * bound, (obj, name)
    with mpmath.workprec(200):
        x = R.family("control", n, 1)
        f_ref, bound = R.reference_at("rastrigin", x)
        # cos from the neighbouring octant: sin instead of cos in one term
        wrong = f_ref + 10 * R.cos_2pi_ref(x[3]) - 10 * mpmath.sin(2 * mpmath.pi * mpmath.mpf(x[3]))
        assert abs(wrong - f_ref) > 1000 * bound
