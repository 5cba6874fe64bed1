"""The ten built-in objectives in extended precision, each with an a-priori rounding bound, and the
input families the objective tests share.

reference(obj, x) -> (f_ref, bound).  f_ref is the MATHEMATICAL function at the doubles given,
evaluated with mpmath at 200 bits (500 bits once some |x| exceeds 1e6: the `large` family squares
1e45 next to terms of size 1).  bound is a float with

    |f - f_ref| <= bound

for ANY double-precision evaluation of the library's definition of the objective, whatever the order
of its sums.  Nothing in it is fitted to a device: it follows from the IEEE model fl(a op b) =
(a op b)(1 + d), |d| <= u = 2^-53, and from the accuracy the functions it calls promise.

The tables (ellipsoid's 10^(6 i/(n-1)), diffpow's 2 + 4 i/(n-1), Griewank's 1/sqrt(i+1)) are DATA: the
doubles fill_objective_aux (bbo_common.hpp) and bbo_objective_aux (oracle/objectives.h) produce,
restated in aux_table() with the same libm calls, not their exact values.

cos(2 pi x): x is reduced exactly first, t = Fraction(x) - round(Fraction(x)), then mp.cos(2 pi t).
Without the reduction mpmath itself is wrong at 1e300 at these precisions
(test_objective_reference.py checks that).

The bound.  For an objective that is a plain sum of n terms,

    bound = (n + 8 + c) u S + n 2^-1074

S   the sum over the terms of the magnitudes of their rounded intermediates (below, per objective),
    taken in mpmath;
n+8 the depth of any summation in the library: a lane group adds ceil(n/G) terms serially and meets
    in log2 G butterfly steps, ceil(n/G) + log2 G <= n + 6; a serial sum has depth n - 1; the MFMA
    accumulator form adds 8 tiles and 4 steps.  A sum of depth d of values whose magnitudes add up to S
    errs by at most ((1 + u)^d - 1) S; the slack between the real depth and n + 8 pays for the second
    order and for the one or two operations that follow the sum (10 n + s, x0^2 + 1e6 s);
c   the roundings inside one term plus the error of its transcendental, in units of u:
        cos_2pi           4   (its own claim: 2 ulp of 1 = 2 * 2^-52, ABSOLUTE: the term's magnitude is 1)
        exp               6   (OpenCL double precision: 3 ulp)
        cos               8   (4 ulp)
        pow              32   (16 ulp)
        sqrt              1   (correctly rounded)
    (the limits the OpenCL specification sets for double precision, the contract a GPU math library
    is held to; a host libm is well inside them, so one bound serves the device, the oracle and
    numpy.)  numpy's objectives form cos(fl(2 pi x)) instead: the argument carries the rounding of the product and of pi, a relative 2 u, so its cosine errs by up to 2 u |2 pi x| more --
    reference(..., cos_arg_rounded=True) adds that, and nothing else changes.
n 2^-1074   one underflow per term (tiny inputs).

Per objective (x2 = x_j^2; every magnitude is of the exact value):
    sphere       term x2                         S = sum x2                      c = 1
    ellipsoid    term a_j x2                     S = sum a_j x2                  c = 2
    cigar        x0^2 + 1e6 sum_{j>0} x2         S = x0^2 + 1e6 sum x2           c = 3
    discus       1e6 x0^2 + sum_{j>0} x2         S = 1e6 x0^2 + sum x2           c = 3
    diffpow      term |x_j|^a_j                  S = sum |x_j|^a_j               c = 32 + 1
    rastrigin    10 n + sum (x2 - 10 cos)        S = 10 n + sum (x2 + 10)        c = 4 + 3
    rosenbrock   term 100 t^2 + w^2, t = x_{j+1} - x2, w = 1 - x_j.  t is a DIFFERENCE: the computed t
                 errs by dt <= u (x2 + |t|) (the square's rounding and the subtraction's), however small
                 t itself is, and the computed t^2 by 2 |t| dt + dt^2 -- second order kept, or the bound
                 is false on the parabola x_{j+1} = fl(x_j^2), where t is nothing but the rounding of a
                 square.  With D = dt / u = x2 + |t|:
                     S = sum [100 (t^2 + 2 |t| D + u D^2) + w^2]                 c = 6
                 (t t, 100 *, w twice through its square, w w, the add).
    schwefel12   term r_j^2, r_j = x_1 + ... + x_j.  The library forms r_j serially (row groups) or as a
                 tile carry plus a 16-lane scan (accumulators); in any order the computed r_j errs by
                 dr_j <= (j - 1) u A_j, A_j = |x_1| + ... + |x_j|, also where r_j itself has cancelled
                 to zero (the `alternating` family).  With D_j = (j - 1) A_j:
                     S = sum [r_j^2 + 2 |r_j| D_j + u D_j^2]                     c = 1
Ackley and Griewank are not sums; their parts are propagated by derivatives (first order, times
1 + 2^-20 for the rest):
    ackley       a = sum x2 with da = (n + 8 + 1) u a;  b = sum cos with db = (n + 8 + 4) u n;
                 r = a / n: dr = da / n + u r;  s = sqrt r: ds = dr / (2 s) + u s (0 at r = 0);
                 w = -0.2 s: dw = 0.2 ds + 2 u |w| (the product and the constant);
                 E1 = exp w: dE1 = E1 dw + 6 u E1;  m = b / n: dm = db / n + u |m|;
                 E2 = exp m: dE2 = E2 dm + 6 u E2;
                 f = -20 E1 - E2 + 20 + e: bound = 20 dE1 + u 20 E1 + dE2 + 4 u (20 E1 + E2 + 20 + e)
                 (three additions and the double nearest e, each at most u of the largest partial sum).
    griewank     a as above, q = a / 4000: dq = da / 4000 + u q;  y_j = x_j a_j: dy = u |y_j|;
                 c_j = cos y_j: dc_j = min(dy_j + 8 u |c_j|, 2) (|cos'| <= 1; two cosines differ by at most
                 2);  P = prod c_j: dP = min(prod (|c_j| + dc_j) (1 + u)^(n + 8) - prod |c_j|, 2 + 2^-20);
                 f = 1 + q - P: bound = dq + dP + 2 u (1 + q + |P| + dP).
"""
import math
from fractions import Fraction

import mpmath
import numpy as np

OBJECTIVES = ("sphere", "rosenbrock", "rastrigin", "ellipsoid", "ackley", "griewank", "cigar",
              "discus", "diffpow", "schwefel12")
FRAG_OBJECTIVES = ("sphere", "rosenbrock", "ellipsoid", "cigar", "discus", "schwefel12")
FAMILIES = ("control", "zeros", "ones", "seams", "tiny", "large", "parabola", "alternating")

U = 2.0 ** -53
ULP_COS_2PI, ULP_EXP, ULP_COS, ULP_POW, ULP_SQRT = 4, 6, 8, 32, 1
FIRST_ORDER = 1. + 2.0 ** -20


def aux_table(obj, n):
    """the doubles of fill_objective_aux, by the same libm calls"""
    t = [(i / (n - 1)) if n > 1 else 0. for i in range(n)]
    if obj == "ellipsoid":
        return [math.pow(10., 6. * v) for v in t]
    if obj == "diffpow":
        return [2. + 4. * v for v in t]
    if obj == "griewank":
        return [1. / math.sqrt(float(i + 1)) for i in range(n)]
    return [0.] * n


def precision_for(x):
    return 500 if np.abs(np.asarray(x, dtype=np.float64)).max(initial=0.) > 1e6 else 200


def cos_2pi_ref(x):
    """cos(2 pi x) at the double x, in the precision mpmath is working at: x reduced exactly first"""
    fx = Fraction(float(x))
    t = fx - round(fx)
    return mpmath.cos(2 * mpmath.pi * (mpmath.mpf(t.numerator) / mpmath.mpf(t.denominator)))


def _sum_bound(n, c, S):
    return float((n + 8 + c) * U * S) + n * 2.0 ** -1074


def reference(obj, x, cos_arg_rounded=False):
    """(f_ref as an mpf, bound as a float) of objective `obj` (a name) at the float64 vector x"""
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    with mpmath.workprec(precision_for(x)):
        mp = mpmath.mpf
        X = [mp(float(v)) for v in x]
        x2 = [v * v for v in X]
        aux = [mp(a) for a in aux_table(obj, n)]
        zero = mp(0)
        # (the extra cosine error of an evaluation that rounds 2 pi x first, in units of u)
        cos_extra = [2 * 2 * mpmath.pi * abs(v) for v in X] if cos_arg_rounded else [zero] * n
        if obj == "sphere":
            f = mpmath.fsum(x2)
            return f, _sum_bound(n, 1, f)
        if obj == "ellipsoid":
            f = mpmath.fsum(a * v for a, v in zip(aux, x2))
            return f, _sum_bound(n, 2, f)
        if obj == "cigar":
            f = x2[0] + 1000000 * mpmath.fsum(x2[1:])
            return f, _sum_bound(n, 3, f)
        if obj == "discus":
            f = 1000000 * x2[0] + mpmath.fsum(x2[1:])
            return f, _sum_bound(n, 3, f)
        if obj == "diffpow":
            f = mpmath.fsum((abs(v) ** a if v != 0 else zero) for v, a in zip(X, aux))
            return f, _sum_bound(n, ULP_POW + 1, f)
        if obj == "rastrigin":
            cs = [cos_2pi_ref(v) for v in x]
            f = 10 * n + mpmath.fsum(v - 10 * c for v, c in zip(x2, cs))
            S = 10 * n + mpmath.fsum(x2) + 10 * n
            extra = float(10 * U * mpmath.fsum(cos_extra))
            return f, _sum_bound(n, ULP_COS_2PI + 3, S) + extra
        if obj == "rosenbrock":
            f, S = zero, zero
            for j in range(n - 1):
                t = X[j + 1] - x2[j]
                w = 1 - X[j]
                D = x2[j] + abs(t)
                f += 100 * t * t + w * w
                S += 100 * (t * t + 2 * abs(t) * D + U * D * D) + w * w
            return f, _sum_bound(n, 6, S)
        if obj == "schwefel12":
            f, S, r, A = zero, zero, zero, zero
            for j in range(n):
                r += X[j]
                A += abs(X[j])
                D = j * A
                f += r * r
                S += r * r + 2 * abs(r) * D + U * D * D
            return f, _sum_bound(n, 1, S)
        if obj == "ackley":
            a = mpmath.fsum(x2)
            b = mpmath.fsum(cos_2pi_ref(v) for v in x)
            da = (n + 8 + 1) * U * a
            db = (n + 8 + ULP_COS_2PI) * U * n + U * mpmath.fsum(cos_extra)
            r = a / n
            s = mpmath.sqrt(r)
            dr = da / n + U * r
            ds = (dr / (2 * s) * FIRST_ORDER + ULP_SQRT * U * s) if s != 0 else zero
            w = -s / 5
            dw = ds / 5 + 2 * U * abs(w)
            E1 = mpmath.exp(w)
            dE1 = E1 * dw * FIRST_ORDER + ULP_EXP * U * E1
            m = b / n
            dm = db / n + U * abs(m)
            E2 = mpmath.exp(m)
            dE2 = E2 * dm * FIRST_ORDER + ULP_EXP * U * E2
            f = -20 * E1 - E2 + 20 + mpmath.e
            bound = 20 * dE1 + U * 20 * E1 + dE2 + 4 * U * (20 * E1 + E2 + 20 + mpmath.e)
            return f, float(bound) + n * 2.0 ** -1074
        if obj == "griewank":
            a = mpmath.fsum(x2)
            da = (n + 8 + 1) * U * a
            q = a / 4000
            dq = da / 4000 + U * q
            P, Pabs, Pup = mp(1), mp(1), mp(1)
            for v, w in zip(X, aux):
                y = v * w
                c = mpmath.cos(y)
                dc = min(U * abs(y) + ULP_COS * U * abs(c), mp(2))
                P *= c
                Pabs *= abs(c)
                Pup *= abs(c) + dc
            dP = min(Pup * (1 + U) ** (n + 8) - Pabs, mp(2) + 2.0 ** -20)
            f = 1 + q - P
            bound = dq + dP + 2 * U * (1 + q + abs(P) + dP)
            return f, float(bound) + n * 2.0 ** -1074
    raise ValueError(obj)


def ratio(value, f_ref, bound):
    """|value - f_ref| / bound, the difference taken in extended precision (0 / 0 = 0)"""
    with mpmath.workprec(500):
        err = abs(mpmath.mpf(float(value)) - f_ref)
        if err == 0:
            return 0.
        return float(err / bound) if bound > 0 else math.inf


# ---- the input families: pure functions of (name, n, seed) --------------------------------------------
def family(name, n, seed=0):
    """one float64 vector of n coordinates of the named family"""
    rng = np.random.default_rng([FAMILIES.index(name), n, seed])
    if name == "control":
        return rng.uniform(-5., 5., n)
    if name == "zeros":
        return np.zeros(n)
    if name == "ones":
        return np.ones(n)
    if name == "seams":
        # m + k/8 with m in -5..5: on the seam, or one ulp above or below it
        x = rng.integers(-5, 6, n) + rng.integers(0, 8, n) / 8.
        step = rng.integers(-1, 2, n)
        up, down = np.nextafter(x, np.inf), np.nextafter(x, -np.inf)
        return np.where(step > 0, up, np.where(step < 0, down, x))
    if name == "tiny":
        return 1e-9 * rng.uniform(-1., 1., n)
    if name == "large":
        return rng.choice([-1., 1.], n) * 10. ** rng.uniform(30., 45., n)
    if name == "parabola":
        x = np.empty(n)
        for j in range(n):
            if j == 0 or x[j - 1] > 1e3:
                x[j] = rng.uniform(1.01, 1.2)
            else:
                x[j] = x[j - 1] * x[j - 1]
        return x
    if name == "alternating":
        a = rng.uniform(1., 5., (n + 1) // 2)
        x = np.empty(2 * a.size)
        x[0::2], x[1::2] = a, -a
        return x[:n]
    raise ValueError(name)


def family_rows(name, n, rows=8):
    """rows vectors of the family (seeds 0 .. rows - 1) as X[rows, n]"""
    return np.stack([family(name, n, s) for s in range(rows)])


_CACHE = {}


def reference_rows(obj, name, n, rows=8, cos_arg_rounded=False):
    """[(f_ref, bound)] for the rows of family_rows(name, n, rows); computed once per process"""
    return [reference_at(obj, x, cos_arg_rounded) for x in family_rows(name, n, rows)]


def reference_at(obj, x, cos_arg_rounded=False):
    """reference(), remembered by the bits of x (the rows of `zeros` and `ones` are one point)"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    key = (obj, x.tobytes(), cos_arg_rounded)
    if key not in _CACHE:
        _CACHE[key] = reference(obj, x, cos_arg_rounded)
    return _CACHE[key]
