"""Rosenbrock (rosenbrock.cpp: Rosenbrock's rotating axes with the Davies-Swann-Campey line search and Palmer's
orthogonalisation) restated in plain Python floats: every sum and product in the reference's order, dnrm2 in its
scaled form, so a run is the reference's bit for bit (scripts/gen_rosenbrock_golden.py checks that against the
real class before it writes tests/golden/rosenbrock_runs.json).

    m = Model(f, n, mfev, tol, step0, decf)
    m.init(guess)
    m.iterate()                 # one iterate() of the reference: a line search and its bookkeeping
    m.optimize(guess)           # init() + iterate() until ierr >= 0: (x1, fev, converged)

`evals` is every point handed to f with its value, in order.  `path` is the last search's path
(direction, rounds of the doubling loop, imin, end), `margin` the smallest relative gap of its deciding
comparisons: a search is one the device's built-in can be held to when it is above OK_MARGIN."""
import ctypes
import ctypes.util
import math
import struct
import zlib
from fractions import Fraction

FORWARD, BACKWARD, STRAIGHT = 1, 2, 3           # path[0]
NO_FINAL, KEPT, RESTORED, BUDGET = 0, 1, 2, 3   # path[3]
PATHS = ("forward", "backward", "straight", "dbl0", "dbl1", "dbl2", "dbl3", "imin0", "imin1", "imin2", "imin3",
         "kept", "restored", "orth", "extra", "zero_norm", "shrink", "converged", "budget")
OK_MARGIN = 1e-6
INF = float("inf")


def crc(values):
    """CRC-32 of the doubles as they lie in memory (little-endian)"""
    flat = [float(v) for v in values]
    return zlib.crc32(struct.pack("<%dd" % len(flat), *flat))


def _gap(a, b):
    if a == b:
        return 0.
    if math.isinf(a) or math.isinf(b):
        return INF
    return abs(a - b) / max(abs(a), abs(b))


def _libm_fma():
    try:
        fn = ctypes.CDLL(ctypes.util.find_library("m")).fma
        fn.argtypes, fn.restype = [ctypes.c_double] * 3, ctypes.c_double
        return fn if fn(1. + 2. ** -52, 1. - 2. ** -52, -1.) == -2. ** -104 else None
    except (OSError, AttributeError, TypeError):
        return None


_FMA = _libm_fma()


def fma(a, b, c):
    """a * b + c rounded once: libm's where it is at hand (fast), exact rationals otherwise"""
    if _FMA is not None:
        return _FMA(a, b, c)
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def cos_2pi(x):
    """bbo_cos_2pi of oracle/objectives.h, operation for operation"""
    t = abs(x - round(x))       # (round: half to even, as rint)
    v = t * 8.
    k = min(int(v), 3)
    f = v - float(k)
    if k & 1:
        f = 1. - f
    y = f * float.fromhex("0x1.921fb54442d18p-1")
    z = y * y
    q = (k + 1) >> 1
    ps = 1.58969099521155010221e-10
    for c in (-2.50507602534068634195e-08, 2.75573137070700676789e-06, -1.98412698298579493134e-04,
              8.33333333332248946124e-03, -1.66666666666666324348e-01):
        ps = fma(ps, z, c)
    sy = fma(y * z, ps, y)
    pc = -1.13596475577881948265e-11
    for c in (2.08757232129817482790e-09, -2.75573143513906633035e-07, 2.48015872894767294178e-05,
              -1.38888888888741095749e-03, 4.16666666666666019037e-02):
        pc = fma(pc, z, c)
    cy = fma(z * z, pc, fma(z, -0.5, 1.))
    c1 = sy if k == 1 else -sy
    return cy if q == 0 else (c1 if q == 1 else -cy)


def objective(name, n):
    """the objectives of the fixture, serial left-to-right sums like oracle/objectives.h"""
    if name == "sphere":
        def f(x):
            s = 0.
            for v in x:
                s += v * v
            return s
    elif name == "rosenbrock":
        def f(x):
            s = 0.
            for i in range(n - 1):
                a = x[i + 1] - x[i] * x[i]
                b = 1. - x[i]
                s += 100. * (a * a) + b * b
            return s
    elif name == "rastrigin":
        def f(x):
            s = 0.
            for v in x:
                s += v * v - 10. * cos_2pi(v)
            return 10. * n + s
    else:
        raise ValueError(name)
    return f


def dnrm2(x):
    """blas.cpp:154: the scaled sum of squares"""
    n = len(x)
    if n < 1:
        return 0.
    if n == 1:
        return abs(x[0])
    scale, ssq = 0., 1.
    for v in x:
        if v != 0.:
            a = abs(v)
            if scale < a:
                ssq = 1. + ssq * (scale / a) * (scale / a)
                scale = a
            else:
                ssq = ssq + (a / scale) * (a / scale)
    return scale * math.sqrt(ssq)


def daxpy1(da, dx, dy):
    """dz = dy + da dx; da == 0 copies dy (blas.cpp:75)"""
    if da == 0.:
        return list(dy)
    return [y + da * x for x, y in zip(dx, dy)]


class Model:
    def __init__(self, f, n, mfev, tol, step0, decf=0.1, repair=False):
        self.f, self.n, self.mfev, self.tol, self.step0, self.rho = f, int(n), int(mfev), tol, step0, decf
        self.repair = repair
        self.evals, self.paths = [], {k: 0 for k in PATHS}
        # (the GPU tests) values to take instead of f's at the interpolation points and at the final point
        self.fs_override = self.final_override = None

    def _f(self, x):
        v = float(self.f(list(x)))
        if v != v:
            v = INF       # (the device's rule; the reference has none)
        self.evals.append((list(x), v))
        return v

    def _cmp(self, a, b):
        self.margin = min(self.margin, _gap(a, b))

    # init() (:56-93)
    def init(self, guess):
        n = self.n
        self.x = [[0.] * n for _ in range(n + 2)]
        self.v = [[0.] * n for _ in range(n + 2)]
        self.d = [0.] * (n + 2)
        self.fs = [0.] * 4
        self.x1 = [0.] * n
        self.x[0] = [float(g) for g in guess[:n]]
        self.stepi = self.step0
        for j in range(1, n + 1):
            self.v[j][j - 1] = 1.
        self.fev, self.i, self.ierr = 0, 1, -1
        self.searches, self.orths = 0, 0
        self.path, self.margin, self.orth = [0, 0, -1, 0], INF, False

    # lineSearch() (:227-332): (err, s, x)
    def line_search(self, pos, s, v):
        self.fs = fs = [0.] * 4
        path = self.path = [FORWARD, 0, -1, NO_FINAL]
        x0 = list(pos)
        fx0 = self._f(x0)
        self.fev += 1
        x = daxpy1(s, v, x0)
        fx = self._f(x)
        self.fev += 1
        self._cmp(fx, fx0)
        doubling = True
        if fx > fx0:
            m2s = -2. * s
            if m2s != 0.:
                x = [xi + m2s * vi for xi, vi in zip(x, v)]       # daxpym
            s = -s
            fx = self._f(x)
            self.fev += 1
            self._cmp(fx, fx0)
            path[0] = BACKWARD
            if fx > fx0:
                path[0] = STRAIGHT
                doubling = False
        if doubling:
            while True:
                s *= 2.
                x0 = list(x)
                fx0 = fx
                x = daxpy1(s, v, x0)
                fx = self._f(x)
                self.fev += 1
                path[1] += 1
                if self.fev > self.mfev:
                    path[3] = BUDGET
                    return 1, s, x
                self._cmp(fx, fx0)
                if not (fx <= fx0 and abs(s) < 1e30):
                    break
            s /= 2.
        pts = [daxpy1(-s, v, x0), list(x0), daxpy1(s, v, x0), daxpy1(2. * s, v, x0)]
        for k in range(4):
            fs[k] = self._f(pts[k])
        if self.fs_override is not None:
            fs[:] = self.fs_override
        self.fev += 4
        imin = fs.index(min(fs))
        if not any(math.isnan(q) for q in fs):
            srt = sorted(fs)
            self._cmp(srt[0], srt[1])
        path[2] = imin
        if imin in (1, 2):
            num = s * (fs[imin - 1] - fs[imin + 1])
            den = 2. * (fs[imin - 1] - 2. * fs[imin] + fs[imin + 1])
            stepf = 0. if imin == 1 else s
            if abs(den) > 0.:
                stepf += num / den
        else:
            stepf = -s if imin == 0 else 2. * s
            return 0, stepf, daxpy1(stepf, v, x0)
        x = daxpy1(stepf, v, x0)
        fx = self._f(x)
        if self.final_override is not None:
            fx = self.final_override
        self.fev += 1
        self._cmp(fx, fs[imin])
        path[3] = KEPT
        if fx > fs[imin]:
            stepf = 0. if imin == 1 else s
            x = daxpy1(stepf, v, x0)
            path[3] = RESTORED
        return 0, stepf, x

    def _count_path(self):
        p, c = self.path, self.paths
        c[("forward", "backward", "straight")[p[0] - 1]] += 1
        if p[0] != STRAIGHT and p[3] != BUDGET:
            c["dbl%d" % min(p[1] - 1, 3)] += 1
        if p[2] >= 0:
            c["imin%d" % p[2]] += 1
        if p[3] == KEPT:
            c["kept"] += 1
        if p[3] == RESTORED:
            c["restored"] += 1

    # iterate() (:95-210)
    def iterate(self):
        n, x, v, d = self.n, self.x, self.v, self.d
        self.margin, self.orth = INF, False
        i = self.i
        err, wa, x[i] = self.line_search(x[i - 1], self.stepi, v[i])
        d[i] = wa
        self.searches += 1
        self._count_path()
        if err:
            self.ierr = 1
            self.paths["budget"] += 1
            return
        if i < n:
            self.i += 1
            return
        if i == n:
            temp = daxpy1(-1., x[0], x[n])
            zn = dnrm2(temp)
            if zn > 0.:
                da = 1. / zn
                v[n + 1] = [t * da for t in temp]
                self.i = n + 1
                self.paths["extra"] += 1
                return
            x[n + 1] = list(x[n])
            d[n + 1] = 0.
            self.paths["zero_norm"] += 1
        else:
            dxn = 0.
            for j in range(n):
                tmp = x[n + 1][j] - x[0][j]
                dxn += tmp * tmp
            dxn = math.sqrt(dxn)
            if dxn >= self.stepi:
                self.orthogonalise()
                d[1] = d[n + 1]
                x[0] = list(x[n])
                x[1] = list(x[n + 1])
                self.i = 2
                return
        self.stepi *= self.rho
        self.paths["shrink"] += 1
        if self.stepi <= self.tol:
            self.x1 = list(x[n + 1])
            self.ierr = 0
            self.paths["converged"] += 1
            return
        x[0] = list(x[n + 1])
        self.i = 1
        if self.fev >= self.mfev:
            self.ierr = 1
            self.paths["budget"] += 1

    # Palmer (:144-185)
    def orthogonalise(self):
        n, v, d = self.n, self.v, self.d
        vold = [list(r) for r in v]
        temp = [0.] * (n + 2)
        for j in range(n, 0, -1):
            temp[j] = d[j] * d[j] if j == n else temp[j + 1] + d[j] * d[j]
        for ii in range(1, n + 1):
            if temp[ii] <= 0.:
                continue
            row = [0.] * n
            for j in range(n):
                a = 0.
                for jj in range(1 if ii == 1 else ii, n + 1):
                    a += d[jj] * vold[jj][j]
                if ii == 1:
                    a /= math.sqrt(temp[ii])
                else:
                    a *= d[ii - 1]
                    a -= vold[ii - 1][j] * temp[ii]
                    a /= math.sqrt(temp[ii] * temp[ii - 1])
                row[j] = a
            v[ii] = row
        self.orth = True
        self.orths += 1
        self.paths["orth"] += 1

    def ok(self):
        return self.margin > OK_MARGIN

    def solution(self):
        """solution() (:212): _x1; under repair the end point of the last completed search where not converged"""
        x = self.x[self.i - 1] if self.repair and self.ierr != 0 else self.x1
        return list(x), self.fev, self.ierr == 0

    def optimize(self, guess):
        self.init(guess)
        while self.ierr < 0:
            self.iterate()
        return self.solution()

    def flat(self, rows):
        return [q for r in rows for q in r]

    def state_crcs(self):
        return [crc(self.flat(self.x)), crc(self.flat(self.v)), crc(self.d)]
