"""NelderMead (nelder_mead.cpp) restated in plain Python floats: every sum and product in the reference's
order, so a run is the reference's bit for bit (scripts/gen_neldermead_golden.py checks that against the
real class before it writes tests/golden/neldermead_runs.json).

    m = Model(f, n, mfev, tol, rad0, minit, pinit, checkev, eps)
    m.init(guess); m.first_simplex()        # what the device's initialize() does
    m.iterate()                             # one iterate() of the reference
    m.optimize(guess)                       # init() + nelmin() whole

`evals` is every point handed to f with its value, in order.  `margin` is the smallest relative gap of the
comparisons the last step (or factorial test) made: a step is one the device can be held to when it is
above OK_MARGIN.  `events` names what nelmin() did: ("stop", it) the stop test fired, ("factorial", passed,
probes counted), ("restart",), ("budget",)."""
import math
import struct
import zlib

COORDINATE_AXIS, SPENDLEY, PFEFFER, RANDOM = range(4)
ORIGINAL, GAO2010, MEHTA2019_CRUDE, MEHTA2019_REFINED = range(4)
MINIT = {"coordinate_axis": 0, "spendley": 1, "pfeffer": 2, "random": 3}
PINIT = {"original": 0, "gao2010": 1, "mehta2019_crude": 2, "mehta2019_refined": 3}
# "branch" of the device
EXPANDED, EXPAND_REFUSED, REFLECTED, INSIDE, SHRINK, OUTSIDE, OUTSIDE_REFUSED = range(1, 8)
BRANCH_NAMES = {EXPANDED: "expanded", EXPAND_REFUSED: "expand_refused", REFLECTED: "reflected", INSIDE: "inside",
                SHRINK: "shrink", OUTSIDE: "outside", OUTSIDE_REFUSED: "outside_refused"}
PATHS = tuple(BRANCH_NAMES.values()) + ("stop_fired", "factorial_passed", "factorial_restart", "budget_exit")
OK_MARGIN = 1e-6
INF = float("inf")


def crc(values):
    """CRC-32 of the doubles as they lie in memory (little-endian)"""
    flat = [float(v) for v in values]
    return zlib.crc32(struct.pack("<%dd" % len(flat), *flat))


def coefficients(pinit, n):
    """initParameters() (:369-401): ccoef, ecoef, rcoef, scoef"""
    if pinit == ORIGINAL:
        return 0.5, 2.0, 1.0, 0.5
    if pinit == GAO2010:
        return 0.75 - 0.5 / n, 1. + 2. / n, 1., 1. - 1. / n
    if pinit == MEHTA2019_CRUDE:
        odd = n % 2
        return (1. + math.cos((n + 3. + odd) * math.pi / (2. * n)), 1. + math.cos((n - 3. - odd) * math.pi / (2. * n)),
                1. + math.cos((n - 1. - odd) * math.pi / (2. * n)), 1. + math.cos((n + 1. + odd) * math.pi / (2. * n)))
    nc = 2 * (9 + (n - 1) // 5)
    return (1. + math.cos((nc + 5.) * math.pi / (2. * nc)), 1. + math.cos((nc - 3.) * math.pi / (2. * nc)),
            1. + math.cos((nc - 1.) * math.pi / (2. * nc)), 1. + math.cos((nc + 3.) * math.pi / (2. * nc)))


def _gap(a, b):
    if a == b:
        return 0.
    if math.isinf(a) or math.isinf(b):
        return INF
    return abs(a - b) / max(abs(a), abs(b))


class Model:
    def __init__(self, f, n, mfev, tol, rad0, minit=SPENDLEY, pinit=MEHTA2019_REFINED, checkev=10, eps=1e-3,
                 repair=False):
        self.f, self.n, self.mfev, self.tol, self.rad = f, int(n), int(mfev), tol, rad0
        self.minit, self.pinit, self.checkev, self.eps, self.repair = int(minit), int(pinit), int(checkev), eps, repair
        self.evals, self.events, self.paths = [], [], {k: 0 for k in PATHS}

    def _f(self, x):
        v = float(self.f(list(x)))
        if v != v:
            v = INF       # (the device's rule; the reference has none)
        self.evals.append((list(x), v))
        return v

    def _cmp(self, a, b):
        self.margin = min(self.margin, _gap(a, b))

    # init() (:53-87)
    def init(self, guess):
        n = self.n
        self.start = [float(v) for v in guess[:n]]
        self.ccoef, self.ecoef, self.rcoef, self.scoef = coefficients(self.pinit, n)
        self.p = [[0.] * n for _ in range(n + 1)]
        self.y = [0.] * (n + 1)
        self.xmin = [0.] * n
        self.step = [self.rad] * n
        self.icount, self.jcount, self.delta = 0, self.checkev, 1.
        self.rq = self.tol * self.tol * n
        self.ynl, self.conv = 0., False
        self.ilo = self.ihi = 0
        self.ylo = 0.
        self.it, self.restarts, self.branch, self.margin = 0, 0, 0, INF

    # initSimplex() (:312-367)
    def init_simplex(self):
        n, st, sp, d, p = self.n, self.start, self.step, self.delta, self.p
        p[n] = list(st)
        if self.minit == COORDINATE_AXIS:
            for j in range(n):
                row = list(st)
                row[j] = st[j] + sp[j] * d
                p[j] = row
        elif self.minit == SPENDLEY:
            pc = 1. / (n * math.sqrt(2.)) * (n - 1. + math.sqrt(n - 1.))
            qc = 1. / (n * math.sqrt(2.)) * (math.sqrt(n + 1.) - 1.)
            for i in range(n):
                p[i] = [st[j] + sp[j] * d * (pc if i == j else qc) for j in range(n)]
        elif self.minit == PFEFFER:
            for i in range(n):
                p[i] = [((0.0075 if st[j] == 0. else st[j] * (1. + 0.05)) if i == j else st[j]) for j in range(n)]
        else:
            raise ValueError("the model has no generator: minit = random is not restated")

    # nelmin()'s first pass (:251-260): what the device's initialize() does
    def first_simplex(self):
        self.init_simplex()
        for j in range(self.n + 1):
            self.y[j] = self._f(self.p[j])
        self.icount += self.n + 1
        self.ilo = self.y.index(min(self.y))
        self.ylo = self.y[self.ilo]

    def _replace(self, x, v):
        self.p[self.ihi] = list(x)
        self.y[self.ihi] = v

    # iterate() (:89-226)
    def iterate(self):
        n, p, y = self.n, self.p, self.y
        self.margin = INF
        self.conv = False
        ihi = 0
        for k in range(1, n + 1):
            if y[ihi] < y[k]:
                ihi = k
        if n >= 1:
            self._cmp(y[ihi], max(v for k, v in enumerate(y) if k != ihi))
        self.ihi, self.ynl = ihi, y[ihi]
        pbar = [0.] * n
        for i in range(n):
            s = 0.
            for k in range(n + 1):
                s += p[k][i]
            s -= p[ihi][i]
            s /= n
            pbar[i] = s
        pstar = [pbar[k] + self.rcoef * (pbar[k] - p[ihi][k]) for k in range(n)]
        ystar = self._f(pstar)
        self.icount += 1
        self._cmp(ystar, self.ylo)
        if ystar < self.ylo:
            p2star = [pbar[k] + self.ecoef * (pstar[k] - pbar[k]) for k in range(n)]
            y2star = self._f(p2star)
            self.icount += 1
            self._cmp(ystar, y2star)
            if ystar < y2star:
                self._replace(pstar, ystar)
                self.branch = EXPAND_REFUSED
            else:
                self._replace(p2star, y2star)
                self.branch = EXPANDED
        else:
            l = 0
            for i in range(n + 1):
                self._cmp(ystar, y[i])
                if ystar < y[i]:
                    l += 1
            if 1 < l:
                self._replace(pstar, ystar)
                self.branch = REFLECTED
            elif l == 0:
                p2star = [pbar[k] + self.ccoef * (p[ihi][k] - pbar[k]) for k in range(n)]
                y2star = self._f(p2star)
                self.icount += 1
                self._cmp(y[ihi], y2star)
                if y[ihi] < y2star:
                    ilo = self.ilo
                    for j in range(n + 1):
                        for k in range(n):
                            p[j][k] = self.scoef * (p[j][k] + p[ilo][k])
                        y[j] = self._f(p[j])
                        self.icount += 1
                    self.ilo = y.index(min(y))
                    self.ylo = y[self.ilo]
                    self.conv = False
                    self.branch = SHRINK
                    self.it += 1
                    self.paths["shrink"] += 1
                    return
                self._replace(p2star, y2star)
                self.branch = INSIDE
            else:
                p2star = [pbar[k] + self.ccoef * (pstar[k] - pbar[k]) for k in range(n)]
                y2star = self._f(p2star)
                self.icount += 1
                self._cmp(y2star, ystar)
                if y2star <= ystar:
                    self._replace(p2star, y2star)
                    self.branch = OUTSIDE
                else:
                    self._replace(pstar, ystar if self.repair else y2star)      # :195-197
                    self.branch = OUTSIDE_REFUSED
        self.paths[BRANCH_NAMES[self.branch]] += 1
        self.it += 1
        if y[ihi] < self.ylo:
            self.ylo = y[ihi]
            self.ilo = ihi
        self.jcount -= 1
        if 0 < self.jcount:
            self.conv = False
            return
        if self.icount <= self.mfev:
            self.jcount = self.checkev
            s = 0.
            for v in y:
                s += v
            s = s / (n + 1.)
            sumsq = 0.
            for v in y:
                sumsq += (v - s) * (v - s)
            self._cmp(sumsq, self.rq)
            if sumsq <= self.rq:
                self.conv = True

    # the factorial test of nelmin() (:270-302); True: passed, False: restart prepared, None: budget
    def factorial(self):
        n = self.n
        self.margin = INF
        self.xmin = list(self.p[self.ilo])
        self.ynl = self.y[self.ilo]
        if self.mfev < self.icount:
            self.events.append(("budget",))
            self.paths["budget_exit"] += 1
            return None
        xmin, count = self.xmin, 0
        for i in range(n):
            self.delta = self.step[i] * self.eps
            xmin[i] += self.delta
            for sign in (0, 1):
                if sign:
                    xmin[i] -= (self.delta + self.delta)
                z = self._f(xmin)
                self.icount += 1
                count += 1
                self._cmp(z, self.ynl)
                if z < self.ynl:
                    self.events.append(("factorial", False, count))
                    self.paths["factorial_restart"] += 1
                    self.start = list(xmin)
                    self.delta = self.eps
                    self.restarts += 1
                    return False
            xmin[i] += self.delta
        self.events.append(("factorial", True, count))
        self.paths["factorial_passed"] += 1
        return True

    # nelmin() (:245-304): 0 converged, 2 budget
    def nelmin(self, first=True):
        while True:
            if first:
                self.first_simplex()
            first = True
            while self.icount < self.mfev:
                self.iterate()
                if self.conv:
                    self.events.append(("stop", self.it))
                    self.paths["stop_fired"] += 1
                    break
            verdict = self.factorial()
            if verdict is None:
                return 2
            if verdict:
                return 0

    def optimize(self, guess):
        self.init(guess)
        ifault = self.nelmin()
        return list(self.xmin), self.icount, ifault == 0

    def ok(self):
        return self.margin > OK_MARGIN

    def state_crc(self):
        return crc([v for r in self.p for v in r] + self.y)
