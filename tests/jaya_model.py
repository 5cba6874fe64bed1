"""NumPy restatement of the reference's JayaSearch (src/multivariate/jaya/jaya.cpp), written from
its description, in two orders:

  order="reference"  one member at a time, in slot order, with the reference's aliasing: the best
                     and the worst member of a sub-population are the LIVE rows, so a member
                     evolved after the best sees its already replaced coordinates.  `_best` is
                     reset to +inf and then max()-ed (jaya.cpp:143, :333), so it stays +inf, the
                     improvement is -inf and then NaN, and from the third generation on k = nks.
                     Random numbers: raw mt19937 words (`Words`), turned into the reference's
                     draws by the libstdc++ rules of SURVEY.md Appendix C.
  order="sync"       the device's semantics: every member of a sub-population uses copies of the
                     best and the worst row as they stood at the start of the generation; on a tie
                     the incumbent is the lowest row; `_best` and the roulette keep the
                     reference's arithmetic (+inf, -inf, NaN and all).  Random numbers are
                     arguments: the slot permutation, the lengths, r1 / r2 (levy: two normals and
                     one more uniform) per row and coordinate, the roulette's uniform.

The pool is held by ROW (`X`, `f`); `occ` maps the reference's slots to rows (its std::shuffle
moves the members, here it moves `occ`).  The same IEEE operations in the same order as the
reference; only libm (pow, exp, tgamma) may differ."""
import math

import numpy as np

ORIGINAL, LEVY, TENT_MAP, LOGISTIC = range(4)
MUTATIONS = {"original": ORIGINAL, "levy": LEVY, "tent_map": TENT_MAP, "logistic": LOGISTIC}
INF = float("inf")


def count_ks(np_, npmin):
    return sum(1 for k in range(1, np_ + 1) if np_ >= npmin * k)     # jaya.cpp:128-131


def sigma_u(beta):
    """jaya.cpp:86-89"""
    return math.pow((math.gamma(1. + beta) * math.sin(beta * math.pi / 2.))
                    / (math.gamma((1. + beta) / 2.) * beta * math.pow(2., (beta - 1.) / 2.)), 1. / beta)


def dnrm2(x):
    """blas.cpp:154-181"""
    n = len(x)
    if n < 1:
        return 0.
    if n == 1:
        return abs(float(x[0]))
    scale, ssq = 0., 1.
    for v in x:
        v = float(v)
        if v != 0.:
            a = abs(v)
            if scale < a:
                ssq = 1. + ssq * (scale / a) * (scale / a)
                scale = a
            else:
                ssq = ssq + (a / scale) * (a / scale)
    return scale * math.sqrt(ssq)


def _exp(v):
    try:
        return math.exp(v)
    except OverflowError:
        return INF


class Words:
    """raw 32-bit outputs of the reference's global mt19937, consumed by the rules of libstdc++ 11
    """

    def __init__(self, words):
        self.w, self.i = [int(v) for v in words], 0
        self.have, self.saved = False, 0.

    def next(self):
        v = self.w[self.i]          # IndexError: the generation wanted more words than recorded
        self.i += 1
        return v

    def exhausted(self):
        return self.i == len(self.w)

    def canonical(self):
        lo = float(self.next())
        hi = float(self.next())
        r = (lo + hi * 4294967296.0) / 18446744073709551616.0
        return math.nextafter(1., 0.) if r >= 1. else r

    def uniform(self, a, b):
        """Random::get(a, b) on doubles, random.hpp:329-337"""
        if not a < b:
            a, b = b, a
        return self.canonical() * (b - a) + a

    def uint(self, a, b):
        """Random::get(i, j) on ints: Lemire's multiply-shift with rejection"""
        if not a < b:
            a, b = b, a
        rng = b - a + 1
        prod = self.next() * rng
        low = prod & 0xFFFFFFFF
        if low < rng:
            thresh = (2 ** 32 - rng) % rng
            while low < thresh:
                prod = self.next() * rng
                low = prod & 0xFFFFFFFF
        return a + (prod >> 32)

    def shuffle(self, v):
        """std::shuffle: two swap positions per draw while the range squared fits 32 bits"""
        n = len(v)
        if n < 2:
            return
        if 0xFFFFFFFF // n >= n:
            i = 1
            if n % 2 == 0:
                j = self.uint(0, 1)
                v[i], v[j] = v[j], v[i]
                i += 1
            while i != n:
                b1 = i + 2
                xx = self.uint(0, (i + 1) * b1 - 1)
                j = xx // b1
                v[i], v[j] = v[j], v[i]
                i += 1
                j = xx % b1
                v[i], v[j] = v[j], v[i]
                i += 1
            return
        for i in range(1, n):
            j = self.uint(0, i)
            v[i], v[j] = v[j], v[i]

    def normal(self):
        """std::normal_distribution<>: Marsaglia's polar method with its cached second value"""
        if self.have:
            self.have = False
            return self.saved
        while True:
            x = 2. * self.canonical() - 1.
            y = 2. * self.canonical() - 1.
            r2 = x * x + y * y
            if not (r2 > 1. or r2 == 0.):
                break
        m = math.sqrt(-2. * math.log(r2) / r2)
        self.saved, self.have = x * m, True
        return y * m


def _no_redraw():
    raise AssertionError("the chaotic map met its redraw guard (xchaos == 0.5 / 0.7)")


class Jaya:
    def __init__(self, f, lower, upper, np_, npmin, adapt=True, k0=2, mutation=LOGISTIC, scale=0.01,
                 beta=1.5, temper=10., tol=0., mfev=10 ** 9, order="sync", f_rows=None):
        assert order in ("reference", "sync")
        self.fun, self.f_rows, self.order = f, f_rows, order
        self.lower, self.upper = np.asarray(lower, float), np.asarray(upper, float)
        self.n, self.np, self.npmin = self.lower.size, int(np_), int(npmin)
        self.adapt, self.k, self.mutation = bool(adapt), int(k0), int(mutation)
        self.scale, self.beta, self.temper, self.tol, self.mfev = scale, beta, temper, tol, mfev
        self.nks = count_ks(self.np, self.npmin)
        assert 1 <= self.k <= self.nks and 0. < beta <= 2.
        self.sigmau = sigma_u(beta)

    # ---- init (jaya.cpp:94-133) from a given pool: the draws are the caller's --------------------
    def start(self, X, f, xchaos):
        self.X = np.array(X, float).reshape(self.np, self.n)
        self.f = np.array(f, float)
        self.xchaos = float(xchaos)
        self.occ = list(range(self.np))
        i = int(np.argmin(self.f))                  # the first strict minimum
        self.fgbest, self.bestx = float(self.f[i]), self.X[i].copy()
        if not self.fgbest < INF:
            self.bestx = np.zeros(self.n)
        self.best = self.pbest = self.fgbest        # the reference's quirk (jaya.cpp:124)
        self.fev, self.gen = self.np, 0
        self.perfindex, self.pstrat = [0.] * self.nks, [1.] * self.nks
        self.len = []
        return self

    def evaluate(self, x):
        v = float(self.fun(x))
        return INF if v != v else v

    # ---- the chaotic maps (jaya.cpp:355-377) ---------------------------------------------------
    def sample_tent(self, redraw):
        if self.xchaos < 0.7:
            self.xchaos /= 0.7
        else:
            while self.xchaos == 0.7:
                self.xchaos = redraw()
            self.xchaos = 10. / 3. * (1. - self.xchaos)
        return self.xchaos

    def sample_logistic(self, redraw):
        while self.xchaos == 0.5:
            self.xchaos = redraw()
        self.xchaos = 4. * self.xchaos * (1. - self.xchaos)
        return self.xchaos

    def _chain(self, redraw):
        return self.sample_tent(redraw) if self.mutation == TENT_MAP else self.sample_logistic(redraw)

    def converged(self):
        """jaya.cpp:200-217, members in slot order"""
        mean = m2 = 0.
        for count, row in enumerate(self.occ, 1):
            x = dnrm2(self.X[row])
            delta = x - mean
            mean += delta / count
            m2 += delta * (x - mean)
        return m2 <= (self.np - 1) * self.tol * self.tol

    def _offsets(self):
        off = [0]
        for q in range(self.k):
            off.append(off[-1] + self.len[q])
        assert off[-1] == self.np
        return off

    def _first_best_worst(self, rows):
        fb = fw = self.f[rows[0]]
        rb = rw = rows[0]
        for r in rows:                              # jaya.cpp:148-157: strict comparisons
            if self.f[r] < fb:
                fb, rb = self.f[r], r
            if self.f[r] > fw:
                fw, rw = self.f[r], r
        return rb, rw

    # ---- one generation, the reference's order (jaya.cpp:136-174) ------------------------------
    def iterate_reference(self, words):
        assert self.order == "reference"
        n, lo, up = self.n, self.lower, self.upper
        words.shuffle(self.occ)
        base = self.np // self.k
        self.len = [base] * self.k
        for _ in range(self.np - base * self.k):
            self.len[words.uint(0, self.k - 1)] += 1
        off = self._offsets()
        self.pbest, self.best = self.best, INF
        redraw = lambda: words.uniform(0., 1.)
        for q in range(self.k):
            rows = self.occ[off[q]:off[q + 1]]
            rb, rw = self._first_best_worst(rows)
            for row in rows:
                x, xb, xw = self.X[row], self.X[rb], self.X[rw]     # views: LIVE rows
                tmp = np.empty(n)
                for j in range(n):
                    xj, bj, wj = float(x[j]), float(xb[j]), float(xw[j])
                    start = xj
                    if self.mutation == LEVY:
                        u = words.normal() * self.sigmau
                        v = words.normal() * 1.
                        step = u / math.pow(abs(v), 1. / self.beta)
                        step_size = self.scale * step * (xj - bj)
                        start = xj + step_size * words.uniform(0., 1.)
                    if self.mutation >= TENT_MAP and row == rb:
                        r1 = self._chain(redraw)
                        r2 = self._chain(redraw)
                    else:
                        r1 = words.uniform(0., 1.)
                        r2 = words.uniform(0., 1.)
                    t = start + r1 * (bj - abs(xj)) - r2 * (wj - abs(xj))
                    m = up[j] if up[j] < t else t
                    tmp[j] = m if lo[j] < m else lo[j]
                ft = float(self.fun(tmp))           # (no NaN guard in the reference)
                self.fev += 1
                if ft < self.f[row]:
                    self.X[row] = tmp
                    self.f[row] = ft
                self.best = max(self.best, float(self.f[row]))
                if self.f[row] < self.fgbest:
                    self.fgbest, self.bestx = float(self.f[row]), self.X[row].copy()
        self.gen += 1
        if self.adapt:
            imp = (self.pbest - self.best) / max(1e-12, abs(self.pbest))
            self.perfindex[self.k - 1] = imp
            self.pstrat[self.k - 1] = _exp(self.temper * imp)
            s = 0.
            for v in self.pstrat:
                s += v
            U = words.uniform(0., s)
            self.k = self.nks
            for q in range(self.nks):
                U -= self.pstrat[q]
                if U <= 0.:
                    self.k = q + 1
                    break

    # ---- one generation, the device's order ------------------------------------------------------
    def iterate_sync(self, occ, lens, r1, r2, levy=None, uroul=0., ftrial=None, redraw=_no_redraw):
        """occ: slot -> row after the shuffle; lens: the k lengths; r1, r2: [np][n] by ROW (the best
        member of a sub-population takes the chain's instead under the chaotic mutations); levy:
        (zu, zv, u) [np][n] each; uroul: the roulette's uniform in [0, 1); ftrial: the trials'
        fitness by row (else the model's own objective)."""
        assert self.order == "sync"
        n, k = self.n, self.k
        self.occ, self.len = [int(v) for v in occ], [int(v) for v in lens[:k]]
        assert sorted(self.occ) == list(range(self.np)) and len(self.len) == k
        off = self._offsets()
        R1, R2 = np.array(r1, float).reshape(self.np, n), np.array(r2, float).reshape(self.np, n)
        B, W = np.empty((self.np, n)), np.empty((self.np, n))
        for q in range(k):
            rows = self.occ[off[q]:off[q + 1]]
            rb, rw = self._first_best_worst(rows)
            B[rows], W[rows] = self.X[rb], self.X[rw]           # copies: the generation's start
            if self.mutation >= TENT_MAP:
                for j in range(n):
                    R1[rb, j] = self._chain(redraw)
                    R2[rb, j] = self._chain(redraw)
        X, ax = self.X, np.abs(self.X)
        start = X
        if self.mutation == LEVY:
            zu, zv, ul = (np.array(a, float).reshape(self.np, n) for a in levy)
            step = (zu * self.sigmau) / np.power(np.abs(zv), 1. / self.beta)
            start = X + self.scale * step * (X - B) * ul
        T = start + R1 * (B - ax) - R2 * (W - ax)
        M = np.where(self.upper < T, self.upper, T)
        T = np.where(self.lower < M, M, self.lower)
        if ftrial is None:
            ft = (np.asarray(self.f_rows(T), float) if self.f_rows is not None
                  else np.array([float(self.fun(t)) for t in T]))
            ft = np.where(ft != ft, INF, ft)
        else:
            ft = np.array(ftrial, float)
        self.trial, self.ftrial = T, ft
        take = ft < self.f
        self.X = np.where(take[:, None], T, X)
        self.f = np.where(take, ft, self.f)
        self.pbest, self.best = self.best, INF     # max(+inf, f): jaya.cpp:143, :333
        i = int(np.argmin(self.f))                  # on a tie the lowest row
        if self.f[i] < self.fgbest:
            self.fgbest, self.bestx = float(self.f[i]), self.X[i].copy()
        self.fev += self.np
        self.gen += 1
        if self.adapt:
            imp = (self.pbest - self.best) / max(1e-12, abs(self.pbest))
            self.perfindex[k - 1] = imp
            self.pstrat[k - 1] = _exp(self.temper * imp)
            s = 0.
            for v in self.pstrat:
                s += v
            U = uroul * s
            self.k = self.nks
            for q in range(self.nks):
                U -= self.pstrat[q]
                if U <= 0.:
                    self.k = q + 1
                    break

    def stop_flag(self):
        """optimize(), jaya.cpp:184-196: the budget is looked at before the spread"""
        if self.fev >= self.mfev:
            return 2
        return 1 if self.converged() else 0


def run_sync(rng, f_rows, lower, upper, np_, npmin, mfev, **kw):
    """a whole run of the synchronous form with NumPy draws: final fgbest (the outcome bands)"""
    lower, upper = np.asarray(lower, float), np.asarray(upper, float)
    m = Jaya(None, lower, upper, np_, npmin, mfev=mfev, order="sync", f_rows=f_rows, **kw)
    assert m.mutation != LEVY
    n = m.n
    xchaos = rng.random()
    if m.mutation == TENT_MAP:
        m.xchaos = xchaos
        X = np.array([[lower[j] + m.sample_logistic(rng.random) * (upper[j] - lower[j])
                       for j in range(n)] for _ in range(np_)])
        xchaos = m.xchaos
    else:
        X = rng.random((np_, n)) * (upper - lower) + lower
    f = np.asarray(f_rows(X), float)
    m.start(X, np.where(f != f, INF, f), xchaos)
    occ = np.arange(np_)
    while m.fev < mfev:
        occ = occ[rng.permutation(np_)]
        base = np_ // m.k
        lens = [base] * m.k
        for _ in range(np_ - base * m.k):
            lens[int(rng.integers(m.k))] += 1
        m.iterate_sync(occ, lens, rng.random((np_, n)), rng.random((np_, n)), uroul=rng.random(),
                       redraw=rng.random)
    return m.fgbest
