"""NumPy restatement of the reference's DSSearch (src/multivariate/pso/ds.cpp), written from its
description, with two entry points:

  iterate_reference(words, imethd)  the reference's own call order: every draw comes from the raw
                     mt19937 words (`jaya_model.Words`, the libstdc++ rules of SURVEY.md Appendix
                     C); under `adapt` the method index is an argument (the reference takes it from
                     a default-seeded std::default_random_engine of its own, ds.h:57).
  iterate_keyed(...) the device's draws: the recorded raw uniforms and words of a generation are
                     arguments, and every decision is recomputed from them with the reference's
                     formulas -- p1, p2, the method from `p`, the strategy, mapmax, the direction
                     rows, the maps, the box repair -- before the same trial / selection / bandit
                     arithmetic runs.

A DSSearch generation settles the scalars, the direction rows, the maps, the trials and their
repair before any member is replaced, so the two differ in where the draws come from and in
nothing else.  The same IEEE operations in the same order as the reference; only libm (log, exp)
may differ."""
import math

import numpy as np

INF = float("inf")
RANDOM1, DIFFERENTIAL, RANDOM2 = range(3)


def gamma_of(nbatch):
    """ds.cpp:81-82"""
    return min(1.0, math.sqrt(4 * math.log(4) / ((math.exp(1) - 1) * nbatch)))


def ranked(f):
    """the rows by f, ties to the lower row"""
    return sorted(range(len(f)), key=lambda i: (f[i], i))


def roulette(p, u):
    """std::discrete_distribution: p / sum, the running sums (the last counts as 1), the first
    one above u"""
    s = ((p[0] + p[1]) + p[2]) + p[3]
    c0 = p[0] / s
    c1 = c0 + p[1] / s
    c2 = c1 + p[2] / s
    return 0 if u < c0 else 1 if u < c1 else 2 if u < c2 else 3


def mapmax_of(p2, n):
    return int(math.ceil(p2 * n))


class Dsa:
    def __init__(self, fobj, lower, upper, np_, adapt=True, nbatch=100, tol=0., stol=0.):
        self.fobj = fobj
        self.lo, self.up = np.asarray(lower, float), np.asarray(upper, float)
        self.n, self.np = self.lo.size, int(np_)
        self.adapt, self.nbatch, self.tol, self.stol = bool(adapt), int(nbatch), tol, stol
        self.gamma = gamma_of(self.nbatch)
        self.paths = {"repair_lo": 0, "repair_up": 0}   # coordinates _repair met under / over their bound

    def start(self, X, f, fev=None):
        self.X = np.array(X, float).reshape(self.np, self.n)
        self.f = np.array(f, float).reshape(self.np)
        self.w, self.p = [1.0] * 4, [0.25] * 4
        self.it, self.fev = 0, self.np if fev is None else fev
        self.nsucc = 0

    # ---- the parts both orders share -------------------------------------------------------
    def _trials(self, R, maps, dirrow):
        """ds.cpp:119-123: x + (R * (double) map) * (dir - x), per coordinate"""
        T = np.empty_like(self.X)
        for i in range(self.np):
            x, d = self.X[i], self.X[dirrow[i]]
            for j in range(self.n):
                T[i, j] = x[j] + (R * float(maps[i][j])) * (d[j] - x[j])
        return T

    def _repair(self, T, coin_uniform):
        """update(), ds.cpp:344-365; coin_uniform(i, j) -> (coin, u), asked only when needed"""
        for i in range(self.np):
            for j in range(self.n):
                lo, up = self.lo[j], self.up[j]
                if T[i, j] < lo:
                    coin, u = coin_uniform(i, j)
                    T[i, j] = u * (up - lo) + lo if coin == 0 else lo
                    self.paths["repair_lo"] += 1
                if T[i, j] > up:
                    coin, u = coin_uniform(i, j)
                    T[i, j] = u * (up - lo) + lo if coin == 0 else up
                    self.paths["repair_up"] += 1
        return T

    def _select(self, T, imethd, ftrial=None):
        """ds.cpp:128-155"""
        if ftrial is None:
            ftrial = [self.fobj(T[i]) for i in range(self.np)]
        ftrial = [INF if v != v else float(v) for v in ftrial]
        nsucc = 0
        for i in range(self.np):
            if ftrial[i] < self.f[i]:
                self.f[i] = ftrial[i]
                self.X[i] = T[i]
                nsucc += 1
        self.fev += self.np
        if self.adapt:
            if self.it % self.nbatch == 0:
                self.w = [1.0] * 4
            reward = (1. * nsucc) / self.np
            self.w[imethd] *= self._exp(self.gamma * (reward / self.p[imethd]) / 4)
            wsum = 0.0
            for q in range(4):
                wsum += self.w[q]
            self.p = [(1.0 - self.gamma) * self.w[q] / wsum + self.gamma / 4 for q in range(4)]
        self.it += 1
        self.nsucc, self.trial, self.ftrial = nsucc, T, np.array(ftrial)

    @staticmethod
    def _exp(v):
        try:
            return math.exp(v)
        except OverflowError:
            return INF

    def converged(self, radius=None):
        """ds.cpp:186-217; radius: a function of a row (the reference: dnrm2), Welford sums"""
        dy = abs(float(self.f.min()) - float(self.f.max()))
        if not dy <= self.tol:
            return False
        if radius is None:
            from jaya_model import dnrm2 as radius
        count, mean, m2 = 0, 0., 0.
        for i in range(self.np):
            x = radius(self.X[i])
            count += 1
            delta = x - mean
            mean += delta / count
            m2 += delta * (x - mean)
        return m2 <= (self.np - 1) * self.stol * self.stol

    def best(self):
        i = int(np.argmin(self.f))          # the first minimum in row order
        return float(self.f[i]), self.X[i].copy()

    # ---- the reference's order --------------------------------------------------------------
    def iterate_reference(self, words, imethd=None):
        n, np_ = self.n, self.np
        p1 = words.uniform(0.0, 0.3)
        p2 = words.uniform(0.0, 0.3)
        if not self.adapt:
            imethd = words.uint(0, 3)
        # genDir, :219-292
        if imethd == 0:
            jind = list(range(np_))
            words.shuffle(jind)
            dirrow = jind
        elif imethd == 1:
            order = ranked(self.f)
            dirrow = []
            for _ in range(np_):
                ub = int(math.ceil(words.uniform(0., 1.) * np_))
                dirrow.append(order[words.uint(0, ub - 1)])
        elif imethd == 2:
            order = ranked(self.f)
            ub = int(math.ceil(words.uniform(0., 1.) * np_))
            dirrow = [order[min(ub, np_ - 1)]] * np_
        else:
            dirrow = [int(np.argmin(self.f))] * np_
        # genMap, :304-342
        maps = [[0] * n for _ in range(np_)]
        if words.uint(0, 1) == 0:
            if words.uniform(0., 1.) < p1:
                strategy = RANDOM1
                for i in range(np_):
                    rand = words.uniform(0.0, 1.0)
                    for j in range(n):
                        maps[i][j] = 1 if words.uniform(0.0, 1.0) < rand else 0
            else:
                strategy = DIFFERENTIAL
                for i in range(np_):
                    maps[i][words.uint(0, n - 1)] = 1
        else:
            strategy = RANDOM2
            mapmax = mapmax_of(p2, n)
            for i in range(np_):
                for _ in range(mapmax):
                    maps[i][words.uint(0, n - 1)] = 1
        u = words.uniform(0., 1.)
        R = 1. / (-2. * (math.log(u) if u > 0. else -INF))
        self.dir = self.X[dirrow].copy()
        T = self._trials(R, maps, dirrow)

        def coin_uniform(i, j):
            if words.uint(0, 1) == 0:
                return 0, words.canonical()     # Random::get(lower, upper) = u (upper - lower) + lower
            return 1, 0.
        T = self._repair(T, coin_uniform)
        self.imethd, self.strategy, self.map, self.R = imethd, strategy, np.array(maps), R
        self._select(T, imethd)

    # ---- the device's draws -----------------------------------------------------------------
    def decide_keyed(self, raw, force_method=-1, force_map=-1):
        """raw = (u_p1, u_p2, u_method, u_coin, u_strategy, u_R) -> p1, p2, method, strategy, mapmax"""
        p1, p2 = raw[0] * 0.3, raw[1] * 0.3
        method = roulette(self.p, raw[2]) if self.adapt else int(raw[2] * 4.)
        if raw[3] < 0.5:
            strategy = RANDOM1 if raw[4] < p1 else DIFFERENTIAL
        else:
            strategy = RANDOM2
        if force_method >= 0:
            method = force_method
        if force_map >= 0:
            strategy = force_map
        return p1, p2, method, strategy, mapmax_of(p2, self.n)

    def iterate_keyed(self, raw, R, dirdraws, mapdraws, bounddraws, ftrial=None, force_method=-1,
                      force_map=-1):
        """dirdraws [np][2]: method 1 the bijection's value, method 2 (u, word), method 3 u at
        [0][0]; mapdraws [np][n + 2 + mcap]: the n map uniforms, the member's `rand`, its word
        (differential), then the words of random-2; bounddraws [np][n][2]: coin, uniform."""
        n, np_ = self.n, self.np
        p1, p2, method, strategy, mapmax = self.decide_keyed(raw, force_method, force_map)
        dd = np.asarray(dirdraws, float).reshape(np_, 2)
        md = np.asarray(mapdraws, float).reshape(np_, -1)
        bd = np.asarray(bounddraws, float).reshape(np_, n, 2)
        if method == 0:
            dirrow = [int(v) for v in dd[:, 0]]
            assert sorted(dirrow) == list(range(np_)), "the shuffle's stand-in must be a bijection"
        elif method == 1:
            order = ranked(self.f)
            dirrow = []
            for i in range(np_):
                ub = min(max(int(math.ceil(dd[i, 0] * np_)), 1), np_)
                dirrow.append(order[(int(dd[i, 1]) * ub) >> 32])
        elif method == 2:
            order = ranked(self.f)
            ub = int(math.ceil(dd[0, 0] * np_))
            dirrow = [order[min(ub, np_ - 1)]] * np_
        else:
            dirrow = [int(np.argmin(self.f))] * np_
        maps = [[0] * n for _ in range(np_)]
        for i in range(np_):
            if strategy == RANDOM1:
                rand = md[i, n]
                for j in range(n):
                    maps[i][j] = 1 if md[i, j] < rand else 0
            elif strategy == DIFFERENTIAL:
                maps[i][(int(md[i, n + 1]) * n) >> 32] = 1
            else:
                for k in range(mapmax):
                    maps[i][(int(md[i, n + 2 + k]) * n) >> 32] = 1
        T = self._trials(R, maps, dirrow)
        T = self._repair(T, lambda i, j: (int(bd[i, j, 0]), bd[i, j, 1]))
        self.imethd, self.strategy, self.map, self.R = method, strategy, np.array(maps), R
        self.dirrow, self.p1, self.p2, self.mapmax = dirrow, p1, p2, mapmax
        self._select(T, method, ftrial)


def keyed_draws(rng, m, mcap):
    """NumPy draws in the layouts the device records, for Dsa.iterate_keyed"""
    n, np_ = m.n, m.np
    raw = list(rng.random(5)) + [1. - rng.random()]         # the last in (0, 1]
    R = 0. if raw[5] == 1. else 1. / (-2. * math.log(raw[5]))
    method = m.decide_keyed(raw)[2]
    dd = np.zeros((np_, 2))
    if method == 0:
        dd[:, 0] = rng.permutation(np_)
    elif method == 1:
        dd[:, 0] = rng.random(np_)
        dd[:, 1] = rng.integers(0, 2 ** 32, np_)
    elif method == 2:
        dd[0, 0] = rng.random()
    md = np.empty((np_, n + 2 + mcap))
    md[:, :n + 1] = rng.random((np_, n + 1))
    md[:, n + 1:] = rng.integers(0, 2 ** 32, (np_, 1 + mcap))
    bd = np.empty((np_, n, 2))
    bd[..., 0] = rng.integers(0, 2, (np_, n))
    bd[..., 1] = rng.random((np_, n))
    return raw, R, dd, md, bd


def run_keyed(rng, fobj, lower, upper, np_, mfev, adapt=True, nbatch=100):
    """a whole run of Dsa.iterate_keyed -- the code the device is held against -- with NumPy draws
    (the outcome bands): the best f when the budget is spent (tol = stol = 0: no other stop)"""
    m = Dsa(fobj, lower, upper, np_, adapt=adapt, nbatch=nbatch)
    X = rng.random((np_, m.n)) * (m.up - m.lo) + m.lo
    m.start(X, [fobj(x) for x in X])
    mcap = int(math.ceil(0.3 * m.n)) + 1
    while m.fev < mfev:
        m.iterate_keyed(*keyed_draws(rng, m, mcap))
    return m.best()[0]
