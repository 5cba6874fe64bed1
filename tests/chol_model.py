"""NumPy restatement of the reference's CholeskyCmaes (Krause, Arbones, Igel 2016;
src/multivariate/cma/cholesky_cmaes.cpp over base_cmaes.cpp), written from its description:
the PROCEDURE of the reference -- mu + 1 positive rank-1 updates of the factor, the radii's
Welford sums in sampling order -- with the `ranked` switch of the device's extension.  The test
suites hold it against the recorded reference (tests/golden/chol_runs.json) and the device
against it.

Sums run left to right in Python floats where the reference's do (same operations, same order;
only libm differs).  `factor="cholesky"` replaces the rank-1 chain by numpy.linalg.cholesky of
    C' = (1 - c1 - cmu) A A^T + c1 pc pc^T + cmu sum_i w_i y_i y_i^T
which is the matrix the chain ends with (both are THE lower factor with a positive diagonal)."""
import math

import numpy as np


def _seq(vals):
    s = 0.
    for v in vals:
        s += v
    return s


def objective(name, n):
    """built-in objectives, serial left-to-right sums like oracle/objectives.h"""
    t = [(i / (n - 1) if n > 1 else 0.) for i in range(n)]
    if name == "sphere":
        return lambda x: _seq(float(v) * float(v) for v in x)
    if name == "rosenbrock":
        def f(x):
            s = 0.
            for i in range(n - 1):
                a = float(x[i + 1]) - float(x[i]) * float(x[i])
                b = 1. - float(x[i])
                s += 100. * (a * a) + b * b
            return s
        return f
    if name == "ellipsoid":
        aux = [math.pow(10., 6. * ti) for ti in t]
        return lambda x: _seq(aux[i] * (float(x[i]) * float(x[i])) for i in range(n))
    if name == "cigar":
        return lambda x: float(x[0]) * float(x[0]) + 1.0e6 * _seq(float(v) * float(v) for v in x[1:])
    if name == "discus":
        return lambda x: 1.0e6 * (float(x[0]) * float(x[0])) + _seq(float(v) * float(v) for v in x[1:])
    if name == "schwefel12":
        def f(x):
            s = run = 0.
            for v in x:
                run += float(v)
                s += run * run
            return s
        return f
    raise ValueError(name)


def objective_rows(name, n):
    """the same objectives over the rows of X with NumPy sums (the `fast` model of large shapes)"""
    t = np.arange(n) / (n - 1) if n > 1 else np.zeros(n)
    if name == "sphere":
        return lambda X: (X * X).sum(1)
    if name == "rosenbrock":
        return lambda X: (100. * (X[:, 1:] - X[:, :-1] ** 2) ** 2 + (1. - X[:, :-1]) ** 2).sum(1)
    if name == "ellipsoid":
        aux = np.array([math.pow(10., 6. * ti) for ti in t])
        return lambda X: (aux * (X * X)).sum(1)
    raise ValueError(name)


class CholModel:
    """fast=True: sampling, the mean, the substitution and the objective (then a function of all
    rows, objective_rows) by NumPy matrix products instead of the reference's serial loops, which
    take minutes per generation at n >= 64.  The factor update stays selectable: "chain" walks the
    reference's mu + 1 rank-1 updates (vectorised over rows), "cholesky" factors C', "both" does
    both, keeps the chain's and records the largest difference"""

    def __init__(self, mfev, tol, stol, np_, sigma0=2., bound=False, ranked=False, factor="chain",
                 fast=False):
        self.mfev, self.tol, self.stol, self.lam = int(mfev), tol, stol, int(np_)
        self.sigma0, self.bound, self.ranked, self.factor = sigma0, bool(bound), bool(ranked), factor
        self.fast = bool(fast)
        self.max_factor_diff = 0.

    # BaseCmaes::init + CholeskyCmaes::init
    def init(self, f, lower, upper, guess):
        n = self.n = len(lower)
        lam = self.lam
        self.f = f
        self.lower, self.upper = np.array(lower, float), np.array(upper, float)
        self.mu = lam // 2
        self.mit = self.mfev // lam
        w = [math.log(0.5 * (lam + 1.)) - math.log(i + 1.) for i in range(self.mu)]
        inv = 1. / _seq(w)
        self.w = [wi * inv for wi in w]
        self.mueff = 1. / _seq(wi * wi for wi in self.w)
        me = self.mueff
        self.chi = math.sqrt(n) * (1. - 1. / (4. * n) + 1. / (21. * n * n))
        self.sigma = self.sigma0
        self.cc = (4. + me / n) / (n + 4. + 2. * me / n)
        self.cs = (me + 2.) / (5. + n + me)
        self.c1 = 2. / ((1.3 + n) * (1.3 + n) + me)
        self.cmu = min(1. - self.c1, 2. * (me - 2. + 1. / me) / ((2. + n) * (2. + n) + me))
        self.damps = 1. + self.cs + 2. * max(0., math.sqrt((me - 1.) / (n + 1.)) - 1.)
        self.pc, self.ps = np.zeros(n), np.zeros(n)
        self.xold = np.zeros(n)
        self.xmean = np.array(guess, float).copy()
        self.it = self.fev = 0
        self.hlen = 10 + int(math.ceil((30. * n) / lam))
        self.ik = int(math.ceil(0.1 + lam / 4.))
        self.hist = [0.] * self.hlen
        self.hbuf, self.hcount = -1, 0
        self.fbest, self.fworst = -math.inf, math.inf
        self.A = np.eye(n)
        self.arx = np.zeros((lam, n))
        self.fit_idx = np.zeros(lam, int)
        self.fit_val = np.zeros(lam)

    def _clamp(self, v):
        return np.maximum(self.lower, np.minimum(v, self.upper)) if self.bound else v

    def sample(self, z):
        z = np.asarray(z, float).reshape(self.lam, self.n)
        n = self.n
        if self.fast:
            self.arx = self._clamp(self.xmean + self.sigma * (z @ self.A.T))
            return
        for k in range(self.lam):
            for i in range(n):
                s = 0.
                for j in range(n):          # inner_product over the whole row (zeros above the diagonal)
                    s += self.A[i, j] * z[k, j]
                self.arx[k, i] = self.xmean[i] + self.sigma * s
            self.arx[k] = self._clamp(self.arx[k])

    def evaluate_sort(self, fvals=None):
        if fvals is not None:
            f = np.asarray(fvals, float)
        else:
            f = np.asarray(self.f(self.arx), float) if self.fast else np.array([self.f(x) for x in self.arx])
        self.fev += self.lam
        order = np.argsort(f, kind="stable")
        self.fit_idx, self.fit_val = order, f[order]

    def _rank1(self, M, v, beta):
        n = self.n
        v = v.copy()
        b = 1.
        for j in range(n):
            ajj, alfaj = M[j, j], v[j]
            gam = ajj * ajj * b + beta * alfaj * alfaj
            a1jj = M[j, j] = math.sqrt(gam / b)
            if j + 1 < n:
                v[j + 1:] -= (alfaj / ajj) * M[j + 1:, j]
                M[j + 1:, j] = (a1jj / ajj) * M[j + 1:, j] + (a1jj * beta * alfaj) / gam * v[j + 1:]
            b += beta * (alfaj / ajj) * (alfaj / ajj)

    def ys(self):
        """the mu vectors of the rank-mu term: the reference takes the FIRST mu candidates in
        sampling order about the NEW mean (cholesky_cmaes.cpp:91-94); ranked: the mu best about
        the old mean"""
        if self.ranked:
            return [(self.arx[self.fit_idx[i]] - self.xold) / self.sigma for i in range(self.mu)]
        return [(self.arx[i] - self.xmean) / self.sigma for i in range(self.mu)]

    def cprime(self):
        a = 1. - self.c1 - self.cmu
        Cp = a * (self.A @ self.A.T) + self.c1 * np.outer(self.pc, self.pc)
        if self.fast:
            Y = np.array(self.ys())
            return Cp + self.cmu * (Y.T * np.asarray(self.w)) @ Y
        for wi, y in zip(self.w, self.ys()):
            Cp += self.cmu * wi * np.outer(y, y)
        return Cp

    def update(self):
        n, mu = self.n, self.mu
        self.xold = self.xmean.copy()
        xm = np.zeros(n)
        if self.fast:
            xm = np.asarray(self.w) @ self.arx[self.fit_idx[:mu]]
        for i in range(0 if self.fast else n):
            s = 0.
            for r in range(mu):
                s += self.w[r] * self.arx[self.fit_idx[r], i]
            xm[i] = s
        self.xmean = self._clamp(xm)
        dmean = (self.xmean - self.xold) / self.sigma
        ccc = math.sqrt(self.cc * (2. - self.cc) * self.mueff)
        self.pc = (1. - self.cc) * self.pc + ccc * dmean
        if self.factor == "chain" or self.factor == "both":
            M = math.sqrt(1. - self.c1 - self.cmu) * np.tril(self.A)
            self._rank1(M, self.pc, self.c1)
            for wi, y in zip(self.w, self.ys()):
                self._rank1(M, y, self.cmu * wi)
        if self.factor != "chain":
            L = np.linalg.cholesky(self.cprime())
            if self.factor == "both":
                self.max_factor_diff = max(self.max_factor_diff, np.abs(L - M).max() / np.abs(M).max())
            else:
                M = L
        # forward substitution with the OLD factor
        t = dmean.copy()
        if self.fast:
            t = np.linalg.solve(self.A, dmean)
        for i in range(0 if self.fast else n):
            s = 0.
            for j in range(i):
                s += self.A[i, j] * t[j]
            t[i] = (t[i] - s) / self.A[i, i]
        csc = math.sqrt(self.cs * (2. - self.cs) * self.mueff)
        self.ps = (1. - self.cs) * self.ps + csc * t
        self.A = M
        # updateSigma, base_cmaes.cpp:176-189
        pslen = float(np.linalg.norm(self.ps)) if self.fast else math.sqrt(_seq(float(v) * float(v) for v in self.ps))
        self.sigma *= math.exp(min(1., (self.cs / self.damps) * (pslen / self.chi - 1.)))
        if self.fit_val[0] == self.fit_val[self.ik]:
            self.sigma *= math.exp(0.2 + self.cs / self.damps)
        if self.it >= self.hlen and self.fworst - self.fbest == 0.:
            self.sigma *= math.exp(0.2 + self.cs / self.damps)

    def update_history(self):
        if self.it < self.mit:
            self.hbuf = (self.hbuf + 1) % self.hlen
            self.hist[self.hbuf] = self.fit_val[0]
            self.hcount = min(self.hcount + 1, self.hlen)
            if self.hcount == self.hlen:
                self.fbest, self.fworst = min(self.hist), max(self.hist)
        self.it += 1

    def generation(self, z, fvals=None):
        self.sample(z)
        self.evaluate_sort(fvals)
        self.update()
        self.update_history()

    def spread_parts(self):
        """the two parts of CholeskyCmaes::converged (:137-161)"""
        part1 = abs(self.fit_val[0] - self.fit_val[-1]) <= self.tol
        if self.fast:
            r = np.linalg.norm(self.arx, axis=1)
            return part1, ((r - r.mean()) ** 2).sum() <= (self.lam - 1) * self.stol * self.stol
        count, mean, m2 = 0, 0., 0.
        for x in self.arx:
            r = math.sqrt(_seq(float(v) * float(v) for v in x))
            count += 1
            delta = r - mean
            mean += delta / count
            m2 += delta * (r - mean)
        return part1, m2 <= (self.lam - 1) * self.stol * self.stol

    def converged(self):
        a, b = self.spread_parts()
        return bool(a and b)

    def best(self):
        return self.xmean if self.it <= 0 else self.arx[self.fit_idx[0]]

    def optimize(self, f, lower, upper, guess, rng):
        """BaseCmaes::optimize with NumPy normals"""
        self.init(f, lower, upper, guess)
        conv = False
        while self.fev < self.mfev:
            self.generation(rng.standard_normal(self.lam * self.n))
            if self.converged():
                conv = True
                break
        return self.best().copy(), self.fev, conv
