"""NumPy restatement of the reference's Hees (Glasmachers & Krause 2020;
src/multivariate/hees/hees.cpp), written from its description, in two forms:

  iterate_reference(words)   the reference's own order: B n normal rows from the raw mt19937 words
                     (`jaya_model.Words.normal`, whose spare value outlives a generation like the
                     reference's `_Z`), every batch orthonormalised by its left-looking modified
                     Gram-Schmidt, G = (1/B) sum_i c_i b^_i b^_i^T over all rows, A <- A G, the mean
                     as sum w x.  Serial Python floats: the same IEEE operations in the same order
                     (only libm's log / exp / sqrt are shared, not restated).  `normals=` takes the
                     rows instead of the words, and `fast=True` does the sums with NumPy for the
                     shapes where the serial loops take minutes (same algorithm, other rounding).
  iterate_device(z)          the device's form: only the first mu rows exist; per batch the live
                     rows are orthonormalised; A += Y^T diag((q - 1) / (|z|^2 B)) b with Y = b A^T
                     (each batch is a complete orthonormal basis and c_i = 1 for i >= mu, so this is
                     A G); m += sigma Y^T dw with dw_i = w_rank(i + mu) - w_rank(i); dz = b^T dw;
                     norms as plain root sums of squares; ties rank to the lower index; a NaN value
                     counts as +inf; converged() as a two-pass sum.

run_reference / run_device restate optimize(), restarts included."""
import math

import numpy as np

from jaya_model import dnrm2

INF = float("inf")


def adaptive_mu(n):
    return int(2. + 1.5 * math.log(1. * n))


def ranks_of(f):
    """rank of every index, ties to the lower index"""
    order = sorted(range(len(f)), key=lambda i: (f[i], i))
    rank = [0] * len(f)
    for r, i in enumerate(order):
        rank[i] = r
    return rank, order


class Hees:
    def __init__(self, fobj, n, np_=0, sigma0=2., tol=0., mfev=10 ** 9):
        self.fobj, self.n = fobj, int(n)
        self.mu = int(np_) if np_ > 0 else adaptive_mu(n)
        self.sigma0, self.tol, self.mfev = float(sigma0), float(tol), int(mfev)

    # ---- init, hees.cpp:49-122 ----------------------------------------------------------------
    def init(self, guess):
        n, mu = self.n, self.mu
        self.m = [float(v) for v in guess][:n]
        self.fm = self._f(self.m)
        self.fev = 1
        self.xbest, self.fbest = list(self.m), self.fm
        self.B = int(math.ceil((1. * mu) / n))
        self.np = self.B * n
        self.sigma, self.kappa, self.etaA, self.gs = self.sigma0, 3., 0.5, 0.
        self.chi = math.sqrt(1. * n) * (1. - 1. / (4. * n) + 1. / (21. * n * n))
        w, wsum = [], 0.
        for i in range(2 * mu):
            w.append(math.log(mu + 0.5) - math.log(min(1. + i, mu + 0.5)))
            wsum += w[i]
        scale = 1. / wsum
        w = [v * scale for v in w]
        w2 = 0.
        for v in w:
            w2 += v * v
        self.w = w
        self.mueff = 1. / w2
        self.mueffm = 1. / (1. / self.mueff - 1. / (2. * mu - 1.) * (1. - 1. / self.mueff))
        self.cs = (self.mueffm + 2.) / (n + self.mueffm + 3.)
        self.ds = 1. + self.cs + 2. * max(0., math.sqrt((self.mueff - 1.) / (n + 1.)) - 1.)
        self.ps = [0.] * n
        self.norms = [0.] * self.np
        self.hess, self.q = [0.] * mu, [0.] * mu
        self.A = np.eye(n)
        self.b = np.zeros((self.np, n))
        self.x = np.zeros((2 * mu, n))
        self.y = np.zeros((mu, n))
        self.f = [0.] * (2 * mu)
        self.rank = [0] * (2 * mu)
        self.order = list(range(2 * mu))
        self.it = 0
        self.skipped = False
        return self

    def _f(self, x):
        return float(self.fobj(x))

    def converged(self):
        """hees.cpp:366-382, Welford"""
        count, mean, m2 = 0, 0., 0.
        for v in self.f:
            count += 1
            delta = v - mean
            mean += delta / count
            m2 += delta * (v - mean)
        return m2 <= count * self.tol * self.tol

    def converged_device(self):
        """the device's two-pass sum of the same spread"""
        f = np.asarray(self.f, float)
        with np.errstate(invalid="ignore"):
            m2 = float(((f - f.sum() / f.size) ** 2).sum())
        return m2 <= f.size * self.tol * self.tol

    # ---- the scalars both forms share -----------------------------------------------------------
    def _curvature(self, norms):
        """hees.cpp:264-292: h, max h, the trust region, q; False when A is to be left alone"""
        mu = self.mu
        maxh = -INF
        for i in range(mu):
            self.hess[i] = (self.f[i + mu] + self.f[i] - 2. * self.fm) / (norms[i] * norms[i])
            if maxh < self.hess[i]:
                maxh = self.hess[i]
        self.maxh = maxh
        if maxh <= 0.:
            return False
        ctrust = maxh / self.kappa
        meanq = 0.
        for i in range(mu):
            if self.hess[i] < ctrust:
                self.hess[i] = ctrust
            self.q[i] = math.log(self.hess[i]) if self.hess[i] < INF else INF
            meanq += self.q[i] / mu
        for i in range(mu):
            v = self.q[i] - meanq
            v *= (-self.etaA * 0.5)
            self.q[i] = math.exp(v) if v == v else v
        return True

    def _step_size(self, dz):
        """hees.cpp:354-363"""
        n = self.n
        csc = math.sqrt(self.cs * (2. - self.cs) * self.mueffm)
        for i in range(n):
            self.ps[i] = (1. - self.cs) * self.ps[i] + csc * float(dz[i])
        self.gs = ((1. - self.cs) * (1. - self.cs)) * self.gs + self.cs * (2. - self.cs)
        return csc

    def _incumbent(self):
        if self.fm < self.fbest:
            self.fbest, self.xbest = self.fm, list(self.m)

    # ---- the reference's order ----------------------------------------------------------------
    def iterate_reference(self, words=None, normals=None, fast=False):
        n, mu, B, npts = self.n, self.mu, self.B, self.np
        if normals is None:
            z = [[words.normal() for _ in range(n)] for _ in range(npts)]
        else:
            z = np.asarray(normals, float).reshape(npts, n).tolist()
        self.z = np.array(z)
        if fast:
            return self._iterate_reference_fast()
        b = [list(r) for r in z]
        norms = [dnrm2(r) for r in b]
        for j in range(B):                                  # :212-224
            for i in range(n):
                vi = b[n * j + i]
                for k in range(i):
                    vk = b[n * j + k]
                    dt = 0.
                    for t in range(n):
                        dt += vk[t] * vi[t]
                    if -dt != 0.:                           # daxpym leaves on a zero factor
                        for t in range(n):
                            vi[t] += (-dt) * vk[t]
                inv = 1. / dnrm2(vi)
                for t in range(n):
                    vi[t] *= inv
        for i in range(npts):                               # :227-229
            for t in range(n):
                b[i][t] *= norms[i]
        A = self.A.tolist()
        x = [[0.] * n for _ in range(2 * mu)]
        for p in range(mu):                                 # :232-239
            for i in range(n):
                dot = 0.
                for t in range(n):
                    dot += A[i][t] * b[p][t]
                x[p][i] = self.m[i] - self.sigma * dot
                x[p + mu][i] = self.m[i] + self.sigma * dot
        self.f = [self._f(x[i]) for i in range(2 * mu)]    # :245-259
        self.fev += 2 * mu
        self.rank, self.order = ranks_of(self.f)
        self.skipped = not self._curvature(norms)
        if not self.skipped:                                # :295-321
            G = [[0.] * n for _ in range(n)]
            for r in range(n):
                for c in range(n):
                    g = 0.
                    for i in range(npts):
                        ci = self.q[i] if i < mu else 1.
                        g += ci / (norms[i] * norms[i] * B) * b[i][r] * b[i][c]
                    G[r][c] = g
            An = [[0.] * n for _ in range(n)]
            for r in range(n):
                for c in range(n):
                    a = 0.
                    for t in range(n):
                        a += A[r][t] * G[t][c]
                    An[r][c] = a
            A = An
        m = [0.] * n                                        # :327-339
        for i in range(2 * mu):
            wk = self.w[self.rank[i]]
            if wk != 0.:
                for t in range(n):
                    m[t] += wk * x[i][t]
        self.m = m
        self.fm = self._f(m)
        self.fev += 1
        self._incumbent()
        dz = [0.] * n                                       # :345-353
        for i in range(mu):
            wm, wp = self.w[self.rank[i]], self.w[self.rank[i + mu]]
            if -wm != 0.:
                for t in range(n):
                    dz[t] += (-wm) * b[i][t]
            if wp != 0.:
                for t in range(n):
                    dz[t] += wp * b[i][t]
        self._step_size(dz)
        s = dnrm2(self.ps) / self.chi - math.sqrt(self.gs)
        self.sigma *= math.exp(min(1., self.cs / self.ds * s))
        self.A, self.b, self.x, self.norms = np.array(A), np.array(b), np.array(x), norms
        self.it += 1

    def _iterate_reference_fast(self):
        n, mu, B, npts = self.n, self.mu, self.B, self.np
        b = self.z.copy()
        norms = np.sqrt((b * b).sum(1))
        for j in range(B):
            for i in range(n):
                vi = b[n * j + i]
                for k in range(i):
                    vk = b[n * j + k]
                    vi -= (vk @ vi) * vk
                vi /= math.sqrt(vi @ vi)
        b *= norms[:, None]
        Y = b[:mu] @ self.A.T
        m = np.array(self.m)
        x = np.vstack([m - self.sigma * Y, m + self.sigma * Y])
        self.f = [self._f(r) for r in x]
        self.fev += 2 * mu
        self.rank, self.order = ranks_of(self.f)
        self.skipped = not self._curvature(norms)
        if not self.skipped:
            c = np.ones(npts)
            c[:mu] = self.q
            G = (b.T * (c / (norms * norms * B))) @ b
            self.A = self.A @ G
        wr = np.array(self.w)[self.rank]
        self.m = (wr @ x).tolist()
        self.fm = self._f(self.m)
        self.fev += 1
        self._incumbent()
        dz = (wr[mu:] - wr[:mu]) @ b[:mu]
        self._step_size(dz)
        s = math.sqrt(sum(v * v for v in self.ps)) / self.chi - math.sqrt(self.gs)
        self.sigma *= math.exp(min(1., self.cs / self.ds * s))
        self.b, self.x, self.norms, self.y = b, x, norms.tolist(), Y
        self.it += 1

    # ---- the device's form --------------------------------------------------------------------
    def ortho_device(self, z):
        """the live rows of every batch, orthonormalised; returns (unit rows, norms of z)"""
        n, mu = self.n, self.mu
        u = np.array(z, float).reshape(mu, n)
        norms = np.sqrt((u * u).sum(1))
        for r0 in range(0, mu, n):
            rows = min(n, mu - r0)
            for k in range(rows):
                vk = u[r0 + k]
                vk /= math.sqrt(vk @ vk)
                if k + 1 < rows:
                    rest = u[r0 + k + 1:r0 + rows]
                    rest -= np.outer(rest @ vk, vk)
        return u, norms

    def iterate_device(self, z, fvals=None, fmean=None):
        """z: the mu x n normals.  fvals / fmean: the 2 mu values and f(m) where the caller has
        them (a crafted objective), else the objective is called in the reference's order"""
        n, mu, B = self.n, self.mu, self.B
        u, norms = self.ortho_device(z)
        self.unit = u.copy()
        b = u * norms[:, None]
        Y = b @ self.A.T
        m = np.array(self.m)
        x = np.vstack([m - self.sigma * Y, m + self.sigma * Y])
        f = [self._f(r) for r in x] if fvals is None else [float(v) for v in fvals]
        self.f = [INF if v != v else v for v in f]
        self.fev += 2 * mu
        self.rank, self.order = ranks_of(self.f)
        with np.errstate(all="ignore"):
            self.skipped = not self._curvature(norms)
            if not self.skipped:
                coef = (np.array(self.q) - 1.) / (norms * norms * B)
                self.A = self.A + Y.T @ (coef[:, None] * b)
        wr = np.array(self.w)[self.rank]
        dw = wr[mu:] - wr[:mu]
        self.m = (m + self.sigma * (dw @ Y)).tolist()
        fm = self._f(self.m) if fmean is None else float(fmean)
        self.fm = INF if fm != fm else fm
        self.fev += 1
        self._incumbent()
        self._step_size(dw @ b)
        s = math.sqrt(sum(v * v for v in self.ps)) / self.chi - math.sqrt(self.gs)
        self.sigma *= math.exp(min(1., self.cs / self.ds * s))
        self.b, self.x, self.norms, self.y = b, x, norms.tolist(), Y
        self.it += 1


# ---- optimize(), hees.cpp:136-199 -------------------------------------------------------------
def _single_reference(fobj, n, guess, words, mfev, tol, np_, sigma0):
    """:140-151; a fresh Hees: its `_Z` starts without a spare value"""
    words.have = False
    h = Hees(fobj, n, np_, sigma0, tol, mfev).init(guess)
    h.conv = False
    while h.fev < mfev:
        h.iterate_reference(words)
        if h.converged():
            h.conv = True
            break
    return h


def run_reference(fobj, n, lower, upper, guess, words, mfev, tol, mres=1, np_=0, sigma0=2.):
    """the reference's optimize() over the recorded words: (x, n_evals, converged, rows), rows =
    the (res, fbest, fev) its table prints"""
    if mres <= 1:
        h = _single_reference(fobj, n, guess, words, mfev, tol, np_, sigma0)
        return h.xbest, h.fev, h.conv, []
    mu = np_ if np_ > 0 else adaptive_mu(n)
    fev, fbest, xbest, rows = 0, INF, [float(v) for v in guess], []
    x0 = [float(v) for v in guess]
    for res in range(1, mres + 1):
        h = _single_reference(fobj, n, x0, words, mfev - fev, tol, mu, sigma0)
        if h.fbest < fbest:
            fbest, xbest = h.fbest, list(h.xbest)
        fev += h.fev
        rows.append((res, fbest, fev))
        if fev >= mfev:
            break
        mu <<= 1
        x0 = [words.uniform(float(lower[i]), float(upper[i])) for i in range(n)]
    return xbest, fev, False, rows


def run_device(fobj, n, guess, draw, mfev, tol=0., np_=0, sigma0=2.):
    """one run of the device's form: draw(generation, mu, n) -> the mu x n normals of a generation.
    Returns the model at its stop (flag 1 = converged, 2 = budget), like bbo_run."""
    h = Hees(fobj, n, np_, sigma0, tol, mfev).init(guess)
    h.flag = 0
    while h.fev < mfev:
        h.iterate_device(draw(h.it, h.mu, n))
        if h.converged_device():
            h.flag = 1
            break
    if not h.flag:
        h.flag = 2
    return h
