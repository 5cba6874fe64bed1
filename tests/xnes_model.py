"""NumPy restatement of xNES, the exponential natural evolution strategy (Glasmachers, Schaul, Yi,
Wierstra & Schmidhuber 2010) as the reference's src/multivariate/nes/xnes.cpp runs it, written from
the algorithm, in two forms that take the normals of a generation (np rows, sampling order):

  iterate_reference(z)   the reference's order: the ranked normals, the dense gradient
                     G = sum_i u_i (z_i z_i^T - I), G_sigma = tr G / n, G_B = G - G_sigma I, the mean with
                     the old sigma and B, sigma, then B <- B exp(eta_B G_B / 2) with the exponential of
                     the symmetric matrix through numpy's eigh: V e^Lambda V^T.
  iterate_device(z)      the device's form (bbo_xnes.hpp): Y = Z B^T is kept, the mean moves by
                     eta_mu sigma sum_k u_k y_k, G_sigma = sum_k u_k |z_k|^2 / n (sum u = 0), and the
                     update of B takes one of two routes:
                       low-rank (n >= lowrank_min_n)  K = Zs Zs^T = L L^T, S = L^T U L = W Lambda W^T,
                                 T = L^-T W, H = T (e^{c Lambda} - 1) T^T,
                                 B <- e^{-c G_sigma} (B + Ys^T H Zs),  c = eta_B / 2;
                                 a pivot that is not finite or not above 2^-40 K_jj leaves B alone
                                 and counts in fact_fail
                       dense     G_B = Zs^T U Zs - G_sigma I = V Lambda V^T, B <- B V e^{c Lambda} V^T
                     The sums the ranking or the factorisation can feel are added in the device's
                     order: a row of 64 lanes strided over the coordinates, then the xor butterfly
                     (`wave_sum`), for |z_k|^2, K and the built-in objectives of `device_objective`;
                     G_sigma and the mean are added rank by rank.  Ties rank to the lower index, a
                     NaN value counts as +inf.  The small eigenproblem is numpy's eigh (the device
                     runs a cyclic Jacobi; both are accurate to a few ulp of the matrix norm).

run_* restate optimize(): `while fev < mfev: iterate(); if converged: break`."""
import math

import numpy as np

INF = float("inf")
PIVOT_FLOOR = 2. ** -40


def popsize(n):
    return 4 + int(3. * math.log(n))


def utilities(np_):
    u = [max(0., math.log(1 + 0.5 * np_) - math.log(i)) for i in range(1, np_ + 1)]
    s = 0.
    for v in u:
        s += v
    return np.array([v / s - (1. / np_) for v in u])


def wave_sum(v):
    """sum of v as a wavefront adds it: lane l takes v[l], v[l + 64], ... in turn, then the xor
    butterfly over the 64 lanes (what lane 0 holds; every lane holds the same bits)"""
    v = np.asarray(v, float)
    part = np.zeros(64)
    for j0 in range(0, v.size, 64):
        chunk = v[j0:j0 + 64]
        part[:chunk.size] += chunk
    idx = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        part = part + part[idx ^ off]
    return float(part[0])


def device_objective(name, n):
    """sphere, rosenbrock and ellipsoid over the rows of X in the device's order (eval_row_group)"""
    t = np.arange(n) / (n - 1) if n > 1 else np.zeros(n)
    aux = np.array([math.pow(10., 6. * v) for v in t])

    def terms(x):
        if name == "sphere":
            return x * x
        if name == "rosenbrock":
            a, b = x[1:] - x[:-1] * x[:-1], 1. - x[:-1]
            return 100. * (a * a) + b * b
        if name == "ellipsoid":
            return aux * (x * x)
        raise ValueError(name)

    return lambda X: np.array([wave_sum(terms(np.asarray(x, float))) for x in np.atleast_2d(X)])


def rank_order(f):
    """rank -> index, ties to the lower index, NaN as +inf"""
    f = [INF if v != v else float(v) for v in f]
    return sorted(range(len(f)), key=lambda i: (f[i], i))


class XNes:
    def __init__(self, frows, n, a0=1., etamu=1., tol=0., mfev=10 ** 9, lowrank_min_n=32):
        self.frows, self.n = frows, int(n)
        self.a0, self.etamu, self.tol, self.mfev = float(a0), float(etamu), float(tol), int(mfev)
        self.lowrank_min_n = int(lowrank_min_n)

    def init(self, guess=None):
        """the mean starts at the origin (the reference ignores the guess); `guess`: from_guess"""
        n = self.n
        self.np = popsize(n)
        self.etasigma = 3. * (3. + math.log(n)) / (5. * n * math.sqrt(n))
        self.etab = self.etasigma
        self.u = utilities(self.np)
        self.mu = np.zeros(n) if guess is None else np.array(guess, float)[:n].copy()
        self.sigma = self.a0
        self.B = np.eye(n)
        self.x = np.zeros((self.np, n))
        self.y = np.zeros((self.np, n))
        self.z = np.zeros((self.np, n))
        self.f = np.zeros(self.np)
        self.order = list(range(self.np))
        self.gsigma = 0.
        self.it = self.fev = 0
        self.fbest, self.xbest = INF, np.zeros(n)
        self.fact_fail, self.skipped = 0, False
        self.route = 1 if n >= self.lowrank_min_n else 0
        self.conv, self.stop = 0. < self.tol, 0     # the points are zeros: |f_best - f_worst| = 0
        return self

    # ---- what both forms share ---------------------------------------------------------------
    def _evaluate(self, z):
        z = np.asarray(z, float).reshape(self.np, self.n)
        self.z = z.copy()
        self.y = z @ self.B.T
        self.x = self.mu + self.sigma * self.y
        f = np.asarray(self.frows(self.x), float).copy()
        f[f != f] = INF
        self.f = f
        self.order = rank_order(f)

    def _finish(self):
        o = self.order
        if self.f[o[0]] < self.fbest:
            self.fbest, self.xbest = float(self.f[o[0]]), self.x[o[0]].copy()
        self.it += 1
        self.fev += self.np
        self.conv = bool(abs(self.f[o[0]] - self.f[o[-1]]) < self.tol)
        if self.conv:
            self.stop = 1
        elif self.fev >= self.mfev:
            self.stop = 2

    def solution(self):
        return self.x[self.order[0]]

    # ---- form (a) ------------------------------------------------------------------------------
    def iterate_reference(self, z):
        n, u = self.n, self.u
        self._evaluate(z)
        zs = self.z[self.order]
        gdelta = u @ zs
        G = (zs.T * u) @ zs - u.sum() * np.eye(n)
        self.gsigma = float(np.trace(G)) / n
        G = G - self.gsigma * np.eye(n)
        self.mu = self.mu + self.etamu * self.sigma * (self.B @ gdelta)
        self.sigma = self.sigma * math.exp(0.5 * self.etasigma * self.gsigma)
        C = 0.5 * self.etab * G
        C = 0.5 * (C + C.T)
        lam, V = np.linalg.eigh(C)
        self.B = self.B @ ((V * np.exp(lam)) @ V.T)
        self.skipped = False
        self._finish()

    # ---- form (b) ------------------------------------------------------------------------------
    def _cholesky(self, K):
        """the device's column Cholesky with its pivot test; None when a pivot fails"""
        m = K.shape[0]
        L = np.zeros_like(K)
        for j in range(m):
            piv = K[j, j]
            for k in range(j):
                piv -= L[j, k] * L[j, k]
            if not (piv > K[j, j] * PIVOT_FLOOR) or not (piv < INF):
                return None
            L[j, j] = math.sqrt(piv)
            for i in range(j + 1, m):
                s = K[i, j]
                for k in range(j):
                    s -= L[i, k] * L[j, k]
                L[i, j] = s / L[j, j]
        return L

    def iterate_device(self, z):
        n, np_, u = self.n, self.np, self.u
        self._evaluate(z)
        o = self.order
        zs, ys = self.z[o], self.y[o]
        gd = np.zeros(n)
        for k in range(np_):
            gd = gd + u[k] * ys[k]
        self.mu = self.mu + (self.etamu * self.sigma) * gd
        nz2 = [wave_sum(zs[k] * zs[k]) for k in range(np_)]
        gs = 0.
        for k in range(np_):
            gs += u[k] * nz2[k]
        gs /= n
        self.gsigma = gs
        self.sigma = self.sigma * math.exp(0.5 * self.etasigma * gs)
        c = 0.5 * self.etab
        self.skipped = False
        if self.route:
            K = np.zeros((np_, np_))
            for a in range(np_):
                for b in range(a, np_):
                    K[a, b] = K[b, a] = wave_sum(zs[a] * zs[b])
            L = self._cholesky(K)
            if L is None:
                self.fact_fail += 1
                self.skipped = True
            else:
                S = L.T @ (u[:, None] * L)
                S = 0.5 * (S + S.T)
                lam, W = np.linalg.eigh(S)
                T = np.linalg.solve(L.T, W)
                H = (T * np.expm1(c * lam)) @ T.T
                self.B = math.exp(-c * gs) * (self.B + ys.T @ (H @ zs))
        else:
            G = (zs.T * u) @ zs - gs * np.eye(n)
            G = 0.5 * (G + G.T)
            lam, V = np.linalg.eigh(G)
            self.B = self.B @ ((V * np.exp(c * lam)) @ V.T)
        self._finish()


def run(model, draws, form="device"):
    """optimize(): generations until converged or the budget; draws(gen) -> the np x n normals"""
    step = model.iterate_device if form == "device" else model.iterate_reference
    gen = 0
    while model.fev < model.mfev:
        step(draws(gen))
        gen += 1
        if model.conv:
            break
    return model
