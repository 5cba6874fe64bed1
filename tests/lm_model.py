"""NumPy restatement of the reference's LmCmaes (Loshchilov 2014 / 2015;
src/multivariate/cma/lm_cmaes.cpp over base_cmaes.cpp), written from its description, in two forms:

  device=False  the reference form: every sum runs left to right in Python floats where the
                reference's does (std::inner_product, the blas loops, the +- n / lambda sum of the
                sigma rule).  tests/test_lm_model.py holds it against tests/golden/lm_runs.json bit
                for bit.
  device=True   the device form: a dot product over n is what the kernels of bbo_lm_kernels.hpp add --
                thread t of 256 sums the terms t, t + 256, ... in order, a xor butterfly adds the 64
                lanes of a wavefront, the four wavefronts are added left to right; the built-in
                objectives are eval_row_group<64>'s (lane l sums the terms l, l + 64, ...); the
                numerator of the sigma rule is an exact integer.  Everything else (the folds per
                coordinate, the weighted mean over the ranks, pc) is the same operation in the same
                order in both forms.

The draws are arguments: per generation ceil(lambda / 2) rows of n + 1 values, z of a "+" candidate
and the normal g of selectSubset (ignored where the reference draws none)."""
import math

import numpy as np

import chol_model

FLAG_MAXITER, FLAG_TOLHISTFUN, FLAG_EQUALFUNVALS, FLAG_SIGMA = 1, 2, 3, 11
_LANE = np.arange(64)


def seq_dot(a, b):
    s = 0.
    for x, y in zip(a.tolist(), b.tolist()):
        s += x * y
    return s


def _butterfly(w):
    """xor butterfly over the last axis (64 lanes): every lane ends with the same bits"""
    for off in (32, 16, 8, 4, 2, 1):
        w = w + w[..., _LANE ^ off]
    return w[..., 0]


def dev_dot(a, b):
    """sum a_j b_j as a workgroup of 256 threads adds it (module text)"""
    n = a.size
    nr = (n + 255) // 256
    prod = np.zeros(nr * 256)
    prod[:n] = a * b
    acc = np.zeros(256)
    for r in range(nr):
        acc = acc + prod[256 * r:256 * (r + 1)]
    w = _butterfly(acc.reshape(4, 64))
    return float(((w[0] + w[1]) + w[2]) + w[3])


def _lane_sum(terms):
    """eval_row_group<64>: lane l adds the terms l, l + 64, ... in order, then the butterfly"""
    n = terms.size
    nr = (n + 63) // 64
    t = np.zeros(nr * 64)
    t[:n] = terms
    acc = np.zeros(64)
    for r in range(nr):
        acc = acc + t[64 * r:64 * (r + 1)]
    return float(_butterfly(acc))


def device_objective(name, n):
    """the built-in objectives in the operation order of bbo_objectives.hpp"""
    t = np.array([(i / (n - 1) if n > 1 else 0.) for i in range(n)])
    if name == "sphere":
        return lambda x: _lane_sum(x * x)
    if name == "rosenbrock":
        def f(x):
            a = x[1:] - x[:-1] * x[:-1]
            b = 1. - x[:-1]
            return _lane_sum(100. * (a * a) + b * b)
        return f
    if name == "ellipsoid":
        aux = np.array([math.pow(10., 6. * ti) for ti in t])
        return lambda x: _lane_sum(aux * (x * x))
    if name == "cigar":
        def f(x):
            sq = x * x
            sq[0] = 0.      # (lane 0 skips j = 0: it adds nothing there)
            return float(x[0]) * float(x[0]) + 1.0e6 * _lane_sum(sq)
        return f
    raise ValueError(name)


def default_memory(n):
    return int(2. * math.sqrt(1. * n))


class LmModel:
    def __init__(self, mfev, tol, np_, memory=0, sigma0=2., bound=False, usenew=True, device=False):
        self.mfev, self.tol, self.lam, self.memory = int(mfev), float(tol), int(np_), int(memory)
        self.sigma0, self.bound, self.usenew, self.device = float(sigma0), bool(bound), bool(usenew), bool(device)
        self.dot = dev_dot if device else seq_dot

    def init(self, f, lower, upper, guess):
        """f: a callable of one point, or the name of a built-in (in the form's own order)"""
        self.lower, self.upper = np.array(lower, float), np.array(upper, float)
        n = self.n = self.lower.size
        if isinstance(f, str):
            f = device_objective(f, n) if self.device else chol_model.objective(f, n)
        self.f = f
        lam = self.lam
        mu = self.mu = lam // 2
        self.mit = self.mfev // lam
        w = [math.log(0.5 * (lam + 1.)) - math.log(i + 1.) for i in range(mu)]
        s = 0.
        for v in w:
            s += v
        w = [v * (1. / s) for v in w]
        lenw = 0.
        for v in w:
            lenw += v * v
        self.w, self.mueff = w, 1. / lenw
        m = self.m = self.memory if self.memory > 0 else default_memory(n)
        if self.usenew:
            self.nsteps, self.t, self.cc = n, max(1, int(math.log(1. * n))), 0.5 / math.sqrt(1. * n)
        else:
            self.nsteps, self.t, self.cc = m, 1, 1. / m
        self.cs, self.c1 = 0.3, 0.1 / math.log(n + 1.)
        self.ccc = math.sqrt(self.cc * (2. - self.cc) * self.mueff)
        self.damps, self.sqrt1mc1, self.zstar = 1., math.sqrt(1. - self.c1), 0.25
        self.sigma, self.s, self.memlen = self.sigma0, 0., 0
        self.jarr, self.larr = [0] * m, [0] * m
        self.b, self.d = np.zeros(m), np.zeros(m)
        self.fp = np.zeros(lam)
        self.pcmat, self.vmat = np.zeros((m, n)), np.zeros((m, n))
        self.pc, self.xold = np.zeros(n), np.zeros(n)
        self.xmean = np.array(guess, float)[:n].copy()
        self.arx = np.zeros((lam, n))
        self.fit_val, self.fit_idx = np.zeros(lam), np.zeros(lam, int)
        self.it = self.fev = 0
        self.hlen = 10 + int(math.ceil((30. * n) / lam))
        self.ik = int(math.ceil(0.1 + lam / 4.))
        self.hbest, self.hkth, self.hbuf, self.hcount = [0.] * self.hlen, [0.] * self.hlen, -1, 0
        self.fbest, self.fworst = -math.inf, math.inf
        self.last_branch = None

    # ---- lm_cmaes.cpp:304-318 -------------------------------------------------------------------
    def select_subset(self, k, g):
        m = self.memlen
        if m <= 1:
            return 0
        msigma = 40 if k == 0 else 4
        return m - int(min(msigma * abs(g), float(m)))

    # ---- :88-127 --------------------------------------------------------------------------------
    def sample(self, draws):
        draws = np.asarray(draws, float).reshape((self.lam + 1) // 2, self.n + 1)
        for k in range(self.lam):
            if k % 2 == 0:
                z = draws[k // 2, :self.n].copy()
                az = z.copy()
                i0 = self.select_subset(k, draws[k // 2, self.n]) if self.usenew else 0
                for i in range(i0, self.memlen):
                    j = self.jarr[i]
                    dot = self.b[j] * self.dot(self.vmat[j], z)
                    az = self.sqrt1mc1 * az
                    if dot != 0.:
                        az = az + dot * self.pcmat[j]
            sign = 1. if k % 2 == 0 else -1.
            self.arx[k] = self.xmean + (sign * self.sigma) * az

    # ---- :215-226, base_cmaes.cpp:211-230 ---------------------------------------------------------
    def evaluate_sort(self, fvals=None):
        if self.it > 0:
            self.fp = self.fit_val.copy()
        f = np.array([self.f(x) for x in self.arx], float) if fvals is None else np.array(fvals, float)
        if self.device:
            f[np.isnan(f)] = np.inf
        self.fev += self.lam
        self.fit_idx = np.argsort(f, kind="stable")
        self.fit_val = f[self.fit_idx]

    # ---- :274-302 -------------------------------------------------------------------------------
    def update_set(self):
        m, it = self.m, self.it // self.t
        jarr, larr = self.jarr, self.larr
        imin = 1
        self.last_branch = "fill"
        if it < m:
            jarr[it] = it
        elif m > 1:
            iminval = larr[jarr[1]] - larr[jarr[0]]
            for i in range(1, m - 1):
                val = larr[jarr[i + 1]] - larr[jarr[i]]
                if val < iminval:
                    iminval, imin = val, i + 1
            self.last_branch = "remove"
            if iminval >= self.nsteps:
                imin = 0
                self.last_branch = "drop0"
            jtmp = jarr[imin]
            for i in range(imin, m - 1):
                jarr[i] = jarr[i + 1]
            jarr[m - 1] = jtmp
        else:
            self.last_branch = "single"
        larr[jarr[min(it, m - 1)]] = self.it
        return 0 if imin == 1 else imin

    # ---- :260-272 -------------------------------------------------------------------------------
    def ainvz(self, a, jlen):
        c = 1. / self.sqrt1mc1
        for i in range(jlen):
            idx = self.jarr[i]
            dot = self.d[idx] * self.dot(self.vmat[idx], a)
            a = c * a
            if -dot != 0.:
                a = a + (-dot) * self.vmat[idx]
        return a

    # ---- :129-181 -------------------------------------------------------------------------------
    def update(self):
        n = self.n
        self.xold = self.xmean.copy()
        xm = np.zeros(n)
        for r in range(self.mu):
            xm = xm + self.w[r] * self.arx[self.fit_idx[r]]
        if self.bound:
            xm = np.maximum(self.lower, np.minimum(xm, self.upper))
        self.xmean = xm
        self.pc = (1. - self.cc) * self.pc + (self.ccc * (self.xmean - self.xold)) / self.sigma
        self.last_branch = None
        if self.it % self.t == 0:
            imin = self.update_set()
            if self.memlen < self.m:
                self.memlen += 1
            self.pcmat[self.jarr[self.memlen - 1]] = self.pc
            for i in range(imin, self.memlen):
                jcur = self.jarr[i]
                a = self.ainvz(self.pcmat[jcur].copy(), i)
                self.vmat[jcur] = a
                vnrm2 = self.dot(a, a)
                sqrtc1 = math.sqrt(1. + (self.c1 / (1. - self.c1)) * vnrm2)
                self.b[jcur] = (self.sqrt1mc1 / vnrm2) * (sqrtc1 - 1.)
                self.d[jcur] = (1. / (self.sqrt1mc1 * vnrm2)) * (1. - 1. / sqrtc1)
        self.update_sigma()

    # ---- :228-258 -------------------------------------------------------------------------------
    def update_sigma(self):
        if self.it == 0:
            return
        lam = self.lam
        if self.device:
            # both lists are sorted: the pooled rank of an element is its own place plus the number
            # of elements of the other list in front of it (a previous value precedes an equal
            # current one)
            prev = np.arange(lam) + np.searchsorted(self.fit_val, self.fp, side="left")
            cur = np.arange(lam) + np.searchsorted(self.fp, self.fit_val, side="right")
            zpsr = float(int(prev.sum()) - int(cur.sum())) / (float(lam) * float(lam)) - self.zstar
        else:
            vals = np.concatenate([self.fp, self.fit_val])
            order = np.argsort(vals, kind="stable")
            zpsr = 0.
            for pos, idx in enumerate(order.tolist()):
                fr = (1. * pos) / lam
                zpsr = zpsr + fr if idx < lam else zpsr - fr
            zpsr /= 1. * lam
            zpsr -= self.zstar
        self.s = (1. - self.cs) * self.s + self.cs * zpsr
        self.sigma *= math.exp(self.s / self.damps)

    # ---- base_cmaes.cpp:191-209 -------------------------------------------------------------------
    def update_history(self):
        if self.it >= self.mit:
            return
        self.hbuf = (self.hbuf + 1) % self.hlen
        self.hbest[self.hbuf] = float(self.fit_val[0])
        self.hkth[self.hbuf] = float(self.fit_val[self.ik])
        if self.hcount < self.hlen:
            self.hcount += 1
        if self.hcount == self.hlen:
            self.fbest, self.fworst = min(self.hbest), max(self.hbest)

    def generation(self, draws, fvals=None):
        self.sample(draws)
        self.evaluate_sort(fvals)
        self.update()
        self.update_history()
        self.it += 1

    # ---- :183-213 -------------------------------------------------------------------------------
    def flag(self):
        if self.it >= self.mit:
            return FLAG_MAXITER
        if self.sigma < 1e-16:
            return FLAG_SIGMA
        if self.it >= self.hlen and self.fworst - self.fbest < self.tol:
            return FLAG_TOLHISTFUN
        if self.hcount >= self.n:
            eq = 0
            for i in range(self.n):
                idx = (self.hlen + self.hbuf - i) % self.hlen
                if self.hbest[idx] == self.hkth[idx]:
                    eq += 1
                    if 3 * eq >= self.n:
                        return FLAG_EQUALFUNVALS
        return 0

    def best(self):
        return self.xmean.copy() if self.it <= 0 else self.arx[self.fit_idx[0]].copy()

    def state(self):
        return {"arx": self.arx.ravel().copy(), "fit_val": self.fit_val.copy(), "fit_idx": self.fit_idx.astype(float),
                "xmean": self.xmean.copy(), "sigma": np.array([self.sigma]), "pc": self.pc.copy(),
                "s": np.array([self.s]), "memlen": np.array([float(self.memlen)]),
                "jarr": np.array(self.jarr, float), "larr": np.array(self.larr, float), "b": self.b.copy(),
                "d": self.d.copy(), "pcmat": self.pcmat.ravel().copy(), "vmat": self.vmat.ravel().copy(),
                "fp": self.fp.copy(), "it": np.array([float(self.it)]), "fev": np.array([float(self.fev)]),
                "flag": np.array([float(self.flag())])}

    def draw(self, rng, rademacher=True):
        """one generation's table from a NumPy generator (the tests' own draws)"""
        half, n = (self.lam + 1) // 2, self.n
        tab = np.empty((half, n + 1))
        tab[:, :n] = np.where(rng.random((half, n)) < 0.5, 1., -1.) if rademacher else rng.standard_normal((half, n))
        tab[:, n] = rng.standard_normal(half)
        return tab
