"""(i)AMaLGaM-IDEA restated in NumPy, in the reference's order of operations (amalgam.cpp), plus the
device's form where the kernels add in another order (bbo_amalgam_kernels.hpp).

The rows of a population stay in SAMPLING order: row m of a generation is the m-th point the
reference samples, i.e. its sorted row m of the generation before; `order` (rank -> row) carries the
sort.  The reference then shuffles rows 1.. and shifts the first nams of them; `perm` (position after
the shuffle -> sampling row, perm[0] = 0) replays that: the shifted rows are perm[1 : nams + 1] and the
mean of the improving rows is added in the order of perm.  Without a perm the order is the sampling
order and only the SET of shifted rows matters -- the device's form.

form = "reference": every sum in the reference's order.
form = "device":    the Gram in slabs of SLAB ranked rows, cov = cov (1 - eta) + (eta / ss) sum of slabs;
                    X = mu + Z chol^T as a matrix product; the mean of the improving rows in sampling
                    order; dot products and the variance of the values by NumPy's reductions.
"""
import math

import numpy as np

SLAB = 256          # AMALGAM_SLAB


def default_np(n, iamalgam):
    return int(10. * math.sqrt(1. * n)) if iamalgam else int(17. + 3. * math.pow(1. * n, 1.5))


def constants(n, np_, iamalgam):
    """amalgam.cpp:112-131"""
    ss = int(0.35 * np_)
    if iamalgam:
        etasigma = 1. - math.exp(-1.1 * math.pow(ss, 1.2) / math.pow(1. * n, 1.6))
        etashift = 1. - math.exp(-1.2 * math.pow(ss, 0.31) / math.sqrt(1. * n))
    else:
        etasigma = etashift = 1.
    alphaams = (0.5 * 0.35 * np_) / (np_ - 1)
    return {"np": np_, "ss": ss, "etasigma": etasigma, "etashift": etashift,
            "nams": int(alphaams * (np_ - 1)), "nismax": 25 + n}


def rank_order(f):
    """rank -> row, ties to the lower index, NaN last"""
    f = np.where(np.isnan(f), np.inf, f)
    return np.argsort(f, kind="stable")


def dchdc(cov):
    """LINPACK's dchdc without pivoting (:455-528): returns the upper factor as far as it got (the
    rest is the Schur complement) and the step of the first pivot <= 0 (n: none)"""
    a = np.array(cov, dtype=np.float64)
    n = a.shape[0]
    for k in range(n):
        if a[k, k] <= 0.:
            return a, k
        t = math.sqrt(a[k, k]) if a[k, k] == a[k, k] else float("nan")
        a[k, k] = t
        a[k, k + 1:] = a[k, k + 1:] / t
        r = a[k, k + 1:]
        a[k + 1:, k + 1:] -= r[:, None] * r[None, :]
    return a, n


def factor(cov, cmult):
    """:401-415: the factor transposed into the lower triangle, the upper zero, times sqrt(cmult)"""
    a, fail = dchdc(cov)
    return np.tril(a.T) * math.sqrt(cmult), fail


class Amalgam:
    def __init__(self, f, n, mfev, stol, np_=0, iamalgam=True, keep_elite=False, form="reference"):
        assert form in ("reference", "device")
        self.f, self.n, self.mfev, self.stol = f, n, mfev, stol
        self.keep_elite, self.form = keep_elite, form
        if np_ <= 0:
            np_ = default_np(n, iamalgam)
        self.c = constants(n, np_, iamalgam)
        self.np, self.ss, self.nams = np_, self.c["ss"], self.c["nams"]
        self.calls = 0

    def _eval(self, x):
        self.calls += 1
        v = float(self.f(x))
        return v if v == v else float("inf")

    # :136-174
    def init(self, x0):
        n, ss = self.n, self.ss
        self.X = np.array(x0, dtype=np.float64).reshape(self.np, n)
        self.fit = np.array([self._eval(x) for x in self.X])
        self.order = rank_order(self.fit)
        self.fev, self.t, self.nis, self.cmult, self.sdr = self.np, 0, 0, 1., 0.
        xs = self.X[self.order[:ss]]
        mu = np.zeros(n)
        for m in range(ss):
            mu = mu + xs[m]
        self.mu = mu * (1. / ss)
        v = np.zeros(n)
        for m in range(ss):
            d = xs[m] - self.mu
            v = v + d * d
            v = v / ss
        self.cov = np.diag(v)
        self.mushift = np.zeros(n)
        self.chol = np.zeros((n, n))
        self.fail_at, self.fact_fail = n, 0
        self.fbest = self.fit[self.order[0]]
        self.xbest = self.X[self.order[0]].copy()

    # :358-416
    def update_distribution(self):
        n, ss, c = self.n, self.ss, self.c
        xs = self.X[self.order[:ss]]
        self.xelite, self.felite = self.X[self.order[0]].copy(), self.fit[self.order[0]]
        muold = self.mu
        mu = np.zeros(n)
        w = 1. / ss
        for m in range(ss):
            mu = mu + w * xs[m]
        self.mu = mu
        eta = c["etasigma"]
        d = xs - mu
        if self.form == "reference":
            cov = self.cov * (1. - eta)
            a = eta / ss
            for m in range(ss):
                cov = cov + (a * d[m])[:, None] * d[m][None, :]
        else:
            g = np.zeros((n, n))
            for m0 in range(0, ss, SLAB):
                g = g + d[m0:m0 + SLAB].T @ d[m0:m0 + SLAB]
            cov = self.cov * (1. - eta) + (eta / ss) * g
        low = np.tril(cov)
        self.cov = low + np.tril(cov, -1).T
        if self.t == 1:
            self.mushift = mu - muold
        elif self.t > 1:
            self.mushift = self.mushift * (1. - c["etashift"]) + c["etashift"] * (mu - muold)
        else:
            self.mushift = np.zeros(n)
        self.chol, self.fail_at = factor(self.cov, self.cmult)
        if self.fail_at < n:
            self.fact_fail += 1

    # :418-453
    def sample(self, z, shifted=None, perm=None):
        n, np_ = self.n, self.np
        z = np.asarray(z, dtype=np.float64).reshape(np_, n)
        if self.form == "reference":
            acc = np.zeros((np_, n))
            for l in range(n):
                acc = acc + self.chol[None, :, l] * z[:, l, None]
            X = self.mu[None, :] + acc
        else:
            X = self.mu[None, :] + z @ self.chol.T
        if self.keep_elite:
            X[0] = self.xelite
        if perm is not None:
            shifted = perm[1:self.nams + 1]
        shifted = sorted(int(r) for r in shifted)
        assert len(set(shifted)) == self.nams and all(1 <= r < np_ for r in shifted)
        for r in shifted:
            X[r] = X[r] + (2. * self.cmult) * self.mushift
        fit = np.empty(np_)
        fit[0] = self.felite
        rows = range(1, np_) if perm is None else [int(r) for r in perm[1:]]
        for r in rows:
            fit[r] = self._eval(X[r])
        self.X, self.fit, self.z = X, fit, z
        self.shifted, self.perm = shifted, perm
        self.fev += np_

    # :213-233, :330-356
    def adapt(self):
        n, np_, fit = self.n, self.np, self.fit
        rows = range(1, np_) if self.perm is None else [int(r) for r in self.perm[1:]]
        better = [r for r in rows if fit[r] < fit[0]]
        imin = int(np.argmin(fit))
        if imin > 0 and fit[imin] < self.fbest:
            self.fbest, self.xbest = fit[imin], self.X[imin].copy()
        self.sdr = 0.
        if better:
            self.nis = 0
            if self.cmult < 1.:
                self.cmult = 1.
            xavg = np.zeros(n)
            for r in better:
                xavg = xavg + self.X[r]
            xavg = xavg * (1. / len(better))
            xavg = xavg + -1. * self.mu
            tmp = xavg.copy()
            sdr = 0.
            for i in range(n):
                if self.form == "reference":
                    s = 0.
                    for l in range(i):
                        s = s + self.chol[i, l] * tmp[l]
                else:
                    s = float(np.dot(self.chol[i, :i], tmp[:i]))
                with np.errstate(all="ignore"):
                    tmp[i] = (tmp[i] - s) / self.chol[i, i]
                if sdr < abs(tmp[i]):
                    sdr = abs(tmp[i])
            self.sdr = sdr
            if sdr > 1.:
                self.cmult *= 1. / 0.9
        else:
            if self.cmult <= 1.:
                self.nis += 1
            if self.cmult > 1. or self.nis >= self.c["nismax"]:
                self.cmult *= 0.9
            if self.cmult < 1. and self.nis < self.c["nismax"]:
                self.cmult = 1.
        self.t += 1
        self.order = rank_order(fit)

    def iterate(self, z, shifted=None, perm=None):
        self.update_distribution()
        self.sample(z, shifted, perm)
        self.adapt()

    # :290-328; 0 = go on, 1 = the algorithm's own rule, 2 = the budget
    def stop(self):
        own = self.cmult < 1e-10
        with np.errstate(all="ignore"):
            if self.form == "reference":
                fmean = 0.
                for v in self.fit:
                    fmean += v / self.np
                fvar = 0.
                for v in self.fit:
                    fvar += (v - fmean) * (v - fmean) / self.np
            else:
                fmean = float(np.sum(self.fit / self.np))
                fvar = float(np.sum((self.fit - fmean) ** 2 / self.np))
        own = own or fvar <= self.stol * self.stol
        return 1 if own else 2 if self.fev >= self.mfev else 0

    def solution(self):
        return self.X[0].copy()

    # :246-255: iterates before it tests
    def optimize(self, x0, draws):
        """draws(model) -> (z, shifted rows) of the next generation"""
        self.init(x0)
        while True:
            z, sh = draws(self)
            self.iterate(z, sh)
            if self.stop():
                return self.solution(), self.fev


def numpy_draws(rng):
    def draws(m):
        z = rng.standard_normal((m.np, m.n))
        sh = 1 + rng.permutation(m.np - 1)[:m.nams]
        return z, sh
    return draws


# ---- the parameter-free mode (:72-98, :180-203, :257-288, :298-308) -------------------------------------

def stage_shape(s, nbase):
    half = s >> 1
    if s & 1 == 0:
        return (1 + half) * nbase, 1 << half
    return (1 << (1 + half)) * nbase, 1


def parameter_free(nbase, mfev, tol, inner, max_stages=30):
    """inner(s, r, np, cap) -> (fev, f of the returned point): a complete inner run with budget cap.
    Returns the table rows (s, runs, np, f*, best f*, fev) up to the reference's stop."""
    inf = float("inf")
    fbest = fbestrun = inf
    budget, fev, rows = mfev, 0, []
    for s in range(max_stages):
        np_, runs = stage_shape(s, nbase)
        fbestrunold, fbestrun = fbestrun, inf
        for r in range(runs):
            used, fitr = inner(s, r, np_, budget)
            fev += used + 1
            budget -= used + 1
            fbestrun = min(fbestrun, fitr)
            fbest = min(fbest, fitr)
        rows.append((s, runs, np_, fbestrun, fbest, fev))
        if fev >= mfev or (fbestrun != fbestrunold and abs(fbestrun - fbestrunold) <= tol):
            break
    return rows


# ---- the built-in objectives the tests use, in the operation order of bbo_objectives.hpp ---------------

def objective(name, n):
    if name == "sphere":
        return lambda x: float(np.sum(np.asarray(x) ** 2))
    if name == "rosenbrock":
        def rosenbrock(x):
            s = 0.
            for i in range(n - 1):
                a, b = x[i + 1] - x[i] * x[i], 1. - x[i]
                s += 100. * (a * a) + b * b
            return s
        return rosenbrock
    if name == "ellipsoid":
        aux = [math.pow(10., 6. * (i / (n - 1) if n > 1 else 0.)) for i in range(n)]

        def ellipsoid(x):
            s = 0.
            for i in range(n):
                s += aux[i] * (x[i] * x[i])
            return s
        return ellipsoid
    raise ValueError(name)


def rosenbrock_fast(x):
    a, b = x[1:] - x[:-1] * x[:-1], 1. - x[:-1]
    return float(np.sum(100. * (a * a) + b * b))


# ---- what the recorded fixture leaves out, regenerated -------------------------------------------------

def crafted(n, rank, drop):
    """B B^T of the given rank (small integers in B) with `drop` taken off the diagonal from `rank` on:
    the factorisation meets a negative pivot at step `rank`"""
    rng = np.random.RandomState(100 + n)
    b = rng.randint(-3, 4, size=(n, rank)).astype(np.float64)
    b[:rank, :rank] += 4. * np.eye(rank)
    a = b @ b.T
    for i in range(rank, n):
        a[i, i] -= drop
    return a



class ReferenceRng:
    """the reference's generator after Random::seed(k): std::mt19937 with libstdc++'s generate_canonical,
    uniform_real_distribution (effolkronium's closed interval) and normal_distribution (polar method)"""

    def __init__(self, seed):
        self.bits = np.random.MT19937()
        self.bits._legacy_seeding(seed)

    def canonical(self):
        a, b = (int(v) for v in self.bits.random_raw(2))
        r = (a + b * 4294967296.) / 18446744073709551616.
        return r if r < 1. else math.nextafter(1., 0.)

    def uniform(self, lo, hi):
        return (math.nextafter(hi, math.inf) - lo) * self.canonical() + lo

    def normals(self, count):
        out = []
        while len(out) < count:
            while True:
                x, y = 2. * self.canonical() - 1., 2. * self.canonical() - 1.
                r2 = x * x + y * y
                if 0. < r2 <= 1.:
                    break
            mult = math.sqrt(-2. * math.log(r2) / r2)
            out += [y * mult, x * mult]
        return out[:count]


def reference_draws(seed, n, np_, f, lo=-5., hi=5.):
    """the initial points of the reference as it holds them after init (sorted) and the normals of its
    first generation, for Random::seed(seed)"""
    rng = ReferenceRng(seed)
    x0 = np.array([[rng.uniform(lo, hi) for _ in range(n)] for _ in range(np_)])
    x0 = x0[rank_order(np.array([f(x) for x in x0]))]
    return x0, np.array(rng.normals(np_ * n)).reshape(np_, n)


def fixture_draws(rec, unpack):
    """x0 and the normals of every generation of a "steps" record of tests/golden/amalgam_runs.json"""
    x0, z1 = reference_draws(rec["seed"], rec["n"], rec["np"], objective(rec["objective"], rec["n"]))
    return x0, [z1.ravel()] + [unpack(st["z"]) for st in rec["states"][1:]]
