"""BasinHopping (basinhopping.cpp) restated in plain Python floats in the reference's operation order, over the
models of its two device-resident minimisers (tests/neldermead_model.py, tests/rosenbrock_model.py), so a run is the
reference's bit for bit (scripts/gen_basinhopping_golden.py checks that against the real classes before it writes
tests/golden/basinhopping_runs.json).

    st = Strategy(stepsize)  or  Strategy(stepsize, accept_rate, interval, factor)      # the caller's object
    m = Model(f, lower, upper, minimizer, st, mit, temp)
    m.init(guess); m.iterate(draws)         # draws: n step uniforms in [-1, 1) and the accept uniform in [0, 1)
    m.optimize(guess, table)                # init() + mit hops: (xbest, fev, False)

`minimizer(start)` returns (x, fev, converged): nm_minimizer / rosen_minimizer make one from a model.  `rows` is
the reference's table (it, f, conv, step, accept, f*, fev) with, per row, the start handed to the minimiser, what it
returned, its evaluation count, and `w - u` of the Metropolis test (None in row -1)."""
import math

import numpy as np

import neldermead_model as nm
import rosenbrock_model as rm

INF = float("inf")
CLOSE = 1e-9        # a decision with |w - u| below it is one the device's exp may take the other way


def reference_draws(seed, n, hops):
    """The uniforms the reference draws in `hops` hops after Random::seed(seed), hop by hop: std::mt19937 seeded as
    numpy's legacy generator seeds it, two words per double (libstdc++'s generate_canonical<double, 53>), n of
    uniform_real_distribution(-1, 1) and one of (0, 1).  scripts/gen_basinhopping_golden.py holds them to the
    draws it reads from a copy of the reference's engine."""
    state = np.random.RandomState(seed).get_state()
    words = np.random.MT19937()
    words.state = {"bit_generator": "MT19937", "state": {"key": state[1], "pos": state[2]}}
    raw = [int(w) for w in words.random_raw(2 * (n + 1) * hops)]
    table = []
    for h in range(hops):
        row = []
        for j in range(n + 1):
            lo, hi = raw[2 * (h * (n + 1) + j):2 * (h * (n + 1) + j) + 2]
            c = (float(lo) + float(hi) * 4294967296.) / 18446744073709551616.
            c = c if c < 1. else 1. - 2. ** -53
            row.append(c * (1. - -1.) + -1. if j < n else c * (1. - 0.) + 0.)
        table.append(row)
    return table


class Strategy:
    def __init__(self, stepsize, accept_rate=None, interval=5, factor=0.9):
        self.stepsize = float(stepsize)
        self.adaptive = accept_rate is not None
        self.accept_rate, self.interval, self.factor = accept_rate, int(interval), factor
        self.nstep = self.naccept = 0

    # takeStep() (:50-57, :72-88)
    def take_step(self, x, lower, upper, u):
        if self.adaptive:
            self.nstep += 1
            if self.nstep % self.interval == 0:
                if (1. * self.naccept) / self.nstep > self.accept_rate:
                    self.stepsize /= self.factor
                else:
                    self.stepsize *= self.factor
        for i in range(len(x)):
            x[i] += self.stepsize * u[i] * (upper[i] - lower[i])
            margin = 0.05 * (upper[i] - lower[i])
            hi, lw = upper[i] - margin, lower[i] + margin
            t = hi if hi < x[i] else x[i]           # std::min(x[i], upper[i] - margin)
            x[i] = t if lw < t else lw              # std::max(lower[i] + margin, .)

    def update(self, accept):
        if self.adaptive and accept:
            self.naccept += 1


def nm_minimizer(f, n, mfev, tol, rad0, **kw):
    return lambda start: nm.Model(f, n, mfev, tol, rad0, **kw).optimize(start)


def rosen_minimizer(f, n, mfev, tol, step0, decf=0.1, repair=False):
    return lambda start: rm.Model(f, n, mfev, tol, step0, decf, repair).optimize(start)


def metropolis_w(fnew, fold, temp):
    """exp(std::min(0., -(fnew - fold) * beta)) (:96-107): a NaN product is not below 0 and gives w = 1"""
    beta = INF if temp == 0. else 1. / temp
    d = fnew - fold                     # (inf - inf is NaN)
    v = -d * beta if not (d == 0. and beta == INF) else float("nan")
    return math.exp(v if v < 0. else 0.)


class Model:
    def __init__(self, f, lower, upper, minimizer, strategy, mit=99, temp=1.):
        self.f, self.lower, self.upper = f, [float(v) for v in lower], [float(v) for v in upper]
        self.n = len(self.lower)
        self.minimizer, self.strategy, self.mit, self.temp = minimizer, strategy, int(mit), temp

    def _energy(self, x):
        v = float(self.f(list(x)))
        return INF if v != v else v     # (the device's rule; the reference has none)

    # init() (:119-153)
    def init(self, guess):
        self.it, self.fev, self.rows = 0, 0, []
        start = [float(v) for v in guess[:self.n]]
        sol, fev, conv = self.minimizer(list(start))
        self.x = list(sol)
        self.energy = self._energy(sol)
        self.fev += fev + 1
        self.xbest, self.fbest = list(self.x), self.energy
        self._row(-1, self.energy, conv, True, start, sol, fev, None)

    def _row(self, it, f, conv, accept, start, sol, fev, gap):
        self.rows.append({"it": it, "f": f, "conv": int(bool(conv)), "step": self.strategy.stepsize,
                          "accept": int(bool(accept)), "fbest": self.fbest, "fev": self.fev,
                          "start": list(start), "sol": list(sol), "inner_fev": fev, "gap": gap})

    # iterate() (:155-190)
    def iterate(self, draws):
        n = self.n
        x1 = list(self.x)
        self.strategy.take_step(x1, self.lower, self.upper, draws)
        sol, fev, conv = self.minimizer(list(x1))
        e = self._energy(sol)
        self.fev += fev + 1
        w = metropolis_w(e, self.energy, self.temp)
        accept = w >= draws[n]
        if accept:
            self.energy, self.x = e, list(sol)
        self.strategy.update(accept)
        if e < self.fbest:
            self.fbest, self.xbest = e, list(sol)
        self._row(self.it, e, conv, accept, x1, sol, fev, w - draws[n])
        self.it += 1

    def optimize(self, guess, table):
        self.init(guess)
        while self.it < self.mit:
            self.iterate(table[self.it])
        return list(self.xbest), self.fev, False

    def close(self):
        """the hops whose decision lies within CLOSE of a tie"""
        return [r["it"] for r in self.rows if r["gap"] is not None and abs(r["gap"]) < CLOSE]
