"""Scalar model of NSHS (nshs.cpp:46-181) in two forms.

reference form   calculate_std as the reference writes it (:172-181): Welford's recurrence in row
                 order, then sqrt(m2 / hms).  Given the reference's uniforms (jaya_model.Words over
                 the recorded mt19937 words) it reproduces every recorded state bit for bit
                 (tests/test_nshs_model.py).
device form      fstd in two passes over a fixed-shape tree sum (tree_sum below): what nshs_select
                 computes in nshs_init, nshs_replace and nshs_steps, operation for operation.

fstd enters the algorithm through `fstd > fstdmin` alone, so the two forms generate the same
candidates as long as that comparison agrees.  Everything else is one IEEE operation on Python
floats per operation of the reference, in the reference's order.  The worst row is a function of
the memory's values (the first maximum), kept as state like the best (the first minimum); the
reference finds it at the start of replace(), which is the same row."""
import math

INF = float("inf")
NAN = float("nan")


def between(u, a, b):
    """Random::get(a, b) on doubles over the raw uniform u, random.hpp:329-337"""
    if not a < b:
        a, b = b, a
    return u * (b - a) + a


def tree_sum(v):
    """the device's sum: lane l of 64 adds v[l], v[l + 64], ... in this order starting from 0.0,
    then the partial sums meet in a butterfly over the offsets 32, 16, .., 1"""
    part = [0.] * 64
    for j, x in enumerate(v):
        part[j % 64] = part[j % 64] + x
    off = 32
    while off:
        part = [part[i] + part[i + off] for i in range(off)]
        off //= 2
    return part[0]


def _sqrt(x):
    return math.sqrt(x) if x >= 0. else NAN     # (NaN compares false: a NaN stays a NaN)


def std_reference(f):
    """calculate_std, :172-181"""
    mean, m2 = 0., 0.
    for i, v in enumerate(f):
        delta = v - mean
        mean += delta / (i + 1)
        m2 += delta * (v - mean)
    return _sqrt(m2 / len(f))


def std_device(f):
    """two passes over tree_sum; an inf among the values gives inf - inf = NaN"""
    mean = tree_sum(f) / len(f)
    m2 = tree_sum([(v - mean) * (v - mean) for v in f])
    return _sqrt(m2 / len(f))


def uniforms_of(words, n, hms, hmcr, pad=0.5):
    """the [n][4] raw uniforms of an iteration from the words the reference consumed (a
    jaya_model.Words): per coordinate the coin, the row j as (j + 0.5) / hms if the coin fired, else
    the fresh value, then the adjustment; a value the reference did not draw is `pad`"""
    out = []
    for _ in range(n):
        coin = words.canonical()
        if coin < hmcr:
            row, fresh = (words.uint(0, hms - 1) + 0.5) / hms, pad
        else:
            row, fresh = pad, words.canonical()
        out.append([coin, row, fresh, words.canonical()])
    return out


class Nshs:
    def __init__(self, f, n, hms, lower, upper, mfev, fstdmin=0.0001, form="reference"):
        self.f, self.n, self.hms = f, n, hms
        self.lower, self.upper = [float(v) for v in lower], [float(v) for v in upper]
        self.mfev, self.fstdmin = mfev, fstdmin
        self.std = {"reference": std_reference, "device": std_device}[form]
        self.mit = mfev - hms
        self.hmcr = 1.0 - 1.0 / (n + 1)
        self.tunerange = 0.0
        for d in range(n):
            self.tunerange = max(self.tunerange, (self.upper[d] - self.lower[d]) / 2)

    def start(self, X, fs=None):
        """init() from a given memory, :60-91"""
        self.x = [[float(v) for v in row] for row in X]
        self.fs = [self.value(row) for row in self.x] if fs is None else [float(v) for v in fs]
        self.cand, self.fcand, self.accepted = [0.] * self.n, 0., False
        self.fev, self.it = self.hms, 0
        self.select()

    def value(self, row):
        v = float(self.f(row))
        return INF if v != v else v

    def select(self):
        """fstd, the first minimum and the first maximum"""
        self.fstd = self.std(self.fs)
        self.wide = self.fstd > self.fstdmin
        self.ibest = min(range(self.hms), key=lambda i: self.fs[i])      # (min and max keep the first)
        self.iworst = max(range(self.hms), key=lambda i: self.fs[i])

    def generate(self, uniforms):
        """:115-147 over [n][4] raw uniforms"""
        for i, (coin, row, fresh, adj) in enumerate(uniforms):
            lo, up = self.lower[i], self.upper[i]
            if coin < self.hmcr:
                j = min(int(row * float(self.hms)), self.hms - 1)
                x = self.x[j][i]
            elif self.wide:
                x = between(fresh, lo, up)
            else:
                mn, mx = up, lo
                for r in self.x:
                    mn = r[i] if r[i] < mn else mn
                    mx = r[i] if mx < r[i] else mx
                x = between(fresh, mn, mx)
            if self.wide:
                bw = ((up - lo) / self.tunerange) * (1.0 - (1. * self.it) / self.mit)
                x += between(adj, -bw, bw)
            else:
                x += between(adj, -self.fstdmin, self.fstdmin)
            x = up if up < x else x
            x = lo if x < lo else x
            self.cand[i] = x

    def evaluate(self, fcand=None):
        self.fcand = self.value(self.cand) if fcand is None else float(fcand)

    def replace(self):
        """:157-169 and the counters"""
        self.accepted = self.fcand < self.fs[self.iworst]
        if self.accepted:
            self.x[self.iworst] = list(self.cand)
            self.fs[self.iworst] = self.fcand
            self.select()
        self.it += 1
        self.fev += 1

    def iterate(self, uniforms, fcand=None):
        self.generate(uniforms)
        self.evaluate(fcand)
        self.replace()
