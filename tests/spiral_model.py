"""NumPy-scalar model of SpiralSearch (spiral.cpp:46-190) in two forms.

reference form   iterate() as the reference writes it: rotate_n of xbest and of x_i, then
                 x_i[d] = r_i t2[d] - r_i t[d] + xbest[d] (:121-135); given the reference's uniforms
                 (jaya_model.Words over the recorded mt19937 words) it reproduces every recorded
                 state bit for bit (tests/test_spiral_model.py).
device form      the difference x_i - xbest rotated once, x_i[d] = r_i (R d)[d] + xbest[d]: half the
                 rotations; what the kernel spiral_rotate computes, operation for operation.

Every product and sum is one IEEE operation on Python floats, in the reference's order; cos and sin
are libm's unless the caller supplies them (the GPU tests feed the device's own)."""
import math

INF = float("inf")


def rotate_n(x, c, s):
    """rotate_n, spiral.cpp:184-190: stage a = 1 .. n - 1 against b = a + 1 .. n, in place"""
    n = len(x)
    for a in range(n - 1):
        xa = x[a]
        for b in range(a + 1, n):
            xb = x[b]
            na = c * xa - s * xb
            x[b] = s * xa + c * xb
            xa = na
        x[a] = xa
    return x


def step_reference(x, xbest, r, c, s):
    """the new row of one point, :126-134"""
    t = rotate_n(list(xbest), c, s)
    t2 = rotate_n(list(x), c, s)
    return [r * t2[d] - r * t[d] + xbest[d] for d in range(len(x))]


def step_device(x, xbest, r, c, s):
    """the same point with the difference rotated once"""
    t = rotate_n([x[d] - xbest[d] for d in range(len(x))], c, s)
    return [r * t[d] + xbest[d] for d in range(len(x))]


def step_device_rows(X, xbest, r, c, s):
    """step_device over all rows at once: X [np][n], r, c, s [np].  Every NumPy operation is one
    IEEE operation per element, so a row's result is step_device's bit for bit."""
    import numpy as np
    X, xbest = np.asarray(X, float), np.asarray(xbest, float)
    r, c, s = (np.asarray(v, float) for v in (r, c, s))
    n = X.shape[1]
    t = [X[:, d] - xbest[d] for d in range(n)]
    for a in range(n - 1):
        xa = t[a]
        for b in range(a + 1, n):
            xb = t[b]
            na = c * xa - s * xb
            t[b] = s * xa + c * xb
            xa = na
        t[a] = xa
    return np.stack([r * t[d] + xbest[d] for d in range(n)], axis=1)


def between(u, a, b):
    """Random::get(a, b) on doubles over the raw uniform u, random.hpp:329-337"""
    if not a < b:
        a, b = b, a
    return u * (b - a) + a


class Spiral:
    def __init__(self, f, np_, r=0.95, theta=1.57079632679, taur=0.0, tautheta=0.1, rlow=0.9, rhigh=1.0,
                 thetalow=0.0, thetahigh=6.28318530718, form="reference"):
        self.f, self.np = f, np_
        self.r0, self.theta0, self.taur, self.tautheta = r, theta, taur, tautheta
        self.rlow, self.rhigh, self.thetalow, self.thetahigh = rlow, rhigh, thetalow, thetahigh
        self.step = {"reference": step_reference, "device": step_device}[form]

    def start(self, X):
        """init() from given points, :84-105"""
        self.x = [[float(v) for v in row] for row in X]
        self.rs = [self.r0] * self.np
        self.thetas = [self.theta0] * self.np
        self.fev = 0
        self.it = 0
        self.select()

    def select(self):
        """:138-148: all points evaluated, the first strict minimum of THESE values"""
        self.fs = [float(self.f(row)) for row in self.x]
        fbest, self.ibest = INF, 0
        for i, v in enumerate(self.fs):
            if v < fbest:
                fbest, self.ibest = v, i
        self.xbest = list(self.x[self.ibest])
        self.fev += self.np

    def draw(self, uniforms):
        """:111-118 over [np][4] raw uniforms (coin of r, value of r, coin of theta, value of theta)"""
        for i, u in enumerate(uniforms):
            if u[0] < self.taur:
                self.rs[i] = between(u[1], self.rlow, self.rhigh)
            if u[2] < self.tautheta:
                self.thetas[i] = between(u[3], self.thetalow, self.thetahigh)

    def rotate(self, cos=None, sin=None):
        for i in range(self.np):
            c = math.cos(self.thetas[i]) if cos is None else float(cos[i])
            s = math.sin(self.thetas[i]) if sin is None else float(sin[i])
            self.x[i] = self.step(self.x[i], self.xbest, self.rs[i], c, s)

    def iterate(self, uniforms, cos=None, sin=None):
        self.draw(uniforms)
        self.rotate(cos, sin)
        self.select()
        self.it += 1


def uniforms_of(words, np_, taur, tautheta, pad=0.5):
    """the [np][4] raw uniforms of a generation from the words the reference consumed (a
    jaya_model.Words): the coin of r, its value if the coin fired, the coin of theta, its value if
    it fired; a value the reference did not draw is `pad`"""
    out = []
    for _ in range(np_):
        ur = words.canonical()
        vr = words.canonical() if ur < taur else pad
        ut = words.canonical()
        vt = words.canonical() if ut < tautheta else pad
        out.append([ur, vr, ut, vt])
    return out
