"""SLPSO (Li, Yang & Nguyen 2012) restated in pure Python in the reference's operation order
(src/multivariate/pso/slpso.cpp; the line numbers below are its).  Every arithmetic step is one IEEE
double operation in the order the reference writes it, so the model fed the reference's own draws
reproduces its states bit for bit (tests/test_slpso_model.py), and the GPU tests lean on the model.

A generation takes its draws from a *source*, an object with
    alpha()  force(kp)  roulette(kp)  partner(kp)  rkd(kp, d)  z(kp, d)  redraw(kp, d)  coin(kp, d)
    shuffle(perm)
Three sources:
    WordsSource   decodes the reference's mt19937 words in the reference's program order
                  (jaya_model.Words) and writes the table below as it goes
    TableSource   reads the table of bbo_slpso_inject_draws / get_state("draws"):
                  [alpha][perm: np][np x (3 + 4 n)] -- per particle step the forcing coin, the roulette
                  canonical and the partner j as (j + 0.5) / np, per coordinate r, the normal of operator
                  1, the redraw of eq. 11 and the coin of Algorithm 2
    RngSource     the model's own generator (a numpy Generator)
"""
import base64
import math
import zlib

import numpy as np

import jaya_model as jm

INF = float("inf")
NSTRAT = 4


def table_len(n, np_):
    return 1 + np_ + np_ * (3 + 4 * n)


def between(u, a, b):
    """Random::get(a, b) on doubles over the canonical u, random.hpp:329-337"""
    if not a < b:
        a, b = b, a
    return u * (b - a) + a


# ---- the fixture's compact form (tests/golden/slpso_runs.json) ---------------------------------------------
# A float array of a state is kept as the entries whose bits differ from the state before it: runs
# [[start, length], ...] under "r" and their values, packed little-endian doubles in base64, under "v";
# an entry of pb that took the value of x at the same place (a new personal best) is named under "rx"
# instead, and an entry of x that is the sum of its old value and the state's v at the same place (a move
# that stayed inside the box) under "rv".  The first state of a record keeps whole arrays (a base64
# string; pb, which equals x there, as "rx").  Nothing is rounded: the packer compares bits.
FLOAT_KEYS = ("x", "v", "pb", "fx", "fpb", "fp", "s", "p", "Uf", "Pl", "abest", "vdavg")


def _b64(a):
    return base64.b64encode(np.asarray(a, "<f8").tobytes()).decode()


def _unb64(s):
    return np.frombuffer(base64.b64decode(s), "<f8").astype(float)


def _bits(a):
    return np.ascontiguousarray(a, dtype="<f8").view(np.uint64)


def _runs(idx):
    runs = []
    for i in idx:
        if runs and runs[-1][0] + runs[-1][1] == i:
            runs[-1][1] += 1
        else:
            runs.append([int(i), 1])
    return runs


def _indices(runs):
    return [i for s, c in runs for i in range(s, s + c)]


def pack_states(states):
    """states: dicts whose FLOAT_KEYS are float sequences, in order; packs them in place"""
    prev = None
    for st in states:
        full = {k: np.asarray(st[k], float) for k in FLOAT_KEYS}
        for k in FLOAT_KEYS:
            cur = full[k]
            if prev is None and not (k == "pb" and (_bits(cur) == _bits(full["x"])).all()):
                st[k] = _b64(cur)
                continue
            old = prev[k] if prev is not None else np.zeros_like(cur) * np.nan
            ch = np.flatnonzero(_bits(cur) != _bits(old))
            ent = {}
            if k == "pb":
                fromx = _bits(cur)[ch] == _bits(full["x"])[ch]
                if fromx.any():
                    ent["rx"] = _runs(ch[fromx])
                ch = ch[~fromx]
            if k == "x":
                moved = _bits(cur)[ch] == _bits(old[ch] + full["v"][ch])
                if moved.any():
                    ent["rv"] = _runs(ch[moved])
                ch = ch[~moved]
            if ch.size:
                ent["r"], ent["v"] = _runs(ch), _b64(cur[ch])
            st[k] = ent
        prev = full


def unpack_states(states):
    """the inverse: every FLOAT_KEYS entry becomes a whole float array"""
    prev = None
    for st in states:
        full = {}
        for k in FLOAT_KEYS:
            ent = st[k]
            if isinstance(ent, str):
                full[k] = _unb64(ent)
                continue
            cur = prev[k].copy() if prev is not None else np.zeros(sum(c for _, c in ent["rx"]))
            if "r" in ent:
                cur[_indices(ent["r"])] = _unb64(ent["v"])
            full[k] = cur
        if not isinstance(st["x"], str) and "rv" in st["x"]:        # (x after v)
            idx = _indices(st["x"]["rv"])
            full["x"][idx] = prev["x"][idx] + full["v"][idx]
        if not isinstance(st["pb"], str) and "rx" in st["pb"]:      # (pb after x)
            idx = _indices(st["pb"]["rx"])
            full["pb"][idx] = full["x"][idx]
        for k in FLOAT_KEYS:
            st[k] = full[k]
        prev = full


def words_crc(words):
    return zlib.crc32(np.asarray(words, "<u4").tobytes())


def device_objective(name, n):
    """the built-in objectives summed as the device sums them (eval_row_group<64>, bbo_objectives.hpp):
    lane g adds the terms j = g, g + 64, ... in this order starting from 0, then the 64 partial sums meet
    in the xor butterfly of group_sum<64> (offsets 32, 16, .., 1).  With it the model's values are the
    device's bit for bit; chol_model.objective is the reference's serial sum"""
    aux = [math.pow(10., 6. * (i / (n - 1) if n > 1 else 0.)) for i in range(n)]

    def term(x, j):
        if name == "sphere":
            return x[j] * x[j]
        if name == "ellipsoid":
            return aux[j] * (x[j] * x[j])
        if name == "rosenbrock":
            t = x[j + 1] - x[j] * x[j]
            u = 1. - x[j]
            return 100. * (t * t) + u * u
        raise ValueError(name)

    terms = n - 1 if name == "rosenbrock" else n

    def f(x):
        x = [float(v) for v in x]
        lanes = [0.] * 64
        for j in range(terms):
            lanes[j % 64] += term(x, j)
        off = 32
        while off:
            lanes = [lanes[l] + lanes[l ^ off] for l in range(64)]
            off >>= 1
        return lanes[0]
    return f


class WordsSource:
    """the reference's program order over one generation's words; `w` is a jaya_model.Words (its cached
    second normal lives on across generations: carry `have` / `saved` over, or keep one object)"""

    def __init__(self, w, n, np_):
        self.w, self.n, self.np = w, n, np_
        self.table = np.zeros(table_len(n, np_))
        self.table[1:1 + np_] = np.arange(np_)

    def _step(self, kp):
        return 1 + self.np + kp * (3 + 4 * self.n)

    def _put(self, off, v):
        self.table[off] = v
        return v

    def alpha(self):
        return self._put(0, self.w.canonical())

    def force(self, kp):
        return self._put(self._step(kp), self.w.canonical())

    def roulette(self, kp):
        return self._put(self._step(kp) + 1, self.w.canonical())

    def partner(self, kp):
        jp = kp
        while jp == kp:                                     # :272-275
            jp = self.w.uint(0, self.np - 1)
        self._put(self._step(kp) + 2, (jp + 0.5) / self.np)
        return jp

    def rkd(self, kp, d):
        return self._put(self._step(kp) + 3 + 4 * d, self.w.canonical())

    def z(self, kp, d):
        return self._put(self._step(kp) + 3 + 4 * d + 1, self.w.normal())

    def redraw(self, kp, d):
        return self._put(self._step(kp) + 3 + 4 * d + 2, self.w.canonical())

    def coin(self, kp, d):
        return self._put(self._step(kp) + 3 + 4 * d + 3, self.w.canonical())

    def shuffle(self, perm):
        self.w.shuffle(perm)
        self.table[1:1 + self.np] = perm


class TableSource:
    def __init__(self, table, n, np_):
        self.t, self.n, self.np = np.asarray(table, float).ravel(), n, np_
        assert self.t.size == table_len(n, np_)

    def _step(self, kp):
        return 1 + self.np + kp * (3 + 4 * self.n)

    def alpha(self):
        return float(self.t[0])

    def force(self, kp):
        return float(self.t[self._step(kp)])

    def roulette(self, kp):
        return float(self.t[self._step(kp) + 1])

    def partner(self, kp):
        return min(int(float(self.t[self._step(kp) + 2]) * float(self.np)), self.np - 1)

    def rkd(self, kp, d):
        return float(self.t[self._step(kp) + 3 + 4 * d])

    def z(self, kp, d):
        return float(self.t[self._step(kp) + 3 + 4 * d + 1])

    def redraw(self, kp, d):
        return float(self.t[self._step(kp) + 3 + 4 * d + 2])

    def coin(self, kp, d):
        return float(self.t[self._step(kp) + 3 + 4 * d + 3])

    def shuffle(self, perm):
        perm[:] = [int(v) for v in self.t[1:1 + self.np]]


class RngSource:
    def __init__(self, rng, n, np_):
        self.rng, self.np = rng, np_

    def _u(self, *_):
        return float(self.rng.random())

    alpha = force = roulette = rkd = redraw = coin = _u

    def z(self, kp, d):
        return float(self.rng.standard_normal())

    def partner(self, kp):
        r = int(self.rng.integers(0, self.np - 1))
        return r + (1 if r >= kp else 0)

    def shuffle(self, perm):
        perm[:] = [perm[i] for i in self.rng.permutation(self.np)]


class Slpso:
    KEYS = ("x", "v", "pb", "fx", "fpb", "fp", "s", "p", "g", "G", "m", "CF", "PF", "Uf", "Pl", "perm",
            "abest", "fabest", "vdavg", "alpha", "omega", "mfes", "fev")

    def __init__(self, f, lower, upper, np_, mfev, stol, omegamin=0.4, omegamax=0.9, eta=1.496, gamma=0.01,
                 vmax=0.2, Ufmax=10.):
        self.f = f
        self.lower, self.upper = [float(v) for v in lower], [float(v) for v in upper]
        self.n, self.np, self.mfev, self.tol = len(self.lower), int(np_), int(mfev), float(stol)
        self.omegamin, self.omegamax, self.eta, self.gamma = omegamin, omegamax, eta, gamma
        self.vmaxk, self.Ufmax = vmax, Ufmax
        self.trace = False               # collect `gaps`
        self.events = set()
        self.repairs = {"low": 0, "high": 0}    # coordinates the eq. 11 redraw met past each wall
        self.gaps = []                  # relative gaps of the fitness comparisons when `trace`

    def evaluate(self, x):
        v = float(self.f(x))
        if v != v:
            v = INF
        self.fev += 1
        return v

    # ---- :56-92, :211-235 -----------------------------------------------------------------------
    def start(self, x, perm):
        """the state after init() given its positions [np][n] and its shuffled permutation"""
        n, np_ = self.n, self.np
        self.mfes, self.omega, self.alpha = 0, self.omegamax, 0.
        self.perm = [int(v) for v in perm]
        self.fev = 0
        self.fabest = INF
        self.abest = [0.] * n
        self.vdavg = [0.] * n
        self.x = [[float(v) for v in row] for row in np.asarray(x, float).reshape(np_, n)]
        self.v = [[0.] * n for _ in range(np_)]
        self.pb = [list(r) for r in self.x]
        self.fx, self.fpb, self.fp = [0.] * np_, [0.] * np_, [0.] * np_
        self.p = [[0.] * NSTRAT for _ in range(np_)]
        self.g = [[0] * NSTRAT for _ in range(np_)]
        self.G = [[0] * NSTRAT for _ in range(np_)]
        self.s = [[1. / NSTRAT] * NSTRAT for _ in range(np_)]
        self.m = [0] * np_
        self.CF, self.PF = [False] * np_, [False] * np_
        self.Uf, self.Pl = [0.] * np_, [0.] * np_
        for k in range(np_):
            self.fx[k] = self.fpb[k] = self.fp[k] = self.evaluate(self.x[k])
            self._par_particle(k)
            if self.fx[k] < self.fabest:
                self.abest = list(self.x[k])
                self.fabest = self.fx[k]
        return self

    def start_random(self, src_rng):
        """init() under the model's own generator"""
        perm = list(range(self.np))
        perm = [perm[i] for i in src_rng.permutation(self.np)]
        x = [[between(float(src_rng.random()), self.lower[d], self.upper[d]) for d in range(self.n)]
             for _ in range(self.np)]
        return self.start(x, perm)

    def start_words(self, w):
        """init() in the reference's program order over the words of `w` (:76, :219)"""
        perm = list(range(self.np))
        w.shuffle(perm)
        x = [[w.uniform(self.lower[d], self.upper[d]) for d in range(self.n)] for _ in range(self.np)]
        return self.start(x, perm)

    def _par_particle(self, index):     # :383-392
        k = self.perm[index]
        progress = math.exp(-math.pow(1.6 * k / self.np, 4.))
        self.Uf[index] = max(1., self.Ufmax * progress)
        self.Pl[index] = max(0.05, 1. - progress)

    def _gap(self, a, b, same_point=False):
        if self.trace and not same_point and a != b and math.isfinite(a) and math.isfinite(b):
            self.gaps.append(abs(a - b) / max(abs(a), abs(b)))

    # ---- :325-336 ------------------------------------------------------------------------------
    def _bounds(self, src, kp, x, v, d):
        x1 = x + v
        if x1 < self.lower[d]:
            self.events.add("redraw_low")
            self.repairs["low"] += 1
            return between(src.redraw(kp, d), self.lower[d], x)
        if x1 > self.upper[d]:
            self.events.add("redraw_high")
            self.repairs["high"] += 1
            return between(src.redraw(kp, d), x, self.upper[d])
        return x1

    def _learn(self, src, kp, mv, target):      # :245-251 and its three copies
        x, v = self.x[mv], self.v[mv]
        for d in range(self.n):
            rkd = src.rkd(kp, d)
            vn = self.omega * v[d] + self.eta * rkd * (target[d] - x[d])
            vmax = self.vmaxk * (self.upper[d] - self.lower[d])
            vn = max(-vmax, min(vn, vmax))
            v[d] = vn
            x[d] = self._bounds(src, kp, x[d], vn, d)

    # ---- :237-323 ------------------------------------------------------------------------------
    def _update(self, src, i, kp):
        mv, moved = kp, True
        if i == 0:
            self._learn(src, kp, kp, list(self.pb[kp]))
        elif i == 1:
            x = self.x[kp]
            before = list(x)
            for d in range(self.n):
                z = src.z(kp, d)
                x[d] = self._bounds(src, kp, x[d], self.vdavg[d] * z, d)
            moved = x != before
        elif i == 2:
            jp = src.partner(kp)
            self._gap(self.fpb[jp], self.fpb[kp])
            if self.fpb[jp] < self.fpb[kp]:
                self.events.add("op2_self")
                self._learn(src, kp, kp, list(self.pb[jp]))
            else:
                self.events.add("op2_partner")
                mv = jp
                self._learn(src, kp, jp, list(self.pb[kp]))
        else:
            self._learn(src, kp, kp, list(self.abest))
        self.fp[mv] = self.fx[mv]
        self.fx[mv] = self.evaluate(self.x[mv])
        return mv, moved

    # ---- :338-354 ------------------------------------------------------------------------------
    def _update_abest(self, src, kp, mv):
        x = self.x[mv]
        for d in range(self.n):
            if src.coin(kp, d) < self.Pl[mv]:
                old = self.abest[d]
                self.abest[d] = x[d]
                fnew = self.evaluate(self.abest)
                self._gap(fnew, self.fabest, same_point=x[d] == old)
                if fnew < self.fabest:
                    self.events.add("alg2_accept")
                    self.fabest = fnew
                else:
                    self.events.add("alg2_reject")
                    self.abest[d] = old

    # ---- :412-439 ------------------------------------------------------------------------------
    def _selection_ratios(self, k):
        s, p, g, G = self.s[k], self.p[k], self.g[k], self.G[k]
        sump = 0.
        for v in p:
            sump += v
        smax = max(s)
        r, sumr = [0.] * NSTRAT, 0.
        for i in range(NSTRAT):
            cki = 0.9 if (g[i] == 0 and s[i] >= smax) else 1.
            r[i] = cki * s[i]
            if sump > 0.:
                r[i] += (p[i] / sump) * self.alpha
            if G[i] > 0:
                r[i] += (1. * g[i]) / G[i] * (1. - self.alpha)
            sumr += r[i]
        for i in range(NSTRAT):
            s[i] = r[i] / sumr * (1. - NSTRAT * self.gamma) + self.gamma

    # ---- :94-153 -------------------------------------------------------------------------------
    def iterate(self, src):
        n, np_ = self.n, self.np
        self.vdavg = [0.] * n
        for k in range(np_):
            v = self.v[k]
            for d in range(n):
                self.vdavg[d] += abs(v[d]) / np_
        self.alpha = src.alpha()
        for kp in range(np_):
            self.PF[kp] = self.CF[kp]
            if np_ * src.force(kp) < self.mfes:
                i = NSTRAT - 1
                self.events.add("forced")
            else:
                s = self.s[kp]
                tot = 0.
                for sv in s:
                    tot += sv
                U = between(src.roulette(kp), 0., tot)
                i = 3
                for j in range(NSTRAT):
                    U -= s[j]
                    if U <= 0.:
                        i = j
                        break
            self.events.add("op%d" % i)
            self.CF[kp] = i == NSTRAT - 1
            k, moved = self._update(src, i, kp)
            self.G[k][i] += 1
            self._gap(self.fx[k], self.fp[k], same_point=not moved)
            if self.fx[k] < self.fp[k]:
                self.g[k][i] += 1
                self.m[k] = 0
                self.p[k][i] += (self.fp[k] - self.fx[k])
                self._update_abest(src, kp, k)
            else:
                self.m[k] += 1
            self._gap(self.fx[k], self.fpb[k], same_point=not moved)
            if self.fx[k] < self.fpb[k]:
                self.pb[k] = list(self.x[k])
                self.fpb[k] = self.fx[k]
                self._gap(self.fx[k], self.fabest, same_point=self.x[k] == self.abest)
                if self.fx[k] < self.fabest:
                    self.abest = list(self.x[k])
                    self.fabest = self.fx[k]
            if self.m[k] >= self.Uf[k]:
                self.events.add("refresh")
                self._selection_ratios(k)
                self.p[k] = [0.] * NSTRAT
                self.g[k] = [0] * NSTRAT
                self.G[k] = [0] * NSTRAT
        self._update_par(src)

    # ---- :362-381, :394-410 --------------------------------------------------------------------
    def _update_par(self, src):
        src.shuffle(self.perm)
        for k in range(self.np):
            self._par_particle(k)
        pfev = max(0., min((1. * self.fev) / self.mfev, 1.))
        self.mfes_real = self.np * (1. - math.exp(-100. * math.pow(pfev, 3.)))
        self.mfes = int(self.mfes_real)
        for k in range(self.np):
            s = self.s[k]
            if not self.CF[k] and self.PF[k]:
                self.events.add("cf_off")
                tot = (0. + s[0] + s[1]) + s[2]
                for i in range(NSTRAT - 1):
                    s[i] /= tot
                s[NSTRAT - 1] = 0.
            if self.CF[k] and not self.PF[k]:
                self.events.add("cf_on")
                self.p[k] = [0.] * NSTRAT
                self.g[k] = [0] * NSTRAT
                self.G[k] = [0] * NSTRAT
                self.s[k] = [1. / NSTRAT] * NSTRAT
        self.omega = self.omegamax - (self.omegamax - self.omegamin) * pfev

    # ---- :173-189 ------------------------------------------------------------------------------
    def converged(self):
        count, mean, m2 = 0, 0., 0.
        for k in range(self.np):
            x = jm.dnrm2(self.x[k])
            count += 1
            delta = x - mean
            mean += delta / count
            delta2 = x - mean
            m2 += delta * delta2
        return m2 <= (self.np - 1) * self.tol * self.tol

    # ---- :159-171 ------------------------------------------------------------------------------
    def optimize(self, make_source):
        """the loop of optimize() after init(); make_source() gives the source of a generation"""
        converge = False
        while self.fev < self.mfev:
            self.iterate(make_source())
            if self.converged():
                converge = True
                break
        return self.fev, converge, self.fabest

    def state(self):
        out = {}
        for k in self.KEYS:
            v = getattr(self, k)
            out[k] = np.array(v, dtype=float).ravel() if isinstance(v, list) else v
        return out


class Mt19937Words(jm.Words):
    """jaya_model.Words over a live std::mt19937 seeded as Random::seed(k) does (init_genrand)"""

    def __init__(self, seed, block=4096):
        super().__init__([])
        self.bg = np.random.MT19937()
        st = np.random.RandomState(int(seed)).get_state()
        self.bg.state = {"bit_generator": "MT19937", "state": {"key": st[1], "pos": int(st[2])}}
        self.block = block

    def take(self, count):
        """the next `count` raw outputs as a list"""
        return [self.next() for _ in range(count)]

    def next(self):
        if self.i == len(self.w):
            self.w = [int(v) for v in self.bg.random_raw(self.block)]
            self.i = 0
        v = self.w[self.i]
        self.i += 1
        return v
