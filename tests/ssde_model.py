"""SSDE (Kumar et al. 2019; Zhao et al. 2022) restated in pure Python in the reference's operation order
(src/multivariate/de/ssde.cpp; the line numbers below are its).  Every arithmetic step is one IEEE double
operation in the order the reference writes it, so the model fed the reference's own draws reproduces its
states bit for bit (tests/test_ssde_model.py), and the GPU tests lean on the model.

randA() (:410-432) is the identity with the shuffled coordinates paired off two by two; the model keeps the
dense matrix out of it and adds a row's (a column's) two terms in the order of their index, as the dense
loops of computeTrialPoint (:434-453) meet them.  The products with the zeros of A change nothing while z
is finite.

A generation takes its draws from a *source*, an object with
    shuffle(iwork)  iL(i)  zr(i)  ub(i, d)  sample3(i, np)  pbest(i, itop)  ci(i, l2)
    zcr(i)  j0(i)  ucross(i, d)  uredraw(i, d)
Three sources:
    WordsSource   decodes the reference's mt19937 words in the reference's program order
                  (jaya_model.Words) and writes the table below as it goes
    TableSource   reads the table of bbo_ssde_inject_draws / get_state("draws"):
                  [perm: n][npinit x (9 + 3 n)] -- per member iL, the normal of prank, p, q, r, pbest, the
                  accepted ci, the normal of CRi, j0, then n uniforms each of b, the crossover, the redraw
    RngSource     the model's own generator: WordsSource over a numpy MT19937
"""
import base64
import math

import numpy as np

import jaya_model as jm
import slpso_model
from slpso_model import between, device_objective, words_crc     # noqa: F401 (the tests take them from here)

INF = float("inf")
HEAD = 9
SIN, COS = math.sin(1e-12), math.cos(1e-12)       # :427-429
FLOAT_KEYS = ("x", "f", "L1", "L2", "LCR")
INT_KEYS = ("k", "kCR", "np", "fev", "convcount")


def table_len(n, npinit):
    return n + npinit * (HEAD + 3 * n)


# ---- the fixture's compact form (tests/golden/ssde_runs.json) ----------------------------------------------
# A float array of a state is kept whole (packed little-endian doubles in base64) in the first state of a
# record and wherever its length changed; otherwise as the entries whose bits differ from the state before:
# runs [[start, length], ...] under "r" and their values under "v".  Nothing is rounded.
def b64(a):
    return base64.b64encode(np.asarray(a, "<f8").tobytes()).decode()


def unb64(s):
    return np.frombuffer(base64.b64decode(s), "<f8").astype(float)


def _bits(a):
    return np.ascontiguousarray(a, dtype="<f8").view(np.uint64)


def pack_states(states):
    prev = None
    for st in states:
        full = {k: np.asarray(st[k], float) for k in FLOAT_KEYS}
        for k in FLOAT_KEYS:
            cur = full[k]
            if prev is None or prev[k].size != cur.size:
                st[k] = b64(cur)
                continue
            ch = np.flatnonzero(_bits(cur) != _bits(prev[k]))
            runs = []
            for i in ch:
                if runs and runs[-1][0] + runs[-1][1] == i:
                    runs[-1][1] += 1
                else:
                    runs.append([int(i), 1])
            st[k] = {"r": runs, "v": b64(cur[ch])} if ch.size else {}
        prev = full


def unpack_states(states):
    prev = None
    for st in states:
        full = {}
        for k in FLOAT_KEYS:
            ent = st[k]
            if isinstance(ent, str):
                full[k] = unb64(ent)
                continue
            cur = prev[k].copy()
            if ent:
                cur[[i for s, c in ent["r"] for i in range(s, s + c)]] = unb64(ent["v"])
            full[k] = cur
        st.update(full)
        prev = full


class Mt19937Words(slpso_model.Mt19937Words):
    """slpso_model.Mt19937Words that counts the words it hands out"""
    count = 0

    def next(self):
        self.count += 1
        return super().next()


class WordsSource:
    """the reference's program order over the words; `w` is a jaya_model.Words (the cached second normal
    of the optimizer's distribution lives on across generations: keep one object, or carry `have` /
    `saved` over).  `attempts` is the largest number of draws a rejection loop took."""

    def __init__(self, w, n, npinit):
        self.w, self.n, self.npinit = w, n, npinit
        self.attempts = 0
        self.table = np.zeros(table_len(n, npinit))

    def _m(self, i):
        return self.n + i * (HEAD + 3 * self.n)

    def _put(self, off, v):
        self.table[off] = v
        return v

    def shuffle(self, iwork):
        self.w.shuffle(iwork)                               # :413 (a re-shuffle of the last)
        self.table[:self.n] = iwork

    def iL(self, i, h):
        return self._put(self._m(i), self.w.uint(0, h - 1))

    def zr(self, i):
        return self._put(self._m(i) + 1, self.w.normal())

    def ub(self, i, d):
        return self._put(self._m(i) + HEAD + d, self.w.uniform(0., 1.))

    def _other(self, np_, taken):
        v, tries = taken[0], 0
        while v in taken:
            v = self.w.uint(0, np_ - 1)
            tries += 1
        self.attempts = max(self.attempts, tries)
        return v

    def sample3(self, i, np_):                              # :459-472
        p = self._other(np_, (i,))
        q = self._other(np_, (i, p))
        r = self._other(np_, (i, p, q))
        o = self._m(i)
        self.table[o + 2:o + 5] = (p, q, r)
        return p, q, r

    def pbest(self, i, itop):
        return self._put(self._m(i) + 5, self.w.uint(0, itop))

    def _cauchy(self):
        return math.tan(math.pi * (self.w.uniform(0., 1.) - 0.5))   # :455-457

    def ci(self, i, l2):                                    # :225-229
        c, tries = self._cauchy() * 0.1 + l2, 1
        while c <= 0.:
            c, tries = self._cauchy() * 0.1 + l2, tries + 1
        self.attempts = max(self.attempts, tries)
        return self._put(self._m(i) + 6, min(1., c))

    def zcr(self, i):
        return self._put(self._m(i) + 7, self.w.normal())

    def j0(self, i):
        return self._put(self._m(i) + 8, self.w.uint(0, self.n - 1))

    def ucross(self, i, d):
        return self._put(self._m(i) + HEAD + self.n + d, self.w.uniform(0., 1.))

    def uredraw(self, i, d):
        return self._put(self._m(i) + HEAD + 2 * self.n + d, self.w.canonical())


class TableSource:
    def __init__(self, table, n, npinit):
        self.t, self.n = np.asarray(table, float).ravel(), n
        assert self.t.size == table_len(n, npinit)
        self.attempts = 0

    def _m(self, i):
        return self.n + i * (HEAD + 3 * self.n)

    def shuffle(self, iwork):
        iwork[:] = [int(v) for v in self.t[:self.n]]

    def iL(self, i, h):
        return int(self.t[self._m(i)])

    def zr(self, i):
        return float(self.t[self._m(i) + 1])

    def ub(self, i, d):
        return float(self.t[self._m(i) + HEAD + d])

    def sample3(self, i, np_):
        o = self._m(i)
        return int(self.t[o + 2]), int(self.t[o + 3]), int(self.t[o + 4])

    def pbest(self, i, itop):
        return int(self.t[self._m(i) + 5])

    def ci(self, i, l2):
        return float(self.t[self._m(i) + 6])

    def zcr(self, i):
        return float(self.t[self._m(i) + 7])

    def j0(self, i):
        return int(self.t[self._m(i) + 8])

    def ucross(self, i, d):
        return float(self.t[self._m(i) + HEAD + self.n + d])

    def uredraw(self, i, d):
        return float(self.t[self._m(i) + HEAD + 2 * self.n + d])


class RngSource(WordsSource):
    """the model's own generator: WordsSource over the raw words of a numpy MT19937"""

    def __init__(self, seed, n, npinit):
        super().__init__(Mt19937Words(seed), n, npinit)


class Ssde:
    """min_np: the floor of the shrink (0: the reference's, which can leave 3 members after the last
    generation of a run; 4: the device's)"""
    KEYS = FLOAT_KEYS + INT_KEYS + ("perm",)

    def __init__(self, f, lower, upper, mfev, npinit, tol, patience=1000, npmin=4, ptop=0.11, h=100, usede=False,
                 repaircr=True, min_np=0):
        self.f = f
        self.lower, self.upper = [float(v) for v in lower], [float(v) for v in upper]
        self.n = len(self.lower)
        self.mfev, self.npinit, self.tol, self.patience = int(mfev), int(npinit), float(tol), int(patience)
        self.npmin, self.ptop, self.H = int(npmin), float(ptop), int(h)
        self.usede, self.repaircr, self.min_np = bool(usede), bool(repaircr), int(min_np)
        self.trace = False
        self.points, self.gaps, self.events = [], [], set()
        self.repairs = {"low": 0, "high": 0}    # coordinates the DE trial's redraw met past each bound

    def evaluate(self, x):
        v = float(self.f(x))
        v = INF if v != v else v
        if self.trace:
            self.points.append((list(x), v))
        return v

    # :59-132
    def start(self, X, fvals=None, fev=None):
        """the pool from given rows: evaluated (or with the given values), sorted, the best npinit kept"""
        rows = [[float(v) for v in r] for r in X]
        vals = [self.evaluate(r) for r in rows] if fvals is None else [float(v) for v in fvals]
        order = sorted(range(len(rows)), key=lambda k: vals[k])
        self._note_sorted([vals[k] for k in order])
        order = order[:self.npinit]
        self.x = [rows[k] for k in order]
        self.fx = [vals[k] for k in order]
        self.np = len(self.x)
        self.fev = len(rows) if fev is None else fev
        self.convcount = 0
        self.iwork = list(range(self.n))
        self.L1, self.L2, self.LCR = [0.5] * self.H, [0.5] * self.H, [0.5] * self.H
        self.k = self.kCR = 1

    def init_reference(self, w):
        """init() from the words: the uniform pool (:90-98) and, with usede, its opposites (:101-112)"""
        n = self.n
        X = [[w.uniform(self.lower[j], self.upper[j]) for j in range(n)] for _ in range(self.npinit)]
        if self.usede:
            X += [[self.lower[j] + self.upper[j] - r[j] for j in range(n)] for r in X]
        self.start(X)

    def _gap(self, a, b):
        if self.trace and a != INF and b != INF:
            m = max(abs(a), abs(b))
            self.gaps.append(abs(a - b) / m if m > 0. else 0.)

    def _note_sorted(self, vals):
        for a, b in zip(vals, vals[1:]):
            self._gap(a, b)

    # :434-453 with the sparse A
    def trial_point(self, i, ci, z, b):
        n, iw = self.n, self.iwork
        partner, role = [0] * n, [0] * n
        for pos in range(n):
            d = iw[pos]
            if n % 2 and pos == n - 1:
                partner[d], role[d] = d, 0
            elif pos % 2 == 0:
                partner[d], role[d] = iw[pos + 1], 1
            else:
                partner[d], role[d] = iw[pos - 1], 2
        work = [0.] * n
        for d in range(n):
            o = partner[d]
            acc = 0.
            if role[d] == 0:
                acc += 1. * z[d]
            else:
                terms = [(d, SIN * z[d]), (o, (COS if role[d] == 1 else -COS) * z[o])]
                for _, t in sorted(terms):
                    acc += t
            work[d] = acc * b[d]
        y = [0.] * n
        xi = self.x[i]
        for d in range(n):
            o = partner[d]
            v = xi[d]
            if role[d] == 0:
                v += ci * 1. * work[d]
            else:
                terms = [(d, ci * SIN * work[d]), (o, ci * (-COS if role[d] == 1 else COS) * work[o])]
                for _, t in sorted(terms):
                    v += t
            y[d] = max(self.lower[d], min(self.upper[d], v))
        return y

    # :134-361
    def iterate(self, src):
        n, x, fx = self.n, self.x, self.fx
        oldbestf = fx[0]
        src.shuffle(self.iwork)
        SR, SC, W, SCR, WCR = [], [], [], [], []
        pairs, pairs_cr = [], []          # (f_i, fy) of the successes: what the weights were formed from
        for i in range(self.np):
            iL = src.iL(i, self.H)
            prank = max(0., min(1., src.zr(i) * 0.1 + self.L1[iL]))
            b = [1. if src.ub(i, r) < prank else 0. for r in range(n)]
            pi, qi, ri = src.sample3(i, self.np)
            itop = max(1, int(self.ptop * self.np))
            pbest = src.pbest(i, itop)
            R = (1. * self.fev) / self.mfev
            if self.usede:
                lead = x[pi] if R < 0.333 else x[pbest] if R < 0.666 else x[0]
                self.events.add("explore" if R < 0.333 else "balance" if R < 0.666 else "exploit")
                z = [lead[d] + x[qi][d] - x[ri][d] - x[i][d] + R * (x[pbest][d] - x[qi][d]) for d in range(n)]
            else:
                lead = x[pi] if i < 0.5 * self.np else x[pbest]
                z = [lead[d] + x[qi][d] - x[ri][d] - x[i][d] for d in range(n)]
            ci = src.ci(i, self.L2[iL])
            y = self.trial_point(i, ci, z, b)
            fy = self.evaluate(y)
            self.fev += 1
            self._gap(fy, fx[i])
            if fy <= fx[i]:
                if fy < fx[i]:
                    SR.append(prank)
                    SC.append(ci)
                    W.append(fx[i] - fy)
                    pairs.append((fx[i], fy))
                    self.events.add("ss_success")
                x[i] = list(y)
                fx[i] = fy
            elif self.usede:
                CRi = max(0., min(1., src.zcr(i) * 0.1 + self.LCR[iL]))
                cr1 = 0.
                j0 = src.j0(i)
                u = [0.] * n
                for d in range(n):
                    if d == j0 or src.ucross(i, d) <= CRi:
                        u[d] = x[pi][d] + R * (x[0][d] - x[qi][d]) + R * (x[0][d] - x[ri][d])
                        if u[d] < self.lower[d] or u[d] > self.upper[d]:
                            self.repairs["low" if u[d] < self.lower[d] else "high"] += 1
                            u[d] = between(src.uredraw(i, d), self.lower[d], self.upper[d])
                            self.events.add("de_redraw")
                        cr1 += 1.
                    else:
                        u[d] = x[i][d]
                cr1 = cr1 / n if self.repaircr else CRi
                fu = self.evaluate(u)
                self.fev += 1
                self._gap(fu, fx[i])
                if fu <= fx[i]:
                    if fu < fx[i]:
                        SCR.append(cr1)
                        WCR.append(fx[i] - fu)
                        pairs_cr.append((fx[i], fu))
                        self.events.add("de_success")
                    x[i] = u
                    fx[i] = fu
                else:
                    self.events.add("de_failure")
        self.successes = (pairs, pairs_cr)
        if SR:
            rn = rd = cn = cd = 0.
            for sr, sc, w in zip(SR, SC, W):
                rn += w * sr * sr
                rd += w * sr
                cn += w * sc * sc
                cd += w * sc
            self.L1[self.k - 1] = _div(rn, rd)
            self.L2[self.k - 1] = _div(cn, cd)
            self.k += 1
            if self.k > self.H:
                self.k = 1
                self.events.add("wrap")
        if self.usede and SCR:
            num = den = 0.
            for cr, w in zip(SCR, WCR):
                num += w * cr * cr
                den += w * cr
            self.LCR[self.kCR - 1] = _div(num, den)
            self.kCR += 1
            if self.kCR > self.H:
                self.kCR = 1
                self.events.add("wrap_cr")
        order = sorted(range(self.np), key=lambda k: fx[k])
        self.x, self.fx = [x[k] for k in order], [fx[k] for k in order]
        self._note_sorted(self.fx)
        self.convcount = 0 if self.fx[0] < oldbestf else self.convcount + 1
        npnew = int(self.npinit + (self.npmin - self.npinit) * (1. * self.fev) / self.mfev)
        if self.np > npnew:
            self.events.add("shrink")
            self.np = max(npnew, self.min_np, 0)
            del self.x[self.np:], self.fx[self.np:]

    # :383-408
    def converged(self):
        count, mean, m2 = 0, 0., 0.
        for r in self.x:
            v = jm.dnrm2(r)
            count += 1
            delta = v - mean
            mean += delta / count
            m2 += delta * (v - mean)
        return m2 <= (self.np - 1) * self.tol * self.tol or self.convcount > self.patience

    # :368-381
    def optimize(self, src_of_generation):
        """the loop of optimize(); src_of_generation() gives the source of the next generation"""
        conv = False
        while self.fev < self.mfev:
            self.iterate(src_of_generation())
            if self.converged():
                conv = True
                break
        return list(self.x[0]), self.fev, conv

    def state(self):
        return {"x": [v for r in self.x for v in r], "f": list(self.fx), "L1": list(self.L1), "L2": list(self.L2),
                "LCR": list(self.LCR), "k": self.k, "kCR": self.kCR, "np": self.np, "fev": self.fev,
                "convcount": self.convcount, "perm": list(self.iwork)}


def _div(a, b):
    """IEEE division: 0 / 0 and x / 0 as the reference's doubles give them"""
    try:
        return a / b
    except ZeroDivisionError:
        return float("nan") if a == 0. or a != a else math.copysign(INF, a) * math.copysign(1., b)


# ---- readers of tests/golden/ssde_runs.json ------------------------------------------------------------------
def box_of(rec):
    """a record's bounds: [lo, up] for every coordinate, or "percoord", the box of tests/_boxes.py"""
    if rec["box"] == "percoord":
        from _boxes import percoord_box
        return [list(v) for v in percoord_box(rec["n"])]
    return [rec["box"][0]] * rec["n"], [rec["box"][1]] * rec["n"]


def model_of(rec, f, min_np=0):
    """the model of a "steps" record (or of any dict with its fields) over the objective f"""
    lo, up = box_of(rec)
    return Ssde(f, lo, up, rec["mfev"], rec["npinit"], rec["tol"],
                rec.get("patience", 1000), rec.get("npmin", 4), rec.get("ptop", 0.11), rec.get("h", 100),
                bool(rec.get("usede", 0)), bool(rec.get("repaircr", 1)), min_np=min_np)


def load_steps(data):
    """the "steps" records with whole float arrays, the evaluated points as arrays and every generation's
    words made again from the record's seed (their number and CRC-32 are checked)"""
    out = []
    for rec in data["steps"]:
        rec = dict(rec, init=dict(rec["init"]), states=[dict(s) for s in rec["states"]])
        unpack_states([rec["init"]] + rec["states"])
        live = Mt19937Words(rec["seed"])
        live.take(rec["init"]["words"])
        for st in rec["states"]:
            words = live.take(st["words"]["count"])
            assert words_crc(words) == st["words"]["crc32"], rec["name"]
            st["words"] = words
            st["pts"], st["vals"] = unb64(st["pts"]).reshape(-1, rec["n"]), unb64(st["vals"])
        out.append(rec)
    return out


def tables_of(rec, f):
    """the draw tables of a record's generations: the model walks the record from the words and keeps
    what WordsSource wrote; also the successes of each generation as ([(f_i, fy)], [(f_i, fu)])"""
    m = model_of(rec, f)
    m.start(rec["init"]["x"].reshape(rec["npinit"], rec["n"]), rec["init"]["f"], fev=rec["init"]["fev"])
    tables, successes, have, saved = [], [], False, 0.
    for st in rec["states"]:
        w = jm.Words(st["words"])
        w.have, w.saved = have, saved
        src = WordsSource(w, rec["n"], rec["npinit"])
        m.iterate(src)
        have, saved = w.have, w.saved
        tables.append(src.table)
        successes.append(m.successes)
    return tables, successes
