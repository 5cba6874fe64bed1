"""Scalar model of ACD (acd.cpp:54-334): adaptive coordinate descent with adaptive encoding.

Every operation is one IEEE operation on Python floats per operation of the reference, in its order.  The
eigendecomposition is HANDED IN: `decompose(model)` is called where the reference runs tred2 / tql2 and the
repairs (:287-332), with the model's C already updated, and returns (B, invB, diagd) as row-major lists
(and may shift the diagonal of model.C as the repair does).  Three of them are here:

recorded(states)   the reference's own B, invB and diagd after each update (tests/golden/acd_runs.json):
                   with them the model reproduces every recorded point, value, sigma, m, p and C bit for bit
eigh_decompose     numpy.linalg.eigh with the reference's repairs, roots and products: a stand-in where no
                   trajectory is compared (seed choice, the repair branches, whole runs as distributions)
(a device's)       tests/test_acd_gpu.py feeds the device's own B, invB and diagd

The objective comes in two forms: chol_model.objective (serial sums: the reference's values) and
slpso_model.device_objective (the device's lane sums and butterfly: the device's values).

The archive is ranked stably with respect to the persisting `order` (Python's sort is stable, as the
reference's insertion sort is for 2 n <= 16)."""
import math

INF = float("inf")


def cmax(a, b):
    """std::max(a, b): a unless a < b"""
    return b if a < b else a


def cmin(a, b):
    """std::min(a, b): a unless b < a"""
    return b if b < a else a


def converge_period(n):
    return 10 + int(20 * math.pow(1. * n, 1.5))     # :118


def dxmax_full(sigma, B):
    """the reference's n^2 loop (:216-222)"""
    n = len(sigma)
    d = 0.
    for ix in range(n):
        for i in range(n):
            d = cmax(d, abs(sigma[ix] * B[i][ix]))
    return d


def column_max(B):
    n = len(B)
    cm = []
    for j in range(n):
        m = 0.
        for i in range(n):
            m = cmax(m, abs(B[i][j]))
        cm.append(m)
    return cm


def dxmax_colmax(sigma, cm):
    """the device's form: max_j sigma[j] colmax[j]"""
    d = 0.
    for s, c in zip(sigma, cm):
        d = cmax(d, abs(s * c))
    return d


def repair_and_root(C, evals):
    """:299-320 on ascending eigenvalues; shifts the diagonal of C in place; returns diagd"""
    n = len(evals)
    d = [float(v) for v in evals]
    if d[0] <= 0.:
        d = [cmax(v, 0.) for v in d]
        shift = d[n - 1] / 1e14
        for i in range(n):
            C[i][i] += shift
            d[i] += shift
    if d[n - 1] > 1e14 * d[0]:
        shift = d[n - 1] / 1e14 - d[0]
        for i in range(n):
            C[i][i] += shift
            d[i] += shift
    return [math.sqrt(v) for v in d]


def basis_products(V, d):
    """:323-332: invB = diag(1 / d) V^T, B = V diag(d)"""
    n = len(d)
    invB = [[V[j][i] / d[i] for j in range(n)] for i in range(n)]
    B = [[V[i][j] * d[j] for j in range(n)] for i in range(n)]
    return B, invB


def eigh_decompose(model):
    import numpy as np
    n = model.n
    A = np.array(model.C)
    A = np.tril(A) + np.tril(A, -1).T           # tred2 reads the lower triangle (:290-294)
    w, V = np.linalg.eigh(A)
    d = repair_and_root(model.C, list(w))
    B, invB = basis_products([[float(V[i][j]) for j in range(n)] for i in range(n)], d)
    return B, invB, d


def recorded(updates):
    """the decompositions of a recorded run, in order; each entry has B, invB, diagd (flat, row-major)"""
    it = iter(updates)

    def decompose(model):
        u = next(it)
        n = model.n
        B = [list(u["B"][i * n:(i + 1) * n]) for i in range(n)]
        invB = [list(u["invB"][i * n:(i + 1) * n]) for i in range(n)]
        return B, invB, list(u["diagd"])
    return decompose


class Acd:
    def __init__(self, f, n, lower, upper, mfev, ftol, xtol, ksucc=2., kunsucc=0.5, decompose=eigh_decompose):
        self.f, self.n = f, n
        self.lower, self.upper = [float(v) for v in lower], [float(v) for v in upper]
        self.mfev, self.ftol, self.xtol, self.ksucc, self.kunsucc = mfev, ftol, xtol, ksucc, kunsucc
        self.decompose = decompose

    def start(self, xbest):
        """init() (:54-120) with x_best given (the reference draws it)"""
        n = self.n
        self.c1 = 0.5 / n
        self.cp = 1. / math.sqrt(1. * n)
        self.ix = self.it = self.itae = self.fev = 0
        self.improved = False
        self.fbest = INF
        self.xbest = [float(v) for v in xbest]
        self.sigma = [(self.upper[i] - self.lower[i]) / 4. for i in range(n)]
        self.X = [[0.] * n for _ in range(2 * n)]
        self.fx = [0.] * (2 * n)
        self.order = list(range(2 * n))
        self.weights = [1. / n] * n
        self.p = [0.] * n
        self.m = [0.] * n
        self.mold = [0.] * n
        self.diagd = [1.] * n
        eye = lambda: [[1. if i == j else 0. for j in range(n)] for i in range(n)]
        self.B, self.invB, self.C = eye(), eye(), eye()
        self.period = converge_period(n)
        self.fhist = [0.] * self.period
        self.evals = []
        self.updated = False
        self.denom = None
        return self

    def points(self):
        """:125-130"""
        n, ix = self.n, self.ix
        x1, x2 = [], []
        for i in range(n):
            dx = self.sigma[ix] * self.B[i][ix]
            x1.append(cmax(self.lower[i], cmin(self.xbest[i] - dx, self.upper[i])))
            x2.append(cmax(self.lower[i], cmin(self.xbest[i] + dx, self.upper[i])))
        return x1, x2

    def value(self, x):
        v = float(self.f(x))
        return INF if v != v else v

    def iterate(self, values=None):
        """:122-178; `values`: (f1, f2) instead of calling the objective"""
        n, ix = self.n, self.ix
        x1, x2 = self.points()
        f1, f2 = values if values is not None else (self.value(x1), self.value(x2))
        self.evals = [(x1, f1), (x2, f2)]
        self.fev += 2
        self.margin = min(_gap(f1, self.fbest), INF)
        success = f1 < self.fbest or f2 < self.fbest
        self.path = ("x1" if f1 < self.fbest else "") + ("x2" if f2 < cmin(self.fbest, f1) else "")
        if f1 < self.fbest:
            self.xbest = list(x1)
            self.fbest = f1
        self.margin = min(self.margin, _gap(f2, self.fbest))
        if f2 < self.fbest:
            self.xbest = list(x2)
            self.fbest = f2
        self.fhist[self.it % self.period] = self.fbest
        if success:
            self.sigma[ix] *= self.ksucc
            self.improved = True
        else:
            self.sigma[ix] *= self.kunsucc
        self.success = success
        self.X[2 * ix], self.fx[2 * ix] = list(x1), f1
        self.X[2 * ix + 1], self.fx[2 * ix + 1] = list(x2), f2
        self.updated = False
        if self.improved and ix == n - 1:
            self.order.sort(key=lambda i: self.fx[i])           # stable
            fs = [self.fx[i] for i in self.order]
            self.margin = min([self.margin] + [_gap(a, b) for a, b in zip(fs, fs[1:])])
            self.update_ae()
            self.improved = False
            self.updated = True
        self.ix = (ix + 1) % n
        self.it += 1

    def mean(self):
        n = self.n
        m = [0.] * n
        for i in range(n):
            row = self.X[self.order[i]]
            for d in range(n):
                m[d] += row[d] * self.weights[i]
        return m

    def update_ae(self):
        """:236-334"""
        n = self.n
        self.itae += 1
        if self.itae == 1:
            self.m = self.mean()
            return
        self.mold = list(self.m)
        self.m = self.mean()
        cp, c1 = self.cp, self.c1
        artmp = []
        for i in range(n):
            a = 0.
            for j in range(n):
                a += self.invB[i][j] * (self.m[j] - self.mold[j])
            artmp.append(a)
        denom = 0.
        for a in artmp:
            denom = denom + a * a
        self.denom = denom
        if denom <= 0.:
            for i in range(n):
                self.p[i] *= (1. - cp)
        else:
            factor = math.sqrt(cp * (2. - cp) * n / denom)
            for i in range(n):
                self.p[i] = (1. - cp) * self.p[i] + factor * (self.m[i] - self.mold[i])
        for i in range(n):
            for j in range(n):
                self.C[i][j] = (1. - c1) * self.C[i][j] + c1 * self.p[i] * self.p[j]
        self.B, self.invB, self.diagd = self.decompose(self)

    def history_rule(self):
        """the first rule of converged() (:207-213) and the ring indices it reads"""
        if self.it > self.period:
            i0 = (self.it - 1 + self.period) % self.period
            i1 = self.it % self.period
            return abs(self.fhist[i1] - self.fhist[i0]) < self.ftol, (i0, i1)
        return False, None

    def converged(self):
        """:204-228; 0, or the rule: 1 the history, 2 the step"""
        if self.history_rule()[0]:
            return 1
        return 2 if dxmax_full(self.sigma, self.B) < self.xtol else 0

    def optimize(self, xbest):
        """:184-196; returns the stop flag: 1 converged, 2 budget"""
        self.start(xbest)
        while self.fev < self.mfev:
            self.iterate()
            if self.converged():
                return 1
        return 2


def _gap(a, b):
    """relative distance of two compared values (inf: nothing to compare)"""
    if a == b:
        return 0.
    if math.isinf(a) or math.isinf(b):
        return INF
    return abs(a - b) / max(abs(a), abs(b))


def residuals(B, invB, C):
    """||B B^T - C||_F / ||C||_F over the lower triangle mirrored, and ||invB B - I||_max"""
    import numpy as np
    B, invB, C = np.array(B), np.array(invB), np.array(C)
    S = np.tril(C) + np.tril(C, -1).T
    r1 = np.linalg.norm(B @ B.T - S) / np.linalg.norm(S)
    r2 = np.abs(invB @ B - np.eye(len(B))).max()
    return float(r1), float(r2)


# ---- the compact form of a recorded run (tests/golden/acd_runs.json) -----------------------------------
# Lossless: unpack_run(pack_run(rec)) == rec, which scripts/gen_acd_golden.py asserts for every run against
# what the reference printed.
#   a point     while B is diagonal it differs from x_best in one coordinate: {"at": [i..], "x": [..], "f": f}
#               holds the coordinates that differ from the x_best the step started from.  A dense point is
#               {"f": f, "not": [[i, x_i]..]}: clamp(x_best -+ sigma[ix] B[i][ix]) from the recorded x_best,
#               sigma and B, and the coordinates where the reference's bits are others (none in the fixture)
#   C           (1 - c1) C' + c1 p_i p_j from the C' recorded before and the recorded p, and in "C_not" the
#               entries where the reference's bits are others (a repair's shift would show there)
#   B, invB     one matrix V with B[i][j] = V[i][j] * d[j] and invB[j][i] = V[i][j] / d[j] bit for bit (found
#               next to B[i][j] / d[j]); the entries for which no such V exists are kept as they are
# "crc" of a step and "C_crc" of an update are zlib.crc32 over the doubles the REFERENCE printed (both
# points; C): unpack_run checks what it rebuilt against them, so the rebuilt numbers are the reference's
# and not merely this file's arithmetic.
import re
import struct
import zlib


def _fh(s):
    return float.fromhex(s)


def _strings(o, f):
    """o with f applied to every float.hex string in it"""
    if isinstance(o, dict):
        return {k: _strings(v, f) for k, v in o.items()}
    if isinstance(o, list):
        return [_strings(v, f) for v in o]
    return f(o) if isinstance(o, str) and "0x" in o else o


def _short(h):
    """float.hex without the mantissa's trailing zeros (float.fromhex reads it back to the same bits)"""
    return re.sub(r"(\.[0-9a-f]*?)0+p", r"\1p", h)


def _long(h):
    return float.fromhex(h).hex()


def _crc(hexes):
    return zlib.crc32(struct.pack("<%dd" % len(hexes), *[_fh(h) for h in hexes]))


def _find_v(b, ib, d):
    v0 = b / d
    for k in range(8):
        for up in (True, False):
            v = v0
            for _ in range(k):
                v = math.nextafter(v, INF if up else -INF)
            if v * d == b and v / d == ib and math.copysign(1., v * d) == math.copysign(1., b):
                return v
    return None


class _Walk:
    """what pack_run and unpack_run both follow: x_best, f_best, sigma, B and C as recorded so far"""

    def __init__(self, rec):
        n = self.n = rec["n"]
        self.box = rec["box"]
        self.xbest, self.fbest = list(rec["init"]["xbest"]), INF
        self.sigma = [_fh(s) for s in rec["init"]["sigma"]]
        self.B = [[1. if i == j else 0. for j in range(n)] for i in range(n)]
        self.C = [1. if i == j else 0. for i in range(n) for j in range(n)]
        self.g = 0

    def predicted(self, k):
        n, ix = self.n, self.g % self.n
        xb = [_fh(s) for s in self.xbest]
        out = []
        for i in range(n):
            dx = self.sigma[ix] * self.B[i][ix]
            out.append(cmax(-self.box, cmin(xb[i] - dx if k == 0 else xb[i] + dx, self.box)).hex())
        return out

    def predicted_c(self, p):
        n, c1 = self.n, 0.5 / self.n
        p = [_fh(s) for s in p]
        return [((1. - c1) * self.C[i * n + j] + c1 * p[i] * p[j]).hex() for i in range(n) for j in range(n)]

    def step_done(self, pts, st):
        """pts: the two points as (x hex list, f hex); st: the step's record (full or compact)"""
        for x, f in pts:
            if _fh(f) < self.fbest:
                self.xbest, self.fbest = list(x), _fh(f)
        self.sigma[self.g % self.n] = _fh(st["sigma"])
        self.g += 1

    def update_done(self, C, B):
        n = self.n
        self.C = [_fh(s) for s in C]
        self.B = [[_fh(B[i * n + j]) for j in range(n)] for i in range(n)]


def pack_run(rec):
    n = rec["n"]
    out = {k: v for k, v in rec.items() if k != "steps"}
    out["steps"] = []
    wk = _Walk(rec)
    for st in rec["steps"]:
        ev, pts, full = st["evals"], [], []
        for k in (0, 1):
            x, f = ev[k * (n + 1):k * (n + 1) + n], ev[k * (n + 1) + n]
            full.append((x, f))
            at = [i for i in range(n) if x[i] != wk.xbest[i]]
            if 2 * len(at) < n:
                pts.append({"at": at, "x": [x[i] for i in at], "f": f})
            else:
                pred = wk.predicted(k)
                pts.append({"f": f, "not": [[i, x[i]] for i in range(n) if x[i] != pred[i]]})
        new = {k: v for k, v in st.items() if k not in ("evals", "update")}
        new["evals"], new["crc"] = pts, _crc(full[0][0] + full[1][0])
        wk.step_done(full, st)
        u = st.get("update")
        if u is not None:
            nu = {k: v for k, v in u.items() if k not in ("C", "B", "invB")}
            if "C" in u:
                C, B, iB, d = u["C"], u["B"], u["invB"], u["diagd"]
                pred = wk.predicted_c(u["p"])
                nu["C_not"] = [[q, C[q]] for q in range(n * n) if C[q] != pred[q]]
                nu["C_crc"] = _crc(C)
                V, keep = [], []
                for i in range(n):
                    for j in range(n):
                        v = _find_v(_fh(B[i * n + j]), _fh(iB[j * n + i]), _fh(d[j]))
                        V.append((0. if v is None else v).hex())
                        if v is None:
                            keep.append([i * n + j, B[i * n + j], iB[j * n + i]])
                nu["V"], nu["V_not"] = V, keep
                wk.update_done(C, B)
            new["update"] = nu
        out["steps"].append(new)
    return _strings(out, _short)


def unpack_run(rec):
    rec = _strings(rec, _long)
    n = rec["n"]
    out = {k: v for k, v in rec.items() if k != "steps"}
    out["steps"] = []
    wk = _Walk(rec)
    for st in rec["steps"]:
        full = []
        for k, p in enumerate(st["evals"]):
            if "at" in p:
                x = list(wk.xbest)
                for i, v in zip(p["at"], p["x"]):
                    x[i] = v
            else:
                x = wk.predicted(k)
                for i, v in p["not"]:
                    x[i] = v
            full.append((x, p["f"]))
        assert _crc(full[0][0] + full[1][0]) == st["crc"], "a rebuilt point is not the reference's"
        new = {k: v for k, v in st.items() if k not in ("evals", "update", "crc")}
        new["evals"] = full[0][0] + [full[0][1]] + full[1][0] + [full[1][1]]
        wk.step_done(full, st)
        u = st.get("update")
        if u is not None:
            nu = {k: v for k, v in u.items() if k not in ("C_not", "C_crc", "V", "V_not")}
            if "V" in u:
                d = [_fh(s) for s in u["diagd"]]
                C = wk.predicted_c(u["p"])
                for q, v in u["C_not"]:
                    C[q] = v
                assert _crc(C) == u["C_crc"], "the rebuilt C is not the reference's"
                B, iB = [None] * (n * n), [None] * (n * n)
                for i in range(n):
                    for j in range(n):
                        v = _fh(u["V"][i * n + j])
                        B[i * n + j] = (v * d[j]).hex()
                        iB[j * n + i] = (v / d[j]).hex()
                for idx, b, ib in u["V_not"]:
                    i, j = divmod(idx, n)
                    B[idx], iB[j * n + i] = b, ib
                nu["C"], nu["B"], nu["invB"] = C, B, iB
                wk.update_done(C, B)
            new["update"] = nu
        out["steps"].append(new)
    return out
