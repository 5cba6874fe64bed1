"""Pure-Python restatement of the reference's PikaiaSearch (src/multivariate/pikaia/pikaia.cpp) for irep = 1,
written from its description: the same IEEE operations in the same order.

Draws come from a source.  `WordsSource` decodes the raw 32-bit words of the reference's global mt19937 in the
reference's program order (jaya_model.Words: Random::get(0., 1.) is one canonical double of two words).
`TableSource` reads the table of bbo_pikaia_inject_draws.  Either way the model logs the table of the
generation (`table`, layout: `table_layout`), so a recorded generation of the reference can be handed to the
device.

`order="rqsort"` ranks with the reference's median-of-three quicksort (insertion sort below 11 keys, not
stable), `order="stable"` with the device's rule: fitness ascending, ties by row.  The fitness the GA maximises
is -f(lower + u (upper - lower)) (one multiply, one add), or f(u) under raw=True.  repair=True stores every
initial value, counts np evaluations per generation, keeps the stored value of the elite row and divides by
|f_best + f_median| in imut 2 / 5."""
import math
import struct
import zlib

ATTEMPTS = 64
MIN_GAP = 1e-6          # two values this close (relative) may rank the other way round on the device
RDIF_GAP = 1e-9         # rdif this close to a threshold may fall on its other side
DEFAULTS = dict(pcross=0.85, imut=2, pmut=0.005, pmutmn=0.0005, pmutmx=0.25, fdif=1., irep=1, ielite=0)
PATHS = ("one_point", "two_point", "no_cross", "uniform", "creep", "carry_up", "carry_down", "clamp_0", "clamp_9",
         "elite_taken", "pmut_raised", "pmut_lowered", "pmut_held")


def crc(values):
    """CRC-32 of the doubles as they lie in memory (little-endian)"""
    flat = [float(v) for v in values]
    return zlib.crc32(struct.pack("<%dd" % len(flat), *flat))


def table_layout(n, np_, nd):
    loci = n * nd
    per_child = 1 + 2 * loci
    per_mating = 1 + ATTEMPTS + 4 + 2 * per_child
    return dict(p2=1, x=1 + ATTEMPTS, child=5 + ATTEMPTS, loci=loci, per_child=per_child, per_mating=per_mating,
                len=(np_ // 2) * per_mating)


def close(a, b, gap=MIN_GAP):
    if a == b:
        return True
    if math.isinf(a) or math.isinf(b):
        return False
    return abs(a - b) <= gap * max(abs(a), abs(b))


def rqsort(a):
    """pikaia.cpp:154-250: the permutation p (0-based rows) that sorts a ascending"""
    n = len(a)
    p = list(range(1, n + 1))
    stack = [(1, n)]
    while stack:
        l, r = stack.pop()
        while True:
            if r - l < 11:
                for i in range(l + 1, r + 1):
                    t = p[i - 1]
                    x = a[t - 1]
                    j = i - 1
                    while j >= l and not a[p[j - 1] - 1] <= x:
                        p[j] = p[j - 1]
                        j -= 1
                    p[j] = t
                break
            m = (l + r) // 2
            t = p[m - 1]
            if a[t - 1] < a[p[l - 1] - 1]:
                p[m - 1] = p[l - 1]
                p[l - 1] = t
                t = p[m - 1]
            if a[t - 1] > a[p[r - 1] - 1]:
                p[m - 1] = p[r - 1]
                p[r - 1] = t
                t = p[m - 1]
                if a[t - 1] < a[p[l - 1] - 1]:
                    p[m - 1] = p[l - 1]
                    p[l - 1] = t
                    t = p[m - 1]
            x = a[t - 1]
            i, j = l + 1, r - 1
            while i <= j:
                while a[p[i - 1] - 1] < x:
                    i += 1
                while x < a[p[j - 1] - 1]:
                    j -= 1
                if i <= j:
                    p[i - 1], p[j - 1] = p[j - 1], p[i - 1]
                    i += 1
                    j -= 1
            if j - l > r - i:
                stack.append((l, j))
                l = i
            else:
                stack.append((i, r))
                r = j
    return [v - 1 for v in p]


def stable_order(a):
    return sorted(range(len(a)), key=lambda i: (a[i], i))


class WordsSource:
    """the reference's program order: every draw is the next canonical double"""

    def __init__(self, words):
        self.w = words

    def get(self, at):
        return self.w.canonical()


class TableSource:
    def __init__(self, table):
        self.t = table

    def get(self, at):
        return float(self.t[at])


class Pikaia:
    def __init__(self, f, n, np_, ngen, nd, lower=None, upper=None, repair=False, raw=False, order="rqsort", **kw):
        par = dict(DEFAULTS)
        par.update(kw)
        assert par["irep"] == 1 and np_ % 2 == 0
        self.f, self.n, self.np, self.ngen, self.nd = f, int(n), int(np_), int(ngen), int(nd)
        self.lower = [0.] * n if lower is None else [float(v) for v in lower]
        self.upper = [1.] * n if upper is None else [float(v) for v in upper]
        self.repair, self.raw = bool(repair), bool(raw)
        self.sort = rqsort if order == "rqsort" else stable_order
        self.pcross, self.imut, self.pmut = float(par["pcross"]), int(par["imut"]), float(par["pmut"])
        self.pmutmn, self.pmutmx, self.fdif = float(par["pmutmn"]), float(par["pmutmx"]), float(par["fdif"])
        self.ielite = int(par["ielite"])
        self.z, self.zinv = math.pow(10., self.nd), math.pow(10., -self.nd)
        self.lay = table_layout(self.n, self.np, self.nd)
        self.paths = {k: 0 for k in PATHS}
        self.evals = []         # (x, f(x)) of the last init / generation, in call order
        self.fev = self.ig = 0
        self.rdif = 0.

    # -- the objective ------------------------------------------------------------------------------------
    def map(self, u):
        if self.raw:
            return list(u)
        return [self.lower[i] + u[i] * (self.upper[i] - self.lower[i]) for i in range(self.n)]

    def fitness(self, u):
        x = self.map(u)
        v = float(self.f(x))
        self.evals.append((x, v))
        fit = v if self.raw else -v
        return -math.inf if fit != fit else fit

    # -- init (:34-69) --------------------------------------------------------------------------------------
    def init_words(self, w):
        self.evals = []
        self.ph = []
        self.fitns = [0.] * self.np
        for ip in range(self.np):
            row = [w.canonical() for _ in range(self.n)]
            self.ph.append(row)
            v = self.fitness(row)
            self.fitns[ip if self.repair else self.np - 1] = v
        self.fev = self.np
        self.order = self.sort(self.fitns)
        self.ig = 1

    def start(self, ph, fitns, order, pmut, ig, fev):
        """a state from outside (the fixture's): nothing is evaluated"""
        self.ph = [list(r) for r in ph]
        self.fitns = [float(v) for v in fitns]
        self.order = [int(v) for v in order]
        self.pmut, self.ig, self.fev = float(pmut), int(ig), int(fev)

    def state(self):
        return dict(ph=[list(r) for r in self.ph], fitns=list(self.fitns), order=list(self.order), pmut=self.pmut,
                    ig=self.ig, fev=self.fev)

    def state_crc(self):
        """phenotypes, fitness and pmut: what does not depend on how ties are ranked"""
        return crc([v for r in self.ph for v in r] + self.fitns + [self.pmut])

    # -- the parts of a generation ------------------------------------------------------------------------
    def _select(self, u, jfit):
        np_, np1 = self.np, self.np + 1
        dice = u * np_ * np1
        rtfit = 0.
        for i in range(np_):
            rtfit = rtfit + np1 + self.fdif * (np1 - 2 * jfit[i])
            if rtfit >= dice:
                return i
        return np_ - 1      # (the device's rule; the reference falls through with a stale index)

    def _encode(self, ph):
        gn = []
        for v in ph:
            ip = int(v * self.z)
            d = []
            for _ in range(self.nd):
                d.append(ip % 10)
                ip //= 10
            gn.extend(reversed(d))
        return gn

    def _decode(self, gn):
        ph = []
        for i in range(self.n):
            ip = 0
            for j in range(self.nd):
                ip = 10 * ip + gn[i * self.nd + j]
            ph.append(ip * self.zinv)
        return ph

    def _mutate(self, gn, draw, base):
        n, nd, L, pmut = self.n, self.nd, self.n * self.nd, self.pmut
        creep = False
        if self.imut >= 4:
            creep = draw(base) <= 0.5
        self.paths["creep" if creep else "uniform"] += 1
        if not creep:
            for i in range(L):
                if draw(base + 1 + i) < pmut:
                    gn[i] = int(draw(base + 1 + L + i) * 10.)
            return 0
        for i in range(n):
            ist = i * nd
            for j in range(nd):
                loc = ist + j
                if not draw(base + 1 + loc) < pmut:
                    continue
                inc = (1 if draw(base + 1 + L + loc) >= 0.5 else 0) * 2 - 1     # std::round, half away from zero
                gn[loc] += inc
                if inc < 0 and gn[loc] < 0:
                    if j == 0:
                        gn[loc] = 0
                        self.paths["clamp_0"] += 1
                    else:
                        self.paths["carry_down"] += 1
                        for k in range(loc, ist, -1):
                            gn[k] = 9
                            gn[k - 1] -= 1
                            if gn[k - 1] >= 0:
                                break
                        else:
                            if gn[ist] < 0:
                                for l in range(ist, loc + 1):
                                    gn[l] = 0
                                self.paths["clamp_0"] += 1
                if inc > 0 and gn[loc] > 9:
                    if j == 0:
                        gn[loc] = 9
                        self.paths["clamp_9"] += 1
                    else:
                        self.paths["carry_up"] += 1
                        for k in range(loc, ist, -1):
                            gn[k] = 0
                            gn[k - 1] += 1
                            if gn[k - 1] <= 9:
                                break
                        else:
                            if gn[ist] > 9:
                                for l in range(ist, loc + 1):
                                    gn[l] = 9
                                self.paths["clamp_9"] += 1
        return 1

    # -- a generation (:71-123) ---------------------------------------------------------------------------
    def iterate(self, src):
        n, nd, np_, lay = self.n, self.nd, self.np, self.lay
        L = n * nd
        self.table = [-1.] * lay["len"]
        self.evals = []
        jfit = [0] * np_
        for k, row in enumerate(self.order):
            jfit[row] = np_ - k
        self.parents, self.cross, self.mode, newph = [], [], [], []
        for m in range(np_ // 2):
            tb = m * lay["per_mating"]

            def draw(off):
                u = src.get(tb + off)
                self.table[tb + off] = u
                return u

            ip1 = self._select(draw(0), jfit)
            ip2 = ip1
            for a in range(ATTEMPTS):
                u = draw(lay["p2"] + a)
                if u < 0.:
                    break
                ip2 = self._select(u, jfit)
                if ip2 != ip1:
                    break
            if ip2 == ip1:
                ip2 = (ip1 + 1) % np_
            gn1, gn2 = self._encode(self.ph[ip1]), self._encode(self.ph[ip2])
            ispl = ispl2 = -1
            if draw(lay["x"]) < self.pcross:
                ispl = int(draw(lay["x"] + 1) * n * nd) + 1
                if draw(lay["x"] + 2) < 0.5:
                    ispl2 = L
                    self.paths["one_point"] += 1
                else:
                    ispl2 = int(draw(lay["x"] + 3) * n * nd) + 1
                    if ispl2 < ispl:
                        ispl, ispl2 = ispl2, ispl
                    self.paths["two_point"] += 1
                for i in range(ispl, ispl2 + 1):
                    gn1[i - 1], gn2[i - 1] = gn2[i - 1], gn1[i - 1]
            else:
                self.paths["no_cross"] += 1
            c1 = self._mutate(gn1, draw, lay["child"])
            c2 = self._mutate(gn2, draw, lay["child"] + lay["per_child"])
            self.parents.append((ip1, ip2))
            self.cross.append((ispl, ispl2))
            self.mode += [c1, c2]
            newph.append(self._decode(gn1))
            newph.append(self._decode(gn2))

        # newpop (:567-592)
        best = self.order[np_ - 1]
        self.elite, self.elite_close = 0, False
        if self.repair:
            fit = [self.fitness(r) for r in newph]
            if self.ielite == 1:
                self.elite_close = close(fit[0], self.fitns[best])
                if fit[0] < self.fitns[best]:
                    newph[0] = list(self.ph[best])
                    fit[0] = self.fitns[best]
                    self.elite = 1
            self.fev += np_
        else:
            if self.ielite == 1:
                f0 = self.fitness(newph[0])
                self.elite_close = close(f0, self.fitns[best])
                if f0 < self.fitns[best]:
                    newph[0] = list(self.ph[best])
                    self.elite = 1
            self.fev += 1
            fit = [self.fitness(r) for r in newph]
            self.fev += np_
        self.paths["elite_taken"] += self.elite
        self.ph, self.fitns = newph, fit
        self.order = self.sort(fit)
        # two rows that differ with values this close may rank the other way round on the device
        srt = stable_order(fit)
        self.close_distinct = any(close(fit[a], fit[b]) and self.ph[a] != self.ph[b] for a, b in zip(srt, srt[1:]))

        # adjmut (:408-434)
        self.rdif, self.rdif_close = 0., False
        if self.imut in (2, 3, 5, 6):
            ib, im = self.order[np_ - 1], self.order[np_ // 2 - 1]
            if self.imut in (2, 5):
                den = fit[ib] + fit[im]
                if self.repair:
                    den = abs(den)
                num = abs(fit[ib] - fit[im])
                rdif = num / den if den != 0. else (math.nan if num == 0. else math.copysign(math.inf, den) * num)
            else:
                rdif = 0.
                for i in range(n):
                    rdif += math.pow(self.ph[ib][i] - self.ph[im][i], 2.)
                rdif = math.sqrt(rdif) / n
            self.rdif = rdif
            self.rdif_close = abs(rdif - 0.05) <= RDIF_GAP or abs(rdif - 0.25) <= RDIF_GAP
            if rdif <= 0.05:
                new = min(self.pmutmx, self.pmut * 1.5)
                self.paths["pmut_raised" if new != self.pmut else "pmut_held"] += 1
                self.pmut = new
            elif rdif >= 0.25:
                new = max(self.pmutmn, self.pmut / 1.5)
                self.paths["pmut_lowered" if new != self.pmut else "pmut_held"] += 1
                self.pmut = new
            else:
                self.paths["pmut_held"] += 1
        self.ig += 1

    def ok(self):
        """the last generation is one the device can be held to"""
        return not (self.close_distinct or self.elite_close or self.rdif_close)

    def best(self):
        """the mapped best row and its objective value"""
        ib = self.order[self.np - 1]
        return self.map(self.ph[ib]), (self.fitns[ib] if self.raw else -self.fitns[ib])
