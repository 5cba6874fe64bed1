"""Pure-Python restatement of the reference's MayflySearch (src/multivariate/mayfly/mayfly.cpp), written from
its description: the same IEEE operations in the same order; only libm's exp may differ from the device's.

Draws come from a source.  `WordsSource` decodes the raw 32-bit words of the reference's global mt19937 in the
reference's program order (jaya_model.Words: Random::get on doubles, std::shuffle, std::normal_distribution
with its cached second value, which lives in the optimizer and so persists from generation to generation, as
does the `_indices` array that every mutation shuffles again).  `TableSource` reads the table of
bbo_mayfly_inject_draws.  Either way the model logs the table of the generation (`table`), so a recorded
generation of the reference can be handed to the device.

The swarms are lists of flies in SLOT order: the reference sorts vectors of pointers, and what the next
generation reads is the order the selection wrote.  The selection is walked literally (records that alias
the swarm's own flies are copied slot after slot, in the order of libstdc++'s std::sort: `std_sort`) and
resolved as the device resolves it (`src`: the record that lands in each slot, a chain over integers, in the
stable order); `chain_ok` says that the two agree, which they must wherever the two orders do.  repair=True
selects from untouched copies and starts every fly at the point it drew."""
import math
import struct
import zlib

import numpy as np

INF = float("inf")
DEFAULTS = dict(a1=1., a2=1.5, a3=1.5, beta=2., dance=5., ddamp=0.8, fl=1., fldamp=0.99, gmin=0.8, gmax=0.8,
                vdamp=0.1, sigma=0.1, pmutdim=0.01, pmutnp=0.05, l=0.95, pgb=False)
MIN_GAP = 1e-6


STATE_KEYS = ("males_x", "males_v", "males_bx", "males_f", "males_bf", "females_x", "females_v", "females_f",
              "xbest", "fbest", "g", "dance", "fl")


def crc(values):
    """CRC-32 of the doubles as they lie in memory (little-endian): how the fixture pins every bit of a
    generation's points and of the state after it"""
    flat = [float(v) for v in values]
    return zlib.crc32(struct.pack("<%dd" % len(flat), *flat))


def state_crc(state):
    flat = []
    for k in STATE_KEYS:
        for r in state[k]:
            flat.extend(r if isinstance(r, (list, tuple)) else [r])
    return crc(flat)


def mt19937_words(seed, count):
    """the first `count` outputs of std::mt19937 seeded with the integer `seed`"""
    st = np.random.RandomState(int(seed)).get_state()
    bg = np.random.MT19937()
    bg.state = {"bit_generator": "MT19937", "state": {"key": st[1], "pos": st[2]}}
    return [int(v) for v in bg.random_raw(int(count))]


def table_layout(n, np_, nmut, nmd):
    uf, um = 0, np_ * n
    po = 2 * np_ * n
    pu = po + np_
    ix = pu + nmut
    z = ix + nmut * nmd
    return dict(uf=uf, um=um, po=po, pu=pu, ix=ix, z=z, len=z + nmut * nmd)


def std_sort(keys):
    """the order libstdc++'s std::sort leaves `keys` in (the introsort of bits/stl_algo.h: median-of-three
    partitions while a range holds more than 16, then one insertion sort), as a list of indices.  Up to 16
    keys it is a plain insertion sort and stable; beyond, equal keys may change places, and where the
    records behind them differ the reference's trajectory depends on it"""
    v = list(range(len(keys)))
    less = lambda a, b: keys[a] < keys[b]

    def swap(i, j):
        v[i], v[j] = v[j], v[i]

    def linear_insert(last):
        val, nxt = v[last], last - 1
        while less(val, v[nxt]):
            v[last] = v[nxt]
            last, nxt = nxt, nxt - 1
        v[last] = val

    def insertion(first, last):
        for i in range(first + 1, last):
            if less(v[i], v[first]):
                val = v[i]
                v[first + 1:i + 1] = v[first:i]
                v[first] = val
            else:
                linear_insert(i)

    def adjust_heap(first, hole, length, val):
        top, child = hole, hole
        while child < (length - 1) // 2:
            child = 2 * (child + 1)
            if less(v[first + child], v[first + child - 1]):
                child -= 1
            v[first + hole] = v[first + child]
            hole = child
        if length % 2 == 0 and child == (length - 2) // 2:
            child = 2 * (child + 1)
            v[first + hole] = v[first + child - 1]
            hole = child - 1
        parent = (hole - 1) // 2
        while hole > top and less(v[first + parent], val):
            v[first + hole] = v[first + parent]
            hole = parent
            parent = (hole - 1) // 2
        v[first + hole] = val

    def heap_sort(first, last):
        length = last - first
        parent = (length - 2) // 2
        while True:
            adjust_heap(first, parent, length, v[first + parent])
            if parent == 0:
                break
            parent -= 1
        while last - first > 1:
            last -= 1
            val = v[last]
            v[last] = v[first]
            adjust_heap(first, 0, last - first, val)

    def loop(first, last, depth):
        while last - first > 16:
            if depth == 0:
                heap_sort(first, last)
                return
            depth -= 1
            mid = first + (last - first) // 2
            a, b, c = first + 1, mid, last - 1
            if less(v[a], v[b]):
                swap(first, b if less(v[b], v[c]) else c if less(v[a], v[c]) else a)
            else:
                swap(first, a if less(v[a], v[c]) else c if less(v[b], v[c]) else b)
            lo, hi = first + 1, last
            while True:
                while less(v[lo], v[first]):
                    lo += 1
                hi -= 1
                while less(v[first], v[hi]):
                    hi -= 1
                if not lo < hi:
                    break
                swap(lo, hi)
                lo += 1
            loop(lo, last, depth)
            last = lo

    n = len(v)
    if n > 1:
        loop(0, n, 2 * (n.bit_length() - 1))
        if n > 16:
            insertion(0, 16)
            for i in range(16, n):
                linear_insert(i)
        else:
            insertion(0, n)
    return v


class Fly:
    __slots__ = ("x", "v", "bx", "f", "bf", "taint")

    def __init__(self, x, v, bx, f, bf, taint=False):
        self.x, self.v, self.bx, self.f, self.bf, self.taint = list(x), list(v), list(bx), f, bf, taint

    def take(self, o, male):
        self.x, self.v, self.f, self.taint = list(o.x), list(o.v), o.f, o.taint
        if male:
            self.bx, self.bf = list(o.bx), o.bf

    def fields(self, male):
        return (self.x, self.v, self.bx, self.f, self.bf) if male else (self.x, self.v, self.f)


class WordsSource:
    """the reference's draws from raw mt19937 words (a jaya_model.Words over the whole run)"""

    def __init__(self, words, n):
        self.w = words
        self.indices = list(range(n))

    def flight(self, blk, j, i):
        return self.w.canonical()

    def shuffle(self, which, count):
        v = list(range(count))
        self.w.shuffle(v)
        return v

    def genes(self, u, nmd):
        self.w.shuffle(self.indices)
        return list(self.indices[:nmd])

    def normal(self, u, q):
        return self.w.normal()


class TableSource:
    """the draws of a table in the layout of bbo_mayfly_inject_draws"""

    def __init__(self, table, n, np_, nmut, nmd):
        self.t, self.n, self.nmd = [float(v) for v in table], n, nmd
        self.o = table_layout(n, np_, nmut, nmd)
        assert len(self.t) == self.o["len"]

    def flight(self, blk, j, i):
        u = self.t[(self.o["um"] if blk else self.o["uf"]) + j * self.n + i]
        assert 0. <= u < 1.
        return u

    def shuffle(self, which, count):
        at = self.o["po"] if which == 0 else self.o["pu"]
        return [int(v) for v in self.t[at:at + count]]

    def genes(self, u, nmd):
        at = self.o["ix"] + u * nmd
        return [int(v) for v in self.t[at:at + nmd]]

    def normal(self, u, q):
        return self.t[self.o["z"] + u * self.nmd + q]


class Mayfly:
    def __init__(self, f, n, np_, lower, upper, mfev, repair=False, **kw):
        par = dict(DEFAULTS)
        par.update(kw)
        self.fun, self.n, self.np, self.mfev, self.repair = f, int(n), int(np_), int(mfev), bool(repair)
        self.lower, self.upper = [float(v) for v in lower], [float(v) for v in upper]
        for k, v in par.items():
            setattr(self, k, v)
        assert self.np >= 2 and self.np % 2 == 0 and self.mfev > 2 * self.np
        self.nmut = int(self.pmutnp * self.np)                      # :135-139
        if self.nmut % 2:
            self.nmut = min(self.nmut + 1, self.np)
        self.nmd = int(math.ceil(self.pmutdim * self.n))            # :403
        self.cm = self.np + self.np // 2 + self.nmut // 2
        self.layout = table_layout(self.n, self.np, self.nmut, self.nmd)
        self.paths = dict(f_attract=0, f_random=0, m_attract=0, m_dance=0, improve_not_last=0, short_window=0,
                          aliased=0, clamp_box=0, clamp_vmax=0)
        self.close_distinct = self.unstable = 0
        self.stable_sort = False        # True: the device's order in every sort
        self.window = 4

    def _eval(self, x):
        v = float(self.fun(x))
        if v != v:
            v = INF
        self.evals.append((list(x), v))
        self.fev += 1
        return v

    # ---- init (:63-163) --------------------------------------------------------------------------------
    def init_words(self, w):
        """the reference's init(): male j, then female j, drawn and evaluated.  The reference builds its flies
        as mayfly { v, x, bx, f, f } over a struct declared _x, _v, _bx (:93, :112): the drawn point becomes
        the VELOCITY and the zero vector the position, so every fly starts at the origin with the value of
        the point it drew.  repair=True starts at the drawn point with no velocity, as the paper does"""
        n = self.n
        self.evals, self.fev = [], 0
        self.fbest, self.best = INF, [0.] * n
        self.males, self.females = [], []
        for j in range(self.np):
            x = [w.uniform(self.lower[i], self.upper[i]) for i in range(n)]
            f = self._eval(x)
            self.males.append(Fly(x, [0.] * n, x, f, f) if self.repair else Fly([0.] * n, x, x, f, f))
            if f < self.fbest:
                self.fbest, self.best = f, list(x)
            x = [w.uniform(self.lower[i], self.upper[i]) for i in range(n)]
            f = self._eval(x)
            self.females.append(Fly(x, [0.] * n, [0.] * n, f, f) if self.repair
                                else Fly([0.] * n, x, [0.] * n, f, f))
            if self.pgb and f < self.fbest:
                self.fbest, self.best = f, list(x)
        self._schedule0()

    def start(self, state):
        """a whole state, as get_state returns it key by key (or as a recorded one)"""
        n, np_ = self.n, self.np
        rows = lambda k: [[float(v) for v in r] for r in np.asarray(state[k], float).reshape(np_, n)]
        vals = lambda k: [float(v) for v in np.asarray(state[k], float).ravel()]
        mx, mv, mbx, fx, fv = rows("males_x"), rows("males_v"), rows("males_bx"), rows("females_x"), rows("females_v")
        mf, mbf, ff = vals("males_f"), vals("males_bf"), vals("females_f")
        self.males = [Fly(mx[j], mv[j], mbx[j], mf[j], mbf[j]) for j in range(np_)]
        self.females = [Fly(fx[j], fv[j], [0.] * n, ff[j], ff[j]) for j in range(np_)]
        self.best, self.fbest = vals("xbest"), float(np.asarray(state["fbest"]).ravel()[0])
        self.evals = []
        self._schedule0()
        one = lambda k: float(np.asarray(state[k]).ravel()[0])
        self.fev, self.it, self.itmax = int(one("fev")), int(one("it")), int(one("itmax"))
        self.g, self.dance_now, self.fl_now = one("g"), one("dance"), one("fl")

    def _schedule0(self):
        self.fev = 2 * self.np
        self.it = 0
        self.itmax = int(math.ceil((self.mfev - self.fev) / (3. * self.np + self.nmut)))     # :159
        self.g, self.dance_now, self.fl_now = self.gmax, self.dance, self.fl

    def state(self):
        m, f = self.males, self.females
        return dict(males_x=[list(y.x) for y in m], males_v=[list(y.v) for y in m], males_bx=[list(y.bx) for y in m],
                    males_f=[y.f for y in m], males_bf=[y.bf for y in m], females_x=[list(y.x) for y in f],
                    females_v=[list(y.v) for y in f], females_f=[y.f for y in f], xbest=list(self.best),
                    fbest=[self.fbest], g=[self.g], dance=[self.dance_now], fl=[self.fl_now], it=[self.it],
                    itmax=[self.itmax], fev=[self.fev])

    # ---- the moves ---------------------------------------------------------------------------------------
    def _move(self, fly, v):
        """the velocity clamp of :319-320 and updatePosition (:356-367)"""
        for i in range(self.n):
            vmax = self.vdamp * (self.upper[i] - self.lower[i])
            c = max(-vmax, min(v[i], vmax))
            if c != v[i]:
                self.paths["clamp_vmax"] += 1
            fly.v[i] = c
            x = fly.x[i] + c
            cx = max(self.lower[i], min(x, self.upper[i]))
            if cx != x:
                self.paths["clamp_box"] += 1
            fly.x[i] = cx
        fly.f = self._eval(fly.x)

    def _female(self, j, src):
        fe, ma, n = self.females[j], self.males[j], self.n
        r = 0.
        for i in range(n):
            r += (fe.x[i] - ma.x[i]) * (fe.x[i] - ma.x[i])
        attract = ma.f < fe.f
        self.branch_f.append(int(attract))
        at = self.layout["uf"] + j * n
        if attract:
            e = self.a3 * math.exp(-self.beta * r)
            v = [self.g * fe.v[i] + e * (ma.x[i] - fe.x[i]) for i in range(n)]
            fe.taint = True
            self.paths["f_attract"] += 1
        else:
            u = [src.flight(0, j, i) for i in range(n)]
            self.table[at:at + n] = u
            v = [self.g * fe.v[i] + self.fl_now * (u[i] * 2. + -1.) for i in range(n)]
            self.paths["f_random"] += 1
        self._move(fe, v)

    def _male(self, j, src):
        ma, n = self.males[j], self.n
        rp = rg = 0.
        for i in range(n):
            rp += (ma.bx[i] - ma.x[i]) * (ma.bx[i] - ma.x[i])
            rg += (self.best[i] - ma.x[i]) * (self.best[i] - ma.x[i])
        attract = ma.f > self.fbest
        self.branch_m.append(int(attract))
        at = self.layout["um"] + j * n
        if attract:
            e1, e2 = self.a1 * math.exp(-self.beta * rp), self.a2 * math.exp(-self.beta * rg)
            v = [self.g * ma.v[i] + e1 * (ma.bx[i] - ma.x[i]) + e2 * (self.best[i] - ma.x[i]) for i in range(n)]
            ma.taint = True
            self.paths["m_attract"] += 1
        else:
            u = [src.flight(1, j, i) for i in range(n)]
            self.table[at:at + n] = u
            v = [self.g * ma.v[i] + self.dance_now * (u[i] * 2. + -1.) for i in range(n)]
            self.paths["m_dance"] += 1
        self._move(ma, v)
        if ma.f < ma.bf:
            ma.bf, ma.bx = ma.f, list(ma.x)

    def _take(self, fly, ordinal, x=None):
        if fly.f < self.fbest:
            self.fbest, self.best, self.took = fly.f, list(fly.x if x is None else x), ordinal
            self.best_taint = fly.taint
            return True
        return False

    def _sorted(self, flies, male, selection=False):
        """(the reference's order, the stable order).  The reference's is std::sort's, which beyond 16 records
        is not stable; the device's is the stable one.  A generation can be held against the device only
        where the two orders put records that are equal in every field the selection copies at the same
        ranks (`unstable` counts the sorts where they do not) and where no two records whose positions
        differ are closer than MIN_GAP (`close_distinct`: another summation order could swap them)"""
        keys = [y.f for y in flies]
        stable = sorted(range(len(flies)), key=lambda t: keys[t])
        ref = stable if self.stable_sort else std_sort(keys)
        # (in a selection a record that is the swarm's own fly reads what landed in its slot: there the
        # ranks that are copied must name the very same records)
        if ref[:self.np] != stable[:self.np] if selection else \
                any(flies[a].fields(male) != flies[b].fields(male) for a, b in zip(ref, stable)):
            self.unstable += 1
        for a, b in zip(stable, stable[1:]):
            fa, fb = keys[a], keys[b]
            close = fa == fb or abs(fa - fb) <= MIN_GAP * max(abs(fa), abs(fb))
            if close and flies[a].x != flies[b].x:
                self.close_distinct += 1
        return ref, stable

    def _select(self, swarm, extra, male):
        """:241-275 for one swarm; returns (T, src) in the stable order"""
        np_ = self.np
        records = list(swarm) + extra
        T, Ts = self._sorted(records, male, True)
        src = []
        for j in range(np_):
            t = Ts[j]
            assert not (t < np_ and t > j)
            src.append(src[t] if (t < j and not self.repair) else t)
            if t < j and not self.repair:
                self.paths["aliased"] += 1
        snapshot = [Fly(y.x, y.v, y.bx, y.f, y.bf, y.taint) for y in records]
        if self.repair:
            for j in range(np_):
                swarm[j].take(snapshot[T[j]], male)
        else:
            for j in range(np_):                # the reference's loop: records[T[j]] may be a slot already written
                swarm[j].take(records[T[j]], male)
        self.chain_ok = self.chain_ok and all(swarm[j].fields(male) == snapshot[src[j]].fields(male)
                                              for j in range(np_))
        return Ts, src

    # ---- iterate() (:165-282) ------------------------------------------------------------------------------
    def iterate(self, src):
        n, np_, nmut, nmd = self.n, self.np, self.nmut, self.nmd
        lay = self.layout
        self.table = [-1.] * lay["len"]
        self.evals, self.took = [], -1
        self.branch_f, self.branch_m = [], []
        self.chain_ok = True        # the chain landed what the reference's loop landed (every generation
        # whose sorts are stable: `unstable` and `close_distinct` did not move)
        for y in self.males + self.females:
            y.taint = False
        self.best_taint = False
        for j in range(np_):
            self._female(j, src)
            if self.pgb:
                self._take(self.females[j], j)
        improved = []
        for j in range(np_):
            self._male(j, src)
            ma = self.males[j]
            if ma.bf < self.fbest:
                self.fbest, self.best, self.took, self.best_taint = ma.bf, list(ma.bx), np_ + j, ma.taint
                improved.append(j)
        self.improved = improved
        self.paths["improve_not_last"] += sum(1 for j in improved if j != np_ - 1)
        j0 = 0
        while j0 < np_:                         # the prefix-commit rounds of the device at the default window
            cnt = min(self.window, np_ - j0)
            hit = [j for j in improved if j0 <= j < j0 + cnt]
            commit = hit[0] - j0 + 1 if hit else cnt
            self.paths["short_window"] += commit < cnt
            j0 += commit
        self.moved_males = [Fly(y.x, y.v, y.bx, y.f, y.bf, y.taint) for y in self.males]
        self.moved_females = [Fly(y.x, y.v, y.bx, y.f, y.bf, y.taint) for y in self.females]
        rm, self.rank_m = self._sorted(self.males, True)
        rf, self.rank_f = self._sorted(self.females, False)
        ms, fs = [self.males[t] for t in rm], [self.females[t] for t in rf]
        off = []
        zero = [0.] * n
        for j in range(np_ // 2):
            p1, p2 = ms[j], fs[j]
            x1, x2 = [], []
            for i in range(n):
                a = self.l * p1.x[i] + (1. - self.l) * p2.x[i]
                x1.append(max(self.lower[i], min(a, self.upper[i])))
                b = self.l * p2.x[i] + (1. - self.l) * p1.x[i]
                x2.append(max(self.lower[i], min(b, self.upper[i])))
            for x in (x1, x2):
                f = self._eval(x)
                off.append(Fly(x, zero, x, f, f, p1.taint or p2.taint))
            for k in (2 * j, 2 * j + 1):
                self._take(off[k], 2 * np_ + k)
        self.offspring = off
        self.perm_o = src.shuffle(0, np_)
        self.table[lay["po"]:lay["po"] + np_] = [float(v) for v in self.perm_o]
        shuffled = [off[k] for k in self.perm_o]
        mutated = []
        self.perm_u = []
        if nmut > 0:
            for u in range(nmut):
                par = shuffled[u]
                genes = src.genes(u, nmd)
                x = list(par.x)
                for q, k in enumerate(genes):
                    z = src.normal(u, q)
                    self.table[lay["ix"] + u * nmd + q] = float(k)
                    self.table[lay["z"] + u * nmd + q] = z
                    sg = self.sigma * (self.upper[k] - self.lower[k])
                    x[k] = max(self.lower[k], min(par.x[k] + sg * z, self.upper[k]))
                f = self._eval(x)
                mutated.append(Fly(x, zero, x, f, f, par.taint))
                self._take(mutated[u], 3 * np_ + u)
            self.perm_u = src.shuffle(1, nmut)
            self.table[lay["pu"]:lay["pu"] + nmut] = [float(v) for v in self.perm_u]
        self.mutated = mutated
        mshuf = [mutated[u] for u in self.perm_u]
        h, hm = np_ // 2, nmut // 2
        self.sel_m, self.src_m = self._select(ms, shuffled[:h] + mshuf[:hm], True)
        self.sel_f, self.src_f = self._select(fs, shuffled[h:] + mshuf[hm:], False)
        self.males, self.females = ms, fs
        self.it += 1
        self.g = self.gmax - ((self.gmax - self.gmin) / self.itmax) * self.it
        self.dance_now *= self.ddamp
        self.fl_now *= self.fldamp

    def duplicates(self, male=True):
        """slots whose content another, earlier slot holds too"""
        seen, dup = [], 0
        for y in (self.males if male else self.females):
            k = y.fields(male)
            if k in seen:
                dup += 1
            else:
                seen.append(k)
        return dup
