"""Scalar model of CRS (crs.cpp:46-181): the recursion of trial() as a state machine over a stack of bits.

The frames of trial() hold no locals, so a frame is one bit: B (the call at :133, returns to :135) or M (the
call at :151, returns to :155).  Every operation is one IEEE operation on Python floats per operation of
the reference, in its order; the objective comes in two forms:

reference form   the objective summed serially (chol_model.objective): given the reference's draws
                 (WordsSource over the recorded mt19937 words) the model reproduces every recorded
                 evaluated point, pool row, value, fev and _trial bit for bit (tests/test_crs_model.py).
device form      the objective summed as the device sums it (slpso_model.device_objective): every state
                 key of the device, bit for bit (tests/test_crs_gpu.py).

The pool is kept sorted by a stable rule: the initial sort is stable and a new point goes behind all equal
values.  A NaN value counts as +inf.  `max_depth` bounds the stack (flag 3: the iteration is abandoned,
the pool untouched, fev keeps what was spent); `repair=True` is the loop of the paper: an out-of-box
reflection and a rejected pair are redrawn, only an accepted point replaces the worst, the budget is also
tested where a pair is rejected, and max_depth bounds the out-of-box redraws in a row.

Draws travel in records of 2 n numbers, the layout of bbo_crs_inject_draws: the n row indices of a trial
(-1 where none is drawn) and the n uniforms of a mutation (0.5 where none is drawn).  A trial takes a new
record; a mutation takes the uniforms of the current record, or of a new one when they are spent."""
INF = float("inf")
B, M = 0, 1


class WordsSource:
    """the reference's program order over the words an iteration consumed (a jaya_model.Words)"""

    def __init__(self, w, n, np_):
        self.w, self.n, self.np = w, n, np_

    def indices(self):
        return [self.w.uint(0, self.np - 1) for _ in range(self.n)]        # :119, :126

    def uniforms(self):
        return [self.w.uniform(0.0, 1.0) for _ in range(self.n)]           # :143


class TableSource:
    """records in the layout of bbo_crs_inject_draws, consumed by the device's rule"""

    def __init__(self, records, n, np_):
        self.r, self.n, self.np = [[float(v) for v in rec] for rec in records], n, np_
        self.i, self.wused = 0, True

    def indices(self):
        self.i += 1
        self.wused = False
        return [min(max(int(v), 0), self.np - 1) for v in self.r[self.i - 1][:self.n]]

    def uniforms(self):
        if self.wused:
            self.i += 1
        self.wused = True
        return list(self.r[self.i - 1][self.n:])

    def exhausted(self):
        return self.i == len(self.r)


class RngSource:
    def __init__(self, rng, n, np_):
        self.rng, self.n, self.np = rng, n, np_

    def indices(self):
        return [int(v) for v in self.rng.integers(0, self.np, self.n)]

    def uniforms(self):
        return [float(v) for v in self.rng.random(self.n)]


class Crs:
    def __init__(self, f, n, np_, lower, upper, mfev, tol, max_depth=4096, repair=False):
        self.f, self.n, self.np = f, n, np_
        self.lower, self.upper = [float(v) for v in lower], [float(v) for v in upper]
        self.mfev, self.tol, self.max_depth, self.repair = mfev, tol, max_depth, repair

    def value(self, x):
        v = float(self.f(x))
        return INF if v != v else v

    def start(self, X, fs=None):
        """init() from given points, :61-78: rows in place, a stable ranking"""
        self.rows = [[float(v) for v in r] for r in X]
        self.fs = [self.value(r) for r in self.rows] if fs is None else [INF if v != v else float(v) for v in fs]
        self.order = sorted(range(self.np), key=lambda i: self.fs[i])       # (sorted is stable)
        self.t, self.t2 = [0.] * self.n, [0.] * self.n
        self.ft = self.ft2 = 0.
        self.fev, self.it, self.trials, self.muts, self.stale = self.np, 0, 0, 0, 0
        self.depth = self.maxdepth = 0
        self.flag = 0
        # (out_lo, out_up: coordinates of rejected trial points under their lower / over their upper bound)
        self.paths = dict(B=0, mut_acc=0, M=0, M_stale=0, M_inner_mut=0, popB_fail=0, out_lo=0, out_up=0)

    # the pool in rank order, as the reference keeps it
    def x(self):
        return [list(self.rows[r]) for r in self.order]

    def fsorted(self):
        return [self.fs[r] for r in self.order]

    def converged(self):
        return abs(self.fs[self.order[0]] - self.fs[self.order[-1]]) < self.tol    # :168-172

    def in_bounds(self, p):
        return not any(p[d] < self.lower[d] or p[d] > self.upper[d] for d in range(self.n))

    def _eval(self, x):
        v = self.value(x)
        self.fev += 1
        self.evals.append((list(x), v))
        return v

    def _record_trial(self, idx):
        self.records.append([float(i) for i in idx] + [0.5] * self.n)
        self.wused = False

    def _record_mutation(self, w):
        if self.wused:
            self.records.append([-1.] * self.n + [0.5] * self.n)
        self.records[-1][self.n:] = list(w)
        self.wused = True

    def iterate(self, src):
        """one iterate() (:81-84); False when it was abandoned (flag 2 in repair, flag 3)"""
        n, best = self.n, self.rows[self.order[0]]
        fworst = self.fs[self.order[-1]]
        self.evals, self.records, self.wused = [], [], True
        stack, self.maxdepth = [], 0
        redraws = 0                             # repair: out-of-box redraws in a row
        how = None                              # how the point at RET came about
        state = "CALL"
        while True:
            if state == "CALL":                 # :114-134 (an index names a place in the SORTED pool)
                idx = src.indices()
                self._record_trial(idx)
                self.trials += 1
                c = [0.0] * n
                for d in range(n):
                    c[d] += best[d] / n
                for j in range(n - 1):
                    row = self.rows[self.order[idx[j]]]
                    for d in range(n):
                        c[d] += row[d] / n
                row = self.rows[self.order[idx[n - 1]]]
                self.t = [2 * c[d] - row[d] for d in range(n)]
                if not self.in_bounds(self.t):
                    self.paths["out_lo"] += sum(self.t[d] < self.lower[d] for d in range(n))
                    self.paths["out_up"] += sum(self.t[d] > self.upper[d] for d in range(n))
                    if self.repair:
                        if redraws >= self.max_depth:
                            return self._abandon(3)
                        redraws += 1
                        self.maxdepth = max(self.maxdepth, redraws)
                        continue
                    if len(stack) >= self.max_depth:
                        return self._abandon(3)
                    stack.append(B)
                    self.paths["B"] += 1
                    self.maxdepth = max(self.maxdepth, len(stack))
                    continue
                redraws = 0
                state = "L1"
            if state == "L1":                   # :135-157
                self.ft = self._eval(self.t)
                if how == "stale" and self.ft >= fworst:
                    self.paths["popB_fail"] += 1
                if self.ft >= fworst:
                    w = src.uniforms()
                    self._record_mutation(w)
                    self.muts += 1
                    self.t2 = [(1.0 + w[d]) * best[d] - w[d] * self.t[d] for d in range(n)]
                    self.ft2 = self._eval(self.t2)
                    if self.ft2 >= fworst:
                        if self.repair:
                            if self.fev >= self.mfev:
                                return self._abandon(2)
                            state = "CALL"
                            continue
                        if len(stack) >= self.max_depth:
                            return self._abandon(3)
                        stack.append(M)
                        self.paths["M"] += 1
                        self.maxdepth = max(self.maxdepth, len(stack))
                        how = None
                        state = "CALL"
                        continue
                    self.ft, self.t = self.ft2, list(self.t2)
                    self.paths["mut_acc"] += 1
                    how = "mutate"
                else:
                    how = "reflect"
                state = "RET"
            if state == "RET":
                again = False
                while stack:
                    if stack.pop() == B:
                        state, again = "L1", True
                        break
                    if how == "reflect":
                        self.paths["M_stale"] += 1
                        how = "stale"
                    elif how == "mutate":
                        self.paths["M_inner_mut"] += 1
                    self.ft, self.t = self.ft2, list(self.t2)      # :155-156: the mutation computed LAST
                if again:
                    continue
                break
        # update(), :160-166
        if self.ft >= fworst:
            self.stale += 1
        row = self.order.pop()
        self.rows[row], self.fs[row] = list(self.t), self.ft
        slot = 0
        while slot < len(self.order) and self.fs[self.order[slot]] <= self.ft:
            slot += 1
        self.order.insert(slot, row)
        self.changed_row, self.slot = row, slot
        self.it += 1
        self.depth = 0
        if not self.flag:
            if self.converged():
                self.flag = 1
            elif self.fev >= self.mfev:
                self.flag = 2
        return True

    def _abandon(self, flag):
        self.flag = flag
        self.depth = 0
        return False
