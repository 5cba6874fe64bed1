"""Shared by tests/test_oracle_substreams.py (CPU) and tests/test_batch_oracle_gpu.py (GPU): the
cases of a batched swarm handle held against one oracle object per population, how those objects
are made, and the per-engine comparators.

Population p of a device handle draws from Philox sub-stream p; oracle object p is the same
optimizer with `set_sub(p)`.  Every comparator below applies the keys and tolerances of the
engine's single-population parity test to ONE population; the line it was taken from is cited
next to each number, and none is wider here."""
import numpy as np

import pyoracle as po

BOX = 5.


def case(engine, n, size, obj, kw=None, P=5, gens=10, seed=0, chunk=None, note=""):
    return dict(engine=engine, n=n, size=size, obj=obj, kw=dict(kw or {}), P=P, gens=gens, seed=seed,
                chunk=chunk, note=note,
                id="%s-n%d-np%d-%s" % (engine, n, size, obj))


# The smallest shapes that reach each seam between populations.  P = 5 is odd: population 4 sits
# alone in the second workgroup of the four-per-workgroup ranker.  `seed`: the one of the engine's
# single-population test unless the oracle-only conditions of test_oracle_substreams.py
# (test_the_probes_are_different_runs) asked for another; `chunk` (APSO): what the device reports
# for that swarm size (asserted on the device), given to the oracle as in test_pso_gpu.py:45-47.
CASES = [
    case("shade", 8, 64, "sphere", dict(mfev=2500, npmin=8), gens=25, seed=99,
         note="LPSR shrinks np while larch differs per population; archive trim"),
    case("shade", 33, 50, "rosenbrock", seed=99, note="odd n, ragged np, count-rank route"),
    case("shade", 12, 20, "ackley", dict(archive=False, repaircr=False, h=3), seed=99,
         note="a memory of 3 slots wraps, per-population k"),
    case("shade", 150, 24, "ellipsoid", P=3, seed=99, note="second column pass of de_generation"),
    case("jade", 8, 16, "rastrigin", seed=99, note="base case"),
    case("jade", 21, 40, "griewank", dict(pelite=0.2, archive=False), seed=99,
         note="elite draw without archive"),
    case("sansde", 8, 16, "rastrigin", seed=123, note="base case"),
    case("sansde", 12, 20, "ackley", dict(crref=1, pupdate=4, crupdate=2), seed=123,
         note="every adaptation period fires inside 10 generations"),
    case("cso", 8, 12, "rastrigin", seed=321, note="base case"),
    case("cso", 7, 31, "sphere", dict(pcompete=4, ring=True), seed=321, note="np rounded up, ring"),
    case("cso", 12, 202, "ackley", dict(pcompete=2, ring=True, correct=False, vmax=0.1), seed=321,
         note="np > 100: phi > 0"),
    case("apso", 8, 12, "rastrigin", seed=4242, chunk=12, note="one chunk"),
    case("apso", 33, 70, "sphere", seed=4242, chunk=48, note="odd n, two chunks"),
    # (seed 4242 leaves all five populations in state 3 after every generation here: 258 is the first
    # of 1 .. 599 with two states after generation 9 and in half of the generations, on the oracle)
    case("apso", 12, 150, "rosenbrock", seed=258, chunk=64,
         note="three chunks, pso_gbest between them per population"),
    case("ccpso", 12, 8, "rastrigin", dict(pps=[2, 3, 6]), gens=30, seed=555,
         note="nswarm differs per population from generation 0"),
    case("ccpso", 16, 6, "sphere", dict(pps=[1, 2, 4, 8, 16], pcauchy=0.3), gens=30, seed=555,
         note="five group sizes live at once"),
    case("ccpso", 300, 24, "ellipsoid", dict(pps=[5, 10, 50]), P=3, gens=15, seed=555,
         note="64 lanes per team"),
]

# the first case of each engine (the negative control's)
FIRST = {}
for _c in CASES:
    FIRST.setdefault(_c["engine"], _c)


def find(engine, n, size):
    return next(c for c in CASES if (c["engine"], c["n"], c["size"]) == (engine, n, size))


def box(n):
    return -BOX * np.ones(n), BOX * np.ones(n)


# ---- construction -------------------------------------------------------------------------------
def oracle_object(lib, c, sub, init=True):
    """the oracle's optimizer of case c in generation-synchronous Philox mode on sub-stream `sub`
    (None: the setter is never called)"""
    e, kw, size = c["engine"], c["kw"], c["size"]
    if e == "shade":
        o = po.shade(lib, kw.get("mfev", 100000), size, 1e-12,
                     **{k: v for k, v in kw.items() if k != "mfev"})
    elif e == "jade":
        o = po.jade(lib, 100000, size, 1e-12, **kw)
    elif e == "sansde":
        o = po.sansde(lib, 10 ** 7, size, 1e-12, **kw)
    elif e == "cso":
        o = po.cso(lib, 10 ** 8, 1e-12, size, **kw)
    elif e == "apso":
        o = po.apso(lib, 10 ** 7, 1e-12, size)
    else:
        o = po.ccpso(lib, 10 ** 8, 1e-12, size, **kw)
    o.set_mode(True, po.RNG_PHILOX, c["seed"])
    if sub is not None:
        o.set_sub(sub)
    if init:
        lo, up = box(c["n"])
        o.init(c["obj"], lo, up, np.zeros(c["n"]))
        if e == "apso":
            o.set_chunk(c["chunk"])
    return o


def device_handle(hip, c, P=None, seed=None):
    """the device's optimizer of case c with P populations (not initialized)"""
    e, kw, size = c["engine"], c["kw"], c["size"]
    ext = dict(seed=c["seed"] if seed is None else seed, populations=c["P"] if P is None else P)
    if e == "shade":
        return hip.SHADE(mfev=kw.get("mfev", 100000), npinit=size, tol=1e-12,
                         **{k: v for k, v in kw.items() if k != "mfev"}, **ext)
    if e == "jade":
        return hip.JADE(mfev=100000, np=size, tol=1e-12, **kw, **ext)
    if e == "sansde":
        return hip.SANSDE(mfev=10 ** 7, np=size, tol=1e-12, **kw, **ext)
    if e == "cso":
        return hip.CSO(mfev=10 ** 8, stol=1e-12, np=size, **kw, **ext)
    if e == "apso":
        return hip.APSO(mfev=10 ** 7, tol=1e-12, np=size, **ext)
    return hip.CCPSO(mfev=10 ** 8, sigmatol=1e-12, np=size, **kw, **ext)


# ---- the keys of the single-population parity tests ------------------------------------------------
def keys_of(c):
    """every key the engine's single-population GPU parity test reads"""
    e = c["engine"]
    if e == "shade":
        return ("np", "fev", "f", "x", "larch", "arch", "MCR", "MF", "k")
    if e == "jade":
        return ("np", "fev", "f", "x", "larch", "arch", "mucr", "muf")
    if e == "sansde":
        return ("x", "f", "cr", "fev", "pns", "pnf", "fpns", "fpnf", "p", "fp", "crm", "crrec", "crdeltaf")
    if e == "cso":
        return ("np", "home", "x", "v", "f", "meanw", "pmean" if c["kw"].get("ring") else "mean", "xbest",
                "fev", "phil", "phih")
    if e == "apso":
        return ("evof", "state", "w", "c1", "c2", "fev", "x", "v", "xb", "f", "xbest", "fbest")
    return ("is", "nswarm", "cpswarm", "fev", "improved", "k", "ibest", "strat", "fx", "fy", "y", "x",
            "yhat", "fyhat", "phat")


def oracle_state(o, c):
    return {k: o.get(k).copy() for k in keys_of(c)}


def device_state(g, c, p):
    return {k: g.get_state(k, p).copy() for k in keys_of(c)}


# ---- comparison -----------------------------------------------------------------------------------
class Worst:
    """the largest relative deviation seen, and which key, population and generation held it"""

    def __init__(self):
        self.err, self.where = -1., ""

    def see(self, err, where):
        if err > self.err:
            self.err, self.where = float(err), where

    def __str__(self):
        return "%.3e (%s)" % (self.err, self.where) if self.err >= 0. else "nothing compared"


class Compare:
    """device population p against oracle object p: `have(key)` / `want(key)` read the two sides"""

    def __init__(self, g, o, p, tag, worst):
        self.g, self.o, self.p, self.worst = g, o, p, worst
        self.tag = "%s population %d" % (tag, p)

    def have(self, k):
        return self.g.get_state(k, self.p)

    def want(self, k):
        return self.o.get(k)

    def close(self, k, rtol, a=None, b=None):
        """|a - b|_max <= rtol |b|_max: the `_close` of every single-population parity file"""
        a = np.asarray(self.have(k) if a is None else a, dtype=float)
        b = np.asarray(self.want(k) if b is None else b, dtype=float)
        what = "%s %s" % (self.tag, k)
        assert a.shape == b.shape, "%s: shape %s vs %s" % (what, a.shape, b.shape)
        if a.size == 0:
            return
        err = np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)
        self.worst.see(err, what)
        assert err <= rtol, "%s: rel err %.3e > %.1e" % (what, err, rtol)

    def same_int(self, k):
        a, b = int(self.have(k)[0]), int(self.want(k)[0])
        assert a == b, "%s %s: %d vs %d" % (self.tag, k, a, b)

    def same_array(self, k):
        np.testing.assert_array_equal(self.have(k), self.want(k), err_msg="%s %s" % (self.tag, k))


def compare_de(cmp, c):
    """tests/test_de_gpu.py:43-56 (_compare)"""
    cmp.same_int("np")                      # :44
    cmp.same_int("fev")                     # :45
    cmp.close("f", 1e-11)                   # :46
    cmp.close("x", 1e-12)                   # :47
    cmp.same_int("larch")                   # :48
    cmp.close("arch", 1e-12)                # :49
    if c["engine"] == "shade":
        cmp.close("MCR", 1e-10)             # :51
        cmp.close("MF", 1e-10)              # :52
        cmp.same_int("k")                   # :53
    else:
        cmp.close("mucr", 1e-10)            # :55
        cmp.close("muf", 1e-10)             # :56


def compare_sansde(cmp, c):
    """tests/test_sansde_gpu.py:42-59: the oracle keeps last generation's order until it sorts at
    the start of the next one, the device reports sorted order"""
    n, npp = c["n"], c["size"]
    og = {k: cmp.want(k) for k in ("x", "f", "cr")}
    idx = np.argsort(og["f"], kind="stable")
    cmp.close("f", 1e-11, b=og["f"][idx])                                   # :47
    cmp.close("x", 1e-12, b=og["x"].reshape(npp, n)[idx].ravel())           # :48
    cmp.close("cr", 1e-12, b=og["cr"][idx])                                 # :49
    cmp.same_int("fev")                                                     # :50
    cmp.same_array("pns")                                                   # :51
    cmp.same_array("pnf")                                                   # :52
    for k in ("fpns", "fpnf"):                                              # :53-55
        a, b = cmp.have(k), cmp.want(k)
        err = np.abs(a - b).max() / max(np.abs(b).max(), 1.)
        cmp.worst.see(err, "%s %s" % (cmp.tag, k))
        assert err <= 1e-10, (cmp.tag, k, err)
    for k in ("p", "fp", "crm", "crrec", "crdeltaf"):                       # :56-59
        a, b = cmp.have(k)[0], cmp.want(k)[0]
        if np.isnan(a) and np.isnan(b):
            continue
        assert abs(a - b) <= 1e-10 * max(abs(b), 1e-300) + 1e-300, (cmp.tag, k, a, b)
        if b != 0.:
            cmp.worst.see(abs(a - b) / abs(b), "%s %s" % (cmp.tag, k))


def compare_cso(cmp, c):
    """tests/test_cso_gpu.py:47-59 (phil / phih are read after the last generation there; they are
    constants of np, so every generation is no less)"""
    cmp.same_array("home")                  # :47
    cmp.close("x", 1e-12)                   # :48
    cmp.close("v", 1e-11)                   # :49
    cmp.close("f", 1e-11)                   # :50
    cmp.close("meanw", 1e-12)               # :51
    if c["kw"].get("ring"):
        cmp.close("pmean", 1e-13)           # :53
    else:
        cmp.close("mean", 1e-12)            # :55
    cmp.close("xbest", 1e-12)               # :56
    cmp.same_int("fev")                     # :57
    assert cmp.have("phil")[0] == cmp.want("phil")[0], cmp.tag + " phil"      # :58
    assert cmp.have("phih")[0] == cmp.want("phih")[0], cmp.tag + " phih"      # :59


def compare_apso(cmp, c):
    """tests/test_pso_gpu.py:56-67"""
    cmp.close("evof", 1e-9)                 # :56
    cmp.same_int("state")                   # :57
    cmp.close("w", 1e-10)                   # :59-60
    cmp.close("c1", 1e-12)
    cmp.close("c2", 1e-12)
    cmp.same_int("fev")                     # :61
    cmp.close("x", 1e-11)                   # :62
    cmp.close("v", 1e-10)                   # :63
    cmp.close("xb", 1e-11)                  # :64
    cmp.close("f", 1e-10)                   # :65
    cmp.close("xbest", 1e-11)               # :66
    cmp.close("fbest", 1e-10)               # :67


def compare_ccpso(cmp, c):
    """tests/test_ccpso_gpu.py:47-58"""
    for k in ("is", "nswarm", "cpswarm", "fev", "improved"):                # :47-48
        cmp.same_int(k)
    cmp.same_array("k")                     # :49
    cmp.same_array("ibest")                 # :50
    cmp.same_array("strat")                 # :51
    cmp.close("fx", 1e-11)                  # :52
    cmp.close("fy", 1e-11)                  # :53
    cmp.close("y", 1e-13)                   # :54
    cmp.close("x", 1e-10)                   # :55
    cmp.close("yhat", 1e-13)                # :56
    cmp.close("fyhat", 1e-11)               # :57
    a, b = cmp.have("phat")[0], cmp.want("phat")[0]
    assert abs(a - b) <= 1e-12, cmp.tag + " phat"                           # :58


COMPARE = {"shade": compare_de, "jade": compare_de, "sansde": compare_sansde, "cso": compare_cso,
           "apso": compare_apso, "ccpso": compare_ccpso}


def compare_init(cmp, c):
    """after initialize: what the engine's single-population test holds before its first generation"""
    e = c["engine"]
    if e in ("shade", "jade"):
        # test_de_gpu.py:77-79: the same words through the same map, then the whole _compare
        np.testing.assert_array_equal(np.sort(cmp.have("x"), axis=None), np.sort(cmp.want("x"), axis=None),
                                      err_msg=cmp.tag)
        compare_de(cmp, c)
    elif e == "sansde":
        np.testing.assert_array_equal(np.sort(cmp.have("x"), axis=None), np.sort(cmp.want("x"), axis=None),
                                      err_msg=cmp.tag)                     # test_sansde_gpu.py:37-38
    elif e == "cso":
        cmp.same_int("np")                  # test_cso_gpu.py:41
        cmp.same_array("x")                 # :42
    elif e == "apso":
        cmp.same_array("x")                 # test_pso_gpu.py:48
        cmp.close("f", 1e-12)               # :49
        cmp.close("fbest", 1e-12)           # :50
    else:
        cmp.same_array("x")                 # test_ccpso_gpu.py:41
        cmp.same_array("yhat")              # :42
