"""The oracle's population sub-stream (Handle.set_sub, philox_normals_sub) held to something
independent of it, on the CPU.

tests/test_batch_oracle_gpu.py compares population p of a batched device handle with an oracle
object on sub-stream p.  That is only worth something if the setter (a) changes nothing at
sub = 0, where the oracle is pinned to the compiled reference and to the golden vectors, and
(b) really moves every draw to the stream it names -- shown here by rebuilding each engine's
initial swarm from raw words of the oracle's `philox` entry point with c3 = (stream << 24) | p --
and if (c) the cases chosen there are runs in which the populations stop looking alike."""
import ctypes as C

import numpy as np
import pytest

import batch_oracle as bo
import pyoracle as po

STREAM_CMA_NORMAL, STREAM_INIT = 1, 2        # oracle/philox.h


def _case_of(engine):
    return bo.FIRST[engine]


@pytest.mark.parametrize("engine", ["shade", "jade", "sansde", "cso", "apso", "ccpso"])
def test_sub_zero_is_never_set(oracle_lib, engine):
    """set_sub(0) against no call at all: five generations in sync Philox mode, every key the GPU
    parity tests read, bit for bit"""
    c = _case_of(engine)
    a, b = bo.oracle_object(oracle_lib, c, None), bo.oracle_object(oracle_lib, c, 0)
    for gen in range(6):
        sa, sb = bo.oracle_state(a, c), bo.oracle_state(b, c)
        for k in bo.keys_of(c):
            assert sa[k].tobytes() == sb[k].tobytes(), (engine, gen, k)
        a.iterate()
        b.iterate()
    a.destroy()
    b.destroy()


def _u01(lo32, hi32):
    """philox.h bbo_u01: the top 53 of 64 bits -> [0, 1)"""
    return float(((int(hi32) << 32) | int(lo32)) >> 11) * 2.0 ** -53


def _initial_swarm(lib, seed, sub, rows, lower, upper):
    """the init() of every swarm struct in bbo_oracle_pop.inc (De :113-127, Sansde :591-604, Cso
    :949-964, Ccpso :1242-1255, Apso :1686-1700): particle i, coordinates 2q and 2q + 1 from ONE
    call philox(seed, i, q, 0, (INIT << 24) | sub) -- words 0, 1 the even coordinate, 2, 3 the odd
    one -- and x = u (upper - lower) + lower"""
    n = lower.size
    c3 = (STREAM_INIT << 24) | sub
    w = (C.c_uint32 * 4)()
    X = np.zeros((rows, n))
    for i in range(rows):
        for j in range(n):
            lib.f("philox")(seed, i, j >> 1, 0, c3, w)
            u = _u01(w[2], w[3]) if j & 1 else _u01(w[0], w[1])
            X[i, j] = np.float64(u) * (upper[j] - lower[j]) + lower[j]
    return X


@pytest.mark.parametrize("sub", [1, 4])
@pytest.mark.parametrize("engine", ["shade", "jade", "sansde", "cso", "apso", "ccpso"])
def test_sub_p_draws_from_the_stream_it_names(oracle_lib, engine, sub):
    """the initial x of an object on sub-stream p, rebuilt from raw Philox words with the sub-stream
    in the low 24 bits of c3: equal bits.  (An uneven box, so the affine map is part of it.)"""
    c = dict(_case_of(engine))
    n, seed = c["n"], c["seed"]
    lower = -5. + 0.125 * np.arange(n)
    upper = 3. + 0.375 * np.arange(n)
    o = bo.oracle_object(oracle_lib, c, sub, init=False)
    o.init(c["obj"], lower, upper, np.zeros(n))
    rows = int(o.scalar("np"))                  # (CSO rounds np up to a multiple of pcompete)
    got = o.get("x").reshape(rows, n)
    want = _initial_swarm(oracle_lib, seed, sub, rows, lower, upper)
    if engine in ("shade", "jade"):
        # De::init sorts the swarm by f (stable): the same rows in the order of their values
        f = np.array([oracle_lib.objective(c["obj"], r) for r in want])
        want = want[np.argsort(f, kind="stable")]
    assert got.tobytes() == want.tobytes(), (engine, sub)
    # and it is not the swarm of the neighbouring streams
    for other in (sub - 1, sub + 1):
        assert not np.array_equal(np.sort(got, axis=None),
                                  np.sort(_initial_swarm(oracle_lib, seed, other, rows, lower, upper), axis=None))
    o.destroy()


def test_set_sub_is_for_the_swarm_classes(oracle_lib):
    cma = po.cma(oracle_lib, "active", 1000, 1e-8, 8)
    with pytest.raises(ValueError):
        cma.set_sub(1)
    for make in (po.bipop, po.ipop):
        drv = make(oracle_lib, po.cma(oracle_lib, "active", 1000, 1e-8, 8), 1000)
        with pytest.raises(ValueError):
            drv.set_sub(1)
        drv.destroy()
    cma.destroy()


def _normals(lib, seed, sub, gen, rows, n):
    out = np.zeros(rows * n)
    lib.f("philox_normals_sub")(seed, sub, gen, rows, n, out)
    return out.reshape(rows, n)


def test_philox_normals_sub(oracle_lib):
    """sub = 0 is philox_normals to the bit; sub = 3 rebuilt entry by entry through normal_quad with
    c3 = (CMA_NORMAL << 24) | 3 and the column layout of philox.h:270-271"""
    seed, gen, rows, n = 20240611, 2, 24, 37
    plain = np.zeros(rows * n)
    oracle_lib.f("philox_normals")(seed, gen, rows, n, plain)
    assert _normals(oracle_lib, seed, 0, gen, rows, n).tobytes() == plain.tobytes()
    z3 = _normals(oracle_lib, seed, 3, gen, rows, n)
    assert not np.array_equal(z3.ravel(), plain)
    quad = np.zeros(4)
    for k, j in ((0, 0), (0, 3), (1, 4), (5, 15), (7, 16), (11, 21), (23, 36), (13, 35)):
        oracle_lib.f("normal_quad")(seed, k, ((j >> 4) << 2) | (j & 3), gen, (STREAM_CMA_NORMAL << 24) | 3, quad)
        assert quad[(j >> 2) & 3].tobytes() == z3[k, j].tobytes(), (k, j)
    # generation and sub-stream are different counters: neither stands in for the other
    assert not np.array_equal(z3, _normals(oracle_lib, seed, 2, 3, rows, n))


# (engine, n, size) -> the key that must take at least two values over the populations, and after how
# many generations; conditions on the INPUTS of tests/test_batch_oracle_gpu.py, held on the oracle alone
PROBES = [
    (("ccpso", 12, 8), "nswarm"),
    (("ccpso", 16, 6), "nswarm"),
    (("shade", 8, 64), "larch"),
    (("apso", 8, 12), "state"),
    (("apso", 33, 70), "state"),
    (("apso", 12, 150), "state"),
]


@pytest.mark.parametrize("which,key", PROBES, ids=["%s-%d-%d-%s" % (w + (k,)) for w, k in PROBES])
def test_the_probes_are_different_runs(oracle_lib, which, key):
    """the five oracle objects hold at least two different swarm counts (CCPSO: after generation 0
    and after the last one), archive fills (SHADE with LPSR: after generation 0, while the archive
    fills) and fuzzy states (APSO: after the last generation and in half of them at least)"""
    c = bo.find(*which)
    assert c["P"] == 5
    objs = [bo.oracle_object(oracle_lib, c, p) for p in range(c["P"])]
    seen = []
    for gen in range(c["gens"]):
        for o in objs:
            o.iterate()
        seen.append([int(o.scalar(key)) for o in objs])
    differ = sum(len(set(row)) >= 2 for row in seen)
    print("%s, seed %d: %s per population after generation 0 %s, after generation %d %s; the populations "
          "differ in %d of %d generations" % (c["id"], c["seed"], key, seen[0], c["gens"] - 1, seen[-1], differ,
                                              len(seen)))
    if key == "larch":
        # the archive fills at its own pace in generation 0 only: from then on it is full in every
        # population (larch == np, the trim keeps it there) and only its contents differ
        assert len(set(seen[0])) >= 2, seen[0]
    else:
        assert len(set(seen[0])) >= 2 or key == "state", seen[0]
        assert len(set(seen[-1])) >= 2, seen[-1]
        assert differ >= len(seen) // 2, seen
    if which == ("shade", 8, 64):
        nps = [int(o.scalar("np")) for o in objs]
        print("  np after %d generations %s" % (c["gens"], nps))
        assert all(v < 64 for v in nps)          # the reduction did run
    for o in objs:
        o.destroy()
