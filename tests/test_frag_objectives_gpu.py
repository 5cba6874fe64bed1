"""GPU: the fitness the CMA samplers form from their own candidates, against a NumPy restatement
of the 16-lanes-per-row arithmetic applied to the `arx` the device returns -- to the bit.

A candidate row is shared by the 16 lanes of a DPP row.  Lane c0 holds the columns 16 t + c0 and
adds their terms in ascending t (a term beyond the dimension adds 0.); the 16 lane sums meet as
    v += ror8(v); v += ror4(v); v += ror2(v); v += ror1(v)
(row16_sum in bbo_objectives.hpp; group_sum<16>'s xor butterfly pairs the same values at every
step, and a + b = b + a, so eval_row_group<16> gives the same bits).  The library builds with
-ffp-contract=off: every product and sum below is an operation of its own, as in NumPy.
    Rosenbrock  term = 100 (tt tt) + u u,  tt = x[j + 1] - x[j] x[j],  u = 1 - x[j],  j + 1 < n;
                lane 15 takes x[j + 1] from lane 0 of the NEXT tile
    Schwefel 1.2  per tile: run = carry + scan(v), scan = the inclusive prefix sum by
                v += shr1(v); v += shr2(v); v += shr4(v); v += shr8(v) with ZEROS shifted in;
                term = run run; carry += row sum of the tile
    Cigar / Discus  x0 reaches every lane as the row sum of (c0 == 0 ? x[0] : 0)
Which code forms f:
    eval_frag_rows<8> on the MFMA accumulators: cma_sample_eval128 (ld = 128 and at least
        `sample128_min` candidates in flight), its FULL build when n = 128, lambda a multiple of
        16, no box and no recorded normals, its masked build otherwise (n = 127, 113)
    eval_row_group<16> from LDS: the tile-per-workgroup sampler cma_sample_eval<1, 8> (n = 128,
        one small population) and cma_sample_eval64 (n = 48: three column tiles)
The expectation is exact (uint64 views are compared): the model states the device's operations one
by one, and nothing in it is approximate.  The recorded normals are held to oracle/philox.h the same
way: Philox4x32-10 is integer arithmetic."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = 4


# ---- the model -------------------------------------------------------------------------------
def _ror(v, k):
    return np.roll(v, k, axis=-1)            # row_ror:k -- lane i reads lane (i - k) mod 16


def _shr(v, k):
    out = np.zeros_like(v)                   # row_shr:k -- lane i reads lane i - k, 0 below lane k
    out[..., k:] = v[..., :-k]
    return out


def _row_sum(v):
    for k in (8, 4, 2, 1):
        v = v + _ror(v, k)
    return v


def _row_scan(v):
    for k in (1, 2, 4, 8):
        v = v + _shr(v, k)
    return v


def _aux_ellipsoid(n):
    return np.array([math.pow(10., 6. * (i / (n - 1))) for i in range(n)])


def _model(obj, X):
    """f of every row of X[rows, n], as lane 0 of the row's 16 lanes holds it"""
    rows, n = X.shape
    NT = (n + 15) // 16
    Xp = np.zeros((rows, NT * 16 + 1))
    Xp[:, :n] = X
    c0 = np.arange(16)
    a = np.zeros((rows, 16))
    carry = np.zeros((rows, 16))
    aux = _aux_ellipsoid(n) if obj == "ellipsoid" else None
    for t in range(NT):
        j = 16 * t + c0
        x = Xp[:, j]
        live = (j < n)[None, :]
        if obj == "sphere":
            a = a + np.where(live, x * x, 0.)
        elif obj == "rosenbrock":
            xn = Xp[:, j + 1]
            tt = xn - x * x
            u = 1. - x
            a = a + np.where((j + 1 < n)[None, :], 100. * (tt * tt) + u * u, 0.)
        elif obj == "ellipsoid":
            w = np.where(j < n, aux[np.minimum(j, n - 1)], 0.)[None, :]
            a = a + np.where(live, w * (x * x), 0.)
        elif obj in ("cigar", "discus"):
            a = a + np.where(live & (j > 0)[None, :], x * x, 0.)
        elif obj == "schwefel12":
            v = np.where(live, x, 0.)
            run = carry + _row_scan(v)
            a = a + np.where(live, run * run, 0.)
            carry = carry + _row_sum(v)
        else:
            raise ValueError(obj)
    a = _row_sum(a)
    if obj in ("cigar", "discus"):
        x0 = _row_sum(np.where((c0 == 0)[None, :], Xp[:, :16], 0.))
        a = x0 * x0 + 1.0e6 * a if obj == "cigar" else 1.0e6 * (x0 * x0) + a
    return a[:, 0].copy()


def test_model_agrees_with_the_plain_formulas():
    """(needs no device output: the restatement is the objective, up to the order of the sums)"""
    import bboptpy_amd as bb
    rng = np.random.default_rng(1)
    for n in (128, 127, 113, 48):
        X = rng.uniform(-3, 3, (5, n))
        for obj in ("sphere", "rosenbrock", "ellipsoid", "cigar", "discus", "schwefel12"):
            want = np.array([getattr(bb.objectives, obj)(x) for x in X])
            np.testing.assert_allclose(_model(obj, X), want, rtol=1e-12)
    # the shifted-in lanes of the scan are zeros: lane 0 of the first tile keeps its own value
    v = np.arange(1., 17.)[None, :]
    assert np.array_equal(_row_scan(v)[0], np.cumsum(v[0]))


# ---- the device ------------------------------------------------------------------------------
def _generation(hip, obj, n, lam, batch, record=False, seed=20241, pops=P):
    """one SAMPLE_EVALUATE phase of `pops` populations; batch: cma_sample_eval128 is the sampler
    (sample128_min = 1), else the dispatch of small launches.  -> X[pops, lam, n], f[pops, lam],
    the recorded normals of population 0 (or None) and the generation counter they were drawn at"""
    from bboptpy_amd import _ffi
    rng = np.random.default_rng(n * 1000 + lam)
    lo, up = -10. * np.ones(n), 10. * np.ones(n)
    guess = rng.uniform(-3, 3, (pops, n))
    g = hip.ActiveCMAES(mfev=10 ** 9, tol=1e-14, np=lam, seed=seed, populations=pops)
    g.initialize(getattr(hip.objectives, obj), lo, up, guess if pops > 1 else guess[0])
    if batch:
        g.set_state("sample128_min", [1.0])
    if record:
        g.set_state("record_normals", [1.0])
    it = int(g.get_state("it")[0])
    g.phase(_ffi.PHASE_SAMPLE_EVALUATE)
    # enum SampleKernel (bbo_cma.hpp): 6 = cma_sample_eval128 -- what the knob selects, and nothing else does here
    assert (int(g.get_state("sample_route")[0]) == 6) == bool(batch)
    X = np.stack([g.get_state("arx", p).reshape(lam, n) for p in range(pops)])
    f = np.stack([g.get_state("fitness", p) for p in range(pops)])
    z = g.get_state("zlast", 0).copy() if record else None
    return X, f, z, it


def _check(obj, X, f, what):
    assert np.isfinite(X).all() and np.isfinite(f).all(), what
    want = np.concatenate([_model(obj, Xp) for Xp in X])
    got = f.ravel()
    bad = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]
    rel = np.abs(got - want).max() / np.abs(want).max()
    print("%s: %d of %d values differ from the model, largest difference %.3e of max |f|"
          % (what, bad.size, got.size, rel))
    assert bad.size == 0, "%s: rows %s, device %s, model %s" % (
        what, bad[:4], got[bad[:4]], want[bad[:4]])


@pytest.mark.parametrize("batch", [False, True], ids=["tile-kernel", "batch-kernel"])
def test_rosenbrock_n128_full_path(hip, batch):
    """n = 128, lambda = 32, nothing recorded: all eight column tiles, lane 15's neighbour from the
    next tile on tiles 0..6 and the masked last term (column 127 has no right-hand neighbour) on
    tile 7; once by the tile-per-workgroup sampler, once by cma_sample_eval128's FULL build"""
    X, f, _, _ = _generation(hip, "rosenbrock", 128, 32, batch)
    _check("rosenbrock", X, f, "rosenbrock n=128 " + ("batch" if batch else "tile"))


def test_the_two_samplers_draw_the_same_candidates(hip):
    """(what makes the pair above two checks of ONE generation: same seed, same X, same f)"""
    Xa, fa, _, _ = _generation(hip, "rosenbrock", 128, 32, False)
    Xb, fb, _, _ = _generation(hip, "rosenbrock", 128, 32, True)
    assert np.array_equal(Xa.view(np.uint64), Xb.view(np.uint64))
    assert np.array_equal(fa.view(np.uint64), fb.view(np.uint64))


@pytest.mark.parametrize("n", [127, 113])
def test_rosenbrock_masked_path(hip, n):
    """ld = 128 > n: cma_sample_eval128's masked build.  The last live column is lane 14 of tile 7
    (n = 127) or lane 0 of tile 7 (n = 113); the padding columns hold 0 and column n must not enter
    (a term that took it would add 100 x[n-1]^4 + (1 - x[n-1])^2, far from a rounding)"""
    X, f, _, _ = _generation(hip, "rosenbrock", n, 32, True)
    _check("rosenbrock", X, f, "rosenbrock n=%d batch" % n)


def test_rosenbrock_three_tiles(hip):
    """n = 48, lambda = 16: cma_sample_eval64, three column tiles"""
    X, f, _, _ = _generation(hip, "rosenbrock", 48, 16, False)
    _check("rosenbrock", X, f, "rosenbrock n=48")


@pytest.mark.parametrize("n", [128, 113])
@pytest.mark.parametrize("obj", ["sphere", "ellipsoid", "cigar", "discus", "schwefel12"])
def test_row_sums_and_scans_on_the_accumulators(hip, obj, n):
    """the other objectives eval_frag_rows offers, lambda = 16, through cma_sample_eval128 (FULL at
    n = 128, masked at 113): row16_sum everywhere, row16_scan in Schwefel 1.2 -- the lanes row_shr
    shifts in must read 0, anything else shows in the first prefix sums of every tile"""
    X, f, _, _ = _generation(hip, obj, n, 16, True)
    _check(obj, X, f, "%s n=%d batch" % (obj, n))


@pytest.mark.parametrize("batch", [False, True], ids=["tile-kernel", "batch-kernel"])
def test_recorded_normals_are_the_oracles(hip, oracle_lib, batch):
    """Philox on the device against oracle/philox.h: the library exposes no raw words, so the
    recorded normals of one generation at n = 128, lambda = 32 (4096 draws: 1024 Philox calls and
    the slow draws' extra ones) are held to the oracle's, bit for bit; and the FULL build, which
    records nothing, must have drawn the same candidates from the same key"""
    n, lam, seed = 128, 32, 424242
    Xr, fr, z, it = _generation(hip, "rosenbrock", n, lam, batch, record=True, seed=seed, pops=1)
    want = np.zeros(lam * n)
    oracle_lib.f("philox_normals")(seed, it, lam, n, want)
    assert z.size == want.size
    bad = int(np.count_nonzero(z.view(np.uint64) != want.view(np.uint64)))
    print("recorded normals (%s): %d of %d differ from the oracle" % (
        "batch" if batch else "tile", bad, z.size))
    assert bad == 0
    X, f, _, _ = _generation(hip, "rosenbrock", n, lam, batch, record=False, seed=seed, pops=1)
    assert np.array_equal(X.view(np.uint64), Xr.view(np.uint64))
    assert np.array_equal(f.view(np.uint64), fr.view(np.uint64))
