"""GPU: the transposed tile loop of cma_sample_eval128 / _tri (the MFMA operands swapped, the LDS copy of
the operand permuted, the objective inside the lane: sample128_epilogue_tr, eval_frag_cols) against the
row-layout loop of the same kernel (`sample128_rowlayout` = 1), to the bit: same normals, the same chain
of 32 accumulations per element, the same order of every objective's sum (tests/test_sample_transposed.py
restates the two orders).  `sample_transposed` says which loop the last launch took."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 128
OBJECTIVES = ("sphere", "rosenbrock", "ellipsoid", "cigar", "discus")


def _host_objective(x):
    return float(np.sum(x * x) + x[0])


def _objective(hip, name):
    return _host_objective if name == "host" else getattr(hip.objectives, name)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same(a, b, what):
    bad = int(np.count_nonzero(_bits(a) != _bits(b)))
    print("%s: %d of %d values differ between the two loops" % (what, bad, a.size))
    assert bad == 0, what


def _active(hip, obj, lam, pops, rowlayout, seed=311):
    rng = np.random.default_rng(lam + pops)
    lo, up = -10. * np.ones(N), 10. * np.ones(N)
    g = hip.ActiveCMAES(mfev=10 ** 9, tol=1e-14, np=lam, seed=seed, populations=pops)
    g.initialize(_objective(hip, obj), lo, up, rng.uniform(-3, 3, (pops, N)))
    g.set_state("sample128_min", [1.0])
    assert g.get_state("sample128_rowlayout")[0] == 0.     # the default
    g.set_state("sample128_rowlayout", [rowlayout])
    return g


def _sample_rank_update(hip, g, pops):
    """one generation up to the update -> arx, fitness, zn2, S of every population, and what the sampler
    reported"""
    from bboptpy_amd import _ffi
    g.phase(_ffi.PHASE_SAMPLE_EVALUATE)
    assert int(g.get_state("sample_route")[0]) == 6        # enum SampleKernel: cma_sample_eval128
    assert int(g.get_state("sample_lean")[0]) == 1
    tr = int(g.get_state("sample_transposed")[0])
    out = {k: np.stack([g.get_state(k, p) for p in range(pops)]) for k in ("arx", "fitness", "zn2")}
    g.phase(_ffi.PHASE_RANK)
    g.phase(_ffi.PHASE_UPDATE)
    out["S"] = np.stack([g.get_state("S", p) for p in range(pops)])
    out["fit_idx"] = np.stack([g.get_state("fit_idx", p) for p in range(pops)])
    return out, tr


def _compare_one_generation(hip, obj, lam, pops, want_transposed):
    got = []
    for rowlayout in (0., 1.):
        g = _active(hip, obj, lam, pops, rowlayout)
        out, tr = _sample_rank_update(hip, g, pops)
        assert tr == (want_transposed if rowlayout == 0. else 0), (obj, rowlayout, tr)
        got.append(out)
    a, b = got
    assert np.isfinite(a["arx"]).all() and np.isfinite(a["fitness"]).all()
    assert np.abs(a["fitness"]).max() > 0. and np.abs(a["S"]).max() > 0.
    for k in ("arx", "fitness", "zn2", "S", "fit_idx"):
        _same(a[k], b[k], "%s lambda=%d P=%d: %s" % (obj, lam, pops, k))


@pytest.mark.parametrize("obj", OBJECTIVES + ("host",))
def test_one_tile_equals_the_row_layout(hip, obj):
    """n = 128, no box, 4 populations, lambda = 16: one tile, wavefront 0 only.  The five objectives of
    eval_frag_cols and a host objective (X and zn2 only on the device)"""
    _compare_one_generation(hip, obj, 16, 4, 1)


def test_schwefel12_keeps_the_row_layout(hip):
    """prefix scans across lanes: `sample_transposed` reads 0 with and without the switch"""
    _compare_one_generation(hip, "schwefel12", 16, 4, 0)


def test_two_tiles_per_wavefront_and_a_ragged_end(hip):
    """16 populations, lambda = 2064: 256 rows per workgroup, every wavefront walks two tiles -- the
    loop's second trip -- and the ninth workgroup of a population has one tile left"""
    _compare_one_generation(hip, "rosenbrock", 2064, 16, 1)


@pytest.mark.parametrize("tri", [1., 0.])
def test_cholesky_operand(hip, tri):
    """CholeskyCMAES, lambda = 16: cma_sample_eval128_tri (7) and, with `chol_tri` = 0, cma_sample_eval128 (6)
    over the factor.  Three generations first, so that the factor has off-diagonals"""
    from bboptpy_amd import _ffi
    pops, lam = 4, 16
    lo, up = -5. * np.ones(N), 5. * np.ones(N)
    guess = np.random.default_rng(4).uniform(-3, 3, (pops, N))
    got = []
    for rowlayout in (0., 1.):
        g = hip.CholeskyCMAES(10 ** 8, 1e-12, 1e-12, lam, 2., False, seed=13, populations=pops)
        g.initialize(hip.objectives.rosenbrock, lo, up, guess.ravel())
        g.set_state("sample128_min", [1.0])
        g.set_state("chol_tri", [tri])
        g.set_state("sample128_rowlayout", [rowlayout])
        for _ in range(3):
            g.iterate()
        g.phase(_ffi.PHASE_SAMPLE_EVALUATE)
        assert int(g.get_state("sample_route")[0]) == (7 if tri else 6)
        assert int(g.get_state("sample_transposed")[0]) == (0 if rowlayout else 1)
        got.append({k: np.stack([g.get_state(k, p) for p in range(pops)]) for k in ("arx", "fitness", "A")})
    a, b = got
    assert np.isfinite(a["arx"]).all() and np.isfinite(a["fitness"]).all()
    assert np.abs(np.tril(a["A"][0].reshape(N, N), -1)).max() > 0.
    for k in ("arx", "fitness"):
        _same(a[k], b[k], "cholesky tri=%d: %s" % (tri, k))


def test_three_generations(hip):
    """ActiveCMAES, 4 populations, lambda = 32, three whole generations with each loop"""
    pops = 4
    got = []
    for rowlayout in (0., 1.):
        g = _active(hip, "rosenbrock", 32, pops, rowlayout)
        for _ in range(3):
            g.iterate()
        assert int(g.get_state("sample_route")[0]) == 6
        assert int(g.get_state("sample_transposed")[0]) == (0 if rowlayout else 1)
        got.append({k: np.stack([g.get_state(k, p) for p in range(pops)])
                    for k in ("xmean", "sigma", "C", "arx", "fitness")})
    a, b = got
    assert np.isfinite(a["C"]).all()
    assert np.abs(a["C"][0].reshape(N, N) - np.diag(np.diag(a["C"][0].reshape(N, N)))).max() > 0.
    for k in ("xmean", "sigma", "C", "arx", "fitness"):
        _same(a[k], b[k], "three generations: %s" % k)


@pytest.mark.parametrize("rowlayout", [0., 1.])
def test_nan_objective_stores_inf(hip, rowlayout):
    """a mean of NaN in population 1: every candidate of it is NaN, its objective is NaN, and +inf is
    what the sampler stores; the other populations are untouched"""
    from bboptpy_amd import _ffi
    pops, lam = 4, 16
    g = _active(hip, "rosenbrock", lam, pops, rowlayout)
    g.set_state("xmean", np.full(N, np.nan), 1)
    g.phase(_ffi.PHASE_SAMPLE_EVALUATE)
    assert int(g.get_state("sample_transposed")[0]) == (0 if rowlayout else 1)
    f = np.stack([g.get_state("fitness", p) for p in range(pops)])
    assert np.isnan(g.get_state("arx", 1)).all()
    assert np.all(f[1] == np.inf)
    assert np.isfinite(f[[0, 2, 3]]).all()
