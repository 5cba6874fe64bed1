"""The fixed-shape batch eigensolver of n = ld = 128 (cma_eigen_fx128) against the generic kernel it
specialises (cma_eigen, kept behind diagnostic bit 2097152): the same arithmetic in the same
order, so B, D, the repaired C, the scalars and the sampler's packed operand are compared bit for
bit, non-finite input included.  33 populations: the smallest batch above eig_split_maxp = 32, so the
one-workgroup kernel is the one under test.  The reduction of the split form (at most 32 matrices:
cma_eigen_r1_fx128 against cma_eigen_r1) is held to the same at 1 and 3 populations."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, P, LAM = 128, 33, 16
GENERIC = 2097152
SKIPPED = P - 1          # the population whose decomposition is not due


def _orth(rng, n):
    q, r = np.linalg.qr(rng.standard_normal((n, n)))
    return q * np.sign(np.diag(r))


def _spd(rng, n, cond):
    lam = np.logspace(0., -np.log10(cond), n) if cond > 1. else np.ones(n)
    q = _orth(rng, n)
    c = (q * lam) @ q.T
    return 0.5 * (c + c.T)


def _handle(hip, n=N, pops=P, dbg=0, bound=False, seed=5):
    g = hip.ActiveCMAES(mfev=10 ** 9, tol=1e-14, np=LAM, bound=bound, seed=seed, populations=pops)
    g.initialize(hip.objectives.sphere, -np.ones(n), np.ones(n), np.zeros((pops, n)))
    if dbg:
        g.set_state("dbg", [float(dbg)])
    return g


def _due(g, p, due=True):
    g.set_state("fev", [10 ** 6], p)
    g.set_state("eigenlastev", [0 if due else 10 ** 6], p)


@pytest.fixture(scope="module")
def inputs(hip):
    """name -> C, one population each; computed once, read-only"""
    rng = np.random.default_rng(128)
    out = {}
    for e in (0, 1, 2, 3, 4, 6, 8, 10, 12):
        out["spd cond 1e%d" % e] = _spd(rng, N, 10. ** e)
    out["identity"] = np.eye(N)
    out["diagonal, repeated"] = np.diag(np.repeat([4., 1., 0.25, 1e-3], N // 4))
    # rank 100, one eigenvalue pushed to -1e-18 of the largest: the first repair (lo <= 0)
    q = _orth(rng, N)
    lam = np.concatenate([np.linspace(1., 3., 100), np.zeros(N - 100)])
    lam[-1] = -1e-18 * lam.max()
    psd = (q * lam) @ q.T
    out["psd rank 100, negative"] = 0.5 * (psd + psd.T)
    out["cond above 1e14"] = _spd(rng, N, 1e16)          # the second repair (hi > 1e14 lo)
    # a covariance of a real run: 30 generations on the ellipsoid
    r = hip.ActiveCMAES(mfev=10 ** 9, tol=1e-14, np=LAM, seed=3)
    r.initialize(hip.objectives.ellipsoid, -5. * np.ones(N), 5. * np.ones(N), np.ones(N))
    r.run(30)
    out["after 30 generations"] = r.get_state("C").reshape(N, N).copy()
    bad = _spd(rng, N, 1e3)
    bad[5, 17] = bad[17, 5] = np.nan
    out["nan entry"] = bad
    for v in out.values():
        v.setflags(write=False)
    assert len(out) < SKIPPED
    return out


def _load(g, inputs, rng_seed=7):
    """population k gets input k; the rest random SPD matrices; the last one is not due"""
    rng = np.random.default_rng(rng_seed)
    mats = list(inputs.values())
    while len(mats) < P:
        mats.append(_spd(rng, N, 10. ** rng.uniform(0., 12.)))
    for p, m in enumerate(mats):
        g.set_state("C", m, p)
        _due(g, p, p != SKIPPED)
    return mats


def _state(g, keys=("B", "D", "C", "BD", "eigenlastev", "eigen_done", "basis_ok")):
    return {k: np.stack([g.get_state(k, p) for p in range(P)]) for k in keys}


def _same_bits(a, b, what):
    for k in a:
        assert np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)), (what, k)


@pytest.fixture(scope="module")
def pair(hip, inputs):
    """the two kernels on the same 33 matrices, then one sampling phase each (same seed: same normals)"""
    from bboptpy_amd import _ffi
    res = {}
    for name, dbg in (("fixed", 0), ("generic", GENERIC)):
        g = _handle(hip, dbg=dbg)
        _load(g, inputs)
        before = _state(g, ("B", "D"))
        g.phase(_ffi.PHASE_EIGEN)
        took = int(g.get_state("eig_fixed128")[0])
        st = _state(g)
        g.phase(_ffi.PHASE_SAMPLE_EVALUATE)
        X = np.stack([g.get_state("arx", p) for p in range(P)])
        res[name] = (before, st, X, took)
    return res


def test_each_handle_took_its_kernel(pair):
    assert pair["fixed"][3] == 1 and pair["generic"][3] == 0


def test_identical_bits_on_every_input(pair, inputs):
    _, fs, fX, _ = pair["fixed"]
    _, gs, gX, _ = pair["generic"]
    for p, name in enumerate(list(inputs) + ["random"] * (P - len(inputs))):
        for k in fs:
            assert np.array_equal(fs[k][p].view(np.uint64), gs[k][p].view(np.uint64)), (name, p, k)
        # (the sampler reads the packed operand B D the eigensolver wrote)
        assert np.array_equal(fX[p].view(np.uint64), gX[p].view(np.uint64)), (name, p, "X")
        if p != SKIPPED:
            assert int(fs["eigen_done"][p][0]) == 1 and int(fs["eigenlastev"][p][0]) == 10 ** 6, name


def test_project_bounds_on_finite_inputs(pair, inputs):
    """the fixed-shape result against the matrix the handle holds afterwards (C with its repair
    shifts: that is what B and D decompose)"""
    _, fs, _, _ = pair["fixed"]
    for p, name in enumerate(inputs):
        if name == "nan entry":
            continue
        B, D, C = fs["B"][p].reshape(N, N), fs["D"][p], fs["C"][p].reshape(N, N)
        assert np.isfinite(B).all() and np.isfinite(D).all(), name
        assert np.linalg.norm(B.T @ B - np.eye(N)) <= 1e-12 * N, name
        assert np.linalg.norm((B * (D * D)) @ B.T - C) <= 1e-11 * np.linalg.norm(C), name
        assert (np.diff(D) >= 0.).all() and D[0] > 0. and D[-1] ** 2 <= 1e14 * D[0] ** 2 * (1. + 1e-12), name


def test_repairs_fired(pair, inputs):
    _, fs, _, _ = pair["fixed"]
    names = list(inputs)
    for name in ("psd rank 100, negative", "cond above 1e14"):
        p = names.index(name)
        shift = np.diag(fs["C"][p].reshape(N, N)) - np.diag(inputs[name])
        assert (shift > 0.).all(), name
    p = names.index("spd cond 1e6")
    assert np.array_equal(fs["C"][p].reshape(N, N), inputs["spd cond 1e6"])


def test_population_not_due_is_skipped_by_both(pair):
    for name in ("fixed", "generic"):
        before, st, _, _ = pair[name]
        assert int(st["eigen_done"][SKIPPED][0]) == 0, name
        assert int(st["eigenlastev"][SKIPPED][0]) == 10 ** 6, name
        for k in ("B", "D"):
            assert np.array_equal(before[k][SKIPPED], st[k][SKIPPED]), (name, k)


def test_stopped_population_is_left_alone_under_honor_stop(hip):
    """run() honours the stop flag: population 7, stopped, keeps B, D, C and eigenlastev although its
    decomposition is due; the other populations come out of both kernels with the same bits"""
    rng = np.random.default_rng(11)
    mats = [_spd(rng, N, 10. ** rng.uniform(0., 8.)) for _ in range(P)]
    out = {}
    for name, dbg in (("fixed", 0), ("generic", GENERIC)):
        g = _handle(hip, dbg=dbg, seed=9)
        for p, m in enumerate(mats):
            g.set_state("C", m, p)
            _due(g, p)
        g.set_state("stop", [1], 7)
        before = _state(g, ("B", "D", "C", "eigenlastev"))
        assert g.run(1) == 1
        after = _state(g, ("B", "D", "C", "eigenlastev", "eigen_done"))
        for k in before:
            assert np.array_equal(before[k][7].view(np.uint64), after[k][7].view(np.uint64)), (name, k)
        assert int(after["eigen_done"][0][0]) == 1 and not np.array_equal(before["B"][0], after["B"][0]), name
        assert int(g.get_state("eig_fixed128")[0]) == (1 if name == "fixed" else 0)
        out[name] = after
    _same_bits(out["fixed"], out["generic"], "after run(1)")


@pytest.mark.parametrize("n,bound", [(127, False), (128, True)])
def test_other_shapes_keep_the_generic_kernel(hip, n, bound):
    from bboptpy_amd import _ffi
    rng = np.random.default_rng(n + bound)
    g = _handle(hip, n=n, bound=bound)
    mats = [_spd(rng, n, 10. ** rng.uniform(0., 10.)) for _ in range(P)]
    for p, m in enumerate(mats):
        g.set_state("C", m, p)
        _due(g, p)
    g.phase(_ffi.PHASE_EIGEN)
    assert int(g.get_state("eig_fixed128")[0]) == 0
    for p in (0, 16, P - 1):
        B, D = g.get_state("B", p).reshape(n, n), g.get_state("D", p)
        assert int(g.get_state("eigen_done", p)[0]) == 1
        assert np.linalg.norm(B.T @ B - np.eye(n)) <= 1e-12 * n
        assert np.linalg.norm((B * (D * D)) @ B.T - mats[p]) <= 1e-11 * np.linalg.norm(mats[p])


@pytest.mark.parametrize("pops", [1, 3])
def test_split_form_reduction_identical_bits(hip, inputs, pops):
    """at most eig_split_maxp matrices: only the reduction kernel differs between the two handles; the
    whole decomposition and the sampled X come out with the same bits, within the project's bounds"""
    from bboptpy_amd import _ffi
    names = ["spd cond 1e6", "psd rank 100, negative", "after 30 generations"][:pops]
    keys = ("B", "D", "C", "BD", "eigenlastev", "eigen_done", "basis_ok")
    out = {}
    for form, dbg in (("fixed", 0), ("generic", GENERIC)):
        g = _handle(hip, pops=pops, dbg=dbg)
        for p, name in enumerate(names):
            g.set_state("C", inputs[name], p)
            _due(g, p)
        g.phase(_ffi.PHASE_EIGEN)
        assert int(g.get_state("eig_fixed128")[0]) == (1 if form == "fixed" else 0)
        st = {k: np.stack([g.get_state(k, p) for p in range(pops)]) for k in keys}
        g.phase(_ffi.PHASE_SAMPLE_EVALUATE)
        st["X"] = np.stack([g.get_state("arx", p) for p in range(pops)])
        out[form] = st
    _same_bits(out["fixed"], out["generic"], "split form, %d populations" % pops)
    for p, name in enumerate(names):
        B, D, C = out["fixed"]["B"][p].reshape(N, N), out["fixed"]["D"][p], out["fixed"]["C"][p].reshape(N, N)
        assert int(out["fixed"]["eigen_done"][p][0]) == 1, name
        assert np.linalg.norm(B.T @ B - np.eye(N)) <= 1e-12 * N, name
        assert np.linalg.norm((B * (D * D)) @ B.T - C) <= 1e-11 * np.linalg.norm(C), name
