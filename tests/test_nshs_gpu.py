"""GPU: the NSHS kernels against tests/nshs_model.py, and the engine's behaviour at the C ABI.

The candidate is held bit for bit: the model's device form is fed the device's own recorded draws
and the state the kernel read, and its candidate, memory, values, fstd, best and worst must be the
device's.  The fused kernel nshs_steps (bbo_run) gives the bits of the three phase kernels
(bbo_iterate) for every number of iterations per launch, with the harmony memory in LDS and in
global memory.  Against the recorded reference: tests/test_nshs_golden_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import nshs_model as nm
from slpso_model import device_objective
from test_hees_model import band
from test_nshs_model import FSTD_BOUND, GOLD, _h

pytestmark = pytest.mark.gpu

CHUNK = 256             # NSHS_DEFAULT_CHUNK: the iterations of one launch of run()
LDS_BYTES = 6144        # NSHS_LDS_BYTES: the harmony memory's share of LDS
STREAM_NSHS = 20
KEYS = ("x", "f", "cand", "fcand", "fbest", "fworst", "fstd", "ibest", "iworst", "wide", "accepted", "it", "fev",
        "flag")


def _bits(a, b, what):
    a, b = np.asarray(a, float).ravel(), np.asarray(b, float).ravel()
    assert a.shape == b.shape, what
    assert a.tobytes() == b.tobytes(), (what, np.flatnonzero(a != b)[:8], a[a != b][:4], b[a != b][:4])


def _snapshot(g, p=0):
    return {k: g.get_state(k, p).copy() for k in KEYS}


def _same_state(sa, sb, tag=""):
    for k in KEYS:
        _bits(sa[k], sb[k], tag + k)


def _start(hip, n, hms, obj="rosenbrock", seed=7, P=1, mfev=10 ** 6, fstdmin=1e-4, box=5., **kw):
    g = hip.NSHS(mfev, hms, fstdmin, seed=seed, populations=P, **kw)
    g.initialize(obj, -box * np.ones(n), box * np.ones(n), np.zeros(P * n))
    return g


def _model_of(g, n, hms, box, mfev, fstdmin, p=0, f=None):
    """the model's device form in the state the device holds"""
    m = nm.Nshs(f, n, hms, [-box] * n, [box] * n, mfev, fstdmin, form="device")
    m.start(g.get_state("x", p).reshape(hms, n), fs=g.get_state("f", p))
    m.it, m.fev = int(g.get_state("it", p)[0]), int(g.get_state("fev", p)[0])
    return m


def _device_is_model(g, m, tag, p=0):
    _bits(g.get_state("x", p), m.x, tag + "x")
    _bits(g.get_state("f", p), m.fs, tag + "f")
    _bits(g.get_state("fstd", p), [m.fstd], tag + "fstd")
    got = [int(g.get_state(k, p)[0]) for k in ("ibest", "iworst", "wide", "it", "fev")]
    assert got == [m.ibest, m.iworst, int(m.wide), m.it, m.fev], (tag, got)
    _bits(g.get_state("fbest", p), [m.fs[m.ibest]], tag + "fbest")
    _bits(g.get_state("fworst", p), [m.fs[m.iworst]], tag + "fworst")


def _phases_against_model(g, m, tag, p=0):
    """one iteration phase by phase: every phase writes what the model makes of the state it read"""
    g.phase(0)
    m.generate(g.get_state("draws", p).reshape(m.n, 4))
    _bits(g.get_state("cand", p), m.cand, tag + "cand")
    g.phase(1)
    m.evaluate(g.get_state("fcand", p)[0])
    g.phase(2)
    m.replace()
    assert int(g.get_state("accepted", p)[0]) == int(m.accepted), tag
    _device_is_model(g, m, tag, p)


def _table(rng, n, every=3):
    """uniforms whose coin fails at every third coordinate (hmcr is at least 1/2)"""
    u = rng.random((n, 4))
    u[:, 0] = np.where(np.arange(n) % every == 0, 0.999999, 0.25 * u[:, 0])
    return u


# rows past one pass of a 256-thread workgroup: one live lane in the second pass (257), an odd n that
# is no multiple of 4 or 64 (301) and the cap, with the objective whose sum the walk then checks
WIDE_SHAPES = {(257, 5): "rosenbrock", (301, 6): "ellipsoid", (512, 8): "rosenbrock"}
CANDIDATE_SHAPES = [(n, hms) for hms in (1, 2, 3, 64, 65, 130) for n in (1, 2, 3, 63, 64, 65, 128, 130)]


@pytest.mark.parametrize("n,hms", CANDIDATE_SHAPES + sorted(WIDE_SHAPES))
def test_the_candidate_is_the_model_bit_for_bit(hip, n, hms):
    """wide (box 5, fstdmin 1e-4) and narrow (box 0.05, fstdmin 0.05: the sphere's values spread by
    less); hms = 1 is narrow whatever fstdmin is, and its column minimum is its maximum.  The first
    iteration takes the device's draws, the second a table whose coin fails at every third
    coordinate, so that the fresh value of either branch is drawn at any n; the third runs fused.
    Past n = 256 the box of 5 takes rosenbrock or the ellipsoid, the walk goes on for 12 iterations
    under the device's draws (phase by phase and fused in turn), and every candidate's value is the
    model's sum in the device's order (slpso_model.device_objective: eval_row_group<64>)."""
    rng = np.random.default_rng(1000 * n + hms)
    for box, fstdmin in ((5., 1e-4), (0.05, 0.05)):
        obj = WIDE_SHAPES[n, hms] if (n, hms) in WIDE_SHAPES and box == 5. else "sphere"
        g = _start(hip, n, hms, obj=obj, seed=100 * n + hms, fstdmin=fstdmin, box=box, record_draws=True)
        # a lane per coordinate up to 256: the walk runs the configuration its n is meant to reach
        assert int(g.get_state("wg")[0]) == (64 if n <= 128 else 128 if n <= 256 else 256)
        m = _model_of(g, n, hms, box, 10 ** 6, fstdmin)
        tag = "n %d hms %d box %g " % (n, hms, box)
        _device_is_model(g, m, tag + "init ")
        assert m.wide == (fstdmin < 1e-3 and hms > 1), tag
        # fstd against the reference's recurrence
        ref = nm.std_reference(m.fs)
        assert abs(m.fstd - ref) <= FSTD_BOUND * ref, (tag, m.fstd, ref)
        _phases_against_model(g, m, tag + "drawn ")
        u = _table(rng, n)
        g.inject_uniforms(u)
        _phases_against_model(g, m, tag + "injected ")
        _bits(g.get_state("draws"), u, tag + "the recorded draws are the injected ones")
        if hms == 1:
            assert not m.wide, tag
        assert g.run(1) == 1        # the same table, fused
        m.generate(u)
        _bits(g.get_state("cand"), m.cand, tag + "fused cand")
        m.evaluate(g.get_state("fcand")[0])
        m.replace()
        _device_is_model(g, m, tag + "fused ")
        if n <= 256:
            continue
        fobj = device_objective(obj, n)
        _bits(g.get_state("f"), [fobj(row) for row in m.x], tag + "the memory's values")
        g.inject_uniforms(None)
        for it in range(12):
            wtag = tag + "iteration %d " % (3 + it)
            if it % 2:
                _phases_against_model(g, m, wtag)
            else:
                assert g.run(1) == 1
                m.generate(g.get_state("draws").reshape(n, 4))
                _bits(g.get_state("cand"), m.cand, wtag + "fused cand")
                m.evaluate(g.get_state("fcand")[0])
                m.replace()
                _device_is_model(g, m, wtag + "fused ")
            _bits(g.get_state("fcand"), [fobj(m.cand)], wtag + "fcand")


@pytest.mark.parametrize("hms", [5, 65, 130])
def test_ties_go_to_the_lowest_row_and_an_equal_candidate_does_not_replace(hip, hms):
    """duplicated values set through set_state("f"); at hms = 65 and 130 the tied rows sit in
    different lanes and in different strides of one lane"""
    n = 3
    g = _start(hip, n, hms, obj="sphere", seed=hms)
    f = np.random.default_rng(hms).uniform(1., 2., hms)
    hi = {5: (1, 3), 65: (1, 64), 130: (2, 66, 129)}[hms]
    lo = {5: (2, 4), 65: (3, 64 - 1, 64 - 2), 130: (5, 69, 128)}[hms]
    f[list(hi)], f[list(lo)] = 3., 0.5
    x0, fev0 = g.get_state("x").copy(), int(g.get_state("fev")[0])
    g.set_state("f", f)
    _bits(g.get_state("f"), f, "f")
    _bits(g.get_state("x"), x0, "x stays")
    assert int(g.get_state("fev")[0]) == fev0                        # nothing was evaluated
    assert int(g.get_state("iworst")[0]) == hi[0] and int(g.get_state("ibest")[0]) == min(lo)
    assert float(g.get_state("fworst")[0]) == 3. and float(g.get_state("fbest")[0]) == 0.5
    _bits(g.get_state("fstd"), [nm.std_device(list(f))], "fstd")
    # a candidate EQUAL to the worst does not replace it (:159 is a strict <)
    g.phase(0)
    cand = g.get_state("cand").copy()
    g.set_state("fcand", [3.])
    g.phase(2)
    assert int(g.get_state("accepted")[0]) == 0 and int(g.get_state("iworst")[0]) == hi[0]
    _bits(g.get_state("f"), f, "f after the equal candidate")
    _bits(g.get_state("x"), x0, "x after the equal candidate")
    # one unit in the last place below it does, in the FIRST of the tied rows; the next is then the worst
    g.set_state("fcand", [np.nextafter(3., 0.)])
    g.phase(2)
    f[hi[0]] = np.nextafter(3., 0.)
    x0 = x0.reshape(hms, n)
    x0[hi[0]] = cand
    assert int(g.get_state("accepted")[0]) == 1 and int(g.get_state("iworst")[0]) == hi[1]
    _bits(g.get_state("f"), f, "f after the better candidate")
    _bits(g.get_state("x"), x0, "x after the better candidate")
    assert int(g.get_state("ibest")[0]) == min(lo) and int(g.get_state("it")[0]) == 2


@pytest.mark.parametrize("poll", [None, 5])
@pytest.mark.parametrize("k", [1, 2, 7, CHUNK, CHUNK + 1, 3 * CHUNK - 1])
def test_a_fused_run_is_as_many_iterations_one_by_one(hip, k, poll):
    """run(K) through nshs_steps against K iterate() calls through the three phase kernels, with
    the default chunk and with poll_every = 5, which divides none of these K"""
    n, hms, P = 9, 20, 3
    kw = {} if poll is None else {"poll_every": poll}
    a = _start(hip, n, hms, seed=5, P=P, record_draws=True)
    b = _start(hip, n, hms, seed=5, P=P, record_draws=True, **kw)
    assert int(b.get_state("chunk")[0]) == (CHUNK if poll is None else poll)
    for _ in range(k):
        a.iterate()
    assert b.run(k) == k
    for p in range(P):
        _same_state(_snapshot(a, p), _snapshot(b, p), "population %d " % p)
        _bits(a.get_state("draws", p), b.get_state("draws", p), "draws")
    assert int(b.get_state("it")[0]) == k and int(b.get_state("fev")[0]) == hms + k


@pytest.mark.parametrize("over", [0, 1])
def test_the_memory_in_global_memory_gives_the_bits_of_the_memory_in_lds(hip, over):
    """at the largest hms whose memory takes the LDS route at n = 128 and at the next one: the dbg
    bit, which makes nshs_steps gather from global memory, changes no bit; hm_in_lds reports the
    route; and the phase kernels agree with both"""
    n = 128
    hms = LDS_BYTES // (8 * n) + over
    runs = []
    for dbg in (0, 1, None):
        g = _start(hip, n, hms, seed=11)
        assert int(g.get_state("lds_bytes")[0]) == LDS_BYTES
        if dbg is None:
            for _ in range(40):
                g.iterate()
        else:
            g.set_state("dbg", [float(dbg)])
            assert int(g.get_state("hm_in_lds")[0]) == (1 if over == 0 and dbg == 0 else 0)
            assert g.run(40) == 40
        runs.append(_snapshot(g))
    assert runs[0]["accepted"].size == 1 and int(runs[0]["it"][0]) == 40
    _same_state(runs[0], runs[1], "forced global ")
    _same_state(runs[0], runs[2], "phases ")


def _sphere2(r):
    return r[0] * r[0] + r[1] * r[1]      # (the device's sum of two terms is this one addition)


def test_a_run_that_crosses_from_wide_to_narrow_is_the_model(hip):
    """sphere, n = 2, hms = 4, box 2, fstdmin = 0.3: the memory contracts and fstd falls through
    fstdmin.  60 iterations through nshs_steps, one per launch so that every iteration's draws can
    be read, against the model fed those draws; then the same 60 in one launch."""
    n, hms, box, fstdmin, its = 2, 4, 2., 0.3, 60
    g = _start(hip, n, hms, obj="sphere", seed=3, fstdmin=fstdmin, box=box, record_draws=True, poll_every=1)
    m = _model_of(g, n, hms, box, 10 ** 6, fstdmin, f=_sphere2)
    _bits(g.get_state("f"), [_sphere2(r) for r in m.x], "the model's objective is the device's")
    branches = []
    for it in range(its):
        branches.append(m.wide)
        assert int(g.get_state("wide")[0]) == int(m.wide)
        assert g.run(1) == 1
        m.iterate(g.get_state("draws").reshape(n, 4))
        _bits(g.get_state("cand"), m.cand, "cand %d" % it)
        _bits(g.get_state("fcand"), [m.fcand], "fcand %d" % it)
        _device_is_model(g, m, "iteration %d " % it)
    assert True in branches and False in branches, branches
    whole = _start(hip, n, hms, obj="sphere", seed=3, fstdmin=fstdmin, box=box)
    assert whole.run(its) == its
    _same_state(_snapshot(g), _snapshot(whole), "one launch ")


def test_the_budget_is_met_exactly_inside_a_launch(hip):
    n, hms = 4, 6
    lo, up, guess = -np.ones(n), np.ones(n), np.zeros(n)
    g = hip.NSHS(hms + 5, hms, seed=2, poll_every=4)
    g.initialize("sphere", lo, up, guess)
    assert g.run(100) == 8          # two launches of four: the second idles after one iteration
    assert int(g.get_state("fev")[0]) == hms + 5 and int(g.get_state("it")[0]) == 5
    assert int(g.get_state("flag")[0]) == 2 and g.solution().converged is False
    frozen = _snapshot(g)
    assert g.run(5) == 0            # `while (fev < mfev)`: nothing once the budget is spent
    _same_state(frozen, _snapshot(g))
    sol = hip.NSHS(hms + 5, hms, seed=2).optimize("sphere", lo, up, guess)
    assert sol.n_evals == hms + 5 and sol.converged is False
    _bits(sol.x, g.get_state("x").reshape(hms, n)[int(g.get_state("ibest")[0])], "x*")
    _bits(sol.x, g.get_state("xbest"), "xbest")
    _bits(g.solution().x, sol.x, "solution()")


@pytest.mark.parametrize("mfev", [6, 3])
def test_a_budget_the_memory_spends_leaves_no_iteration(hip, mfev):
    from bboptpy_amd import _ffi
    n, hms = 4, 6
    lo, up, guess = -np.ones(n), np.ones(n), np.zeros(n)
    g = hip.NSHS(mfev, hms, seed=2)
    g.initialize("sphere", lo, up, guess)          # the memory is evaluated
    x = g.get_state("x").reshape(hms, n)
    _bits(g.get_state("f"), [nm.tree_sum(list(r * r)) for r in x], "f")
    assert int(g.get_state("fev")[0]) == hms and g.run(10) == 0
    for call in (g.iterate, lambda: g.phase(0)):
        with pytest.raises(_ffi.BboError) as ei:
            call()
        assert ei.value.status == -2 and "mfev <= hms" in str(ei.value)
    sol = hip.NSHS(mfev, hms, seed=2).optimize("sphere", lo, up, guess)
    assert sol.n_evals == hms and sol.converged is False
    _bits(sol.x, x[int(g.get_state("ibest")[0])], "x*")


def test_population_zero_of_a_batch_is_the_single_run(hip):
    n, hms, P = 7, 20, 5
    one, many = _start(hip, n, hms, seed=33), _start(hip, n, hms, seed=33, P=P)
    assert one.run(30) == 30 and many.run(30) == 30
    _same_state(_snapshot(one), _snapshot(many))
    xs = [many.get_state("x", p).tobytes() for p in range(P)]
    cs = [many.get_state("cand", p).tobytes() for p in range(P)]
    assert len(set(xs)) == P and len(set(cs)) == P      # every population its own sub-stream


def test_more_workgroups_than_the_device_holds_at_once(hip):
    n, hms, P, its = 8, 4, 4100, 50
    g = hip.NSHS(hms + its, hms, seed=19, populations=P)
    g.initialize("rosenbrock", -2. * np.ones(n), 2. * np.ones(n), np.zeros(P * n))
    assert g.run(10 ** 6) == CHUNK
    assert all(int(g.get_state("fev", p)[0]) == hms + its for p in range(P))
    assert all(int(g.get_state("flag", p)[0]) == 2 for p in (0, 1, P // 2, P - 1))
    single = hip.NSHS(hms + its, hms, seed=19)
    single.initialize("rosenbrock", -2. * np.ones(n), 2. * np.ones(n), np.zeros(n))
    single.run(10 ** 6)
    _same_state(_snapshot(single), _snapshot(g, 0))


def _u01(lo, hi):
    return float(((hi << 32) | lo) >> 11) * 2. ** -53


def _draws_of(seed, p, n, it):
    from bboptpy_amd.distributed import philox4x32_10
    out = np.empty((n, 4))
    for i in range(n):
        w0 = philox4x32_10(seed, i, 0, it, (STREAM_NSHS << 24) | p)
        w1 = philox4x32_10(seed, i, 1, it, (STREAM_NSHS << 24) | p)
        out[i] = [_u01(w0[0], w0[1]), _u01(w0[2], w0[3]), _u01(w1[0], w1[1]), _u01(w1[2], w1[3])]
    return out


def _percoord_start(n, hms):
    from _boxes import percoord_box
    lo, up = percoord_box(n)
    # a memory spread over each coordinate's own interval
    X0 = lo + (up - lo) * np.random.default_rng(1000 * n + hms).random((hms, n))
    return lo, up, X0


def _percoord_model(n, hms, lo, up, X0, fs=None):
    m = nm.Nshs(device_objective("sphere", n), n, hms, lo, up, 10 ** 6, 1e-4, form="device")
    m.start(X0, fs=fs)
    return m


@pytest.mark.parametrize("n,hms", [(37, 6), (257, 5)])
def test_bounds_that_differ_in_every_coordinate_bind_and_the_walk_is_the_model(hip, n, hms):
    """tests/_boxes.py's box: nshs_coordinate's fresh value between lower[i] and upper[i], its bandwidth
    (upper[i] - lower[i]) / tunerange and its clamp read another pair of bounds in every coordinate, and tunerange
    is half the LARGEST width.  First the model alone, under the draws of the device's counters computed on the
    host (_draws_of): its candidates reach their lower bound, their upper bound and stay strictly inside, three
    coordinates of each at least.  Then the device from the same memory, phase by phase and fused in turn, bit
    for bit.  n = 37 is off every tile; 257 puts one live lane into the second pass."""
    from _boxes import binding_witness
    seed, its = 100 * n + hms, 10
    lo, up, X0 = _percoord_start(n, hms)
    w = _percoord_model(n, hms, lo, up, X0)
    cands = []
    for it in range(its):
        w.iterate(_draws_of(seed, 0, n, it))
        cands.append(np.array(w.cand))
    binding_witness(cands, lo, up)
    assert w.tunerange == ((up - lo) / 2.).max() and w.wide
    g = hip.NSHS(10 ** 6, hms, 1e-4, seed=seed, record_draws=True)
    g.initialize("sphere", lo, up, np.zeros(n))
    Xi = g.get_state("x").reshape(hms, n)
    assert (Xi >= lo).all() and (Xi <= up).all()        # the initial memory, coordinate by coordinate
    assert g.get_state("tunerange")[0] == w.tunerange
    g.set_state("x", X0)
    m = _percoord_model(n, hms, lo, up, X0, fs=g.get_state("f"))
    _device_is_model(g, m, "n %d start " % n)
    for it in range(its):
        tag = "n %d iteration %d " % (n, it)
        if it % 2:
            _phases_against_model(g, m, tag)
        else:
            assert g.run(1) == 1
            m.generate(g.get_state("draws").reshape(n, 4))
            _bits(g.get_state("cand"), m.cand, tag + "fused cand")
            m.evaluate(g.get_state("fcand")[0])
            m.replace()
            _device_is_model(g, m, tag + "fused ")
        _bits(g.get_state("draws"), _draws_of(seed, 0, n, it), tag + "draws")
        c = g.get_state("cand")
        assert (c >= lo).all() and (c <= up).all()


def test_recorded_draws_are_their_counters_and_injecting_them_repeats_the_iteration(hip):
    """the draws are keyed by (coordinate, block, iteration, stream | population) and by nothing
    else: the fused kernel, the phase kernels and a batch record the same uniforms.  Injected into
    another handle (another seed, the same memory) they reproduce the iteration bit for bit."""
    n, hms, P, seed = 5, 9, 2, 77
    g = _start(hip, n, hms, seed=seed, P=P)
    with pytest.raises(Exception):
        g.get_state("draws")
    g.set_state("record_draws", [1.])
    other = _start(hip, n, hms, seed=seed + 1, P=P)
    for it in range(4):
        before = [g.get_state("x", p).copy() for p in range(P)]
        if it % 2:
            g.iterate()
        else:
            assert g.run(1) == 1
        for p in range(P):
            _bits(g.get_state("draws", p), _draws_of(seed, p, n, it), "draws of iteration %d" % it)
            other.set_state("x", before[p], p)
            other.set_state("it", [float(it)], p)
        other.inject_uniforms(np.stack([g.get_state("draws", p).reshape(n, 4) for p in range(P)]))
        if it % 2:
            assert other.run(1) == 1
        else:
            other.iterate()
        for p in range(P):
            sa, sb = _snapshot(g, p), _snapshot(other, p)
            for k in ("x", "f", "cand", "fcand", "fstd", "ibest", "iworst", "wide", "accepted", "it"):
                _bits(sa[k], sb[k], "iteration %d population %d %s" % (it, p, k))
    other.set_state("record_draws", [1.])
    other.inject_uniforms(None)         # back on the device generator
    other.iterate()
    _bits(other.get_state("draws", 1), _draws_of(seed + 1, 1, n, 4), "the generator's draws")


def test_a_host_callable_is_the_builtin_and_is_called_fev_times(hip):
    """n = 1 sphere: x * x is exact on both sides, so 50 iterations agree bit for bit"""
    lo, up, guess = -3. * np.ones(1), 3. * np.ones(1), np.zeros(1)
    calls = []

    def sphere(x):
        calls.append(1)
        return float(x[0] * x[0])

    runs = []
    for obj in ("sphere", sphere):
        g = hip.NSHS(10 ** 6, 5, seed=13)
        g.initialize(obj, lo, up, guess)
        assert g.run(50) == 50
        runs.append(_snapshot(g))
    _same_state(runs[0], runs[1])
    assert len(calls) == int(runs[1]["fev"][0]) == 55
    del calls[:]
    sol = hip.NSHS(40, 5, seed=13).optimize(sphere, lo, up, guess)
    assert sol.n_evals == len(calls) == 40 and not sol.converged


def test_set_state_x_reevaluates_and_reselects(hip):
    n, hms = 4, 70
    g = _start(hip, n, hms, obj="sphere", seed=3)
    x = np.random.default_rng(5).uniform(1., 4., (hms, n))
    x[66] = x[9] = [0.5, -0.25, 0.125, 0.]
    x[40] = -x[9]                   # the same value from another point
    x[65] = x[12] = [4.5, 4.5, 4.5, 4.5]
    g.set_state("x", x)
    assert int(g.get_state("ibest")[0]) == 9 and int(g.get_state("iworst")[0]) == 12
    assert int(g.get_state("fev")[0]) == hms and int(g.get_state("it")[0]) == 0
    _bits(g.get_state("xbest"), x[9], "xbest")
    _bits(g.get_state("f")[[9, 40, 66]], [x[9] @ x[9]] * 3, "the tied values")
    _bits(g.get_state("fstd"), [nm.std_device(list(g.get_state("f")))], "fstd")
    # a NaN value ranks last, and an inf among the values is the narrow branch
    lo, up = -np.ones(2), np.ones(2)
    nan = hip.NSHS(1000, 20, seed=4)
    nan.initialize(lambda v: float("nan") if v[0] > 0. else float(v @ v), lo, up, np.zeros(2))
    f = nan.get_state("f")
    assert np.isinf(f).any() and not np.isnan(f).any() and np.isfinite(f[int(nan.get_state("ibest")[0])])
    assert np.isnan(nan.get_state("fstd")[0]) and int(nan.get_state("wide")[0]) == 0
    assert np.isinf(nan.get_state("fworst")[0]) and int(nan.get_state("iworst")[0]) == int(np.argmax(f))


@pytest.mark.parametrize("obj", ["sphere", "rosenbrock"])
def test_outcome_bands_match_the_reference(hip, obj):
    b, P = GOLD["bands"], 64
    n = b["n"]
    g = hip.NSHS(b["mfev"], b["hms"], b["fstdmin"], seed=2024, populations=P)
    g.initialize(obj, -b["box"] * np.ones(n), b["box"] * np.ones(n), np.zeros(P * n))
    g.run(10 ** 6)
    got = [float(g.get_state("fbest", p)[0]) for p in range(P)]
    assert all(int(g.get_state("fev", p)[0]) == b["mfev"] for p in range(P))
    band(got, _h(b[obj]), obj + " device")


def test_configure_statuses_and_refusals(hip):
    from bboptpy_amd import _ffi
    L = _ffi.lib()
    d = _ffi.NshsParams()
    L.bbo_nshs_params_default(C.byref(d))
    other = hip.DSA(1000, 1e-6, 1e-6, 12, seed=1)
    oh = other._ensure_handle()
    assert L.bbo_nshs_configure(oh, C.byref(d)) == _ffi.ERR_ARG
    assert "not an NSHS handle" in L.bbo_last_error(oh).decode()
    assert L.bbo_nshs_phase(oh, 0) == _ffi.ERR_ARG and L.bbo_nshs_inject_uniforms(oh, None, 0) == _ffi.ERR_ARG
    g = hip.NSHS(1000, 20, seed=1)
    h = g._ensure_handle()
    assert L.bbo_nshs_configure(h, C.byref(d)) == 0
    assert L.bbo_nshs_configure(h, None) == _ffi.ERR_ARG
    for value in (float("nan"), float("inf"), -1e-9):
        bad = _ffi.NshsParams()
        bad.fstdmin = value
        assert L.bbo_nshs_configure(h, C.byref(bad)) == _ffi.ERR_ARG and "fstdmin" in L.bbo_last_error(h).decode()
    d.fstdmin = 0.
    assert L.bbo_nshs_configure(h, C.byref(d)) == 0             # zero is legal
    d.fstdmin = 0.0001
    assert L.bbo_nshs_configure(h, C.byref(d)) == 0
    assert L.bbo_nshs_phase(h, 0) == -2                         # BBO_ERR_STATE: before bbo_init
    n = 2
    lo, up = -np.ones(n), np.ones(n)
    # the limits, each named
    with pytest.raises(_ffi.BboError) as ei:
        hip.NSHS(1000, 5).initialize("sphere", -np.ones(513), np.ones(513), np.zeros(513))
    assert ei.value.status == _ffi.ERR_ARG and "512" in str(ei.value)
    for hms in (0, 4097):
        with pytest.raises(_ffi.BboError) as ei:
            hip.NSHS(1000, hms).initialize("sphere", lo, up, np.zeros(n))
        assert ei.value.status == _ffi.ERR_ARG and "4096" in str(ei.value)
    with pytest.raises(_ffi.BboError) as ei:
        hip.NSHS(1000, 5).initialize("sphere", lo, np.array([1., np.inf]), np.zeros(n))
    assert ei.value.status == _ffi.ERR_ARG and "finite" in str(ei.value)
    big = hip.NSHS(5000, 4096, seed=3)                          # the largest memory: the global route
    big.initialize("sphere", -np.ones(512), np.ones(512), np.zeros(512))
    assert int(big.get_state("hm_in_lds")[0]) == 0 and int(big.get_state("wg")[0]) == 256
    assert big.run(3) == 3 and int(big.get_state("fev")[0]) == 4099
    # an objective program: refused by the class and by the library, naming who takes one
    prog = hip.DeviceObjective('extern "C" __device__ double bbo_user_objective(const double *x, int n, '
                               'const double *data) { return x[0] * x[0]; }')
    with pytest.raises(ValueError) as ei:
        g.initialize(prog, lo, up, np.zeros(n))
    assert "NSHS does not take a DeviceObjective" in str(ei.value) and "JADE" in str(ei.value)
    ob = _ffi.Objective()
    ob.kind, ob.user = _ffi.OBJ_PROGRAM, prog._handle
    st = L.bbo_init(h, n, lo, up, np.zeros(n), C.byref(ob))
    msg = L.bbo_last_error(h).decode()
    assert st == -1 and "NSHS" in msg and "CMAES" in msg and "SHADE" in msg, (st, msg)
    g.initialize("sphere", lo, up, np.zeros(n))
    assert L.bbo_nshs_configure(h, C.byref(d)) == -2            # BBO_ERR_STATE
    assert "after bbo_init" in L.bbo_last_error(h).decode()
    assert L.bbo_nshs_phase(h, 3) == _ffi.ERR_ARG and L.bbo_nshs_phase(h, -1) == _ffi.ERR_ARG
    with pytest.raises(_ffi.BboError):                          # one table per population, n x 4
        g.inject_uniforms(np.zeros(3))
    with pytest.raises(_ffi.BboError):                          # [0, 1)
        g.inject_uniforms(np.ones((n, 4)))
    for key, val in (("wg", 32.), ("dbg", 2.), ("x", np.zeros(3)), ("f", np.zeros(3)), ("fev", -1.), ("ibest", 0.)):
        with pytest.raises(_ffi.BboError):
            g.set_state(key, val)
    with pytest.raises(_ffi.BboError) as ei:
        g.get_state("draws")
    assert ei.value.status == -2
    with pytest.raises(_ffi.BboError) as ei:
        g.get_state("sigma")
    assert ei.value.status == -6
    assert g.get_state("fstdmin")[0] == 0.0001 and g.get_state("hmcr")[0] == 1.0 - 1.0 / 3 and g.get_state("mit")[0] == 980
    # one profile slot per kernel: init, generate, evaluate, replace, steps (ms, calls each)
    g.set_state("profile", [1.])
    g.iterate()
    g.run(3)
    prof = g.get_state("profile")
    assert prof.size == 10 and list(prof[1::2]) == [0., 1., 1., 1., 1.] and (prof[2::2] > 0.).all()
    # NSHS is no base of a restart driver
    p = _ffi.default_params(_ffi.ALGO_IPOP)
    p.mfev, p.np = 1000, 8
    out = C.c_void_p()
    fn = C.CDLL(_ffi.LIB_PATH).bbo_create_restart
    fn.argtypes, fn.restype = [C.c_void_p, C.c_void_p, C.c_void_p], C.c_int
    assert fn(C.byref(p), h, C.byref(out)) == _ffi.ERR_ARG and not out.value
    assert "CMA-ES handle" in L.bbo_last_error(None).decode()
