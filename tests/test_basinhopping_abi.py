"""CPU checks of BasinHopping at the drop-in boundary: the three classes against tests/golden/class_surface.json,
bbo_bh_params_default, the entry points that need no handle, bbo_bh_draws against the oracle's Philox, and the
arguments the classes refuse before a handle exists."""
import ctypes as C
import inspect
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ("BasinHopping", "BasinHopping_StepStrategy", "BasinHopping_AdaptStrategy")
SYMBOLS = ("bbo_bh_params_default", "bbo_create_basin", "bbo_bh_configure", "bbo_bh_phase", "bbo_bh_inject_draws",
           "bbo_bh_draws")
STREAM_BH_STEP, STREAM_BH_ACCEPT = 47, 48       # bbo_rng.hpp


def _surface():
    with open(os.path.join(ROOT, "tests", "golden", "class_surface.json")) as fh:
        return json.load(fh)["classes"]


def _nm(bb, **kw):
    return bb.NelderMead(400, 1e-8, 0.5, **kw)


def test_algorithm_number_header_and_symbols():
    import bboptpy_amd as bb
    from bboptpy_amd import _ffi
    assert bb.BasinHopping._algo == _ffi.ALGO_BASIN_HOPPING == 28
    text = open(os.path.join(ROOT, "include", "bbopt_hip.h")).read()
    assert "BBO_ALGO_BASIN_HOPPING = 28" in text and "bbo_bh_params;" in text
    raw = C.CDLL(_ffi.LIB_PATH)
    for name in SYMBOLS:
        assert name in text and name in _ffi.EXPORTED_SYMBOLS and hasattr(raw, name)
    p = _ffi.default_params(_ffi.ALGO_BASIN_HOPPING)
    assert (p.algo, p.populations, p.poll_every) == (28, 1, 0)
    assert (_ffi.BH_PHASE_STEP, _ffi.BH_PHASE_COLLECT, _ffi.BH_PHASE_EVALUATE, _ffi.BH_PHASE_DECIDE) == (0, 1, 2, 3)
    assert _ffi.EXTENSIONS["bh"][:2] == (_ffi.BhParams, True) and list(_ffi.EXTENSIONS["bh"][2]) == ["draws"]


def test_the_layout_of_bbo_params_is_untouched():
    from bboptpy_amd import _ffi
    # (the values of the commit before BasinHopping: its arguments travel in bbo_bh_params, none in bbo_params)
    assert C.sizeof(_ffi.Params) == 288 and _ffi.Params.stol.offset == 272 and _ffi.Params.seed.offset == 136
    assert _ffi.Params.ranked.offset == 280 and _ffi.Params._fields_[-1][0] == "ranked"
    assert _ffi.Params.populations.offset == 148 and _ffi.Params.poll_every.offset == 152


def test_bh_params_default_and_the_statuses_that_need_no_handle():
    from bboptpy_amd import _ffi
    L = _ffi.lib()
    d = _ffi.BhParams()
    C.memset(C.byref(d), 0xA5, C.sizeof(d))
    L.bbo_bh_params_default(C.byref(d))
    assert (d.stepsize, d.adaptive, d.accept_rate, d.interval, d.factor, d.temp) == (1., 1, 0.5, 5, 0.9, 1.)
    assert (d.mit, d.print, d.lockstep, d.substream, d.nstep0, d.naccept0) == (99, 1, -1, 0, 0, 0)
    assert C.sizeof(_ffi.BhParams) == 72
    L.bbo_bh_params_default(None)       # tolerated
    assert L.bbo_bh_configure(None, C.byref(d)) == _ffi.ERR_ARG
    assert L.bbo_bh_phase(None, 0) == _ffi.ERR_ARG
    assert L.bbo_bh_inject_draws(None, None, 0) == _ffi.ERR_ARG
    # no minimiser handle: refused before anything is made
    p, h = _ffi.default_params(_ffi.ALGO_BASIN_HOPPING), C.c_void_p()
    assert L.bbo_create_basin(C.byref(p), None, C.byref(h)) == _ffi.ERR_ARG and not h.value
    assert b"bbo_create_basin" in L.bbo_last_error(None)
    out = np.zeros(4)
    for bad in ((1, -1, 0, 3), (1, 0, -1, 3), (1, 0, 0, 0), (1, 0, 0, 129), (1, 1 << 24, 0, 3)):
        assert L.bbo_bh_draws(*bad, np.zeros(130)) == _ffi.ERR_ARG
    assert L.bbo_bh_draws(1, 0, 0, 3, out) == 0


def test_the_draws_are_the_oracles_philox_at_their_address(oracle_lib):
    import bboptpy_amd as bb
    from bboptpy_amd.distributed import philox4x32_10
    out = (C.c_uint32 * 4)()

    def u01(w):
        return (((w[1] << 32) | w[0]) >> 11) * 2. ** -53

    for seed, sub, hop, n in ((0x9E3779B97F4A7C15, 0, 0, 1), (7, 3, 2, 5), (2 ** 64 - 1, (1 << 24) - 1, 99, 128)):
        got = bb.BasinHopping.draws(seed, sub, hop, n)
        assert got.shape == (n + 1,)
        for j in range(n):
            oracle_lib.f("philox")(seed, j, 0, hop, (STREAM_BH_STEP << 24) | sub, out)
            assert tuple(out) == philox4x32_10(seed, j, 0, hop, (STREAM_BH_STEP << 24) | sub)
            assert got[j] == u01(tuple(out)) * 2. - 1. and -1. <= got[j] < 1.
        oracle_lib.f("philox")(seed, 0, 0, hop, (STREAM_BH_ACCEPT << 24) | sub, out)
        assert got[n] == u01(tuple(out)) and 0. <= got[n] < 1.
    # the address is (seed, substream, hop, coordinate): a longer n only adds coordinates
    a, b = bb.BasinHopping.draws(5, 1, 4, 3), bb.BasinHopping.draws(5, 1, 4, 9)
    assert (a[:3] == b[:3]).all() and a[3] == b[9]
    assert (bb.BasinHopping.draws(5, 2, 4, 3) != a).all() and (bb.BasinHopping.draws(5, 1, 5, 3) != a).all()


def test_class_surface_matches_the_reference():
    """names, order, defaults, bases and **ext of the three classes: the logic of tests/test_abi.py"""
    import bboptpy_amd as bb
    surf = _surface()
    E = inspect.Parameter.empty
    for name in CLASSES:
        cls, ref = getattr(bb, name), surf[name]
        assert name in bb.__all__
        ps = inspect.signature(cls.__init__).parameters
        mine = [(k, v.default) for k, v in ps.items() if k not in ("self", "ext")]
        want = [(kw["name"], E if kw["required"] else kw["default"]) for kw in ref["init"]["keywords"]]
        assert [k for k, _ in mine] == [k for k, _ in want], name
        for (k, got), (_, exp) in zip(mine, want):
            assert (got is E) == (exp is E), (name, k)
            if exp is not E:
                assert got == exp and type(got) is type(exp), (name, k, got, exp)
        if ref["base"] is None:
            assert cls.__mro__[1] is object, name
        else:
            assert getattr(bb, ref["base"]) in cls.__mro__[1:], name
    ps = inspect.signature(bb.BasinHopping.__init__).parameters
    assert any(v.kind is inspect.Parameter.VAR_KEYWORD for v in ps.values())
    with pytest.raises(TypeError):
        bb.BasinHopping(_nm(bb), bb.BasinHopping_StepStrategy(0.1), True, 9, 1., True)
    with pytest.raises(TypeError):
        bb.BasinHopping(_nm(bb), bb.BasinHopping_StepStrategy(0.1), np=7)
    with pytest.raises(TypeError):
        bb.BasinHopping_StepStrategy()
    for name in ("optimize", "initialize", "iterate", "solution", "run", "phase", "inject_draws", "draws"):
        assert callable(getattr(bb.BasinHopping, name))
    assert bb.BasinHopping._accepts_program is False


def test_constructor_marshals_the_strategy_and_both_structs():
    import bboptpy_amd as bb
    st = bb.BasinHopping_AdaptStrategy(0.3, 0.4, 3, 0.8)
    st.nstep, st.naccept = 6, 2
    b = bb.BasinHopping(_nm(bb, populations=3), st, False, 8, 0.5, seed=9, poll_every=2, lockstep=True, substream=5)
    p, s = b._params, b._bh
    assert (p.algo, p.seed, p.populations, p.poll_every) == (28, 9, 3, 2)       # populations: the minimiser's
    assert (s.stepsize, s.adaptive, s.accept_rate, s.interval, s.factor, s.temp) == (0.3, 1, 0.4, 3, 0.8, 0.5)
    assert (s.mit, s.print, s.lockstep, s.substream, s.nstep0, s.naccept0) == (8, 0, 1, 5, 6, 2)
    s = bb.BasinHopping(bb.Rosenbrock(400, 1e-6, 0.5), bb.BasinHopping_StepStrategy(0.1))._bh
    assert (s.stepsize, s.adaptive, s.mit, s.print, s.temp, s.lockstep) == (0.1, 0, 99, 1, 1., -1)
    assert bb.BasinHopping(_nm(bb), st, lockstep=False)._bh.lockstep == 0
    assert b._native is True and bb.BasinHopping(_nm(bb), st, native=False)._native is False
    d = bb.BasinHopping_AdaptStrategy()
    assert (d.stepsize, d.accept_rate, d.interval, d.factor, d.nstep, d.naccept) == (1., 0.5, 5, 0.9, 0, 0)


def test_invalid_arguments_are_refused():
    import bboptpy_amd as bb
    BH, plain = bb.BasinHopping, bb.BasinHopping_StepStrategy(0.1)
    with pytest.raises(ValueError, match="interval must be >= 1"):
        bb.BasinHopping_AdaptStrategy(interval=0)
    for factor in (0., -0.5, np.inf, np.nan):
        with pytest.raises(ValueError, match="factor must be finite and positive"):
            bb.BasinHopping_AdaptStrategy(factor=factor)
    for temp in (-1., np.nan):
        with pytest.raises(ValueError, match="temp must be >= 0"):
            BH(_nm(bb), plain, temp=temp)
    with pytest.raises(ValueError, match="mit must be >= 0"):
        BH(_nm(bb), plain, mit=-1)
    BH(_nm(bb), plain, mit=0, temp=0.)
    with pytest.raises(ValueError, match="as many populations as there are chains"):
        BH(_nm(bb, populations=2), plain, populations=3)
    with pytest.raises(ValueError, match=r"NelderMead\(minit=random\) draws its simplex by the restart count alone"):
        BH(bb.NelderMead(400, 1e-8, 0.5, bb.NelderMead.random), plain)
    with pytest.raises(TypeError, match="stepstrat must be"):
        BH(_nm(bb), 0.1)
    BH(bb.NelderMead(400, 1e-8, 0.5, bb.NelderMead.random), plain, native=False)       # the Python-driven path takes it
    with pytest.raises(TypeError, match="minimizer must have optimize"):
        BH(object(), plain)

    class Foreign:
        def optimize(self, f, lower, upper, guess):
            return bb.MultivariateSolution(guess, 0, False)

    assert BH(bb.CRS(1000, 20, 1e-8), plain)._native is False and BH(Foreign(), plain)._native is False
    with pytest.raises(ValueError, match="only NelderMead and Rosenbrock of this package are native"):
        BH(Foreign(), plain, native=True)
    with pytest.raises(ValueError, match="the Python-driven path holds one population"):
        BH(Foreign(), plain, populations=2)
    with pytest.raises(ValueError, match="the bounds must be finite"):
        BH(Foreign(), plain, print=False).initialize(lambda x: 0., np.full(3, -np.inf), np.ones(3), np.zeros(3))
    for lo, up in ((np.full(3, -np.inf), np.ones(3)), (-np.ones(3), np.array([1., np.inf, 1.])), (np.full(3, np.nan), np.ones(3))):
        with pytest.raises(ValueError, match="BasinHopping: a step is a fraction of upper - lower: the bounds must be finite"):
            BH(_nm(bb), plain)._problem("sphere", lo, up, np.zeros(3))
    with pytest.raises(ValueError, match=r"BasinHopping: dimension must be in \[1, 128\]"):
        BH(_nm(bb), plain)._problem("sphere", -np.ones(129), np.ones(129), np.zeros(129))

    class Fake(bb.DeviceObjective):
        def __init__(self):
            self._handle = None

        def __del__(self):
            pass

    with pytest.raises(ValueError, match="BasinHopping does not take a DeviceObjective yet"):
        BH(_nm(bb), plain)._problem(Fake(), -np.ones(3), np.ones(3), np.zeros(3))


def test_the_python_driven_path_runs_a_foreign_minimizer_without_a_device(capsys):
    """the chain's arithmetic in Python on the draws of bbo_bh_draws: a minimiser that returns its start makes the
    chain a plain Metropolis walk, which tests/basinhopping_model.py walks too"""
    import bboptpy_amd as bb
    import basinhopping_model as bm
    import _tabular

    def f(x):
        return float(np.sum(np.asarray(x) ** 2))

    class Stay:
        def optimize(self, f, lower, upper, guess):
            return bb.MultivariateSolution(guess, 3, True)

    n, seed, mit = 3, 11, 6
    lo, up, guess = -2. * np.ones(n), 2. * np.ones(n), np.array([1., -1., 0.5])
    st = bb.BasinHopping_AdaptStrategy(0.2, 0.5, 2, 0.9)
    b = bb.BasinHopping(Stay(), st, True, mit, 0.5, seed=seed, substream=4)
    with pytest.raises(RuntimeError, match="run\\(\\) needs a device-resident minimizer"):
        b.run(1)
    sol = b.optimize(f, lo, up, guess)
    ms = bm.Strategy(0.2, 0.5, 2, 0.9)
    m = bm.Model(f, lo, up, lambda start: (list(start), 3, True), ms, mit, 0.5)
    m.optimize(guess, [list(bb.BasinHopping.draws(seed, 4, hop, n)) for hop in range(mit)])
    log = b.get_state("log").reshape(-1, 7)
    assert log.shape == (mit + 1, 7)
    for row, r in zip(log, m.rows):
        assert row.tolist() == [r["it"], r["f"], r["conv"], r["step"], r["accept"], r["fbest"], r["fev"]]
    assert b.get_state("log_start").reshape(-1, n).tolist() == [r["start"] for r in m.rows]
    assert sol.x.tolist() == m.xbest and sol.n_evals == m.fev == 4 * (mit + 1) and sol.converged is False
    assert (st.stepsize, st.nstep, st.naccept) == (ms.stepsize, ms.nstep, ms.naccept) and st.nstep == mit
    assert int(b.get_state("flag")[0]) == 2 and int(b.get_state("it")[0]) == mit
    out = capsys.readouterr().out.splitlines()
    W = [5, 25, 5, 25, 6, 25, 10]
    want = [_tabular.fmt_row(["it", "f", "conv", "step", "accept", "f*", "fev"], W), _tabular.rule(W)]
    want += [_tabular.fmt_row([r["it"], r["f"], r["conv"], r["step"], r["accept"], r["fbest"], r["fev"]], W) for r in m.rows]
    assert out == want


def test_no_device_no_run():
    """without a GPU the native class raises BBO_ERR_NO_DEVICE: there is no CPU path and no quiet fall-back"""
    import bboptpy_amd as bb
    from bboptpy_amd import _ffi
    if _ffi.lib().bbo_device_count() > 0:
        return
    for minimizer in (_nm(bb), bb.Rosenbrock(400, 1e-6, 0.5)):
        b = bb.BasinHopping(minimizer, bb.BasinHopping_AdaptStrategy(), False, 3)
        with pytest.raises(_ffi.BboError) as ei:
            b.optimize(bb.objectives.sphere, -np.ones(4), np.ones(4), np.zeros(4))
        assert ei.value.status == -4 and b._py is None
