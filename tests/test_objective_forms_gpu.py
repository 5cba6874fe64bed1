"""GPU: every device statement of the ten built-in objectives, and the product's host statement,
against the extended-precision reference of objective_reference.py -- each value inside the
a-priori rounding bound derived there (the bound is not fitted to the device).

    the forms, through bbo_probe_objective (bbo_probe.hip): eval_row_group<16> from LDS, <64> from a
        global row with an even stride, <64> from a swizzled LDS row, <16> unrolled by four, and
        eval_frag_rows<8> on the accumulator layout; whatever lies behind a row's n coordinates is
        1e300 (in the accumulator form too: its masks, not its callers' zeroed padding, are held), so
        a term that reads column n is no rounding.  Every objective the form offers, every input family, 8 rows, the n at which
        a lane group is partly filled, exactly filled and wraps.
    exact expectations: zeros give 0 where the function is a sum of terms that vanish (and n - 1 for
        Rosenbrock, a sum of ones), Rastrigin needs cos_2pi(0) == 1, Griewank cos(0) == 1; ones give
        Rosenbrock 0.
    across the forms of one objective the values agree to twice the bound.
    bbo_cma_evaluate: builtin_objective_host, the one point the restart drivers, CCPSO's local search
        and AMALGAM evaluate on the host -- with cos_2pi it holds on `large` as the kernels do
        (std::cos(2 pi x), which it called before, returned the cosine of a rounded product: Ackley
        was off by up to e - 1/e there).
    the call sites: every optimizer class, every objective, the points its handle exposes against
        the values it exposes next to them (SITES below)."""
import numpy as np
import pytest

import objective_reference as R

ROWS = 8
FORM_NAMES = {0: "row_group<16>/LDS", 1: "row_group<64>/global", 2: "row_group<64>/swizzled",
              3: "row_group<16>/unroll4", 4: "frag_rows<8>"}
NS_16 = (1, 2, 3, 15, 16, 17, 31, 33, 127, 128)
NS_64 = (1, 2, 63, 64, 65, 129, 130, 513)
FORM_NS = {0: NS_16, 1: NS_64, 2: NS_64, 3: NS_16, 4: NS_16}
ZERO_AT_ZEROS = ("sphere", "ellipsoid", "cigar", "discus", "diffpow", "schwefel12", "rastrigin", "griewank")


def form_objectives(form):
    return R.FRAG_OBJECTIVES if form == 4 else R.OBJECTIVES


_POINTS, _DEVICE = {}, {}


def points(n):
    """X[families * ROWS, n]: the rows of every family, in the order of R.FAMILIES"""
    if n not in _POINTS:
        _POINTS[n] = np.concatenate([R.family_rows(name, n, ROWS) for name in R.FAMILIES])
    return _POINTS[n]


def device_values(hip, form, n):
    """{objective: f[families * ROWS]} of one form at one n: one probe call per objective, once"""
    from bboptpy_amd import _ffi
    if (form, n) not in _DEVICE:
        _DEVICE[form, n] = {obj: _ffi.probe_objective(obj, form, points(n)) for obj in form_objectives(form)}
    return _DEVICE[form, n]


def ratios(obj, n, values):
    """error / bound of values[families * ROWS] against the reference, and the bounds"""
    X = points(n)
    ref = [R.reference_at(obj, x) for x in X]
    return (np.array([R.ratio(v, f, b) for v, (f, b) in zip(values, ref)]),
            np.array([b for _, b in ref]))


@pytest.mark.gpu
@pytest.mark.parametrize("form,n", [(form, n) for form in sorted(FORM_NS) for n in FORM_NS[form]])
def test_every_form_inside_the_bound(hip, form, n):
    got = device_values(hip, form, n)
    X = points(n)
    line = []
    for obj in form_objectives(form):
        r, _ = ratios(obj, n, got[obj])
        worst = int(np.argmax(r))
        line.append("%s %.3f" % (obj, r[worst]))
        assert r[worst] <= 1., "%s, %s, n = %d, family %s row %d: device %r is %.4g bounds from the reference" % (
            FORM_NAMES[form], obj, n, R.FAMILIES[worst // ROWS], worst % ROWS, got[obj][worst], r[worst])
        # the exact expectations
        z = slice(R.FAMILIES.index("zeros") * ROWS, (R.FAMILIES.index("zeros") + 1) * ROWS)
        o = slice(R.FAMILIES.index("ones") * ROWS, (R.FAMILIES.index("ones") + 1) * ROWS)
        assert not X[z].any() and (X[o] == 1.).all()
        if obj in ZERO_AT_ZEROS:
            assert (got[obj][z] == 0.).all(), (FORM_NAMES[form], obj, n, got[obj][z])
        if obj == "rosenbrock":
            assert (got[obj][z] == n - 1.).all() and (got[obj][o] == 0.).all(), (FORM_NAMES[form], n)
    print("RATIO form %d (%s) n = %d: %s" % (form, FORM_NAMES[form], n, "  ".join(line)))


@pytest.mark.gpu
@pytest.mark.parametrize("n", sorted(set(NS_16) & set(NS_64)) + [17, 128, 65, 513])
def test_the_forms_agree_with_each_other(hip, n):
    """the forms that take this n, pairwise: each inside its bound, so no two further apart than twice it"""
    forms = [form for form in sorted(FORM_NS) if n in FORM_NS[form]]
    assert len(forms) >= 2
    for obj in R.OBJECTIVES:
        have = [form for form in forms if obj in form_objectives(form)]
        vals = {form: device_values(hip, form, n)[obj] for form in have}
        bounds = None
        for form in have:
            r, bounds = ratios(obj, n, vals[form])
            assert (r <= 1.).all(), (FORM_NAMES[form], obj, n)
        for a in have:
            for b in have:
                if a < b:
                    d = np.abs(vals[a] - vals[b])
                    assert (d <= 2. * bounds).all(), "%s and %s differ on %s at n = %d by %.3g bounds" % (
                        FORM_NAMES[a], FORM_NAMES[b], obj, n, (d / bounds).max())


@pytest.mark.gpu
def test_the_probe_refuses_what_a_form_does_not_offer(hip):
    from bboptpy_amd import _ffi
    x = np.zeros((1, 4))
    for obj in ("rastrigin", "ackley", "griewank", "diffpow"):
        with pytest.raises(_ffi.BboError) as e:
            _ffi.probe_objective(obj, 4, x)
        assert e.value.status == _ffi.ERR_ARG
    for bad in (lambda: _ffi.probe_objective("sphere", 4, np.zeros((1, 129))),
                lambda: _ffi.probe_objective("sphere", 5, x),
                lambda: _ffi.probe_objective(10, 0, x),
                lambda: _ffi.probe_objective("sphere", 0, np.zeros((1, 1025)))):
        with pytest.raises(_ffi.BboError) as e:
            bad()
        assert e.value.status == _ffi.ERR_ARG


# ---- the product's host statement ---------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 17, 65, 130])
def test_cma_evaluate_inside_the_bound(hip, n):
    """bbo_cma_evaluate = builtin_objective_host at one point, every objective and family (`large` too).
    With std::cos(2 pi x) in place of cos_2pi the same formula, restated with libm on the host, put Ackley
    1.2e14 bounds off on `large` and 239 bounds off on `parabola` (|x| up to 1e6); Rastrigin stayed inside
    (0.13): its x^2 terms carry the bound where the cosine is lost."""
    lo, up = -10. * np.ones(n), 10. * np.ones(n)
    line = []
    for obj in R.OBJECTIVES:
        g = hip.CMAES(mfev=1000, tol=1e-12, np=8, seed=1)
        g.initialize(getattr(hip.objectives, obj), lo, up, np.zeros(n))
        worst = 0.
        for name in R.FAMILIES:
            for seed in range(2):
                x = R.family(name, n, seed)
                f_ref, bound = R.reference_at(obj, x)
                got = g.evaluate(x)
                r = R.ratio(got, f_ref, bound)
                worst = max(worst, r)
                assert r <= 1., "bbo_cma_evaluate, %s on %s, n = %d, seed %d: %r is %.4g bounds from the reference" % (
                    obj, name, n, seed, got, r)
        line.append("%s %.3f" % (obj, worst))
    print("RATIO host n = %d: %s" % (n, "  ".join(line)))


@pytest.mark.gpu
def test_cma_evaluate_of_a_point_that_is_not_finite(hip):
    """cos_2pi on the host: NaN for a NaN or infinite coordinate (as std::cos gave), not a conversion of it"""
    g = hip.CMAES(mfev=1000, tol=1e-12, np=8, seed=1)
    for obj in ("rastrigin", "ackley"):
        g.initialize(getattr(hip.objectives, obj), -np.ones(3), np.ones(3), np.zeros(3))
        for bad in (np.nan, np.inf, -np.inf):
            assert np.isnan(g.evaluate(np.array([0.25, bad, 0.5]))), (obj, bad)


# ---- the call sites ------------------------------------------------------------------------------------
BUDGET = 100000
DBG_SAMPLE_4WAVES = 268435456.      # enum CmaDbg (bbo_cma.hpp): cma_sample_eval<4> where <1, 16> would run


def _ccpso_pps(n):
    """swarm sizes that divide n"""
    return [s for s in (1, 2, 5, 10, 13, 17) if n % s == 0]


class Site:
    """one optimizer class: how to make it with the smallest population it takes, the (points, values)
    pairs of state keys its handle exposes -- values[i] is the objective at row i of points -- and the
    dimensions.  extra: the cases that reach another evaluation kernel of the class, each a dict of
    n, np (CMA-ES family), make_kw, state (keys set after initialize), objectives and routes
    ({objective: sample_route}, where the class reports one)"""

    def __init__(self, make, pairs, ns=(1, 17, 65, 130), clamp_kw=None, clamp_make=None, extra=()):
        self.make, self.pairs, self.ns = make, pairs, ns
        self.clamp_kw = clamp_kw        # not None: the class clamps to the box (with these constructor arguments)
        self.clamp_make = clamp_make    # the clamped pass with a larger population, where one member stays inside
        self.extra = extra


def _cma(cls, *args, np_min=4):
    return lambda hip, n, np=np_min, **kw: getattr(hip, cls)(BUDGET, 0., *args, np, seed=3, **kw)


def _restart(cls):
    # the drivers' iterate() is a whole inner run: small budgets keep two of them short
    return lambda hip, n, **kw: getattr(hip, cls)(hip.CMAES(200, 0., 4, seed=3), 2000, seed=3)


def _all(route):
    return {obj: route for obj in R.OBJECTIVES}


SEP_SUM = ("sphere", "ellipsoid", "rastrigin", "cigar", "discus", "diffpow")      # sep_sum_objective
# enum SampleKernel (bbo_cma.hpp), the ids `sample_route` reports:
#  0 sep_sample_eval<16>   1 sep_sample_eval<64, 512>   2 its lean build   3 sep_sample_sum<256, 0>   4 <256, 4>
#  5 sep_sample_eval<64>   6 cma_sample_eval128   7 its triangular form   8 cma_sample_eval<1, 8>   9 triangular
# 10 cma_sample_eval64<1, 8>   11 <1>   12 <2>   13 cma_sample_eval<1, 16>   14 cma_sample_eval<4>   15 <8>
SEP_512 = {obj: (3. if obj in SEP_SUM else 2.) for obj in R.OBJECTIVES}
SEP_1024 = {obj: (2. if obj not in SEP_SUM else 3. if obj in ("rastrigin", "diffpow") else 4.) for obj in R.OBJECTIVES}
FRAG = lambda route: {obj: route for obj in R.FRAG_OBJECTIVES}
BATCH = {"sample128_min": [1.]}

SITES = {
    # the main list reaches 10 (n = 1, 17), 12 (65) and 13 (130)
    "CMAES": Site(_cma("CMAES"), [("arx", "fitness")], clamp_kw={"bound": True}, extra=[
        dict(n=48, routes=_all(11.)), dict(n=128, routes=_all(8.)),
        dict(n=130, state={"dbg": [DBG_SAMPLE_4WAVES]}, routes=_all(14.)), dict(n=260, routes=_all(15.))]),
    "ActiveCMAES": Site(_cma("ActiveCMAES"), [("arx", "fitness")], clamp_kw={"bound": True}, extra=[
        dict(n=128, routes=_all(8.)), dict(n=128, np=16, state=BATCH, routes=FRAG(6.))]),
    # the main list reaches 0
    "SepCMAES": Site(_cma("SepCMAES"), [("arx", "fitness")], clamp_kw={"bound": True}, extra=[
        dict(n=300, routes=_all(1.)), dict(n=512, np=16, routes=SEP_512),
        dict(n=1024, np=16, routes=SEP_1024), dict(n=2049, routes=_all(5.))]),
    "CholeskyCMAES": Site(_cma("CholeskyCMAES", 0.), [("arx", "fitness")], clamp_kw={"bound": True}, extra=[
        dict(n=128, routes=_all(9.)), dict(n=128, np=16, state=BATCH, routes=FRAG(7.))]),
    "LmCMAES": Site(_cma("LmCMAES", np_min=2), [("arx", "f")]),
    "IPopCMAES": Site(_restart("IPopCMAES"), [("xbest", "fbest")]),
    "BiPopCMAES": Site(_restart("BiPopCMAES"), [("xbest", "fbest")]),
    "JADE": Site(lambda hip, n: hip.JADE(BUDGET, 4, 0., seed=3), [("x", "f")]),
    "SHADE": Site(lambda hip, n: hip.SHADE(BUDGET, 4, 0., seed=3), [("x", "f")]),
    "SANSDE": Site(lambda hip, n: hip.SANSDE(BUDGET, 4, 0., seed=3), [("x", "f")]),
    # cso_compete<G, true> with G = 16 (ld <= 128), 32 (<= 256: n = 130), 64 (<= 512), <16, false> beyond
    "CSO": Site(lambda hip, n: hip.CSO(BUDGET, 0., 3, seed=3), [("x", "f"), ("xbest", "fbest")], clamp_kw={},
                extra=[dict(n=300), dict(n=514)]),
    # ccp_eval<16> up to ld = 256, ccp_eval<64> beyond
    "CCPSO": Site(lambda hip, n: hip.CCPSO(BUDGET, 0., 3, _ccpso_pps(n), seed=3), [("yhat", "fyhat")], clamp_kw={},
                  extra=[dict(n=260)]),
    "JAYA": Site(lambda hip, n: hip.JAYA(BUDGET, 0., 2, 1, seed=3), [("X", "f")], clamp_kw={}),
    "DSA": Site(lambda hip, n: hip.DSA(BUDGET, 0., 0., 1, seed=3), [("X", "f"), ("bestx", "fbest")], clamp_kw={},
                clamp_make=lambda hip, n: hip.DSA(BUDGET, 0., 0., 8, seed=3)),
    "HEES": Site(lambda hip, n: hip.HEES(BUDGET, 0., np=1, seed=3),
                 [("arx", "fit_val"), ("xbest", "fbest"), ("xmean", "fm")]),
    "xNES": Site(lambda hip, n: hip.xNES(BUDGET, 0., seed=3), [("arx", "fit_val"), ("xbest", "fbest")]),
    "AMALGAM": Site(lambda hip, n: hip.AMALGAM(BUDGET, 0., 0., 3, noparam=False, print=False, seed=3),
                    [("arx[1:]", "fit_val[1:]"), ("xbest", "fbest")]),
    "SpiralSearch": Site(lambda hip, n: hip.SpiralSearch(BUDGET, 0., 1, seed=3), [("x", "f"), ("xbest", "fbest")]),
    "NSHS": Site(lambda hip, n: hip.NSHS(BUDGET, 1, seed=3),
                 [("x", "f"), ("xbest", "fbest"), ("cand", "fcand")], clamp_kw={},
                 clamp_make=lambda hip, n: hip.NSHS(BUDGET, 12, seed=3)),
    "SLPSO": Site(lambda hip, n: hip.SLPSO(BUDGET, 0., 2, seed=3), [("x", "fx"), ("abest", "fabest")]),
    "CRS": Site(lambda hip, n: hip.CRS(BUDGET, 2, 0., seed=3), [("x", "f")]),
    "SSDE": Site(lambda hip, n: hip.SSDE(BUDGET, 4, 0., seed=3), [("x", "f")], clamp_kw={}),
    "ACD": Site(lambda hip, n: hip.ACD(BUDGET, 0., 0., seed=3), [("xbest", "fbest")], ns=(1, 17, 65, 128), clamp_kw={}),
    "Mayfly": Site(lambda hip, n: hip.Mayfly(2, BUDGET, seed=3),
                   [("xbest", "fbest"), ("males_x", "males_f"), ("females_x", "females_f"),
                    ("males_bx", "males_bf"), ("moved_males_x", "moved_males_f"),
                    ("moved_females_x", "moved_females_f"), ("off_x", "off_f")], clamp_kw={}),
    "APSO": Site(lambda hip, n: hip.APSO(BUDGET, 0., 2, seed=3),
                 [("x", "f"), ("xb", "fb"), ("xbest", "fbest")], clamp_kw={}),
}
SITES_DOC = """One row per optimizer class of bboptpy_amd.multivariate (the restart drivers are made over a CMAES
base; their iterate() is a whole inner run, and what they expose of it is xbest / fbest).

Populations: the lower limit the engine's own parameter check states (bbo_create / bbo_init refuse less):
np = 4 for CMAES, ActiveCMAES, SepCMAES, CholeskyCMAES and the DE family (JADE, SHADE with npmin = 4,
SANSDE), 2 for LmCMAES, JAYA (npmin = 1), SLPSO, CRS, Mayfly (even) and APSO, 3 for CCPSO (its ring) and
AMALGAM, 4 for SSDE, 1 for DSA, SpiralSearch, NSHS (hms) and HEES (mu).  CSO's check says 2, but a
competition takes pcompete = 3 particles: 3 is the smallest swarm in which one is held.  xNES has no
population argument (4 + int(3 ln n)) and ACD none at all.  The cases that name another np need it to
reach their kernel (whole 16-row tiles for the lean and the batch samplers).

n: the class minimum 1, then 17, 65 and 130 (ACD: 128, its limit), plus every n (and switch) at which the
class evaluates with another kernel -- Site.extra:
    the CMA-ES engine chooses among sixteen samplers (CmaEngine::sample_route) and reports the choice as
    `sample_route`, asserted in every case of these four classes.  CMAES: cma_sample_eval64<1> at 48,
    cma_sample_eval<1, 8> at 128, cma_sample_eval<8> at 260, and cma_sample_eval<4>, which takes more than
    32 row tiles (np > 512) at 128 < n <= 256, through the diagnostic switch that selects it at np = 4.
    ActiveCMAES: cma_sample_eval128 with sample128_min = 1.  CholeskyCMAES: the triangular forms of both
    n = 128 samplers.  SepCMAES: the guarded sep_sample_eval<64, 512> at 300, its lean build and
    sep_sample_sum<256, 0> at 512, sep_sample_sum<256, 4> at 1024, sep_sample_eval<64> at 2049.
    CSO: cso_compete's lane group is a function of n alone (16, 32 at 130, 64 at 300, the unfused form at
    514); CCPSO: ccp_eval<64> from n = 257 on (260 has divisors for the swarm sizes).  Neither reports a
    route, so their cases assert nothing beyond the values.
    The other engines pick the rows of a workgroup by n (rows_per_wg16) but evaluate with one kernel.

The clamped pass runs the classes that clamp candidates to the box -- the CMA-ES family with bound = True,
CSO, CCPSO and APSO (correct = True, their default), JAYA, DSA, NSHS, SSDE, ACD, Mayfly -- for ten
iterations in [1/8, 1/2]^n (DSA with 8 members and NSHS with a memory of 12: their single member / harmony
stays inside the box that long).  LmCMAES clamps only its mean, never a candidate; HEES, xNES, AMALGAM,
SpiralSearch, SLPSO, CRS and the DE family redraw or ignore the box and leave no coordinate on it.

Classes that expose no population-wide pair, and what stands in: CCPSO -- its tables fx / fy hold the
values of CONTEXT vectors (yhat with one swarm's coordinates replaced), which no key returns as points;
the pair it does expose is yhat / fyhat.  IPopCMAES / BiPopCMAES -- xbest / fbest; the generation of
their base is the CMAES row.  ACD -- xbest / fbest: its archive x / f has 2 n slots that fill over the
first sweep and are zero until then.  The slots of a pending point (cand / fcand of SLPSO, CRS, SSDE;
cand2 of CRS; cand / value of ACD) hold a point only inside a phase walk and are no pair after a whole
iterate().  AMALGAM's row 0 is the elite, which the sampler redraws while its stored value stays (the
reference's behaviour): rows 1.. are held.  The CMA-ES family's fit_val is the SORTED copy of fitness and
pairs with arx only through fit_idx; fitness is the pair."""


def _state(g, key):
    skip = key.endswith("[1:]")
    return g.get_state(key[:-4] if skip else key), skip


def _exposed(g, site, n):
    """[(pair name, points[rows, n], values[rows])]"""
    out = []
    for pk, vk in site.pairs:
        (P, skip), (V, _) = _state(g, pk), _state(g, vk)
        assert V.size >= 1 and P.size == V.size * n, "%s / %s: %d points for %d values" % (pk, vk, P.size, V.size)
        P = P.reshape(V.size, n)
        out.append((pk + "/" + vk, P[1:] if skip else P, V[1:] if skip else V))
    return out


def _hold_site(hip, name, n, objectives, lo, up, make_kw=None, state=None, routes=None, np_=None, iterations=2,
               make=None):
    site = SITES[name]
    rng = np.random.default_rng(n)
    worst, seen = {}, []
    for obj in objectives:
        kw = dict(make_kw or {})
        if np_ is not None:
            kw["np"] = np_
        g = (make or site.make)(hip, n, **kw)
        g.initialize(getattr(hip.objectives, obj), lo * np.ones(n), up * np.ones(n), rng.uniform(lo, up, n))
        for key, value in (state or {}).items():
            g.set_state(key, value)
        for _ in range(iterations):
            g.iterate()
        if routes is not None:
            assert g.get_state("sample_route")[0] == routes[obj], (name, obj, g.get_state("sample_route"))
        for pair, P, V in _exposed(g, site, n):
            for x, v in zip(P, V):
                f_ref, bound = R.reference_at(obj, x)
                r = R.ratio(v, f_ref, bound)
                worst[obj] = max(worst.get(obj, 0.), r)
                assert r <= 1., "%s %s, %s, n = %d: the value %r is %.4g bounds from the reference at its point" % (
                    name, pair, obj, n, v, r)
            seen.append(P)
    print("RATIO site %s n = %d: %s" % (name, n, "  ".join("%s %.3f" % (o, worst[o]) for o in objectives)))
    return np.concatenate([P.ravel() for P in seen])


def test_the_table_names_every_optimizer_class():
    """(no device) a new engine cannot arrive without a row"""
    from bboptpy_amd import multivariate
    import bboptpy_amd
    classes = {k for k, v in vars(bboptpy_amd).items()
               if isinstance(v, type) and issubclass(v, multivariate.MultivariateSearch)
               and v not in (multivariate.MultivariateSearch, multivariate.BaseCMAES)}
    also = {k for k, v in vars(multivariate).items()
            if isinstance(v, type) and issubclass(v, multivariate.MultivariateSearch) and not k.startswith("_")
            and v not in (multivariate.MultivariateSearch, multivariate.BaseCMAES)}
    assert classes == also, "multivariate.py defines an optimizer the package does not export (or the reverse)"
    assert classes == set(SITES), "no row in SITES: %s; no such class: %s" % (
        sorted(classes - set(SITES)), sorted(set(SITES) - classes))
    for name, site in SITES.items():
        assert site.pairs and len(site.ns) >= 4 and min(site.ns) == 1, name
        for case in site.extra:
            assert set(case) <= {"n", "np", "make_kw", "state", "objectives", "routes"} and "n" in case, name


@pytest.mark.gpu
@pytest.mark.parametrize("name,n", [(name, n) for name in SITES for n in SITES[name].ns])
def test_call_sites_inside_the_bound(hip, name, n):
    """initialize, two iterations, every exposed (points, values) pair, all ten objectives"""
    _hold_site(hip, name, n, R.OBJECTIVES, -5., 5.)


@pytest.mark.gpu
@pytest.mark.parametrize("name,case", [(name, i) for name in SITES for i in range(len(SITES[name].extra))])
def test_call_sites_second_kernel(hip, name, case):
    """the n (population, switch) at which the class evaluates with another kernel; where the class reports
    its route (`sample_route`) the kernel is asserted"""
    c = SITES[name].extra[case]
    routes = c.get("routes")
    _hold_site(hip, name, c["n"], c.get("objectives") or (list(routes) if routes else R.OBJECTIVES), -5., 5.,
               make_kw=c.get("make_kw"), state=c.get("state"), routes=routes, np_=c.get("np"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", [name for name in SITES if SITES[name].clamp_kw is not None])
def test_call_sites_clamped_onto_the_seams(hip, name):
    """the box [1/8, 1/2]^n: a clamped coordinate sits exactly on an octant seam of cos_2pi -- 1/8, where
    the octant index steps from 0 to 1, or 1/2, the end of the reduced range -- where Rastrigin and Ackley
    take the cosine from the neighbouring polynomial.  Ten iterations: two leave ACD's best point, CCPSO's
    context vector and a small CSO swarm inside the box"""
    site = SITES[name]
    coords = _hold_site(hip, name, 17, ("rastrigin", "ackley"), 0.125, 0.5, make_kw=site.clamp_kw, iterations=10,
                        make=site.clamp_make)
    assert ((coords >= 0.125) & (coords <= 0.5)).all(), name
    on = int((coords == 0.125).sum()), int((coords == 0.5).sum())
    print("SEAMS %s: %d coordinates at 1/8, %d at 1/2 of %d" % (name, on[0], on[1], coords.size))
    assert on[0] + on[1] > 0, name
