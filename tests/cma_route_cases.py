"""The cases of tests/test_cma_routes_gpu.py: every branch of CmaEngine::sample_route and
CmaEngine::update_route at the smallest shape that reaches it, and how one case is run.  Shared with
the job that records the kernel trace (profiles/sample_update_routes.txt): the expected kernels below
were read off that trace of the commit before the route functions existed, not off those functions."""
import numpy as np

# enum SampleKernel (bbo_cma.hpp), in its order: the contract of the key `sample_route`.  The names are
# the trace's (template arguments written out); sep_sample_sum without its objective argument.
SAMPLE_NAMES = ("sep_sample_eval<16, 256, false>", "sep_sample_eval<64, 512, false>",
                "sep_sample_eval<64, 512, true>", "sep_sample_sum<256, 0>", "sep_sample_sum<256, 4>",
                "sep_sample_eval<64, 256, false>",
                "cma_sample_eval128", "cma_sample_eval128_tri", "cma_sample_eval<1, 8, false>",
                "cma_sample_eval<1, 8, true>", "cma_sample_eval64<1, 8>", "cma_sample_eval64<1, 32>",
                "cma_sample_eval64<2, 32>", "cma_sample_eval<1, 16, false>", "cma_sample_eval<4, 4, false>",
                "cma_sample_eval<8, 4, false>")
# enum UpdateKernel, in its order: the contract of the key `update_route` (cma_whiten<MAXT> is one id)
UPDATE_NAMES = ("chol_paths", "chol_cprime", "chol_factor", "sep_moments", "sep_paths", "cma_whiten128",
                "cma_whiten", "cma_gram128s", "cma_gram128", "cma_gram", "cma_paths", "cma_paths_lazy",
                "cma_paths_lazy1k", "cma_cov")


def _case(algo, n, lam, want, lean=None, P=1, obj="sphere", box=False, dbg=0, mode="phase", **knobs):
    return dict(algo=algo, n=n, lam=lam, want=want, lean=lean, P=P, obj=obj, box=box, dbg=dbg, mode=mode,
                knobs=knobs)


SEP, ACT, CHOL, CMA = "SepCMAES", "ActiveCMAES", "CholeskyCMAES", "CMAES"
ROWS = "sep_sample_eval<64, 512, false>"
WIDE, WIDE_TRI = "cma_sample_eval<1, 8, false>", "cma_sample_eval<1, 8, true>"
E64 = "cma_sample_eval64<2, 32>"

# want: the sampler's kernel; lean: the value of `sample_lean` where the case is about it
SAMPLE_CASES = {
    "sep n8": _case(SEP, 8, 8, "sep_sample_eval<16, 256, false>"),
    "sep n260 padded columns": _case(SEP, 260, 16, ROWS, lean=0),
    "sep n272": _case(SEP, 272, 16, "sep_sample_sum<256, 0>", lean=1),
    "sep n272 padded rows": _case(SEP, 272, 8, ROWS, lean=0),
    "sep n272 rosenbrock": _case(SEP, 272, 16, "sep_sample_eval<64, 512, true>", lean=1, obj="rosenbrock"),
    "sep n272 rows in LDS": _case(SEP, 272, 16, "sep_sample_eval<64, 512, true>", lean=1, dbg=1048576),
    "sep n272 guarded": _case(SEP, 272, 16, ROWS, lean=0, dbg=256),
    "sep n1024": _case(SEP, 1024, 16, "sep_sample_sum<256, 4>", lean=1),
    "sep n1024 rastrigin": _case(SEP, 1024, 16, "sep_sample_sum<256, 0>", lean=1, obj="rastrigin"),
    "sep n2064": _case(SEP, 2064, 8, "sep_sample_eval<64, 256, false>"),
    "n24": _case(ACT, 24, 8, "cma_sample_eval64<1, 8>"),
    "n40": _case(ACT, 40, 8, "cma_sample_eval64<1, 32>"),
    "n100": _case(ACT, 100, 8, E64),
    "n128": _case(ACT, 128, 16, WIDE),
    "n128 no wide tiles": _case(ACT, 128, 16, E64, sample_wide_max=0),
    "n128 512 tiles": _case(ACT, 128, 8192, WIDE),
    "n128 513 tiles": _case(ACT, 128, 8208, E64),
    "n128 batch kernel": _case(ACT, 128, 16, "cma_sample_eval128", lean=1, obj="rosenbrock", sample128_min=1),
    "n120 batch kernel": _case(ACT, 120, 16, "cma_sample_eval128", lean=0, obj="rosenbrock", sample128_min=1),
    "n128 batch kernel rastrigin": _case(ACT, 128, 16, WIDE, obj="rastrigin", sample128_min=1),
    "n128 32768 rows": _case(ACT, 128, 4096, "cma_sample_eval128", lean=1, P=8, obj="rosenbrock"),
    "n128 32640 rows": _case(ACT, 128, 4080, E64, P=8, obj="rosenbrock"),
    "chol n128": _case(CHOL, 128, 16, WIDE_TRI),
    "chol n128 full operand": _case(CHOL, 128, 16, WIDE, chol_tri=0),
    "chol n128 batch kernel": _case(CHOL, 128, 16, "cma_sample_eval128_tri", lean=1, sample128_min=1),
    "chol n128 batch kernel full operand": _case(CHOL, 128, 16, "cma_sample_eval128", lean=1, sample128_min=1,
                                                 chol_tri=0),
    "n132": _case(ACT, 132, 16, "cma_sample_eval<1, 16, false>"),
    "n132 four wavefronts": _case(ACT, 132, 16, "cma_sample_eval<4, 4, false>", dbg=268435456),
    "n132 32 tiles": _case(ACT, 132, 512, "cma_sample_eval<1, 16, false>"),
    "n132 33 tiles": _case(ACT, 132, 528, "cma_sample_eval<4, 4, false>"),
    "n260": _case(ACT, 260, 16, "cma_sample_eval<8, 4, false>"),
}

# want: the kernels of launch_update in launch order.  None in front: a whitening that runs exactly when the
# ranking was the one-wavefront form (rank_route 0), which hands no norms down
LAZY1K = ["cma_paths_lazy1k", "cma_cov"]
UPDATE_CASES = {
    "cma n8": _case(CMA, 8, 8, ["cma_gram", "cma_paths", "cma_cov"]),
    "cma n24": _case(CMA, 24, 8, ["cma_gram", "cma_paths_lazy", "cma_cov"]),
    "cma n100": _case(CMA, 100, 8, ["cma_gram"] + LAZY1K),
    "cma n100 256 threads": _case(CMA, 100, 8, ["cma_gram", "cma_paths_lazy", "cma_cov"], dbg=131072),
    "cma n128": _case(CMA, 128, 16, ["cma_gram128s"] + LAZY1K),
    "cma n128 gram from LDS": _case(CMA, 128, 16, ["cma_gram128"] + LAZY1K, dbg=512),
    "active n128 box": _case(ACT, 128, 16, ["cma_whiten<2>", "cma_gram128s", "cma_paths", "cma_cov"], box=True),
    "active n40 box": _case(ACT, 40, 8, ["cma_whiten<1>", "cma_gram", "cma_paths", "cma_cov"], box=True),
    "active n132": _case(ACT, 132, 16, [None, "cma_whiten<4>", "cma_gram"] + LAZY1K),
    "active n260": _case(ACT, 260, 16, [None, "cma_whiten<8>", "cma_gram", "cma_paths", "cma_cov"]),
    "active n128 32768 worst rows": _case(ACT, 128, 4096, ["cma_whiten128", "cma_gram128s", "cma_paths", "cma_cov"],
                                          P=16, box=True),
    # (mu = 2040 is padded to 2048: still 32768 rows; 2032 is the first count below)
    "active n128 32640 worst rows": _case(ACT, 128, 4080, ["cma_whiten128", "cma_gram128s", "cma_paths", "cma_cov"],
                                          P=16, box=True),
    "active n128 32512 worst rows": _case(ACT, 128, 4064, ["cma_whiten<2>", "cma_gram128s", "cma_paths", "cma_cov"],
                                          P=16, box=True),
    "active n132 box": _case(ACT, 132, 16, ["cma_whiten<4>", "cma_gram", "cma_paths", "cma_cov"], box=True),
    "active n260 box": _case(ACT, 260, 16, ["cma_whiten<8>", "cma_gram", "cma_paths", "cma_cov"], box=True),
    "active n128 batch generation": _case(ACT, 128, 64, [None, "cma_whiten<2>", "cma_gram128s", "cma_paths_lazy1k"],
                                          P=40, mode="generation"),
    "chol n24": _case(CHOL, 24, 8, ["chol_paths", "chol_cprime", "chol_factor"]),
    "chol n132": _case(CHOL, 132, 16, ["chol_paths", "chol_cprime", "chol_factor"]),
    "sep n24": _case(SEP, 24, 8, ["sep_moments", "sep_paths"]),
}


def objective_rows(obj, X):
    """the objective of every row of X, in numpy"""
    if obj == "sphere":
        return (X * X).sum(1)
    if obj == "rosenbrock":
        return (100. * (X[:, 1:] - X[:, :-1] ** 2) ** 2 + (1. - X[:, :-1]) ** 2).sum(1)
    if obj == "rastrigin":
        return 10. * X.shape[1] + (X * X - 10. * np.cos(2. * np.pi * X)).sum(1)
    raise ValueError(obj)


def make_handle(hip, case):
    """the initialised handle of a case, its knobs set"""
    n, lam, P = case["n"], case["lam"], case["P"]
    ext = dict(seed=3, populations=P)
    if case["algo"] == CHOL:
        g = hip.CholeskyCMAES(10 ** 9, 1e-12, 1e-12, lam, 2., case["box"], **ext)
    else:
        g = getattr(hip, case["algo"])(10 ** 9, 1e-12, lam, 2., case["box"], **ext)
    guess = np.random.default_rng(n + lam).uniform(-3, 3, (P, n))
    g.initialize(getattr(hip.objectives, case["obj"]), -5. * np.ones(n), 5. * np.ones(n), guess if P > 1 else guess[0])
    if case["dbg"]:
        g.set_state("dbg", [float(case["dbg"])])
    for key, v in case["knobs"].items():
        g.set_state(key, [float(v)])
    return g


def run_sample(g):
    from bboptpy_amd import _ffi
    g.phase(_ffi.PHASE_SAMPLE_EVALUATE)


def run_update(g, case):
    """the launches of one update: the three phases, or (mode "generation") one profiled iterate()"""
    from bboptpy_amd import _ffi
    if case["mode"] == "generation":
        g.set_state("profile", [1.0])
        g.iterate()
    else:
        g.phase(_ffi.PHASE_SAMPLE_EVALUATE)
        g.phase(_ffi.PHASE_RANK)
        g.phase(_ffi.PHASE_UPDATE)
