"""Which kernels a decomposition launches (CmaEngine::eig_route, read back through the key `eig_route`),
case by case: every branch of the route at the smallest shape that reaches it.  The A/B tests of the
eigensolver compare "the form under a diagnostic bit" with the default; this file is what shows that the
two sides ran different kernels.  The expected sequences were read off a kernel trace of the commit before
the route function existed, not off that function.  Each route is also held to the residual and
orthogonality bounds of tests/test_cma_gpu.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# enum EigKernel (bbo_cma.hpp), in its order: the contract of the key
NAMES = ("cma_eigen_small", "cma_eigen_128", "cma_eigen_256", "cma_eigen", "cma_eigen_fx128", "cma_eigen_fx128u",
         "cma_eigen_r1", "cma_eigen_r1_fx128", "cma_eigen_g1", "cma_tred_mw", "cma_tred_tail", "cma_eig_halves",
         "cma_eigen_g2", "cma_eig_secular", "cma_eig_lowner", "cma_eig_fcols", "cma_eigen_g",
         "cma_tred_mw512", "cma_tred_mw_chain", "cma_eigen_b4", "cma_eigen_b",
         "cma_eig_gemm1", "cma_eig_gemm", "cma_eig_wy4", "cma_eig_wy4_512", "cma_eig_wy",
         "cma_post", "cma_post_mfma")
K_COV = 5            # the slot of cma_cov in `profile` (pairs of ms, launches)

TOP = ["cma_eig_halves", "cma_eigen_g2", "cma_eig_secular"]                  # the top merge up to its secular equation
CLOSED = TOP + ["cma_eig_lowner", "cma_eig_fcols", "cma_eig_gemm1", "cma_eig_wy4"]
MW = ["cma_tred_mw", "cma_tred_tail"]

# (n, populations, dbg, mode, box) -> kernels.  mode: "phase" = phase(PHASE_EIGEN), "generation" = iterate()
CASES = {
    "n8": (8, 4, 0, "phase", False, ["cma_eigen_small"]),
    "n8 big kernel": (8, 4, 16, "phase", False, ["cma_eigen_128", "cma_post_mfma"]),
    "n24": (24, 2, 0, "phase", False, ["cma_eigen_128"]),
    "n48": (48, 2, 0, "phase", False, ["cma_eigen_256"]),
    "n100 split": (100, 1, 0, "phase", False, ["cma_eigen_r1"] + CLOSED),
    "n100 batch": (100, 40, 0, "phase", False, ["cma_eigen"]),
    "n100 one workgroup": (100, 1, 4194304, "phase", False, ["cma_eigen"]),
    "n128 split": (128, 1, 0, "phase", False, ["cma_eigen_r1_fx128"] + CLOSED),
    "n128 split generic": (128, 1, 2097152, "phase", False, ["cma_eigen_r1"] + CLOSED),
    "n128 batch fused": (128, 40, 0, "generation", False, ["cma_eigen_fx128"]),
    "n128 batch unfused": (128, 40, 32, "generation", False, ["cma_eigen_fx128u"]),
    "n128 batch phase": (128, 40, 0, "phase", False, ["cma_eigen_fx128u"]),
    "n128 batch generic": (128, 40, 2097152, "phase", False, ["cma_eigen"]),
    "n128 batch box": (128, 40, 0, "phase", True, ["cma_eigen", "cma_post_mfma"]),
    "n132": (132, 1, 0, "phase", False, MW + CLOSED),
    "n133 odd": (133, 1, 0, "phase", False, MW + TOP + ["cma_eigen_g2", "cma_eig_gemm1", "cma_eig_wy4"]),
    "n132 reduction on one workgroup": (132, 1, 16777216, "phase", False, ["cma_eigen_g1"] + CLOSED),
    "n132 all steps spread": (132, 1, 536870912, "phase", False, ["cma_tred_mw"] + CLOSED),
    "n132 one workgroup": (132, 1, 4194304, "phase", False, ["cma_eigen_g", "cma_eig_gemm1", "cma_eig_wy4"]),
    "n132 top merge in one kernel": (132, 1, 67108864, "phase", False,
                                     MW + ["cma_eig_halves", "cma_eigen_g2", "cma_eig_gemm1", "cma_eig_wy4"]),
    "n132 tile per wavefront": (132, 1, 134217728, "phase", False,
                                MW + TOP + ["cma_eigen_g2", "cma_eig_gemm1", "cma_eig_wy", "cma_post"]),
    # (40 x 8 workgroups: more than the spread budget of a device admits)
    "n132 batch": (132, 40, 0, "phase", False,
                   ["cma_eigen_g1", "cma_eig_halves", "cma_eigen_g2", "cma_eig_gemm", "cma_eig_wy", "cma_post"]),
    "n260": (260, 1, 0, "phase", False, ["cma_tred_mw512", "cma_tred_mw_chain", "cma_tred_tail", "cma_eigen_b4",
                                         "cma_eig_gemm1", "cma_eig_wy4_512", "cma_post"]),
    "n260 no chain": (260, 1, 536870912, "phase", False, ["cma_tred_mw512", "cma_tred_tail", "cma_eigen_b4",
                                                          "cma_eig_gemm1", "cma_eig_wy4_512", "cma_post"]),
    "n260 reduction on one workgroup": (260, 1, 16777216, "phase", False,
                                        ["cma_eigen_b", "cma_eig_gemm1", "cma_eig_gemm", "cma_post"]),
}


def _spd(n, p):
    rng = np.random.default_rng(1000 * n + p)
    X = rng.normal(size=(n, 3 * n))
    return X @ X.T / (3 * n) + np.eye(n)


def run_case(hip, n, pops, dbg, mode, box):
    """the handle after one decomposition of a set C in every population (shared with the trace job)"""
    from bboptpy_amd import _ffi
    lam = 64 if mode == "generation" else max(4, min(2 * n, 64))
    g = hip.ActiveCMAES(mfev=10 ** 7, tol=1e-12, np=lam, seed=1, populations=pops, bound=box)
    g.initialize(hip.objectives.sphere, -np.ones(n), np.ones(n), np.zeros((pops, n)))
    if dbg:
        g.set_state("dbg", [float(dbg)])
    for p in range(pops):
        g.set_state("C", _spd(n, p), p)
        g.set_state("fev", [10 ** 6], p)           # makes the decomposition due (cmaes.cpp:233)
        g.set_state("eigenlastev", [0], p)
    if mode == "generation":
        g.set_state("profile", [1.0])
        g.iterate()
    else:
        g.phase(_ffi.PHASE_EIGEN)
    return g


@pytest.mark.parametrize("case", sorted(CASES))
def test_route(hip, case):
    n, pops, dbg, mode, box, want = CASES[case]
    g = run_case(hip, n, pops, dbg, mode, box)
    got = [NAMES[int(k)] for k in g.get_state("eig_route")]
    assert got == want
    if "cma_tred_mw" in want or "cma_tred_mw512" in want:
        assert int(g.get_state("eig_mw_fail")[0]) == 0 and int(g.get_state("eig_mw_reserved")[0]) > 0
    if mode == "generation":
        fused = want == ["cma_eigen_fx128"]
        assert int(g.get_state("cov_fused")[0]) == (1 if fused else 0)
        launches = g.get_state("profile").reshape(-1, 2)[K_COV, 1]
        assert (launches == 0) if fused else (launches == 1)
    for p in sorted({0, pops - 1}):
        assert int(g.get_state("eigen_done", p)[0]) == 1
        Cm = g.get_state("C", p).reshape(n, n)
        B, D = g.get_state("B", p).reshape(n, n), g.get_state("D", p)
        assert np.linalg.norm(B @ np.diag(D * D) @ B.T - Cm) <= 1e-11 * np.linalg.norm(Cm)
        assert np.linalg.norm(B.T @ B - np.eye(n)) <= 1e-12 * n
