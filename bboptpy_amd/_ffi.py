"""ctypes binding of libbbopt_hip.so (include/bbopt_hip.h).

The library is the product: if it cannot be loaded, or no gfx950 device is visible,
everything here raises -- there is deliberately no CPU fallback.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libbbopt_hip.so")

# bbo_algo
ALGO_CMAES, ALGO_ACTIVE_CMAES, ALGO_SHADE, ALGO_JADE, ALGO_APSO, ALGO_IPOP, ALGO_BIPOP, \
    ALGO_SEP_CMAES, ALGO_SANSDE, ALGO_CSO, ALGO_CCPSO, ALGO_CHOLESKY_CMAES, ALGO_JAYA, ALGO_DSA, \
    ALGO_HEES, ALGO_SPIRAL, ALGO_NSHS, ALGO_LM_CMAES, ALGO_XNES, ALGO_AMALGAM, ALGO_SLPSO, \
    ALGO_CRS, ALGO_SSDE, ALGO_ACD, ALGO_MAYFLY, ALGO_PIKAIA, ALGO_NELDER_MEAD, ALGO_ROSENBROCK, \
    ALGO_BASIN_HOPPING = range(29)
# bbo_objective_kind
OBJ_BUILTIN, OBJ_SCALAR_CB, OBJ_BATCH_CB, OBJ_PROGRAM = 0, 1, 2, 3
# bbo_status (the ones Python tells apart)
ERR_ARG = -1
# bbo_cma_phase
PHASE_SAMPLE_EVALUATE, PHASE_RANK, PHASE_UPDATE, PHASE_EIGEN, PHASE_HISTORY_STOP = range(5)
# bbo_hees_phase
HEES_PHASE_SAMPLE, HEES_PHASE_RANK, HEES_PHASE_UPDATE, HEES_PHASE_FINISH = range(4)
# bbo_spiral_phase
SPIRAL_PHASE_DRAW, SPIRAL_PHASE_ROTATE, SPIRAL_PHASE_EVALUATE, SPIRAL_PHASE_BEST = range(4)
# bbo_nshs_phase
NSHS_PHASE_GENERATE, NSHS_PHASE_EVALUATE, NSHS_PHASE_REPLACE = range(3)
# bbo_lm_phase
LM_PHASE_SAMPLE, LM_PHASE_EVALUATE, LM_PHASE_RANK, LM_PHASE_UPDATE, LM_PHASE_HISTORY_STOP = range(5)
# bbo_xnes_phase
XNES_PHASE_SAMPLE, XNES_PHASE_RANK, XNES_PHASE_STEP, XNES_PHASE_ADAPT = range(4)
# bbo_amalgam_phase
AMALGAM_PHASE_DISTRIBUTION, AMALGAM_PHASE_SAMPLE, AMALGAM_PHASE_ADAPT = range(3)
# bbo_slpso_phase
SLPSO_PHASE_ADVANCE, SLPSO_PHASE_EVALUATE, SLPSO_PHASE_ABSORB = range(3)
# bbo_crs_phase
CRS_PHASE_ADVANCE, CRS_PHASE_EVALUATE, CRS_PHASE_ABSORB = range(3)
# bbo_ssde_phase
SSDE_PHASE_ADVANCE, SSDE_PHASE_EVALUATE, SSDE_PHASE_ABSORB = range(3)
# bbo_acd_phase
ACD_PHASE_ADVANCE, ACD_PHASE_EVALUATE, ACD_PHASE_ABSORB = range(3)
# bbo_nm_phase
NM_PHASE_ADVANCE, NM_PHASE_EVALUATE, NM_PHASE_ABSORB = range(3)
# NelderMead "flag": the factorial test passed, mfev < fev
NM_FLAG_CONVERGED, NM_FLAG_BUDGET = 1, 2
# bbo_rosen_phase
ROSEN_PHASE_ADVANCE, ROSEN_PHASE_EVALUATE, ROSEN_PHASE_ABSORB = range(3)
# Rosenbrock "flag": stepi <= tol, the budget
ROSEN_FLAG_CONVERGED, ROSEN_FLAG_BUDGET = 1, 2
# bbo_bh_phase
BH_PHASE_STEP, BH_PHASE_COLLECT, BH_PHASE_EVALUATE, BH_PHASE_DECIDE = range(4)
# BasinHopping "flag": mit reached
BH_FLAG_MIT = 2
# ACD "flag" and "rule"
ACD_FLAG_CONVERGED, ACD_FLAG_BUDGET = 1, 2
ACD_RULE_FTOL, ACD_RULE_XTOL = 1, 2
# CRS "flag": the tolerance, the budget, the depth cap
CRS_FLAG_TOL, CRS_FLAG_BUDGET, CRS_FLAG_DEPTH = 1, 2, 3
# LmCMAES "flag": the CMA engines' codes and sigma < 1e-16
LM_FLAG_MAXITER, LM_FLAG_TOLHISTFUN, LM_FLAG_EQUALFUNVALS, LM_FLAG_SIGMA = 1, 2, 3, 11

BUILTIN_IDS = {"sphere": 0, "rosenbrock": 1, "rastrigin": 2, "ellipsoid": 3, "ackley": 4,
               "griewank": 5, "cigar": 6, "discus": 7, "diffpow": 8, "schwefel12": 9}

SCALAR_FN = C.CFUNCTYPE(C.c_double, C.POINTER(C.c_double), C.c_int, C.c_void_p,
                        C.POINTER(C.c_int))
BATCH_FN = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_double), C.c_int, C.c_int, C.c_int,
                       C.POINTER(C.c_double), C.c_void_p)


class Params(C.Structure):
    _fields_ = [
        ("algo", C.c_int), ("mfev", C.c_int), ("tol", C.c_double), ("np", C.c_int),
        ("sigma0", C.c_double), ("bound", C.c_int), ("alphacov", C.c_double),
        ("eigenrate", C.c_double),
        ("archive", C.c_int), ("repaircr", C.c_int), ("pelite", C.c_double),
        ("cdamp", C.c_double), ("jade_sigma", C.c_double), ("h", C.c_int), ("npmin", C.c_int),
        ("correct", C.c_int),
        ("print", C.c_int), ("nipop", C.c_int), ("ksigmadec", C.c_double),
        ("boundlambda", C.c_int), ("maxlargeruns", C.c_int), ("kbudget", C.c_double),
        ("seed", C.c_uint64), ("device", C.c_int), ("populations", C.c_int),
        ("poll_every", C.c_int), ("adjustlr", C.c_int),
        ("crref", C.c_int), ("pupdate", C.c_int), ("crupdate", C.c_int),
        ("pcompete", C.c_int), ("ring", C.c_int), ("vmax", C.c_double),
        ("npps", C.c_int), ("pps", C.c_int * 16), ("pcauchy", C.c_double),
        ("stol", C.c_double), ("ranked", C.c_int),
    ]


class JayaParams(C.Structure):
    """bbo_jaya_params: JAYA's constructor arguments that bbo_params has no field for"""
    _fields_ = [("adapt", C.c_int), ("k0", C.c_int), ("mutation", C.c_int), ("kcheb", C.c_int),
                ("scale", C.c_double), ("beta", C.c_double), ("temper", C.c_double)]


class DsaParams(C.Structure):
    """bbo_dsa_params: DSA's constructor arguments that bbo_params has no field for"""
    _fields_ = [("adapt", C.c_int), ("nbatch", C.c_int)]


class HeesParams(C.Structure):
    """bbo_hees_params: HEES's constructor arguments that bbo_params has no field for"""
    _fields_ = [("mres", C.c_int), ("print", C.c_int)]


class SpiralParams(C.Structure):
    """bbo_spiral_params: SpiralSearch's constructor arguments that bbo_params has no field for"""
    _fields_ = [(k, C.c_double) for k in ("r", "theta", "taur", "tautheta", "rlow", "rhigh",
                                          "thetalow", "thetahigh")]


class NshsParams(C.Structure):
    """bbo_nshs_params: the constructor argument of NSHS that bbo_params has no field for"""
    _fields_ = [("fstdmin", C.c_double)]


class LmParams(C.Structure):
    """bbo_lm_params: LmCMAES's constructor arguments that bbo_params has no field for"""
    _fields_ = [("memory", C.c_int), ("rademacher", C.c_int), ("usenew", C.c_int)]


class XnesParams(C.Structure):
    """bbo_xnes_params: xNES's constructor arguments that bbo_params has no field for"""
    _fields_ = [("a0", C.c_double), ("etamu", C.c_double), ("from_guess", C.c_int)]


class AmalgamParams(C.Structure):
    """bbo_amalgam_params: AMALGAM's constructor arguments that bbo_params has no field for"""
    _fields_ = [(k, C.c_int) for k in ("iamalgam", "noparam", "print", "keep_elite", "concurrent",
                                       "substream")]


class SlpsoParams(C.Structure):
    """bbo_slpso_params: SLPSO's constructor arguments that bbo_params has no field for"""
    _fields_ = [(k, C.c_double) for k in ("omegamin", "omegamax", "eta", "gamma", "vmax", "Ufmax")]


class CrsParams(C.Structure):
    """bbo_crs_params: the extensions of CRS that bbo_params has no field for"""
    _fields_ = [("max_depth", C.c_int), ("repair", C.c_int)]


class SsdeParams(C.Structure):
    """bbo_ssde_params: the arguments of SSDE that bbo_params has no field for"""
    _fields_ = [("patience", C.c_int), ("npmin", C.c_int), ("ptop", C.c_double), ("h", C.c_int),
                ("usede", C.c_int), ("repaircr", C.c_int)]


class AcdParams(C.Structure):
    """bbo_acd_params: the arguments of ACD that bbo_params has no field for"""
    _fields_ = [("ksucc", C.c_double), ("kunsucc", C.c_double), ("from_guess", C.c_int),
                ("speculate", C.c_int)]


class MayflyParams(C.Structure):
    """bbo_mayfly_params: the arguments of Mayfly that bbo_params has no field for"""
    _fields_ = [(k, C.c_double) for k in ("a1", "a2", "a3", "beta", "dance", "ddamp", "fl", "fldamp", "gmin",
                                          "gmax", "vdamp", "sigma", "pmutdim", "pmutnp", "l")] \
        + [("pgb", C.c_int), ("repair", C.c_int), ("substream", C.c_int)]


class PikaiaParams(C.Structure):
    """bbo_pikaia_params: the arguments of PIKAIA that bbo_params has no field for"""
    _fields_ = [(k, C.c_double) for k in ("pcross", "pmut", "pmutmn", "pmutmx", "fdif")] \
        + [(k, C.c_int) for k in ("imut", "irep", "ielite", "repair", "raw", "substream")]


class NmParams(C.Structure):
    """bbo_nm_params: the arguments of NelderMead that bbo_params has no field for"""
    _fields_ = [("minit", C.c_int), ("pinit", C.c_int), ("checkev", C.c_int), ("eps", C.c_double),
                ("repair", C.c_int), ("speculate", C.c_int), ("lds", C.c_int), ("substream", C.c_int)]


class RosenParams(C.Structure):
    """bbo_rosen_params: the arguments of Rosenbrock that bbo_params has no field for"""
    _fields_ = [("decf", C.c_double), ("repair", C.c_int), ("wide", C.c_int), ("substream", C.c_int)]


class BhParams(C.Structure):
    """bbo_bh_params: the step strategy and the arguments of BasinHopping"""
    _fields_ = [("stepsize", C.c_double), ("adaptive", C.c_int), ("accept_rate", C.c_double), ("interval", C.c_int),
                ("factor", C.c_double), ("temp", C.c_double)] \
        + [(k, C.c_int) for k in ("mit", "print", "lockstep", "substream", "nstep0", "naccept0")]


class Objective(C.Structure):
    _fields_ = [("kind", C.c_int), ("builtin", C.c_int), ("scalar", SCALAR_FN),
                ("batch", BATCH_FN), ("user", C.c_void_p)]


class BboError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("libbbopt_hip status %d: %s" % (status, message))
        self.status = status


_lib = None
_dp = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
_ip = C.POINTER(C.c_int)
_h, _i = C.c_void_p, C.c_int
_TABLE = [C.c_void_p, C.c_int]      # an injected table and its length; NULL: the device draws

# the entry points every handle has, and those of the CMA-ES, CCPSO and program objects:
# name -> (argtypes, restype); no argtypes: the function takes none
CORE = {
    "bbo_params_default": ([C.POINTER(Params), _i], None),
    "bbo_create": ([C.POINTER(Params), C.POINTER(_h)], _i),
    "bbo_create_restart": ([C.POINTER(Params), _h, C.POINTER(_h)], _i),
    "bbo_create_basin": ([C.POINTER(Params), _h, C.POINTER(_h)], _i),
    "bbo_bh_draws": ([C.c_uint64, _i, _i, _i, _dp], _i),
    "bbo_destroy": ([_h], _i),
    "bbo_init": ([_h, _i, _dp, _dp, _dp, C.POINTER(Objective)], _i),
    "bbo_iterate": ([_h], _i),
    "bbo_solution": ([_h, _dp, _ip, _ip], _i),
    "bbo_solution_of": ([_h, _i, _dp, _ip, _ip], _i),
    "bbo_optimize": ([_h, _i, _dp, _dp, _dp, C.POINTER(Objective), _dp, _ip, _ip], _i),
    "bbo_run": ([_h, _i, _ip], _i),
    "bbo_get": ([_h, C.c_char_p, _i, C.c_void_p, _i], _i),
    "bbo_set": ([_h, C.c_char_p, _i, _dp, _i], _i),
    "bbo_cma_phase_run": ([_h, _i], _i),
    "bbo_cma_inject_normals": ([_h] + _TABLE, _i),
    "bbo_cma_set_params": ([_h, _i, C.c_double, _i], _i),
    "bbo_cma_set_seed": ([_h, C.c_uint64], _i),
    "bbo_cma_evaluate": ([_h, _dp, C.POINTER(C.c_double)], _i),
    "bbo_ccpso_set_shard": ([_h, _i, _i], _i),
    "bbo_ccpso_set_local": ([_h, _h, _i], _i),
    "bbo_ccpso_phase": ([_h, _i], _i),
    "bbo_ccpso_table_record": ([_h], _i),
    "bbo_ccpso_export_tables": ([_h, C.c_void_p, _i], _i),
    "bbo_ccpso_merge_tables": ([_h, C.c_void_p, _i, _i], _i),
    "bbo_program_create": ([C.c_char_p, C.c_char_p, C.c_void_p, _i, C.POINTER(_h)], _i),
    "bbo_program_destroy": ([_h], _i),
    "bbo_probe_objective": ([_i, _i, _i, _i, _dp, _dp], _i),
    "bbo_last_error": ([_h], C.c_char_p),
    "bbo_version": (None, C.c_char_p),
    "bbo_device_count": (None, _i),
}

# the engines with an extension struct: prefix -> (the struct of bbo_<prefix>_params_default and
# bbo_<prefix>_configure, whether bbo_<prefix>_phase exists, the bbo_<prefix>_inject_<what> entry points
# with their arguments behind the handle)
EXTENSIONS = {
    "jaya": (JayaParams, False, {}),
    "dsa": (DsaParams, False, {}),
    "hees": (HeesParams, True, {"normals": _TABLE}),
    "spiral": (SpiralParams, True, {"uniforms": _TABLE}),
    "nshs": (NshsParams, True, {"uniforms": _TABLE}),
    "lm": (LmParams, True, {"draws": _TABLE}),
    "xnes": (XnesParams, True, {"normals": _TABLE}),
    "amalgam": (AmalgamParams, True, {"draws": _TABLE + _TABLE, "points": _TABLE}),
    "slpso": (SlpsoParams, True, {"draws": _TABLE}),
    "crs": (CrsParams, True, {"draws": _TABLE}),
    "ssde": (SsdeParams, True, {"draws": _TABLE}),
    "acd": (AcdParams, True, {}),
    "mayfly": (MayflyParams, False, {"draws": _TABLE}),
    "pikaia": (PikaiaParams, False, {"draws": _TABLE}),
    "nm": (NmParams, True, {}),
    "rosen": (RosenParams, True, {}),
    "bh": (BhParams, True, {"draws": _TABLE}),
}


def _signatures():
    """every exported function: name -> (argtypes, restype)"""
    sig = dict(CORE)
    for prefix, (struct, has_phase, injects) in EXTENSIONS.items():
        sig["bbo_%s_params_default" % prefix] = ([C.POINTER(struct)], None)
        sig["bbo_%s_configure" % prefix] = ([_h, C.POINTER(struct)], _i)
        if has_phase:
            sig["bbo_%s_phase" % prefix] = ([_h, _i], _i)
        for what, args in injects.items():
            sig["bbo_%s_inject_%s" % (prefix, what)] = ([_h] + args, _i)
    return sig


EXPORTED_SYMBOLS = tuple(_signatures())


def lib():
    """load the HIP library once; raises if it has not been built"""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "bboptpy_amd: %s is missing. Build it with `python __graft_entry__.py` (hipcc, "
            "gfx950). There is no CPU fallback." % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    for name, (argtypes, restype) in _signatures().items():
        fn = getattr(L, name)
        if argtypes is not None:
            fn.argtypes = argtypes
        fn.restype = restype
    _lib = L
    return L


def check(status, handle=None):
    if status < 0:
        msg = lib().bbo_last_error(handle)
        raise BboError(status, msg.decode() if msg else "")
    return status


def probe_objective(objective, form, X):
    """diagnostics (bbo_probe_objective): built-in `objective` (a name or an id) at the rows of
    X[rows, n] through device form `form`; the raw values, one per row"""
    X = np.ascontiguousarray(np.atleast_2d(np.asarray(X, dtype=np.float64)))
    f = np.empty(X.shape[0])
    check(lib().bbo_probe_objective(BUILTIN_IDS.get(objective, objective), int(form), X.shape[1],
                                    X.shape[0], X, f))
    return f


def default_params(algo):
    p = Params()
    lib().bbo_params_default(C.byref(p), algo)
    return p
