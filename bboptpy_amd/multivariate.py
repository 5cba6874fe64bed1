"""Python class surface of the reference, over the HIP C ABI.

Mirrors the pybind11 module `_bboptpy` for the algorithms on the hot path
(/root/reference/py/multivariate_py.cpp): same class names, the same class hierarchy
(ActiveCMAES -> CMAES -> BaseCMAES -> MultivariateSearch, :99-115), the same positional
order, keyword names and defaults of every constructor (:103-171, :265-269), the four
methods optimize / initialize / iterate / solution (:376-420) and the MultivariateSolution
result object (:360-371).  Every constructor additionally accepts keyword-only extensions
that have no reference counterpart: `seed` (Philox key; default = fresh entropy, like the
reference's random_device seeding), `device`, `populations`, and `poll_every`
(CholeskyCMAES also `ranked`).

All computation happens in libbbopt_hip.so on the GPU.  A Python callable objective is
supported through the host-callback path (X leaves HBM once per generation); the objects in
`bboptpy_amd.objectives` select the built-in on-device objectives instead.
"""
import ctypes as C
import enum
import os
import sys

import numpy as _np

from . import _ffi
from .objectives import Builtin, DeviceObjective


class MultivariateSolution:
    """result record, multivariate.h:81-115 / multivariate_py.cpp:360-371"""

    def __init__(self, x, n_evals, converged):
        self._x = _np.array(x, dtype=_np.float64)
        self._n_evals = int(n_evals)
        self._converged = bool(converged)

    @property
    def x(self):
        return self._x.copy()   # the reference returns a fresh array each time (:362-364)

    @property
    def converged(self):
        return self._converged

    @property
    def n_evals(self):
        return self._n_evals

    def __str__(self):
        # multivariate_solution::toString, multivariate.h:97-114 (std::to_string == "%f")
        sol = "".join("%f " % v for v in self._x)
        return ("x*: " + sol + "\n"
                + "objective calls: %d\n" % self._n_evals
                + "constraint calls: 0\n"
                + "B/B constraint calls: 0\n"
                + "converged: " + ("yes" if self._converged else "no/unknown"))

    def __repr__(self):
        return "<MultivariateSolution n_evals=%d converged=%s>" % (self._n_evals,
                                                                   self._converged)


def _as_vec(a, name):
    v = _np.ascontiguousarray(_np.asarray(a, dtype=_np.float64)).ravel()
    if v.size == 0:
        raise ValueError("%s must not be empty" % name)
    return v


class _ObjectiveBinding:
    """keeps the ctypes callback (and the user's callable) alive for the handle's life,
    like the std::function captured by value in multivariate_py.cpp:385-388"""

    def __init__(self, f, n):
        self.error = None
        self.struct = _ffi.Objective()
        self._keep = None
        if isinstance(f, DeviceObjective):
            self._keep = f       # the program lives as long as the optimizer holds this binding
            self.struct.kind = _ffi.OBJ_PROGRAM
            self.struct.user = f._handle
            return
        if isinstance(f, Builtin):
            self.struct.kind = _ffi.OBJ_BUILTIN
            self.struct.builtin = f.builtin_id
            return
        if isinstance(f, str):
            if f not in _ffi.BUILTIN_IDS:
                raise ValueError("unknown built-in objective %r" % f)
            self.struct.kind = _ffi.OBJ_BUILTIN
            self.struct.builtin = _ffi.BUILTIN_IDS[f]
            return
        if not callable(f):
            raise TypeError("objective must be callable or a built-in objective")
        binding = self
        if getattr(f, "_bbo_vectorized", False):
            def batch(xptr, rows, ncol, ld, fout, user):
                try:
                    X = _np.ctypeslib.as_array(xptr, shape=(rows, ld))[:, :ncol].copy()
                    vals = _np.asarray(f(X), dtype=_np.float64).ravel()
                    if vals.size != rows:
                        raise ValueError("vectorized objective returned %d values for %d rows"
                                         % (vals.size, rows))
                    _np.ctypeslib.as_array(fout, shape=(rows,))[:] = vals
                    return 0
                except BaseException as e:   # propagate like pybind's error_already_set
                    binding.error = e
                    return 1
            self._keep = _ffi.BATCH_FN(batch)
            self.struct.kind = _ffi.OBJ_BATCH_CB
            self.struct.batch = self._keep
        else:
            def scalar(xptr, ncol, user, failed):
                try:
                    x = _np.ctypeslib.as_array(xptr, shape=(ncol,)).copy()
                    return float(f(x))
                except BaseException as e:
                    binding.error = e
                    failed[0] = 1
                    return 0.0
            self._keep = _ffi.SCALAR_FN(scalar)
            self.struct.kind = _ffi.OBJ_SCALAR_CB
            self.struct.scalar = self._keep


# (the same list, in the library's words: Engine::reject_program, csrc/bbo_engine.hpp)
PROGRAM_FAMILIES = ("CMAES, ActiveCMAES, SepCMAES, CholeskyCMAES (and IPopCMAES / BiPopCMAES over them), "
                    "JADE, SHADE, SANSDE, PIKAIA")


class MultivariateSearch:
    """MultivariateOptimizer (multivariate.h:132-146) as bound at multivariate_py.cpp:374-420"""

    _algo = None
    _accepts_program = False     # DeviceObjective: the CMA-ES and DE families
    # the engine's prefix in the C ABI where it has an extension struct: the struct is self._<prefix>, handed
    # to bbo_<prefix>_configure when the handle is made; bbo_<prefix>_phase is what _phase() calls
    _extension = None

    def __init__(self, *, seed=None, device=0, populations=1, poll_every=None):
        _ffi.lib()   # fail loudly at construction when the HIP library is missing
        self._params = _ffi.default_params(self._algo)
        if poll_every is not None:      # generations between host polls of the stop flags in run()
            self._params.poll_every = max(1, int(poll_every))
        if seed is None:
            seed = int.from_bytes(os.urandom(8), "little")
        self._params.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self._params.device = int(device)
        self._params.populations = int(populations)
        self._handle = None
        self._binding = None
        self._n = None
        self._record_draws = False      # (extension of some engines) set_state("record_draws") at initialize()

    # -- handle management --------------------------------------------------------
    def _create(self):
        L = _ffi.lib()
        h = C.c_void_p()
        _ffi.check(L.bbo_create(C.byref(self._params), C.byref(h)))
        if self._extension is not None:
            configure = getattr(L, "bbo_%s_configure" % self._extension)
            status = configure(h, C.byref(getattr(self, "_" + self._extension)))
            if status < 0:
                msg = L.bbo_last_error(h)
                L.bbo_destroy(h)
                raise _ffi.BboError(status, msg.decode() if msg else "")
        return h

    def _ensure_handle(self):
        if self._handle is None:
            self._handle = self._create()
        return self._handle

    def __del__(self):
        try:
            if getattr(self, "_handle", None) is not None:
                _ffi.lib().bbo_destroy(self._handle)
                self._handle = None
        except Exception:
            pass

    def reseed(self, seed):
        """(extension) a new generator seed for the next initialize() / optimize(); the handle
        is re-created (the seed is part of bbo_params)"""
        self._params.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        if self._handle is not None:
            _ffi.lib().bbo_destroy(self._handle)
            self._handle = None

    def _check(self, status):
        if status < 0:
            err = self._binding.error if self._binding is not None else None
            if err is not None:
                self._binding.error = None
                raise err
            _ffi.check(status, self._handle)
        return status

    def _problem(self, f, lower, upper, guess):
        lower = _as_vec(lower, "lower")
        n = lower.size            # like the reference, n comes from `lower` (:380)
        upper = _as_vec(upper, "upper")
        guess = _as_vec(guess, "guess")
        pops = self._params.populations
        if upper.size < n or guess.size < n * pops:
            raise ValueError("upper/guess are shorter than lower (n = %d)" % n)
        if isinstance(f, DeviceObjective) and not self._accepts_program:
            raise ValueError("%s does not take a DeviceObjective yet: objective programs are supported by %s"
                             % (type(self).__name__, PROGRAM_FAMILIES))
        self._binding = _ObjectiveBinding(f, n)
        self._n = n
        return n, lower, _np.ascontiguousarray(upper[:n]), _np.ascontiguousarray(
            guess[:n * pops])

    # -- the four reference methods --------------------------------------------------
    def optimize(self, f, lower, upper, guess):
        n, lower, upper, guess = self._problem(f, lower, upper, guess)
        h = self._ensure_handle()
        x = _np.zeros(n)
        fev, conv = C.c_int(), C.c_int()
        self._check(_ffi.lib().bbo_optimize(h, n, lower, upper, guess,
                                            C.byref(self._binding.struct), x,
                                            C.byref(fev), C.byref(conv)))
        return MultivariateSolution(x, fev.value, conv.value)

    def initialize(self, f, lower, upper, guess):
        n, lower, upper, guess = self._problem(f, lower, upper, guess)
        h = self._ensure_handle()
        self._check(_ffi.lib().bbo_init(h, n, lower, upper, guess,
                                        C.byref(self._binding.struct)))
        if self._record_draws:
            self.set_state("record_draws", [1.])

    def iterate(self):
        if self._handle is None:
            raise RuntimeError("iterate() called before initialize()")
        self._check(_ffi.lib().bbo_iterate(self._handle))

    def solution(self, population=0):
        if self._handle is None:
            raise RuntimeError("solution() called before initialize()")
        x = _np.zeros(self._n)
        fev, conv = C.c_int(), C.c_int()
        self._check(_ffi.lib().bbo_solution_of(self._handle, int(population), x,
                                               C.byref(fev), C.byref(conv)))
        return MultivariateSolution(x, fev.value, conv.value)

    # -- extensions ---------------------------------------------------------------------
    def run(self, max_generations):
        """advance up to max_generations on the device without returning to Python;
        returns the number of generations launched"""
        if self._handle is None:
            raise RuntimeError("run() called before initialize()")
        done = C.c_int()
        self._check(_ffi.lib().bbo_run(self._handle, int(max_generations), C.byref(done)))
        return done.value

    def get_state(self, key, population=0):
        """named optimizer state as a float64 array (keys: DESIGN.md)"""
        if self._handle is None:
            raise RuntimeError("get_state() called before initialize()")
        L = _ffi.lib()
        cnt = self._check(L.bbo_get(self._handle, key.encode(), population, None, 0))
        out = _np.zeros(max(cnt, 1))
        self._check(L.bbo_get(self._handle, key.encode(), population,
                              out.ctypes.data_as(C.c_void_p), cnt))
        return out[:cnt]

    def set_state(self, key, value, population=0):
        v = _np.ascontiguousarray(_np.asarray(value, dtype=_np.float64)).ravel()
        self._check(_ffi.lib().bbo_set(self._handle, key.encode(), population, v, v.size))

    # -- what the engines' extension methods are made of ---------------------------------
    def _phase(self, which):
        self._check(getattr(_ffi.lib(), "bbo_%s_phase" % self._extension)(self._handle, int(which)))

    def _inject(self, fn_name, table):
        """a table of draws for the generations that follow; None: the device draws"""
        fn = getattr(_ffi.lib(), fn_name)
        if table is None:
            self._check(fn(self._handle, None, 0))
            return
        t = _np.ascontiguousarray(_np.asarray(table, dtype=_np.float64)).ravel()
        self._check(fn(self._handle, t.ctypes.data_as(C.c_void_p), t.size))

    def _pending(self):
        """the populations that have a point waiting for its value"""
        return sum(int(self.get_state("pending", p)[0]) for p in range(self._params.populations))

    @staticmethod
    def _require_finite_box(n, lower, upper, what):
        if not (_np.isfinite(lower[:n]).all() and _np.isfinite(upper[:n]).all()):
            raise ValueError("%s: the bounds must be finite" % what)


class BaseCMAES(MultivariateSearch):
    """BaseCmaes, multivariate_py.cpp:99-101 (abstract in the reference)"""
    _accepts_program = True

    def phase(self, which):
        self._check(_ffi.lib().bbo_cma_phase_run(self._handle, int(which)))

    def set_params(self, np, sigma0, mfev):
        """BaseCmaes::setParams (base_cmaes.cpp:136-148; not bound to Python by the reference,
        used by its restart drivers): new lambda, sigma0 and budget for the next initialize() /
        optimize() of this object, which keeps B and C's off-diagonals (cmaes.cpp:53-59)"""
        p = self._params
        p.np, p.sigma0, p.mfev = int(np), float(sigma0), int(mfev)
        if self._handle is not None:
            self._check(_ffi.lib().bbo_cma_set_params(self._handle, p.np, p.sigma0, p.mfev))
        if p.bound:
            p.bound = 0     # the handle printed the reference's warning (or will not need to)

    def set_seed(self, seed):
        """(extension) a new Philox key WITHOUT re-creating the handle (reseed() does)"""
        self._params.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        if self._handle is not None:
            self._check(_ffi.lib().bbo_cma_set_seed(self._handle, self._params.seed))

    def evaluate(self, x):
        """the bound objective at one point (the restart drivers' extra evaluation,
        bipop_cmaes.cpp:86)"""
        if self._handle is None:
            raise RuntimeError("evaluate() called before initialize()")
        x = _np.ascontiguousarray(_np.asarray(x, dtype=_np.float64)).ravel()
        if x.size != self._n:
            raise ValueError("evaluate: x must have n = %d coordinates" % self._n)
        out = C.c_double()
        self._check(_ffi.lib().bbo_cma_evaluate(self._handle, x, C.byref(out)))
        return out.value

    def inject_normals(self, z):
        self._inject("bbo_cma_inject_normals", z)


class CMAES(BaseCMAES):
    """CMAES(mfev, tol, np, sigma0=2., bound=False, eigenrate=0.25) -- :103-108"""
    _algo = _ffi.ALGO_CMAES

    def __init__(self, mfev, tol, np, sigma0=2., bound=False, eigenrate=0.25, **ext):
        super().__init__(**ext)
        p = self._params
        p.mfev, p.tol, p.np = int(mfev), float(tol), int(np)
        p.sigma0, p.bound, p.eigenrate = float(sigma0), int(bool(bound)), float(eigenrate)


class ActiveCMAES(CMAES):
    """ActiveCMAES(mfev, tol, np, sigma0=2., bound=False, alphacov=2., eigenrate=0.25)
    -- :110-115"""
    _algo = _ffi.ALGO_ACTIVE_CMAES

    def __init__(self, mfev, tol, np, sigma0=2., bound=False, alphacov=2., eigenrate=0.25,
                 **ext):
        super().__init__(mfev, tol, np, sigma0, bound, eigenrate, **ext)
        self._params.alphacov = float(alphacov)


class SepCMAES(BaseCMAES):
    """SepCMAES(mfev, tol, np, sigma0=2., bound=False, adjustlr=True) -- :131-135
    (diagonal covariance, Ros & Hansen 2008; sep_cmaes.cpp)"""
    _algo = _ffi.ALGO_SEP_CMAES

    def __init__(self, mfev, tol, np, sigma0=2., bound=False, adjustlr=True, **ext):
        super().__init__(**ext)
        p = self._params
        p.mfev, p.tol, p.np = int(mfev), float(tol), int(np)
        p.sigma0, p.bound, p.adjustlr = float(sigma0), int(bool(bound)), int(bool(adjustlr))


class CholeskyCMAES(BaseCMAES):
    """CholeskyCMAES(mfev, tol, stol, np, sigma0=2., bound=False) -- :118-120
    (Cholesky-factor CMA-ES without eigendecomposition, Krause, Arbones, Igel 2016;
    cholesky_cmaes.cpp).  Keyword-only extension `ranked` (default False = the reference): the
    rank-mu term of the factor update takes the mu best candidates about the old mean instead of
    the reference's first mu in sampling order about the new mean."""
    _algo = _ffi.ALGO_CHOLESKY_CMAES

    def __init__(self, mfev, tol, stol, np, sigma0=2., bound=False, **ext):
        ranked = ext.pop("ranked", False)
        super().__init__(**ext)
        p = self._params
        p.mfev, p.tol, p.stol, p.np = int(mfev), float(tol), float(stol), int(np)
        p.sigma0, p.bound, p.ranked = float(sigma0), int(bool(bound)), int(bool(ranked))


class LmCMAES(BaseCMAES):
    """LmCMAES(mfev, tol, np, memory=0, sigma0=2., bound=False, rademacher=True, usenew=True) -- :123-128
    (limited-memory CMA-ES, Loshchilov 2014 / 2015; lm_cmaes.cpp): m direction vectors instead of a
    covariance matrix, O(m n) per candidate, n up to 4096.  memory <= 0 means m = int(2 sqrt(n)).
    `bound` clamps the mean to the box and never a candidate, as in the reference.  An engine of its
    own: no base of IPopCMAES / BiPopCMAES and no objective programs yet, and the methods BaseCMAES
    adds for the restart drivers (set_params, set_seed, evaluate) and inject_normals raise
    NotImplementedError; the draws are injected with inject_draws."""
    _algo = _ffi.ALGO_LM_CMAES
    _extension = "lm"
    _accepts_program = False

    def __init__(self, mfev, tol, np, memory=0, sigma0=2., bound=False, rademacher=True, usenew=True, **ext):
        super().__init__(**ext)
        p = self._params
        p.mfev, p.tol, p.np = int(mfev), float(tol), int(np)
        p.sigma0, p.bound = float(sigma0), int(bool(bound))
        s = self._lm = _ffi.LmParams()
        s.memory, s.rademacher, s.usenew = int(memory), int(bool(rademacher)), int(bool(usenew))

    def phase(self, which):
        """one part of a generation: 0 sample, 1 evaluate, 2 rank, 3 update of mean / pc / memory /
        sigma, 4 history + counters + stop test"""
        self._phase(which)

    def inject_draws(self, table):
        """the draws of the following G generations, [G][populations][ceil(np / 2)][n + 1]: per "+"
        candidate its z (normals, or +-1) and the normal of the subset selection (ignored where the
        reference draws none); None: the device draws"""
        self._inject("bbo_lm_inject_draws", table)

    def _not_here(self, what):
        raise NotImplementedError("LmCMAES has no %s: it runs on an engine of its own, outside the "
                                  "restart drivers' CMA-ES engine" % what)

    def inject_normals(self, z):
        self._not_here("inject_normals (use inject_draws)")

    def set_params(self, np, sigma0, mfev):
        self._not_here("set_params")

    def set_seed(self, seed):
        self._not_here("set_seed (use reseed)")

    def evaluate(self, x):
        self._not_here("evaluate")


class _RestartDriver(MultivariateSearch):
    _accepts_program = True

    def __init__(self, base, **ext):
        if isinstance(base, LmCMAES):
            raise TypeError("LmCMAES is no base of a restart driver yet: base must be a CMAES, ActiveCMAES, "
                            "SepCMAES or CholeskyCMAES optimizer")
        if not isinstance(base, BaseCMAES):
            raise TypeError("base must be a CMA-ES optimizer (CMAES / ActiveCMAES / SepCMAES / "
                            "CholeskyCMAES)")
        if base._params.populations != 1:
            raise ValueError("restart drivers need a base optimizer with populations=1")
        super().__init__(**ext)
        self._base = base   # kept alive here; the reference only borrows the pointer
        self._base_handle = None

    def _create(self):
        h = C.c_void_p()
        base_h = self._base._ensure_handle()
        _ffi.check(_ffi.lib().bbo_create_restart(C.byref(self._params), base_h, C.byref(h)))
        self._base_handle = base_h
        return h

    def _ensure_handle(self):
        # the driver's handle borrows the base's engine: if the base re-created its handle
        # (reseed()), the driver's is stale and is rebuilt over the new one
        if self._handle is not None and self._base._handle is not self._base_handle:
            _ffi.lib().bbo_destroy(self._handle)
            self._handle = None
        return super()._ensure_handle()

    def _live(self):
        if self._handle is not None and self._base._handle is not self._base_handle:
            raise RuntimeError("the base optimizer was re-created (reseed) after this restart "
                               "driver was initialized: call initialize() / optimize() again")

    def iterate(self):
        self._live()
        super().iterate()

    def run(self, max_generations):
        self._live()
        return super().run(max_generations)


class IPopCMAES(_RestartDriver):
    """IPopCMAES(base, mfev, print=False, sigma0=2., nipop=True, ksigmadec=1.6,
    boundlambda=True) -- :137-142"""
    _algo = _ffi.ALGO_IPOP

    def __init__(self, base, mfev, print=False, sigma0=2., nipop=True, ksigmadec=1.6,
                 boundlambda=True, **ext):
        super().__init__(base, **ext)
        p = self._params
        p.mfev, p.print, p.sigma0 = int(mfev), int(bool(print)), float(sigma0)
        p.nipop, p.ksigmadec, p.boundlambda = int(bool(nipop)), float(ksigmadec), int(
            bool(boundlambda))


class BiPopCMAES(_RestartDriver):
    """BiPopCMAES(base, mfev, print=False, sigma0=2., maxlargeruns=9, nbipop=True,
    ksigmadec=1.6, kbudget=2.) -- :144-151"""
    _algo = _ffi.ALGO_BIPOP

    def __init__(self, base, mfev, print=False, sigma0=2., maxlargeruns=9, nbipop=True,
                 ksigmadec=1.6, kbudget=2., **ext):
        super().__init__(base, **ext)
        p = self._params
        p.mfev, p.print, p.sigma0 = int(mfev), int(bool(print)), float(sigma0)
        p.maxlargeruns, p.nipop = int(maxlargeruns), int(bool(nbipop))
        p.ksigmadec, p.kbudget = float(ksigmadec), float(kbudget)


class JADE(MultivariateSearch):
    """JADE(mfev, np, tol, archive=True, repaircr=True, pelite=0.05, cdamp=0.1, sigma=0.07)
    -- :159-164"""
    _algo = _ffi.ALGO_JADE
    _accepts_program = True

    def __init__(self, mfev, np, tol, archive=True, repaircr=True, pelite=0.05, cdamp=0.1,
                 sigma=0.07, **ext):
        super().__init__(**ext)
        p = self._params
        p.mfev, p.np, p.tol = int(mfev), int(np), float(tol)
        p.archive, p.repaircr = int(bool(archive)), int(bool(repaircr))
        p.pelite, p.cdamp, p.jade_sigma = float(pelite), float(cdamp), float(sigma)


class SHADE(MultivariateSearch):
    """SHADE(mfev, npinit, tol, archive=True, repaircr=True, h=100, npmin=4) -- :166-171"""
    _algo = _ffi.ALGO_SHADE
    _accepts_program = True

    def __init__(self, mfev, npinit, tol, archive=True, repaircr=True, h=100, npmin=4, **ext):
        super().__init__(**ext)
        p = self._params
        p.mfev, p.np, p.tol = int(mfev), int(npinit), float(tol)
        p.archive, p.repaircr, p.h, p.npmin = int(bool(archive)), int(bool(repaircr)), int(
            h), int(npmin)


class SANSDE(MultivariateSearch):
    """SANSDE(mfev, np, tol, repaircr=True, crref=5, pupdate=50, crupdate=25) -- :174-177
    (self-adaptive DE with neighbourhood search, Yang et al. 2008; sansde.cpp)"""
    _algo = _ffi.ALGO_SANSDE
    _accepts_program = True

    def __init__(self, mfev, np, tol, repaircr=True, crref=5, pupdate=50, crupdate=25, **ext):
        super().__init__(**ext)
        p = self._params
        p.mfev, p.np, p.tol = int(mfev), int(np), float(tol)
        p.repaircr = int(bool(repaircr))
        p.crref, p.pupdate, p.crupdate = int(crref), int(pupdate), int(crupdate)


class CSO(MultivariateSearch):
    """CSO(mfev, stol, np, pcompete=3, ring=False, correct=True, vmax=0.2) -- :272-275
    (competitive swarm optimizer, Cheng & Jin 2015; cso.cpp)"""
    _algo = _ffi.ALGO_CSO

    def __init__(self, mfev, stol, np, pcompete=3, ring=False, correct=True, vmax=0.2, **ext):
        super().__init__(**ext)
        p = self._params
        p.mfev, p.tol, p.np = int(mfev), float(stol), int(np)
        p.pcompete, p.ring = int(pcompete), int(bool(ring))
        p.correct, p.vmax = int(bool(correct)), float(vmax)


class CCPSO(MultivariateSearch):
    """CCPSO(mfev, sigmatol, np, pps, npps, correct=True, pcauchy=-1., local=None, localfreq=10)
    -- :291-295 (cooperatively coevolving PSO, Li & Yao 2012; ccpso.cpp).  `pps` lists the
    candidate swarm sizes (each must divide n).

    `local` (ccpso.cpp:116-118, 371-435): another optimizer.  Every `localfreq` generations one
    weight per swarm, scaling that swarm's coordinates of the context vector, is optimized by it
    inside the box that keeps the scaled vector in bounds, and the result replaces the context
    vector if it is better.  The generations run on the device; the search's objective evaluates
    on the host (the callable itself, or the built-in's formula), one population only.  Each
    search starts `local` afresh with the seed base + search index (the reference's CMA-ES
    objects start from the previous search's matrices, cmaes.cpp:53-54 -- not reproduced).
    A CMA-ES optimizer of THIS package is handed to the library (bbo_ccpso_set_local: the whole
    loop then runs behind bbo_iterate / bbo_optimize, as for a C caller); any other object with
    optimize(f, lower, upper, guess) -> solution carrying .x and .n_evals is driven from here
    between device generations through bbo_get / bbo_set."""
    _algo = _ffi.ALGO_CCPSO

    def __init__(self, mfev, sigmatol, np, pps, npps=None, correct=True, pcauchy=-1., local=None,
                 localfreq=10, **ext):
        super().__init__(**ext)
        pps = [int(v) for v in pps]
        npps = len(pps) if npps is None else int(npps)
        if not 1 <= npps <= min(16, len(pps)):
            raise ValueError("CCPSO: npps must be in [1, min(16, len(pps))]")
        p = self._params
        p.mfev, p.tol, p.np = int(mfev), float(sigmatol), int(np)
        p.npps = npps
        for k in range(npps):
            p.pps[k] = pps[k]
        p.correct, p.pcauchy = int(bool(correct)), float(pcauchy)
        if local is not None:
            if not callable(getattr(local, "optimize", None)):
                raise TypeError("CCPSO: local must provide optimize(f, lower, upper, guess)")
            if p.populations != 1:
                raise ValueError("CCPSO: the local optimizer works on one population")
        self._local, self._localfreq = local, int(localfreq)
        self._nlocal = 0
        self._local_seed0 = getattr(getattr(local, "_params", None), "seed", 0)
        # a CMA-ES object of this package: the search runs inside the library
        self._local_native = isinstance(local, BaseCMAES)
        self._local_handle = None

    def _attach_local(self):
        """(native local optimizer) hand its handle to the engine; again whenever either handle
        has been re-created"""
        lh = self._local._ensure_handle()
        if self._local_handle is not lh:
            self._check(_ffi.lib().bbo_ccpso_set_local(self._handle, lh, self._localfreq))
            self._local_handle = lh

    def _create(self):
        h = super()._create()
        self._local_handle = None
        return h

    def __del__(self):
        # detach first: the engine only borrows the local optimizer's handle
        try:
            if getattr(self, "_handle", None) is not None and getattr(self, "_local_native", False):
                _ffi.lib().bbo_ccpso_set_local(self._handle, None, 0)
        except Exception:
            pass
        super().__del__()

    # ---- swarm groups sharded over GPUs (bboptpy_amd.distributed.ShardedCCPSO) ---------------
    def set_shard(self, rank, world):
        """this object evaluates the swarms [nswarm rank / world, nswarm (rank + 1) / world)"""
        self._check(_ffi.lib().bbo_ccpso_set_shard(self._ensure_handle(), int(rank), int(world)))

    def phase(self, which):
        """0: regroup + evaluate this rank's swarms; 1: the rest of the generation"""
        self._check(_ffi.lib().bbo_ccpso_phase(self._handle, int(which)))

    def table_record(self):
        return self._check(_ffi.lib().bbo_ccpso_table_record(self._handle))

    def export_tables(self, out=None, device_ptr=None):
        """this rank's fitness record (fX | fY) into a host array, or to a device pointer"""
        if device_ptr is not None:
            self._check(_ffi.lib().bbo_ccpso_export_tables(self._handle, C.c_void_p(device_ptr), 1))
            return None
        if out is None:
            out = _np.zeros(self.table_record())
        self._check(_ffi.lib().bbo_ccpso_export_tables(self._handle,
                                                       out.ctypes.data_as(C.c_void_p), 0))
        return out

    def merge_tables(self, gathered=None, world=1, device_ptr=None):
        """every swarm's rows from the record of the rank that evaluated it"""
        if device_ptr is not None:
            self._check(_ffi.lib().bbo_ccpso_merge_tables(self._handle, C.c_void_p(device_ptr),
                                                          int(world), 1))
            return
        g = _np.ascontiguousarray(gathered, dtype=_np.float64)
        self._check(_ffi.lib().bbo_ccpso_merge_tables(self._handle, g.ctypes.data_as(C.c_void_p),
                                                      int(world), 0))

    # ---- the reference's loop with the local search between generations ------------------
    def initialize(self, f, lower, upper, guess):
        if self._local is not None and self._local_native:
            self._ensure_handle()
            self._attach_local()
            return super().initialize(f, lower, upper, guess)
        super().initialize(f, lower, upper, guess)
        if isinstance(f, str):
            from . import objectives as _objectives
            f = getattr(_objectives, f, None)
        self._f_host = f if callable(f) else None
        self._lower_h, self._upper_h = _as_vec(lower, "lower"), _as_vec(upper, "upper")[:self._n]
        self._nlocal = 0

    def iterate(self):
        if self._local is not None and self._local_native:
            self._attach_local()
            return super().iterate()
        gen = int(self.get_state("it")[0]) if self._local is not None else 0
        super().iterate()
        if self._local is not None and self._localfreq > 0 and gen % self._localfreq == 0:
            self._local_search()

    def run(self, max_generations):
        if self._local is not None and not self._local_native:
            raise RuntimeError("CCPSO.run() with a local optimizer driven from Python: use iterate()")
        if self._local is not None:
            self._attach_local()
        return super().run(max_generations)

    def optimize(self, f, lower, upper, guess):
        if self._local is None:
            return super().optimize(f, lower, upper, guess)
        if self._local_native:
            self._ensure_handle()
            self._attach_local()
            return super().optimize(f, lower, upper, guess)
        self.initialize(f, lower, upper, guess)
        mfev = self._params.mfev
        while True:                                   # ccpso.cpp:135-148
            self.iterate()
            if int(self.get_state("fev")[0]) >= mfev:
                converged = False
                break
            if int(self.get_state("conv")[0]):
                converged = True
                break
        return MultivariateSolution(self.get_state("yhat"), int(self.get_state("fev")[0]),
                                    converged)

    def _local_search(self):
        """CCPSOSearch::localSearch, ccpso.cpp:371-435"""
        n = self._n
        f = self._f_host
        if f is None:
            raise RuntimeError("CCPSO: the local optimizer needs a callable objective")
        yhat = self.get_state("yhat")
        k = self.get_state("k").astype(int)           # position -> coordinate, swarm-major
        cps, nsw = int(self.get_state("cpswarm")[0]), int(self.get_state("nswarm")[0])
        group = _np.empty(n, dtype=int)
        group[k] = _np.repeat(_np.arange(nsw), cps)
        scale = _np.where(_np.abs(yhat) < 1e-3, _np.where(yhat > 0., 1e-3, -1e-3), yhat)
        lb, ub = self._lower_h / scale, self._upper_h / scale
        lb, ub = _np.minimum(lb, ub), _np.maximum(lb, ub)
        wlb = _np.full(nsw, -_np.inf)
        wub = _np.full(nsw, _np.inf)
        _np.maximum.at(wlb, group, lb)
        _np.minimum.at(wub, group, ub)
        wguess = _np.maximum(wlb, _np.minimum(1., wub))

        def faux(w):
            return float(f(yhat * _np.asarray(w, dtype=_np.float64)[group]))

        if hasattr(self._local, "reseed"):
            self._local.reseed(self._local_seed0 + self._nlocal)
        self._nlocal += 1
        sol = self._local.optimize(faux, wlb, wub, wguess)
        w = _np.asarray(sol.x, dtype=_np.float64)
        fev = int(self.get_state("fev")[0]) + int(sol.n_evals)
        trial = yhat * w[group]
        inside = (not self._params.correct) or bool(
            _np.all((trial >= self._lower_h) & (trial <= self._upper_h)))
        if inside:
            fwy = float(f(trial))
            fev += 1
            if fwy < float(self.get_state("fyhat")[0]):
                self.set_state("yhat", trial)
                self.set_state("fyhat", [fwy])
                self.set_state("improved", [1.])
        self.set_state("fev", [float(fev)])


class JAYA(MultivariateSearch):
    """JAYA(mfev, tol, np, npmin, adapt=True, k0=2, mutation=JAYA.JAYA_Mutation.logistic,
    scale=0.01, beta=1.5, kcheb=2, temper=10.) -- :213-234 (self-adaptive multi-population Jaya
    with Levy-flight and chaotic mutations, Rao 2016, Rao & Saroj 2017; jaya.cpp).  `guess` is
    ignored, as in the reference; `kcheb` is stored and unused, as in the reference."""
    _algo = _ffi.ALGO_JAYA
    _extension = "jaya"

    class JAYA_Mutation(enum.IntEnum):
        """JayaSearch::jaya_mutation_method, bound with export_values (:214-219)"""
        original = 0
        levy = 1
        tent_map = 2
        logistic = 3

    original, levy, tent_map, logistic = (JAYA_Mutation.original, JAYA_Mutation.levy,
                                          JAYA_Mutation.tent_map, JAYA_Mutation.logistic)

    def __init__(self, mfev, tol, np, npmin, adapt=True, k0=2, mutation=JAYA_Mutation.logistic,
                 scale=0.01, beta=1.5, kcheb=2, temper=10., **ext):
        super().__init__(**ext)
        p = self._params
        p.mfev, p.tol, p.np, p.npmin = int(mfev), float(tol), int(np), int(npmin)
        j = self._jaya = _ffi.JayaParams()
        j.adapt, j.k0, j.mutation = int(bool(adapt)), int(k0), int(self.JAYA_Mutation(mutation))
        j.kcheb, j.scale, j.beta, j.temper = int(kcheb), float(scale), float(beta), float(temper)


class DSA(MultivariateSearch):
    """DSA(mfev, tol, stol, np, adapt=True, nbatch=100) -- :189-191 (Differential Search,
    Civicioglu 2012, with the reference's Rexp3 bandit over the four direction methods; ds.cpp).
    `guess` is ignored, as in the reference."""
    _algo = _ffi.ALGO_DSA
    _extension = "dsa"

    def __init__(self, mfev, tol, stol, np, adapt=True, nbatch=100, **ext):
        super().__init__(**ext)
        p = self._params
        p.mfev, p.tol, p.stol, p.np = int(mfev), float(tol), float(stol), int(np)
        d = self._dsa = _ffi.DsaParams()
        d.adapt, d.nbatch = int(bool(adapt)), int(nbatch)


class HEES(MultivariateSearch):
    """HEES(mfev, tol, mres=1, print=False, np=0, sigma0=2.) -- :206-211 (Hessian Estimation
    Evolution Strategy, Glasmachers & Krause 2020; hees.cpp).  `np` is mu, the number of mirrored
    pairs: 2 np + 1 evaluations per generation; np = 0 means int(2 + 1.5 ln n).  optimize() with
    mres > 1 restarts with doubled np from uniform points of the box (a finite box, populations=1);
    initialize / iterate / run ignore mres, as in the reference.  The bounds never clamp."""
    _algo = _ffi.ALGO_HEES
    _extension = "hees"

    def __init__(self, mfev, tol, mres=1, print=False, np=0, sigma0=2., **ext):
        super().__init__(**ext)
        p = self._params
        p.mfev, p.tol, p.np, p.sigma0 = int(mfev), float(tol), int(np), float(sigma0)
        h = self._hees = _ffi.HeesParams()
        h.mres, h.print = int(mres), int(bool(print))
        if h.mres > 1 and p.populations != 1:
            raise ValueError("HEES: restarts (mres > 1) work on populations=1 only")

    def optimize(self, f, lower, upper, guess):
        if self._hees.print:
            sys.stdout.flush()      # the table is written by the library
        return super().optimize(f, lower, upper, guess)

    def phase(self, which):
        """one part of a generation: 0 sample + evaluate, 1 rank, 2 update, 3 finish"""
        self._phase(which)

    def inject_normals(self, z):
        """the normals of the following generations: per population the reference's (B n) x n
        table, B = ceil(mu / n), of which the first mu rows are used; None: the device draws"""
        self._inject("bbo_hees_inject_normals", z)


class xNES(MultivariateSearch):
    """xNES(mfev, tol, a0=1., etamu=1.) -- the exponential natural evolution strategy (Glasmachers et
    al. 2010; xnes.cpp).  The population size is 4 + int(3 ln n).  As in the reference the mean starts
    at the ORIGIN with sigma = a0 and `guess` and the bounds are not used; from_guess=True (an
    extension, keyword-only) starts the mean at `guess`.  solution() is the best point of the last
    generation; get_state("xbest") / ("fbest") hold the best ever seen.  n is at most 512."""
    _algo = _ffi.ALGO_XNES
    _extension = "xnes"

    def __init__(self, mfev, tol, a0=1., etamu=1., *, from_guess=False, **ext):
        super().__init__(**ext)
        p = self._params
        p.mfev, p.tol = int(mfev), float(tol)
        x = self._xnes = _ffi.XnesParams()
        x.a0, x.etamu, x.from_guess = float(a0), float(etamu), int(bool(from_guess))

    def phase(self, which):
        """one part of a generation: 0 sample + evaluate, 1 rank, 2 small step, 3 adapt"""
        self._phase(which)

    def inject_normals(self, z):
        """the normals of the following G generations, [G][populations][np][n] in sampling order;
        None: the device draws"""
        self._inject("bbo_xnes_inject_normals", z)


class AMALGAM(MultivariateSearch):
    """AMALGAM(mfev, tol, stol, np=0, iamalgam=True, noparam=True, print=True) -- AMaLGaM-IDEA and
    iAMaLGaM-IDEA (Bosman, Grahl & Thierens 2009; amalgam.cpp).  np = 0 means int(10 sqrt n) for
    iAMaLGaM and int(17 + 3 n^1.5) for AMaLGaM.  The population starts uniform in the box (a finite box
    is mandatory); `guess` is not read.  As in the reference the sampler redraws the x of the elite
    row 0 and keeps its old value, and solution() is that row; keep_elite=True (an extension,
    keyword-only) leaves its x alone.  get_state("xbest") / ("fbest") hold the best point ever
    evaluated.  noparam=True, the default, is the parameter-free mode: iterate() is one stage of
    2^(s/2) inner runs on growing populations, run as the populations of one inner handle
    (concurrent=True) or one after another (concurrent=False) with the same results; it needs
    populations=1 and print=True writes the reference's table.  n is at most 512, np in [3, 65536]."""
    _algo = _ffi.ALGO_AMALGAM
    _extension = "amalgam"
    _accepts_program = False

    def __init__(self, mfev, tol, stol, np=0, iamalgam=True, noparam=True, print=True, *,
                 keep_elite=False, concurrent=True, **ext):
        substream = ext.pop("substream", 0)
        super().__init__(**ext)
        p = self._params
        p.mfev, p.tol, p.stol, p.np = int(mfev), float(tol), float(stol), int(np)
        a = self._amalgam = _ffi.AmalgamParams()
        a.iamalgam, a.noparam, a.print = int(bool(iamalgam)), int(bool(noparam)), int(bool(print))
        a.keep_elite, a.concurrent, a.substream = int(bool(keep_elite)), int(bool(concurrent)), int(substream)
        if a.noparam and p.populations != 1:
            raise ValueError("AMALGAM: the parameter-free mode (noparam=True) works on populations=1 only")
        self._points = None

    def _flush(self):
        if self._amalgam.print and self._amalgam.noparam:
            sys.stdout.flush()      # the table is written by the library

    def optimize(self, f, lower, upper, guess):
        self._flush()
        self._send_points()
        return super().optimize(f, lower, upper, guess)

    def initialize(self, f, lower, upper, guess):
        self._flush()
        self._send_points()
        super().initialize(f, lower, upper, guess)

    def _send_points(self):
        if self._points is None:
            return
        x, self._points = self._points, None
        self._check(_ffi.lib().bbo_amalgam_inject_points(
            self._ensure_handle(), x.ctypes.data_as(C.c_void_p), x.size))

    def phase(self, which):
        """one part of a generation: 0 distribution, 1 sample + evaluate, 2 adapt + stop"""
        self._phase(which)

    def inject_points(self, x):
        """the initial points of the next initialize() / optimize(), [populations][np][n]"""
        self._points = None if x is None else _np.ascontiguousarray(
            _np.asarray(x, dtype=_np.float64)).ravel()

    def inject_draws(self, z, rows=None):
        """the draws of the following G generations: the normals [G][populations][np][n] in
        sampling order and the rows that take the anticipated mean shift, [G][populations][nams],
        each in 1 .. np - 1; None: the device draws"""
        if z is None:
            self._check(_ffi.lib().bbo_amalgam_inject_draws(self._handle, None, 0, None, 0))
            return
        z = _np.ascontiguousarray(_np.asarray(z, dtype=_np.float64)).ravel()
        r = _np.ascontiguousarray(_np.asarray([] if rows is None else rows, dtype=_np.int32)).ravel()
        self._check(_ffi.lib().bbo_amalgam_inject_draws(
            self._handle, z.ctypes.data_as(C.c_void_p), z.size, r.ctypes.data_as(C.c_void_p), r.size))


class SpiralSearch(MultivariateSearch):
    """SpiralSearch(mfev, tol, np=20, r=0.95, theta=1.57079632679, taur=0.0, tautheta=0.1, rlow=0.9,
    rhigh=1.0, thetalow=0.0, thetahigh=6.28318530718) -- :344-351 (adaptive spiral optimization,
    Tamura & Yasuda 2011, Yuzgec & Inac 2016; spiral.cpp).  `tol` is stored and unused and `guess` is
    ignored, as in the reference; the box seeds the points and never clamps them; `converged` is
    always False."""
    _algo = _ffi.ALGO_SPIRAL
    _extension = "spiral"

    def __init__(self, mfev, tol, np=20, r=0.95, theta=1.57079632679, taur=0.0, tautheta=0.1,
                 rlow=0.9, rhigh=1.0, thetalow=0.0, thetahigh=6.28318530718, **ext):
        super().__init__(**ext)
        p = self._params
        p.mfev, p.tol, p.np = int(mfev), float(tol), int(np)
        s = self._spiral = _ffi.SpiralParams()
        s.r, s.theta, s.taur, s.tautheta = float(r), float(theta), float(taur), float(tautheta)
        s.rlow, s.rhigh, s.thetalow, s.thetahigh = float(rlow), float(rhigh), float(thetalow), float(thetahigh)

    def phase(self, which):
        """one part of a generation: 0 draw, 1 rotate, 2 evaluate, 3 best"""
        self._phase(which)

    def inject_uniforms(self, u):
        """the raw uniforms of the following generations, [populations][np][4] in [0, 1): per point
        the coin of r, the value of r, the coin of theta, the value of theta; None: the device draws"""
        self._inject("bbo_spiral_inject_uniforms", u)


class NSHS(MultivariateSearch):
    """NSHS(mfev, hms, fstdmin=0.0001) -- :200-205 (novel self-adaptive harmony search, Luo 2013;
    nshs.cpp).  Steady-state: one iteration is one candidate and one evaluation; run() advances whole
    chunks of iterations per launch (`poll_every` iterations; default: the engine's own chunk).
    `guess` is ignored, as in the reference; `converged` is always False; the budget is met exactly.
    Extension `record_draws=True` keeps the four raw uniforms of every coordinate of the last
    iteration (get_state("draws"))."""
    _algo = _ffi.ALGO_NSHS
    _extension = "nshs"
    _accepts_program = False

    def __init__(self, mfev, hms, fstdmin=0.0001, **ext):
        record_draws = ext.pop("record_draws", False)
        super().__init__(**ext)
        p = self._params
        p.mfev, p.np = int(mfev), int(hms)
        s = self._nshs = _ffi.NshsParams()
        s.fstdmin = float(fstdmin)
        self._record_draws = bool(record_draws)

    def phase(self, which):
        """one part of an iteration: 0 generate, 1 evaluate, 2 replace"""
        self._phase(which)

    def inject_uniforms(self, u):
        """the raw uniforms of the following iterations, [populations][n][4] in [0, 1): per
        coordinate the coin, the row (row j as (j + 0.5) / hms), the fresh value, the adjustment;
        None: the device draws"""
        self._inject("bbo_nshs_inject_uniforms", u)


class SLPSO(MultivariateSearch):
    """SLPSO(mfev, stol, np, omegamin=0.4, omegamax=0.9, eta=1.496, gamma=0.01, vmax=0.2, Ufmax=10.) --
    :292-299 (self-learning particle swarm, Li, Yang & Nguyen 2012; slpso.cpp).  One iterate() walks the
    swarm particle by particle, each improving move followed by the coordinate walk of Algorithm 2 over
    the swarm's best point.  `guess` is ignored, as in the reference, and a finite box is mandatory.  The
    budget is tested between generations: n_evals may pass mfev by up to one generation.
    Extension `record_draws=True` keeps the draws of the last generation in the layout of
    inject_draws (get_state("draws"))."""
    _algo = _ffi.ALGO_SLPSO
    _extension = "slpso"
    _accepts_program = False
    MAX_N, MAX_NP = 512, 4096

    def __init__(self, mfev, stol, np, omegamin=0.4, omegamax=0.9, eta=1.496, gamma=0.01, vmax=0.2,
                 Ufmax=10., **ext):
        record_draws = ext.pop("record_draws", False)
        super().__init__(**ext)
        p = self._params
        p.mfev, p.stol, p.np = int(mfev), float(stol), int(np)
        s = self._slpso = _ffi.SlpsoParams()
        s.omegamin, s.omegamax, s.eta = float(omegamin), float(omegamax), float(eta)
        s.gamma, s.vmax, s.Ufmax = float(gamma), float(vmax), float(Ufmax)
        self._record_draws = bool(record_draws)

    def _problem(self, f, lower, upper, guess):
        n, lower, upper, guess = super()._problem(f, lower, upper, guess)
        if not 2 <= self._params.np <= self.MAX_NP:
            raise ValueError("SLPSO: np must be in [2, %d]" % self.MAX_NP)
        if not 1 <= n <= self.MAX_N:
            raise ValueError("SLPSO: dimension must be in [1, %d]" % self.MAX_N)
        self._require_finite_box(n, lower, upper, "SLPSO draws its swarm from [lower, upper]")
        return n, lower, upper, guess

    def table_len(self):
        """doubles per population of the table of inject_draws and of get_state("draws")"""
        np_ = self._params.np
        return 1 + np_ + np_ * (3 + 4 * self._n)

    def phase(self, which):
        """the generation one evaluation at a time: 0 advance to the next pending point ("cand"), 1
        evaluate it, 2 absorb the value.  Phase 0 returns the number of populations that have a point
        pending: 0 when the generation is complete."""
        self._phase(which)
        if int(which) != 0:
            return None
        return self._pending()

    def inject_draws(self, table):
        """the draws of the following generations, [populations][1 + np + np (3 + 4 n)]: alpha, the
        permutation after its shuffle, then per particle step the forcing coin, the roulette uniform, the
        partner j as (j + 0.5) / np and per coordinate r, the normal of operator 1, the redraw of eq. 11
        and the coin of Algorithm 2; None: the device draws"""
        self._inject("bbo_slpso_inject_draws", table)


class CRS(MultivariateSearch):
    """CRS(mfev, np, tol) -- :339-342 (controlled random search with local mutation, Kaelo & Ali 2006;
    crs.cpp).  Steady-state: an iteration replaces the worst of the np stored points, after as many
    trials and evaluations as the reference's recursive trial() takes; run() advances chunks of whole
    iterations (`poll_every`; default: the engine's own chunk) in launches of bounded length.  `guess` is
    ignored, as in the reference, and a finite box is mandatory.  The budget is tested between
    iterations: n_evals may pass mfev.  The default walks the reference's recursion, quirks included
    (get_state("stale") counts the iterations whose replacement was no better than the worst point).
    Extensions, keyword-only: `repair=True` is the loop of the paper (redraw instead of recursing, only
    an accepted point replaces the worst); `max_depth` bounds the recursion (flag 3, where the reference
    overflows its stack); `record_draws=True` keeps the draws of the last iteration in the layout of
    inject_draws (get_state("draws"))."""
    _algo = _ffi.ALGO_CRS
    _extension = "crs"
    _accepts_program = False
    MAX_N, MAX_NP = 512, 65536

    def __init__(self, mfev, np, tol, **ext):
        repair = ext.pop("repair", False)
        max_depth = ext.pop("max_depth", 4096)
        record_draws = ext.pop("record_draws", False)
        super().__init__(**ext)
        p = self._params
        p.mfev, p.np, p.tol = int(mfev), int(np), float(tol)
        s = self._crs = _ffi.CrsParams()
        s.max_depth, s.repair = int(max_depth), int(bool(repair))
        self._record_draws = bool(record_draws)

    def _problem(self, f, lower, upper, guess):
        n, lower, upper, guess = super()._problem(f, lower, upper, guess)
        if not 2 <= self._params.np <= self.MAX_NP:
            raise ValueError("CRS: np must be in [2, %d]" % self.MAX_NP)
        if not 1 <= n <= self.MAX_N:
            raise ValueError("CRS: dimension must be in [1, %d]" % self.MAX_N)
        self._require_finite_box(n, lower, upper, "CRS draws its pool from [lower, upper]")
        return n, lower, upper, guess

    def phase(self, which):
        """the iteration one evaluation at a time: 0 advance to the next pending point ("cand" in stage
        1, "cand2" in stage 2), 1 evaluate it ("value"), 2 absorb the value and advance again.  Phases 0
        and 2 return the number of populations that have a point pending: 0 when the iteration is
        complete."""
        self._phase(which)
        if int(which) == 1:
            return None
        return self._pending()

    def inject_draws(self, table):
        """the draws of the following trials, [populations][records][2 n]: per record the n row indices
        of a trial (-1 where none is drawn) and the n uniforms of a mutation; None: the device draws"""
        self._inject("bbo_crs_inject_draws", table)


class SSDE(MultivariateSearch):
    """SSDE(mfev, npinit, tol, patience=1000, npmin=4, ptop=0.11, h=100, usede=False, repaircr=True)
    (spherical search, Kumar et al. 2019, with the DE fallback of Zhao et al. 2022; ssde.cpp).  The pool is
    updated in place, member after member, so a generation is one launch of one workgroup per population
    that walks the reference's iterate(); the device earns its keep across `populations`.  `guess` is
    ignored, as in the reference, and a finite box is mandatory.  The budget is tested between
    generations: n_evals may pass mfev by up to one generation.  The pool never shrinks under 4 members
    and ptop must lie in (0, 1).  `record_draws=True` (an extension) keeps the draws of the last
    generation in the layout of inject_draws (get_state("draws"))."""
    _algo = _ffi.ALGO_SSDE
    _extension = "ssde"
    _accepts_program = False
    MAX_N, MIN_NP, MAX_NP = 512, 4, 4096

    def __init__(self, mfev, npinit, tol, patience=1000, npmin=4, ptop=0.11, h=100, usede=False,
                 repaircr=True, **ext):
        record_draws = ext.pop("record_draws", False)
        super().__init__(**ext)
        p = self._params
        p.mfev, p.np, p.tol = int(mfev), int(npinit), float(tol)
        s = self._ssde = _ffi.SsdeParams()
        s.patience, s.npmin, s.ptop, s.h = int(patience), int(npmin), float(ptop), int(h)
        s.usede, s.repaircr = int(bool(usede)), int(bool(repaircr))
        self._record_draws = bool(record_draws)

    def _problem(self, f, lower, upper, guess):
        n, lower, upper, guess = super()._problem(f, lower, upper, guess)
        if not self.MIN_NP <= self._params.np <= self.MAX_NP:
            raise ValueError("SSDE: npinit must be in [4, %d]" % self.MAX_NP)
        if not 1 <= n <= self.MAX_N:
            raise ValueError("SSDE: dimension must be in [1, %d]" % self.MAX_N)
        self._require_finite_box(n, lower, upper, "SSDE draws its pool from [lower, upper]")
        return n, lower, upper, guess

    def phase(self, which):
        """the generation one evaluation at a time: 0 advance to the next pending point ("cand"), 1
        evaluate it ("fcand"), 2 absorb the value.  Phases 0 and 2 return the number of populations that
        have a point pending: 0 when the generation is complete."""
        self._phase(which)
        if int(which) == 1:
            return None
        return self._pending()

    def inject_draws(self, table):
        """the draws of the following generations, [populations][n + npinit * (9 + 3 n)]: the permutation,
        then per member iL, the normal of prank, p, q, r, pbest, ci, the normal of CRi, j0 and the n
        uniforms each of b, the crossover and the redraw; None: the device draws"""
        self._inject("bbo_ssde_inject_draws", table)


class ACD(MultivariateSearch):
    """ACD(mfev, ftol, xtol, ksucc=2., kunsucc=0.5) -- :44-48 (adaptive coordinate descent, Loshchilov,
    Schoenauer & Sebag 2011; acd.cpp).  A coordinate search along the columns of B with an archive of 2 n
    points; behind every sweep that improved, the rank-one update of C and its eigendecomposition give
    the next B.  iterate() is ONE coordinate step (two evaluations, x1 then x2); run(g) counts coordinate
    steps and polls once per sweep (`poll_every` = 0, the default) or every `poll_every` steps.  x_best
    starts uniform in the box: a finite box is mandatory and `guess` is not read, as in the reference;
    from_guess=True (an extension, keyword-only) starts population p at its row of `guess`.  The budget
    is tested between steps: n_evals may pass mfev by 1.  get_state("flag") is 1 converged, 2 budget;
    get_state("rule") says which rule converged: 1 ftol over the history, 2 xtol.  n is at most 128: the
    eigensolver's routes beyond that are driven from inside the CMA-ES engine only.  `speculate` (the
    speculative sweep over the next pending coordinates) was built, measured slower at 4096 populations
    and dropped: only False is accepted."""
    _algo = _ffi.ALGO_ACD
    _extension = "acd"
    _accepts_program = False
    MAX_N = 128

    def __init__(self, mfev, ftol, xtol, ksucc=2., kunsucc=0.5, *, from_guess=False, speculate=False,
                 **ext):
        super().__init__(**ext)
        if speculate:
            raise ValueError("ACD: the speculative sweep was measured and dropped; speculate must be False")
        p = self._params
        p.mfev, p.tol, p.stol = int(mfev), float(ftol), float(xtol)
        a = self._acd = _ffi.AcdParams()
        a.ksucc, a.kunsucc = float(ksucc), float(kunsucc)
        a.from_guess, a.speculate = int(bool(from_guess)), 0

    def _problem(self, f, lower, upper, guess):
        n, lower, upper, guess = super()._problem(f, lower, upper, guess)
        if not 1 <= n <= self.MAX_N:
            raise ValueError("ACD: dimension must be in [1, %d]" % self.MAX_N)
        self._require_finite_box(n, lower, upper, "ACD draws x_best from [lower, upper]")
        return n, lower, upper, guess

    def phase(self, which):
        """a coordinate step one part at a time: 0 form x1 and x2 ("cand", 2 x n), 1 evaluate them
        ("value"), 2 absorb the values, finish the step and, where due, update the encoding.  Phase 0
        returns the number of populations that have a pair pending."""
        self._phase(which)
        if int(which) != 0:
            return None
        return self._pending()


class Mayfly(MultivariateSearch):
    """Mayfly(np, mfev, a1=1., a2=1.5, a3=1.5, beta=2., dance=5., ddamp=0.8, fl=1., fldamp=0.99, gmin=0.8,
    gmax=0.8, vdamp=0.1, sigma=0.1, pmutdim=0.01, pmutnp=0.05, l=0.95, pgb=False) -- the binding the reference
    writes out at :236-246 and leaves commented away (the mayfly optimizer of Zervoudakis & Tsafarakis 2020
    with the PGB-IMA switch; mayfly.cpp).  A generation moves np females and np males, mates the sorted
    swarms into np offspring, mutates nmut of them and selects: 3 np + nmut evaluations, all of them parallel
    across the individuals but the male loop, which runs as rounds of `window` males.  `guess` is ignored, as
    in the reference, and a finite box is mandatory.  np must be even (the reference leaves the last
    offspring of an odd swarm unwritten, a zero vector of value 0 that wins the selection) and mfev must
    exceed 2 np (the initial swarms; else the reference divides 0 by 0).  The budget is tested between
    generations: n_evals passes mfev by less than one generation; converged is always False.  The default
    reproduces the reference's in-place selection, which leaves about half of each swarm an exact duplicate.
    The reference also builds its flies with x and v exchanged, so every fly starts at the origin with the
    point it drew as its velocity; that is reproduced too.
    Extensions, keyword-only: `repair=True` selects from untouched copies and starts every fly at the point it
    drew, as the paper does; `substream=s` lets population p draw from sub-stream s + p;
    `record_draws=True` keeps the draws of the last generation in the layout of inject_draws
    (get_state("draws"))."""
    _algo = _ffi.ALGO_MAYFLY
    _extension = "mayfly"
    _accepts_program = False
    MAX_N, MAX_NP = 512, 4096

    def __init__(self, np, mfev, a1=1., a2=1.5, a3=1.5, beta=2., dance=5., ddamp=0.8, fl=1., fldamp=0.99,
                 gmin=0.8, gmax=0.8, vdamp=0.1, sigma=0.1, pmutdim=0.01, pmutnp=0.05, l=0.95, pgb=False, *,
                 repair=False, record_draws=False, substream=0, **ext):
        super().__init__(**ext)
        p = self._params
        p.np, p.mfev = int(np), int(mfev)
        m = self._mayfly = _ffi.MayflyParams()
        for k, v in (("a1", a1), ("a2", a2), ("a3", a3), ("beta", beta), ("dance", dance), ("ddamp", ddamp),
                     ("fl", fl), ("fldamp", fldamp), ("gmin", gmin), ("gmax", gmax), ("vdamp", vdamp),
                     ("sigma", sigma), ("pmutdim", pmutdim), ("pmutnp", pmutnp), ("l", l)):
            setattr(m, k, float(v))
        m.pgb, m.repair, m.substream = int(bool(pgb)), int(bool(repair)), int(substream)
        self._record_draws = bool(record_draws)

    def _problem(self, f, lower, upper, guess):
        n, lower, upper, guess = super()._problem(f, lower, upper, guess)
        np_, mfev = self._params.np, self._params.mfev
        if np_ < 2 or np_ > self.MAX_NP:
            raise ValueError("Mayfly: np must be in [2, %d]" % self.MAX_NP)
        if np_ % 2:
            raise ValueError("Mayfly: np must be even: the reference leaves the last offspring of an odd swarm "
                             "unwritten, a zero vector of value 0 that enters the selection")
        if mfev <= 2 * np_:
            raise ValueError("Mayfly: mfev must exceed 2 np, the evaluations of the initial swarms "
                             "(itmax would be <= 0 and g = 0/0)")
        if not 1 <= n <= self.MAX_N:
            raise ValueError("Mayfly: dimension must be in [1, %d]" % self.MAX_N)
        self._require_finite_box(n, lower, upper, "Mayfly draws its swarms from [lower, upper]")
        return n, lower, upper, guess

    def table_len(self):
        """the length of one population's table of inject_draws"""
        return int(self.get_state("table_len")[0])

    def inject_draws(self, table):
        """the draws of the following generations, [populations][2 np n + np + nmut + 2 nmut nmd]: the
        canonical uniforms of the females' random flights and of the males' dances (-1 where a fly takes the
        attraction form), the shuffles of the offspring and of the mutated flies as permutations, and per
        mutated fly its nmd displaced genes and their normals; None: the device draws"""
        self._inject("bbo_mayfly_inject_draws", table)


class PIKAIA(MultivariateSearch):
    """PIKAIA(np, ngen, nd, pcross=0.85, imut=2, pmut=0.005, pmutmn=0.0005, pmutmx=0.25, fdif=1., irep=1,
    ielite=0) -- the constructor of the reference's PikaiaSearch (pikaia.h:25-27), which it binds to no Python
    class (the genetic algorithm of Charbonneau & Knapp, a translation of the HAO Fortran 77 code; pikaia.cpp).
    A generation is np / 2 matings: two parents by a rank roulette, every coordinate of a phenotype in [0, 1)
    encoded as nd decimal digits, one- or two-point crossover of the digit string with probability pcross, per
    locus with probability pmut a fresh digit (imut 1-3) or, for imut 4-6 after a coin, +-1 with the carry into
    the same gene (creep); then np evaluations, the ranking and, for imut 2, 3, 5, 6, the adjustment of pmut.
    The default MINIMISES f over the box like every class here: the objective is handed
    x = lower + u * (upper - lower) and the GA's fitness is -f(x), which is the reference run on that wrapped
    function; a finite box is mandatory and `guess` is not read.  The only stop is ngen generations, and
    converged is then True, as the reference reports.  n_evals is the reference's counter: np + ngen (np + 1),
    whatever ielite is.  The reference's init stores the value of the last row only, so the first generation
    selects on tied zeros; that is reproduced.  So is the signed denominator of imut 2 / 5: on a non-negative
    objective (fitness <= 0) pmut only ever rises, reaches pmutmx in about ten generations and the run stalls;
    use repair=True or imut 3 / 6 there.  irep 2 and 3 (steady state) are refused: they are a sequential walk
    with the evaluations inside it and are not built.  np must be even (the reference leaves the last row of an
    odd new population a zero vector), nd at most 9.  A callable is called np + ielite times per generation,
    new row 1 first when ielite = 1; a NaN ranks worst.  Takes a DeviceObjective (whose NaN is stored as +inf: under
    raw=True a +inf from a program ranks worst as well).
    Extensions, keyword-only: `raw=True` is the literal reference (the objective sees u in the unit cube, the
    box is ignored, +f is maximised); `repair=True` stores every initial value, counts np evaluations per
    generation, keeps the stored value of the elite row and divides by |f_best + f_median| in imut 2 / 5;
    `substream=s` lets population p draw from sub-stream s + p; `record_draws=True` keeps the draws of the
    last generation in the layout of inject_draws (get_state("draws"))."""
    _algo = _ffi.ALGO_PIKAIA
    _extension = "pikaia"
    _accepts_program = True
    MAX_N, MAX_NP, MAX_ND = 512, 4096, 9

    def __init__(self, np, ngen, nd, pcross=0.85, imut=2, pmut=0.005, pmutmn=0.0005, pmutmx=0.25, fdif=1., irep=1,
                 ielite=0, *, repair=False, raw=False, record_draws=False, substream=0, **ext):
        super().__init__(**ext)
        np_, ngen, nd, imut, irep, ielite = int(np), int(ngen), int(nd), int(imut), int(irep), int(ielite)
        if irep != 1:
            raise ValueError("PIKAIA: irep must be 1 (full generational replacement): the steady-state plans "
                             "irep = 2, 3 insert every child at once and the next select reads the ranks that "
                             "insertion left, a sequential walk with the evaluations inside it that is not built")
        if np_ < 2 or np_ > self.MAX_NP:
            raise ValueError("PIKAIA: np must be in [2, %d]" % self.MAX_NP)
        if np_ % 2:
            raise ValueError("PIKAIA: np must be even: the reference leaves the last row of an odd new "
                             "population unwritten, a zero vector")
        if not 1 <= nd <= self.MAX_ND:
            raise ValueError("PIKAIA: nd must be in [1, 9]: int(ph * 10**nd) overflows an int from nd = 10")
        if not 1 <= imut <= 6:
            raise ValueError("PIKAIA: imut must be in [1, 6]")
        if ielite not in (0, 1):
            raise ValueError("PIKAIA: ielite is 0 or 1")
        for name, v in (("pcross", pcross), ("pmut", pmut), ("pmutmn", pmutmn), ("pmutmx", pmutmx)):
            if not 0. <= float(v) <= 1.:
                raise ValueError("PIKAIA: %s is a probability and must lie in [0, 1]" % name)
        if float(pmutmn) > float(pmutmx):
            raise ValueError("PIKAIA: pmutmn must not exceed pmutmx")
        if not 0. <= float(fdif) <= 1.:
            raise ValueError("PIKAIA: fdif must lie in [0, 1]: beyond 1 the weights of select turn negative")
        if ngen < 1:
            raise ValueError("PIKAIA: ngen must be >= 1")
        if np_ + ngen * (np_ + 1) > 2 ** 31 - 1:
            raise ValueError("PIKAIA: np + ngen (np + 1) evaluations must fit the int counter (INT_MAX)")
        p = self._params
        p.np, p.mfev, p.h = np_, ngen, nd       # (ngen and nd travel in `mfev` and `h`, include/bbopt_hip.h)
        g = self._pikaia = _ffi.PikaiaParams()
        g.pcross, g.pmut, g.pmutmn, g.pmutmx, g.fdif = float(pcross), float(pmut), float(pmutmn), float(pmutmx), float(fdif)
        g.imut, g.irep, g.ielite = imut, irep, ielite
        g.repair, g.raw, g.substream = int(bool(repair)), int(bool(raw)), int(substream)
        self._record_draws = bool(record_draws)

    def _problem(self, f, lower, upper, guess):
        n, lower, upper, guess = super()._problem(f, lower, upper, guess)
        if not 1 <= n <= self.MAX_N:
            raise ValueError("PIKAIA: dimension must be in [1, %d]" % self.MAX_N)
        if not self._pikaia.raw:
            self._require_finite_box(n, lower, upper, "PIKAIA maps its phenotypes from the unit cube onto "
                                     "[lower, upper] (raw=True hands the objective the unit cube itself)")
        return n, lower, upper, guess

    def table_len(self):
        """the length of one population's table of inject_draws"""
        return int(self.get_state("table_len")[0])

    def inject_draws(self, table):
        """the draws of the following generations, [populations][np / 2][69 + 2 (1 + 2 n nd)]: per mating the
        uniform of the first parent, 64 slots for the attempts at the second, the crossover's coin, ispl, the
        coin one- / two-point and ispl2, then per child the coin creep / uniform, n nd locus uniforms and n nd
        value uniforms (new digit int(10 u), or creep step round(u) 2 - 1); -1 wherever the reference draws
        nothing; None: the device draws"""
        self._inject("bbo_pikaia_inject_draws", table)


class NelderMead(MultivariateSearch):
    """NelderMead(mfev, tol, rad0, minit=NelderMead.spendley, pinit=NelderMead.mehta2019_refined, checkev=10,
    eps=1e-3) -- :307-337 (the simplex search of Nelder & Mead as O'Neill's AS 47 with restarts, the adaptive
    coefficients of Gao & Han 2012 and Mehta 2020, four initial simplexes; nelder_mead.cpp).  One workgroup per
    simplex, a lane per coordinate: `populations=P` starts P independent searches from the P rows of `guess`, a
    multi-start the reference has no counterpart for.  n is at most 128.  The bounds are read by minit=random
    alone (which needs a finite box); the search ignores them, as in the reference.
    optimize() is the reference's: init() and nelmin() whole -- the steps while n_evals < mfev and the stop test
    (every checkev steps) has not fired, the factorial test of 2 n probes at xmin[i] +- rad0 eps, a restart from
    the first probe that improved -- and returns xmin as nelmin() leaves it, converged = the factorial test
    passed.  Reproduced literally: the centroid summed afresh every step, first maximum / first minimum on ties,
    the in-place shrink that moves the best row too, the refused outside contraction that stores pstar with
    the value of the contracted point (nelder_mead.cpp:195-197; repair=True, keyword-only, stores its own), the
    drift the probes' restore leaves in xmin.
    Departure: the reference's step protocol is broken (its init() builds no simplex, so iterate() after
    initialize() walks zeros, and solution() returns a scratch vector).  Here initialize() builds and evaluates
    the first simplex as nelmin()'s first pass does (n_evals = n + 1), iterate() is one iterate() of the
    reference from there, solution() gives the best row, n_evals and the stop test's verdict of the last step.
    run(g) counts simplex steps and is nelmin() for up to g of them.  get_state("flag") is 1 converged, 2 budget;
    "branch" is the last step's path (1 expansion kept, 2 expansion refused, 3 reflection, 4 inside contraction,
    5 shrink, 6 outside contraction, 7 outside contraction refused).  A NaN value counts as +inf.
    Extensions, keyword-only: `repair`; `lds=True / False` keeps the simplex of a launch in LDS / in HBM (same results;
    the default chooses: HBM only at n near 128 with thousands of populations, where it was measured faster); `substream=s` lets population p draw minit=random from sub-stream s + p; `speculate` (pstar and the
    three possible second points of a step evaluated at once on four wavefronts) was built, bit-identical, measured
    slower at 1, 256 and 4096 populations alike and dropped: only False is accepted."""
    _algo = _ffi.ALGO_NELDER_MEAD
    _extension = "nm"
    _accepts_program = False
    MAX_N = 128

    class NelderMead_SimplexInit(enum.IntEnum):
        """NelderMead::simplex_initializer, bound with export_values (:310-317)"""
        coordinate_axis = 0
        spendley = 1
        pfeffer = 2
        random = 3

    class NelderMead_ParamInit(enum.IntEnum):
        """NelderMead::parameter_initializer, bound with export_values (:319-328)"""
        original = 0
        gao2010 = 1
        mehta2019_crude = 2
        mehta2019_refined = 3

    coordinate_axis, spendley, pfeffer, random = (NelderMead_SimplexInit.coordinate_axis,
                                                  NelderMead_SimplexInit.spendley, NelderMead_SimplexInit.pfeffer,
                                                  NelderMead_SimplexInit.random)
    original, gao2010, mehta2019_crude, mehta2019_refined = (NelderMead_ParamInit.original, NelderMead_ParamInit.gao2010,
                                                             NelderMead_ParamInit.mehta2019_crude,
                                                             NelderMead_ParamInit.mehta2019_refined)

    def __init__(self, mfev, tol, rad0, minit=NelderMead_SimplexInit.spendley,
                 pinit=NelderMead_ParamInit.mehta2019_refined, checkev=10, eps=1e-3, *, repair=False,
                 speculate=False, lds=None, substream=0, **ext):
        super().__init__(**ext)
        if speculate:
            raise ValueError("NelderMead: the speculative step was measured and dropped; speculate must be False")
        if int(checkev) < 1:
            raise ValueError("NelderMead: checkev must be >= 1")
        if not _np.isfinite(float(rad0)):
            raise ValueError("NelderMead: rad0 must be finite")
        if not _np.isfinite(float(eps)):
            raise ValueError("NelderMead: eps must be finite")
        if int(mfev) < 1:
            raise ValueError("NelderMead: mfev must be positive")
        p = self._params
        p.mfev, p.tol, p.sigma0 = int(mfev), float(tol), float(rad0)    # (rad0 travels in `sigma0`)
        s = self._nm = _ffi.NmParams()
        s.minit, s.pinit = int(self.NelderMead_SimplexInit(minit)), int(self.NelderMead_ParamInit(pinit))
        s.checkev, s.eps = int(checkev), float(eps)
        s.repair, s.speculate, s.substream = int(bool(repair)), 0, int(substream)
        s.lds = -1 if lds is None else int(bool(lds))

    def _problem(self, f, lower, upper, guess):
        n, lower, upper, guess = super()._problem(f, lower, upper, guess)
        if not 1 <= n <= self.MAX_N:
            raise ValueError("NelderMead: dimension must be in [1, %d]" % self.MAX_N)
        if self._nm.minit == int(self.NelderMead_SimplexInit.random):
            self._require_finite_box(n, lower, upper, "NelderMead: minit = random draws the simplex from [lower, upper]")
        return n, lower, upper, guess

    def phase(self, which):
        """a step from batch to batch of evaluations: 0 advance to the next pending batch ("pending" points: one,
        or the n + 1 rows of a shrunk simplex), 1 evaluate it ("value"), 2 absorb the values and advance to the
        next batch of the same step.  Phases 0 and 2 return the number of populations that have a batch pending;
        the step is complete when it is 0."""
        self._phase(which)
        if int(which) == 1:
            return None
        return self._pending()


class Rosenbrock(MultivariateSearch):
    """Rosenbrock(mfev, tol, step0, decf=0.1) -- the constructor of the reference's Rosenbrock (rosenbrock.h:55),
    which it binds to no Python class: Rosenbrock's rotating-axes search with the line search of Davies, Swann and
    Campey (doubling of the step, then a Lagrange quadratic through three of four points) and Palmer's
    orthogonalisation of the directions (rosenbrock.cpp).  A local method that draws no random number.  One
    workgroup per search: `populations=P` starts P independent searches from the P rows of `guess`, a multi-start
    the reference has no counterpart for.  n is at most 128.  The bounds are stored and never read, as in the
    reference, so no finite box is required.  step0 and decf must not be 0 and tol not negative: with a step of 0
    a search would double until the budget ends it.  (The objective of the same name is bb.objectives.rosenbrock.)
    optimize() is the reference's: init() and iterate() until it ends -- converged when the step, multiplied by
    decf whenever a stage moved less than the step, is at most tol; on the budget when n_evals >= mfev is met inside
    the doubling loop or behind a stage, so n_evals passes mfev by a few evaluations.
    **On a budget exit optimize() returns the ZERO vector**: the reference writes its result only when it converges
    (rosenbrock.cpp:197), and this is reproduced; `repair=True` (keyword-only) returns the end point of the last
    completed line search where the run did not converge, and changes nothing else.
    initialize() / iterate() / solution() are the reference's: initialize() evaluates nothing, one iterate() is one
    line search (about eight evaluations) with its bookkeeping, solution() is the same vector as optimize()'s,
    under the same `repair` rule.  run(g) counts line searches.  get_state("flag") is 1 converged, 2 budget;
    "path" is the last search's path (direction 1 forward / 2 backward / 3 straight to the interpolation, rounds of
    the doubling loop, imin, end 0 none / 1 kept / 2 restored / 3 budget).  A callable is called exactly as often
    as in the reference and in its order, the second call at x0 included.  Departure: a NaN value counts as +inf.
    Extensions, keyword-only: `repair`; `wide=True / False` evaluates the points of a batch at once on a wavefront
    each / in turn on one wavefront (same results; the default is True except at n <= 64 with at least four
    populations per CU, as measured); `substream` is accepted
    for symmetry with the other engines and unused."""
    _algo = _ffi.ALGO_ROSENBROCK
    _extension = "rosen"
    _accepts_program = False
    MAX_N = 128

    def __init__(self, mfev, tol, step0, decf=0.1, *, repair=False, wide=None, substream=0, **ext):
        super().__init__(**ext)
        if int(mfev) < 1:
            raise ValueError("Rosenbrock: mfev must be positive")
        if not _np.isfinite(float(step0)) or float(step0) == 0.:
            raise ValueError("Rosenbrock: step0 must be finite and not 0")
        if not _np.isfinite(float(decf)) or float(decf) == 0.:
            raise ValueError("Rosenbrock: decf must be finite and not 0")
        if not float(tol) >= 0.:
            raise ValueError("Rosenbrock: tol must be >= 0: with a step of 0 a search doubles until the budget ends it")
        p = self._params
        p.mfev, p.tol, p.sigma0 = int(mfev), float(tol), float(step0)    # (step0 travels in `sigma0`)
        s = self._rosen = _ffi.RosenParams()
        s.decf, s.repair, s.substream = float(decf), int(bool(repair)), int(substream)
        s.wide = -1 if wide is None else int(bool(wide))

    def _problem(self, f, lower, upper, guess):
        n, lower, upper, guess = super()._problem(f, lower, upper, guess)
        if not 1 <= n <= self.MAX_N:
            raise ValueError("Rosenbrock: dimension must be in [1, %d]" % self.MAX_N)
        return n, lower, upper, guess

    def phase(self, which):
        """a line search from batch to batch of evaluations: 0 advance to the next pending batch ("pending"
        points: 2, 1 or 4), 1 evaluate it ("value"), 2 absorb the values and advance to the next batch of the same
        search.  Phases 0 and 2 return the number of populations that have a batch pending; the search and its
        bookkeeping are complete when it is 0."""
        self._phase(which)
        if int(which) == 1:
            return None
        return sum(int(self.get_state("pending", p)[0]) > 0 for p in range(self._params.populations))


class APSO(MultivariateSearch):
    """APSO(mfev, tol, np, correct=True) -- :265-269"""
    _algo = _ffi.ALGO_APSO

    def __init__(self, mfev, tol, np, correct=True, **ext):
        super().__init__(**ext)
        p = self._params
        p.mfev, p.tol, p.np, p.correct = int(mfev), float(tol), int(np), int(bool(correct))


class BasinHopping_StepStrategy:
    """BasinHopping_StepStrategy(stepsize) -- StepsizeStrategy, :83-85 (basinhopping.cpp:46-60): a hop moves every
    coordinate by stepsize U[-1, 1) (upper - lower) and clamps it to the box less 5 % on each side.  The object is
    the caller's: BasinHopping reads `stepsize` (and an adaptive strategy's `nstep`, `naccept`) at initialize() and,
    on a one-population handle, writes them back after optimize() / iterate() / run()."""
    _adaptive = False

    def __init__(self, stepsize):
        self.stepsize = float(stepsize)
        self.nstep = self.naccept = 0
        if not _np.isfinite(self.stepsize):
            raise ValueError("BasinHopping: stepsize must be finite")


class BasinHopping_AdaptStrategy(BasinHopping_StepStrategy):
    """BasinHopping_AdaptStrategy(stepsize=1., accept_rate=0.5, interval=5, factor=0.9) -- AdaptiveStepsizeStrategy,
    :87-90 (basinhopping.cpp:62-94): every `interval` steps the step is divided by `factor` when more than
    `accept_rate` of the hops so far were accepted, and multiplied by it otherwise.  Departures: interval < 1 and a
    factor that is not finite and positive are refused."""
    _adaptive = True

    def __init__(self, stepsize=1., accept_rate=0.5, interval=5, factor=0.9):
        super().__init__(stepsize)
        self.accept_rate, self.interval, self.factor = float(accept_rate), int(interval), float(factor)
        if self.interval < 1:
            raise ValueError("BasinHopping: interval must be >= 1")
        if not (_np.isfinite(self.factor) and self.factor > 0.):
            raise ValueError("BasinHopping: factor must be finite and positive")
        if self.accept_rate != self.accept_rate:
            raise ValueError("BasinHopping: accept_rate must not be NaN")


class BasinHopping(MultivariateSearch):
    """BasinHopping(minimizer, stepstrat, print=True, mit=99, temp=1.) -- :91-97 (basin hopping of Wales & Doye as
    SciPy states it; basinhopping.cpp): a Metropolis chain whose every hop is a step of `stepstrat` from the
    incumbent, a whole run of `minimizer` from there, one extra evaluation of what it returned, and the test
    exp(min(0, -(new - old) / temp)) >= U[0, 1); temp = 0 accepts only what is not worse.  optimize() is init() and
    `mit` hops and returns the best point, n_evals = the minimisations' counts + 1 each, converged = False always.
    With a NelderMead or a Rosenbrock of this package as the minimizer the chain lives on the device: one chain per
    population of the minimizer (`populations`, by default the minimizer's), re-armed there between hops, so no point,
    value or decision crosses to the host; with a built-in objective the chains hop asynchronously, each starting its
    next minimisation in the launch after its last one ended.  `lockstep=True` hops only when every minimisation has
    ended (same results; the default is asynchronous except at n > 64 with at least 256 chains, as measured).  Every draw is addressed by (seed, substream + population, hop, coordinate), so a chain does
    not depend on scheduling, the chunk sizes or `populations`.  initialize() is init() (log row -1), iterate() one
    hop of every chain that has hops left, run(g) up to g.  get_state: "log" (rows of it, f, conv, step, accept,
    f*, fev, the reference's table), "log_start" / "log_sol" (the start handed to the minimizer and what it
    returned, per row), "log_fev", "x", "energy", "xbest", "fbest", "stepsize", "nstep", "naccept", "it", "fev",
    "flag" (2: mit reached).  print=True prints the reference's table for population 0.
    Reproduced literally: std::min(0., v) lets a NaN product accept (temp = 0 with equal energies); the strategy's
    history is not reset by init(); a Rosenbrock minimizer that ends on its budget returns the ZERO vector, which
    is evaluated and hopped from (that class's `repair=True` changes it).  Departures: a NaN energy counts as +inf;
    a box that is not finite, temp < 0 and mit < 0 are refused.  NelderMead(minit=random) is refused on the device
    (it would draw the same simplex on every hop).
    Any other object with optimize(f, lower, upper, guess) -- and `native=False` for the two above -- takes the
    Python-driven path: one population, the chain's arithmetic in Python on the same draws (bbo_bh_draws), the
    minimizer called once per hop; run() raises there.  Extensions, in **ext: `seed`, `populations`, `poll_every`,
    `lockstep`, `native`, `substream`, `device`."""
    _algo = _ffi.ALGO_BASIN_HOPPING
    _extension = "bh"
    _accepts_program = False
    MAX_N = 128
    _WIDTHS = (5, 25, 5, 25, 6, 25, 10)     # basinhopping.cpp:148

    def __init__(self, minimizer, stepstrat, print=True, mit=99, temp=1., **ext):
        lockstep, native = ext.pop("lockstep", None), ext.pop("native", None)
        substream = int(ext.pop("substream", 0))
        if not isinstance(stepstrat, BasinHopping_StepStrategy):
            raise TypeError("stepstrat must be a BasinHopping_StepStrategy or a BasinHopping_AdaptStrategy")
        if not callable(getattr(minimizer, "optimize", None)):
            raise TypeError("minimizer must have optimize(f, lower, upper, guess)")
        walks = isinstance(minimizer, (NelderMead, Rosenbrock))
        if native and not walks:
            raise ValueError("BasinHopping: only NelderMead and Rosenbrock of this package are native minimizers")
        self._native = walks if native is None else bool(native)
        if self._native:
            ext.setdefault("populations", minimizer._params.populations)
            ext.setdefault("device", minimizer._params.device)
        super().__init__(**ext)
        if int(mit) < 0:
            raise ValueError("BasinHopping: mit must be >= 0")
        if not float(temp) >= 0.:
            raise ValueError("BasinHopping: temp must be >= 0")
        if not 0 <= substream < 1 << 24:
            raise ValueError("BasinHopping: substream must be in [0, 2^24)")
        p = self._params
        if self._native:
            if minimizer._params.populations != p.populations:
                raise ValueError("BasinHopping: the minimizer must hold as many populations as there are chains "
                                 "(populations=%d, the minimizer's %d)" % (p.populations, minimizer._params.populations))
            if minimizer._params.device != p.device:
                raise ValueError("BasinHopping: the minimizer must live on the same device")
            if isinstance(minimizer, NelderMead) and minimizer._nm.minit == int(NelderMead.random):
                raise ValueError("BasinHopping: NelderMead(minit=random) draws its simplex by the restart count alone, "
                                 "the same one on every hop: it is no native minimizer (use another minit, or native=False)")
        elif p.populations != 1:
            raise ValueError("BasinHopping: the Python-driven path holds one population")
        self._minimizer, self._stepstrat = minimizer, stepstrat
        self._minimizer_handle = None
        self._table = None
        self._py = None
        s = self._bh = _ffi.BhParams()
        _ffi.lib().bbo_bh_params_default(C.byref(s))
        s.print, s.mit, s.temp = int(bool(print)), int(mit), float(temp)
        s.lockstep, s.substream = -1 if lockstep is None else int(bool(lockstep)), substream
        self._read_strategy()

    def _read_strategy(self):
        s, st = self._bh, self._stepstrat
        s.stepsize, s.adaptive = float(st.stepsize), int(st._adaptive)
        s.nstep0, s.naccept0 = int(st.nstep), int(st.naccept)
        if st._adaptive:
            s.accept_rate, s.interval, s.factor = float(st.accept_rate), int(st.interval), float(st.factor)

    def _write_strategy(self):
        if self._params.populations == 1 and self._handle is not None:
            st = self._stepstrat
            st.stepsize = float(self.get_state("stepsize")[0])
            st.nstep, st.naccept = int(self.get_state("nstep")[0]), int(self.get_state("naccept")[0])

    # -- the handle borrows the minimizer's ------------------------------------------------
    def _create(self):
        h = C.c_void_p()
        mh = self._minimizer._ensure_handle()
        _ffi.check(_ffi.lib().bbo_create_basin(C.byref(self._params), mh, C.byref(h)))
        self._minimizer_handle = mh
        return h

    def _ensure_handle(self):
        # (as the restart drivers: a minimizer that re-created its handle leaves this one stale)
        if self._handle is not None and self._minimizer._handle is not self._minimizer_handle:
            _ffi.lib().bbo_destroy(self._handle)
            self._handle = None
        return super()._ensure_handle()

    def _live(self):
        if self._handle is not None and self._minimizer._handle is not self._minimizer_handle:
            raise RuntimeError("the minimizer was re-created (reseed) after this BasinHopping was initialized: call "
                               "initialize() / optimize() again")

    def _problem(self, f, lower, upper, guess):
        n, lower, upper, guess = super()._problem(f, lower, upper, guess)
        if not 1 <= n <= self.MAX_N:
            raise ValueError("BasinHopping: dimension must be in [1, %d]" % self.MAX_N)
        self._require_finite_box(n, lower, upper, "BasinHopping: a step is a fraction of upper - lower")
        return n, lower, upper, guess

    # -- the reference's methods -------------------------------------------------------------
    def initialize(self, f, lower, upper, guess):
        if not self._native:
            return self._py_initialize(f, lower, upper, guess)
        n, lower, upper, guess = self._problem(f, lower, upper, guess)
        self._read_strategy()
        h = self._ensure_handle()
        L = _ffi.lib()
        self._check(L.bbo_bh_configure(h, C.byref(self._bh)))
        if self._bh.print:
            sys.stdout.flush()      # the table is written by the library
        self._minimizer._binding, self._minimizer._n = self._binding, n      # (its engine calls the same objective)
        self._check(L.bbo_init(h, n, lower, upper, guess, C.byref(self._binding.struct)))
        if self._table is not None:
            self._inject("bbo_bh_inject_draws", self._table)
        self._write_strategy()

    def optimize(self, f, lower, upper, guess):
        self.initialize(f, lower, upper, guess)
        if not self._native:
            while self._py["it"] < self._bh.mit:
                self._py_hop()
            return self.solution()
        self.run(self._bh.mit)
        return self.solution()

    def iterate(self):
        if not self._native:
            if self._py is None:
                raise RuntimeError("iterate() called before initialize()")
            if self._py["it"] < self._bh.mit:
                self._py_hop()
            return
        self._live()
        super().iterate()
        self._write_strategy()

    def run(self, max_generations):
        if not self._native:
            raise RuntimeError("run() needs a device-resident minimizer: with a Python-driven minimizer the chain "
                               "advances in Python (iterate())")
        self._live()
        done = super().run(max_generations)
        self._write_strategy()
        return done

    def solution(self, population=0):
        if self._native:
            return super().solution(population)
        if self._py is None:
            raise RuntimeError("solution() called before initialize()")
        return MultivariateSolution(self._py["xbest"], self._py["fev"], False)

    def phase(self, which):
        """0 every idle chain with hops left takes its step and re-arms its minimizer (which then walks through its
        own handle), 1 collect the results of the minimisations that have stopped, 2 evaluate the pending energy
        points, 3 decide"""
        self._phase(which)

    def inject_draws(self, table):
        """the draws of the hops that follow instead of the generator: per hop n step uniforms in [-1, 1) and one
        accept uniform in [0, 1), for every chain; None: the generator.  Before initialize() the table is kept and
        injected there."""
        self._table = None if table is None else _np.ascontiguousarray(_np.asarray(table, dtype=_np.float64)).ravel()
        if self._native and self._handle is not None and self._n is not None:
            self._inject("bbo_bh_inject_draws", self._table)

    @staticmethod
    def draws(seed, substream, hop, n):
        """the n step uniforms and the accept uniform of one hop, as the device draws them (bbo_bh_draws)"""
        out = _np.zeros(n + 1)
        _ffi.check(_ffi.lib().bbo_bh_draws(int(seed) & 0xFFFFFFFFFFFFFFFF, int(substream), int(hop), int(n), out))
        return out

    # -- the Python-driven path ----------------------------------------------------------------
    def get_state(self, key, population=0):
        if self._native:
            return super().get_state(key, population)
        if self._py is None:
            raise RuntimeError("get_state() called before initialize()")
        py, st = self._py, self._stepstrat
        one = {"energy": py.get("energy"), "fbest": py.get("fbest"), "stepsize": st.stepsize, "nstep": st.nstep,
               "naccept": st.naccept, "it": py["it"], "fev": py["fev"], "n": self._n,
               "flag": 2 if py["it"] >= self._bh.mit else 0}
        if key in one:
            return _np.array([one[key]], dtype=_np.float64)
        if key in ("x", "xbest", "log", "log_start", "log_sol", "log_fev"):
            return _np.array(py[key], dtype=_np.float64).ravel()
        raise KeyError("unknown state key %r" % key)

    def _row(self, cells):
        print("".join(" | " + (c if isinstance(c, str) else "%d" % c if isinstance(c, int) else "%.17g" % c).rjust(w)
                      for c, w in zip(cells, self._WIDTHS)) + " | ")

    def _py_minimize(self, start):
        sol = self._minimizer.optimize(self._py["f"], self._py["lower"], self._py["upper"], start)
        x = sol.x
        f = self._py["f"]
        e = float(f(x))
        return x, (_np.inf if e != e else e), sol.n_evals, bool(sol.converged)

    def _py_initialize(self, f, lower, upper, guess):
        lower, upper, guess = _as_vec(lower, "lower"), _as_vec(upper, "upper"), _as_vec(guess, "guess")
        n = lower.size
        if not 1 <= n <= self.MAX_N:
            raise ValueError("BasinHopping: dimension must be in [1, %d]" % self.MAX_N)
        self._require_finite_box(n, lower, upper, "BasinHopping: a step is a fraction of upper - lower")
        if not callable(f):
            raise TypeError("the Python-driven path evaluates the energy on the host: the objective must be callable")
        self._n = n
        py = self._py = {"f": f, "lower": lower, "upper": upper[:n].copy(), "it": 0, "fev": 0,
                         "log": [], "log_start": [], "log_sol": [], "log_fev": []}
        x, e, fev, conv = self._py_minimize(guess[:n].copy())
        py["x"], py["energy"], py["xbest"], py["fbest"] = x.copy(), e, x.copy(), e
        py["fev"] += fev + 1
        st = self._stepstrat
        py["log"].append([-1., e, float(conv), st.stepsize, 1., e, float(py["fev"])])
        py["log_start"].append(guess[:n].copy()), py["log_sol"].append(x.copy()), py["log_fev"].append(fev)
        if self._bh.print:
            self._row(["it", "f", "conv", "step", "accept", "f*", "fev"])
            print(" |" + "=" * (sum(self._WIDTHS) + 3 * (len(self._WIDTHS) - 1) + 2) + "| ")
            self._row([-1, e, int(conv), st.stepsize, 1, e, py["fev"]])

    def _py_hop(self):
        """iterate() of the reference (basinhopping.cpp:155-190) in its operation order, on the device's draws"""
        py, st, n = self._py, self._stepstrat, self._n
        hop = py["it"]
        if self._table is not None and (hop + 1) * (n + 1) <= self._table.size:
            u = self._table[hop * (n + 1):(hop + 1) * (n + 1)]
        else:
            u = self.draws(self._params.seed, self._bh.substream, hop, n)
        if st._adaptive:
            st.nstep += 1
            if st.nstep % st.interval == 0:
                if (1. * st.naccept) / st.nstep > st.accept_rate:
                    st.stepsize /= st.factor
                else:
                    st.stepsize *= st.factor
        x1 = py["x"].copy()
        lo, up = py["lower"], py["upper"]
        for i in range(n):
            x1[i] += st.stepsize * u[i] * (up[i] - lo[i])
            margin = 0.05 * (up[i] - lo[i])
            hi, lw = up[i] - margin, lo[i] + margin
            t = hi if hi < x1[i] else x1[i]
            x1[i] = t if lw < t else lw
        x, e, fev, conv = self._py_minimize(x1.copy())
        py["fev"] += fev + 1
        beta = _np.inf if self._bh.temp == 0. else 1. / self._bh.temp
        with _np.errstate(invalid="ignore"):
            v = -(_np.float64(e) - _np.float64(py["energy"])) * _np.float64(beta)
        accept = bool(_np.exp(v if v < 0. else 0.) >= u[n])
        if accept:
            py["energy"], py["x"] = e, x.copy()
            if st._adaptive:
                st.naccept += 1
        if e < py["fbest"]:
            py["fbest"], py["xbest"] = e, x.copy()
        py["log"].append([float(hop), e, float(conv), st.stepsize, float(accept), py["fbest"], float(py["fev"])])
        py["log_start"].append(x1), py["log_sol"].append(x.copy()), py["log_fev"].append(fev)
        if self._bh.print:
            self._row([hop, e, int(conv), st.stepsize, int(accept), py["fbest"], py["fev"]])
        py["it"] += 1
