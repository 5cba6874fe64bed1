/*
 * bbopt_hip.h -- C ABI of libbbopt_hip.so, the MI355X (gfx950) population-based
 * black-box optimizer core.
 *
 * The reference (mike-gimelfarb/bboptpy) has NO C ABI: its plugin surface is the
 * C++ abstract class MultivariateOptimizer bound to Python with pybind11
 *     /root/reference/src/multivariate/multivariate.h:132-146   (init / iterate /
 *                                                                solution / optimize)
 *     /root/reference/py/multivariate_py.cpp:374-420            (MultivariateSearch)
 * This header is the C statement of exactly that four-method interface plus the
 * constructor argument lists of the algorithms on the hot path.  Every entry
 * point names the reference interface it replaces.  Plain pointers and sizes
 * only; all device memory, HIP streams and kernels live behind the handle.
 *
 * Threading: one host thread per handle at a time (the reference is single
 * threaded and holds the GIL for a whole optimize(), multivariate_py.cpp:376-395).
 * Errors: every function returns BBO_OK (0) or a negative bbo_status;
 * bbo_last_error() gives the text (the reference throws std::invalid_argument /
 * propagates Python exceptions instead, apso.cpp:381,448).
 */
#ifndef BBOPT_HIP_H_
#define BBOPT_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bbo_handle_s *bbo_handle;

typedef enum {
    BBO_OK = 0,
    BBO_ERR_ARG = -1,        /* bad argument / unsupported shape                 */
    BBO_ERR_STATE = -2,      /* call out of order (e.g. iterate before init)     */
    BBO_ERR_HIP = -3,        /* a HIP runtime call or kernel failed              */
    BBO_ERR_NO_DEVICE = -4,  /* no gfx950 device visible: there is NO CPU path   */
    BBO_ERR_CALLBACK = -5,   /* the host objective callback reported failure     */
    BBO_ERR_KEY = -6         /* unknown state key in bbo_get / bbo_set           */
} bbo_status;

/* Algorithms on the hot path; names are the reference's Python class names
 * (py/multivariate_py.cpp:103-115,137-171,265-269). */
typedef enum {
    BBO_ALGO_CMAES = 0,        /* Cmaes        src/multivariate/cma/cmaes.h:40        */
    BBO_ALGO_ACTIVE_CMAES = 1, /* ActiveCmaes  src/multivariate/cma/active_cmaes.h:40 */
    BBO_ALGO_SHADE = 2,        /* ShadeSearch  src/multivariate/de/shade.h:42         */
    BBO_ALGO_JADE = 3,         /* JadeSearch   src/multivariate/de/jade.h:49          */
    BBO_ALGO_APSO = 4,         /* APSOSearch   src/multivariate/pso/apso.h:38         */
    BBO_ALGO_IPOP_CMAES = 5,   /* IPopCmaes    src/multivariate/cma/ipop_cmaes.h:55   */
    BBO_ALGO_BIPOP_CMAES = 6,  /* BiPopCmaes   src/multivariate/cma/bipop_cmaes.h:49  */
    BBO_ALGO_SEP_CMAES = 7,    /* SepCmaes     src/multivariate/cma/sep_cmaes.h:36    */
    BBO_ALGO_SANSDE = 8,       /* SaNSDESearch src/multivariate/de/sansde.h:40        */
    BBO_ALGO_CSO = 9,          /* CSOSearch    src/multivariate/pso/cso.h:44          */
    BBO_ALGO_CCPSO = 10,       /* CCPSOSearch  src/multivariate/pso/ccpso.h:46        */
    BBO_ALGO_CHOLESKY_CMAES = 11, /* CholeskyCmaes src/multivariate/cma/cholesky_cmaes.h:37 */
    BBO_ALGO_JAYA = 12,        /* JayaSearch   src/multivariate/jaya/jaya.h:50        */
    BBO_ALGO_DSA = 13,         /* DSSearch     src/multivariate/pso/ds.h:33           */
    BBO_ALGO_HEES = 14,        /* Hees         src/multivariate/hees/hees.h:53        */
    BBO_ALGO_SPIRAL = 15,      /* SpiralSearch src/multivariate/spiral/spiral.h:39    */
    BBO_ALGO_NSHS = 16,        /* NSHS         src/multivariate/harmony/nshs.h        */
    BBO_ALGO_LM_CMAES = 17,    /* LmCmaes      src/multivariate/cma/lm_cmaes.h:43     */
    BBO_ALGO_XNES = 18,        /* xNES         src/multivariate/nes/xnes.h:48         */
    BBO_ALGO_AMALGAM = 19,     /* Amalgam      src/multivariate/amalgam/amalgam.h     */
    BBO_ALGO_SLPSO = 20,       /* SLPSOSearch  src/multivariate/pso/slpso.h           */
    BBO_ALGO_CRS = 21,         /* CrsSearch    src/multivariate/crs/crs.h             */
    BBO_ALGO_SSDE = 22,        /* SSDESearch   src/multivariate/de/ssde.h             */
    BBO_ALGO_ACD = 23,         /* ACD          src/multivariate/acd/acd.h             */
    BBO_ALGO_MAYFLY = 24,      /* MayflySearch src/multivariate/mayfly/mayfly.h       */
    BBO_ALGO_PIKAIA = 25,      /* PikaiaSearch src/multivariate/pikaia/pikaia.h       */
    BBO_ALGO_NELDER_MEAD = 26, /* NelderMead   src/multivariate/simplex/nelder_mead.h */
    BBO_ALGO_ROSENBROCK = 27,  /* Rosenbrock   src/multivariate/rosenbrock/rosenbrock.h */
    BBO_ALGO_BASIN_HOPPING = 28 /* BasinHopping src/multivariate/basin/basinhopping.h  */
} bbo_algo;

/* Built-in objectives evaluated on the device (the reference ships none; id 1 is
 * the README objective, README.md:111-112).  Same ids as oracle/objectives.h. */
typedef enum {
    BBO_OBJ_SPHERE = 0,
    BBO_OBJ_ROSENBROCK = 1,
    BBO_OBJ_RASTRIGIN = 2,
    BBO_OBJ_ELLIPSOID = 3,
    BBO_OBJ_ACKLEY = 4,
    BBO_OBJ_GRIEWANK = 5,
    BBO_OBJ_CIGAR = 6,
    BBO_OBJ_DISCUS = 7,
    BBO_OBJ_DIFFPOW = 8,
    BBO_OBJ_SCHWEFEL12 = 9
} bbo_objective_id;

/* Host objective callbacks -- the compatibility path for an arbitrary Python `f`
 * (replaces the std::function<double(const double*)> of multivariate.h:32 and the
 * per-evaluation NumPy wrapper of multivariate_py.cpp:385-388).
 *   scalar: one candidate, returns f(x); set *failed != 0 to abort the run.
 *   batch:  `rows` candidates of `n` coordinates, row stride `ld` doubles;
 *           writes f_out[rows]; returns 0 on success.                          */
typedef double (*bbo_scalar_fn)(const double *x, int n, void *user, int *failed);
typedef int (*bbo_batch_fn)(const double *X, int rows, int n, int ld, double *f_out,
        void *user);

typedef enum {
    BBO_OBJECTIVE_BUILTIN = 0,
    BBO_OBJECTIVE_SCALAR_CALLBACK = 1,
    BBO_OBJECTIVE_BATCH_CALLBACK = 2,
    BBO_OBJECTIVE_PROGRAM = 3   /* a bbo_program (below) in `user`: evaluated on the device     */
} bbo_objective_kind;

typedef struct {
    int kind;              /* bbo_objective_kind                                  */
    int builtin;           /* bbo_objective_id when kind == BUILTIN               */
    bbo_scalar_fn scalar;
    bbo_batch_fn batch;
    void *user;            /* the callbacks' cookie; the bbo_program when kind == PROGRAM */
} bbo_objective;

/* ---- objective programs (extension): the caller's own objective on the device -----------------
 * The caller hands over HIP source that defines ONE device function,
 *     extern "C" __device__ double bbo_user_objective(const double *x, int n, const double *data);
 * (x: the candidate, n coordinates, in global memory or in LDS -- a plain pointer serves both;
 * data: the caller's table).  bbo_program_create compiles it at run time (hiprtc, opened with
 * dlopen at the first call: the library loads and everything else works without it) with
 * -O3 -ffp-contract=off, the rule of the library's own kernels: a function written in the operation
 * order of a host function returns the same bits.  A handle initialised with
 * { kind = BBO_OBJECTIVE_PROGRAM, user = program } evaluates whole populations with it on its own
 * stream: candidates and fitness never leave device memory, bbo_run polls every `poll_every`
 * generations as for a built-in.  A NaN result ranks last (+inf), as for the callbacks.
 *   arch   NULL: the architecture string device 0 reports, unchanged; else e.g. "gfx950" -- then no
 *          device is touched, the call works on a machine without a GPU.  xnack+ is refused.
 *   data   data_count doubles, copied (data_count may be 0); uploaded to every device the program
 *          is used on.  The code object is loaded once per device at the first bbo_init using it.
 * Errors: BBO_ERR_ARG when the source does not compile, does not define bbo_user_objective, or
 * hiprtc is absent; bbo_last_error(NULL) then carries the compiler's log with the caller's own
 * lines and columns ("objective.hip:LINE:COL").  Supported by CMAES, ActiveCMAES, SepCMAES,
 * CholeskyCMAES, IPOP / BIPOP over them, JADE, SHADE, SANSDE; APSO, CSO, CCPSO return BBO_ERR_ARG
 * from bbo_init.  A handle shares ownership of the program from bbo_init on:
 * bbo_program_destroy may be called while handles still use it.  The function must read only
 * x[0, n) and its table, and must terminate. */
typedef struct bbo_program_s *bbo_program;
int bbo_program_create(const char *source, const char *arch, const double *data, int data_count,
        bbo_program *out);
int bbo_program_destroy(bbo_program p);

/* Constructor arguments.  Field names and defaults are the reference's keyword
 * arguments (py/multivariate_py.cpp): zero-initialise, call bbo_params_default(),
 * then overwrite.  Fields an algorithm does not use are ignored. */
typedef struct {
    int algo;              /* bbo_algo                                            */
    /* shared */
    int mfev;              /* maximum objective evaluations                       */
    double tol;            /* stop tolerance (meaning differs per family, SURVEY A-17) */
    int np;                /* population size: CMA `np` (lambda), JADE/APSO `np`, SHADE `npinit` */
    /* CMAES(mfev,tol,np,sigma0=2,bound=False,eigenrate=0.25)            :103-108
     * ActiveCMAES(...,alphacov=2,eigenrate=0.25)                         :110-115
     * SepCMAES(mfev,tol,np,sigma0=2,bound=False,adjustlr=True)          :131-135 */
    double sigma0;
    int bound;
    double alphacov;
    double eigenrate;
    /* JADE(mfev,np,tol,archive=True,repaircr=True,pelite=.05,cdamp=.1,sigma=.07) :159-164
     * SHADE(mfev,npinit,tol,archive=True,repaircr=True,h=100,npmin=4)            :166-171 */
    int archive;
    int repaircr;
    double pelite;
    double cdamp;
    double jade_sigma;
    int h;
    int npmin;
    /* APSO(mfev,tol,np,correct=True)                                     :265-269 */
    int correct;
    /* IPopCMAES(base,mfev,print=False,sigma0=2,nipop=True,ksigmadec=1.6,boundlambda=True) :137-142
     * BiPopCMAES(base,mfev,print=False,sigma0=2,maxlargeruns=9,nbipop=True,
     *            ksigmadec=1.6,kbudget=2)                                        :144-151
     * (the `base` optimizer is passed to bbo_create_restart) */
    int print;
    int nipop;             /* IPOP `nipop` / BIPOP `nbipop`                       */
    double ksigmadec;
    int boundlambda;
    int maxlargeruns;
    double kbudget;
    /* ---- extensions (no reference counterpart; defaults keep reference behaviour) */
    uint64_t seed;         /* Philox key.  The reference seeds from random_device +
                              clock and has no seed API (random.hpp:150-163)      */
    int device;            /* HIP device ordinal                                  */
    int populations;       /* independent populations advanced in lockstep by one
                              handle (>= 1); population p uses sub-stream p       */
    int poll_every;        /* generations between host polls of the device stop
                              flag inside bbo_optimize / bbo_run (default 8)      */
    /* ---- appended in round 1 (SepCMAES): keeps the layout of everything above */
    int adjustlr;          /* SepCmaes `adjustlr` (sep_cmaes.cpp:60-62)            */
    /* SANSDE(mfev,np,tol,repaircr=True,crref=5,pupdate=50,crupdate=25)  :174-177 */
    int crref;             /* generations between redraws of the per-individual CR */
    int pupdate;           /* generations between updates of the strategy probability */
    int crupdate;          /* generations between updates of the CR mean and of fp */
    /* CSO(mfev,stol,np,pcompete=3,ring=False,correct=True,vmax=0.2)     :272-275
     * (`stol` travels in `tol`, `correct` is shared with APSO) */
    int pcompete;          /* particles per competition                            */
    int ring;              /* ring neighbourhood instead of the swarm mean         */
    double vmax;           /* velocity clamp as a fraction of the box width        */
    /* CCPSO(mfev,sigmatol,np,pps,npps,correct=True,pcauchy=-1,local=None,localfreq=10) :291-295
     * (`sigmatol` travels in `tol`; the optional local optimizer: bbo_ccpso_set_local below) */
    int npps;              /* number of candidate swarm sizes                      */
    int pps[16];           /* the candidate swarm sizes (each must divide n)       */
    double pcauchy;        /* fixed Cauchy rate in (0,1), else adaptive            */
    /* ---- appended for CholeskyCMAES: keeps the layout of everything above.  The library reads
     * and writes these two fields only when algo == BBO_ALGO_CHOLESKY_CMAES or BBO_ALGO_DSA (a
     * caller that can name algorithm 13 was compiled against this struct), so a caller compiled
     * against an earlier header (a shorter struct, none of whose algorithms is one of these) stays
     * binary compatible: bbo_params_default and bbo_create* never touch memory past its struct.
     * CholeskyCMAES(mfev,tol,stol,np,sigma0=2,bound=False)              :118-120
     * DSA(mfev,tol,stol,np,adapt=True,nbatch=100)                       :189-191
     * (`adapt` and `nbatch`: bbo_dsa_params below) */
    double stol;           /* tolerance on the spread of the candidates' (DSA: the members') radii */
    int ranked;            /* (extension, default 0) rank-mu term of the factor update:
                              0 = the reference's (cholesky_cmaes.cpp:91-94): the FIRST mu
                                  candidates in sampling order, centred on the NEW mean;
                              1 = the textbook form: the mu best, centred on the old mean */
} bbo_params;

void bbo_params_default(bbo_params *p, int algo);

/* ---- life cycle ----------------------------------------------------------------
 * bbo_create            <- the Python constructors (py/multivariate_py.cpp:103-171,265-269)
 * bbo_create_restart    <- IPopCmaes / BiPopCmaes constructors taking `BaseCmaes *base`
 *                          (ipop_cmaes.cpp:56, bipop_cmaes.cpp:54): a CMAES, ActiveCMAES,
 *                          SepCMAES or CholeskyCMAES handle.  `base` stays owned
 *                          by the caller and must outlive the driver, as in the reference.
 * bbo_destroy           <- destructor                                                  */
int bbo_create(const bbo_params *params, bbo_handle *out);
int bbo_create_restart(const bbo_params *params, bbo_handle base, bbo_handle *out);
int bbo_destroy(bbo_handle h);

/* ---- the four methods of MultivariateOptimizer (multivariate.h:132-146) ----------
 * lower/upper/guess are borrowed for the call and copied, like base_cmaes.cpp:63-64,124.
 * With populations > 1, guess holds populations*n doubles (one row per population).
 *
 * bbo_init      <- init(const multivariate_problem&, const double *guess)
 *                  Python: initialize(f, lower, upper, guess)  multivariate_py.cpp:397-416
 * bbo_iterate   <- iterate()                                   multivariate_py.cpp:418
 * bbo_solution  <- solution() -> {x, n_evals, converged}       multivariate_py.cpp:360-371,420
 *                  (population 0; bbo_solution_of for the others)
 * bbo_optimize  <- optimize(problem, guess) = init + loop      multivariate_py.cpp:376-395 */
int bbo_init(bbo_handle h, int n, const double *lower, const double *upper,
        const double *guess, const bbo_objective *objective);
int bbo_iterate(bbo_handle h);
int bbo_solution(bbo_handle h, double *x_out, int *n_evals, int *converged);
int bbo_solution_of(bbo_handle h, int population, double *x_out, int *n_evals,
        int *converged);
int bbo_optimize(bbo_handle h, int n, const double *lower, const double *upper,
        const double *guess, const bbo_objective *objective, double *x_out, int *n_evals,
        int *converged);

/* ---- throughput entry point (extension) -------------------------------------------
 * Runs up to max_generations generations without returning to the caller, stopping
 * early when every population's own stop rule has fired (the loop body of
 * base_cmaes.cpp:166-172 / shade.cpp:247-253 / apso.cpp:118-124 kept on the device).
 * generations_done counts launched generations; a population that stopped earlier is
 * frozen exactly at its stopping generation. */
int bbo_run(bbo_handle h, int max_generations, int *generations_done);

/* ---- state access (parity tests, checkpointing) ------------------------------------
 * Named read/write access to the optimizer state, the counterpart of the reference's
 * protected members (base_cmaes.h:52-63, cmaes.h:42-46, shade.h:44-51, apso.h:46-66).
 * bbo_get returns the element count (>= 0) or a negative bbo_status; call with cap 0
 * to size a buffer.  Keys are listed in HISTORY.md (last section) and DESIGN.md section 9.
 * One key changes semantics the reference's user can see: APSO "chunk" -- the number of particles
 * that move between two refreshes of the swarm's best inside a generation (the reference refreshes
 * after every particle, apso.cpp:194-197; the default here is np / 16 in whole workgroups, at least
 * 64; 0 or any value from np up = the whole swarm sees the best of the generation start; a NaN,
 * infinite or negative value is BBO_ERR_ARG). */
/* CholeskyCMAES (BBO_ALGO_CHOLESKY_CMAES): the keys the dense variants share (arx, xmean, xold,
 * sigma, pc, ps, fit_val, fit_idx, it, fev, flag, zlast, record_normals, ...) plus "A" (the lower
 * Cholesky factor of the covariance, n x n row-major, upper triangle exactly 0; readable and
 * writable) and "chol_repairs" (sticky count of pivots the factor update had to lift to a positive
 * value: 0 unless rounding broke a factorisation); B, C, D, invsqrtC return BBO_ERR_KEY.  Its stop
 * rule (cholesky_cmaes.cpp:137-161: |f_best - f_worst| <= tol and the squared deviations of the
 * candidates' radii sum to <= (lambda - 1) stol^2) reports "flag" 11; flags 1-10 belong to the
 * other variants.  "chol_tri" (default 1): at n = 128 the samplers issue only the products of
 * the factor's lower block triangle; 0 selects the full-operand samplers (the same bits).
 * Writable on this variant only, for crafting states of its stop rule: "arx" and "fitness"
 * (lambda values in sampling order; the ranking "fit_idx" is NOT redone). */
int bbo_get(bbo_handle h, const char *key, int population, double *out, int cap);
int bbo_set(bbo_handle h, const char *key, int population, const double *in, int count);

/* One phase of a CMA-ES generation, for step-level parity tests
 * (the template-method hooks of base_cmaes.h:80-92). */
typedef enum {
    BBO_PHASE_SAMPLE_EVALUATE = 0, /* samplePopulation + objective       cmaes.cpp:65-80       */
    BBO_PHASE_RANK = 1,            /* sort part of evaluateAndSortPopulation base_cmaes.cpp:221 */
    BBO_PHASE_UPDATE = 2,          /* updateDistribution without eigen   active_cmaes.cpp:71-164 */
    BBO_PHASE_EIGEN = 3,           /* eigenDecomposition                 cmaes.cpp:229-283
                                      (SepCMAES, CholeskyCMAES: nothing to do, BBO_OK)          */
    BBO_PHASE_HISTORY_STOP = 4     /* updateHistory, it++, converged()   base_cmaes.cpp:191-209, cmaes.cpp:151-227 */
} bbo_cma_phase;
int bbo_cma_phase_run(bbo_handle h, int phase);

/* Injects the standard normals of the next sampling phase (populations*lambda*n doubles,
 * row-major) instead of drawing them on the device; used by the parity tests to feed the
 * reference's own draws.  Pass NULL to return to the device generator. */
int bbo_cma_inject_normals(bbo_handle h, const double *z, int count);

/* BaseCmaes::setParams(np, sigma, mfev) (base_cmaes.cpp:136-148): what the reference's restart
 * drivers call on their borrowed `base` before every inner run (bipop_cmaes.cpp:83,220,251;
 * ipop_cmaes.cpp:92,140).  Like the reference it switches `bound` off with a warning on stderr.
 * Takes effect at the next bbo_init / bbo_optimize; B and C keep their off-diagonals across
 * re-inits of one handle with the same n (cmaes.cpp:53-59). */
int bbo_cma_set_params(bbo_handle h, int np, double sigma0, int mfev);

/* (extension) a new Philox key for the next bbo_init / bbo_optimize of this handle; the
 * reference has no seed API (random.hpp:150-163). */
int bbo_cma_set_seed(bbo_handle h, uint64_t seed);

/* One evaluation of the handle's objective at x (n doubles), with the objective bound by the
 * last bbo_init / bbo_optimize: the restart drivers' re-evaluation of the point an inner run
 * returned (`_f._f(&x[0])`, bipop_cmaes.cpp:86,223,254; ipop_cmaes.cpp:95,143). */
int bbo_cma_evaluate(bbo_handle h, const double *x, double *f_out);

/* ---- CCPSO swarm groups sharded over GPUs (extension) --------------
 * The 2 (n/s) np context-vector evaluations of a CCPSO generation (CCPSOSearch::updateSwarm,
 * ccpso.cpp:241-260, each through evaluate :152-171) are independent while yhat is frozen.
 * With bbo_ccpso_set_shard(rank, world) a handle evaluates only its block of swarms,
 *   [nswarm * rank / world, nswarm * (rank + 1) / world),
 * and a generation becomes: phase 0 (regroup + evaluate this block) on every rank, ONE
 * all-gather of the fitness records, bbo_ccpso_merge_tables, phase 1 (the rest of updateSwarm,
 * updatePosition, the stop test: replicated, identical on every rank).  A record is
 * bbo_ccpso_table_record(h) doubles: only the rows of the swarms this rank evaluated, fX block
 * | fY block, each ceil(max swarms / world) * np doubles (max swarms = n / the smallest swarm
 * size); `device_memory` != 0 says the caller's pointer is device memory (e.g. an RCCL buffer),
 * else host memory.  One population.  While world > 1, bbo_iterate / bbo_run / bbo_optimize
 * return BBO_ERR_STATE: only the phase / merge protocol advances a sharded handle.
 * BUFFER LIFETIME with device_memory != 0: bbo_ccpso_merge_tables only ENQUEUES the merge kernel
 * on the handle's stream and returns; `gathered` must stay allocated and unmodified until the
 * next call on this handle that waits for the stream -- bbo_ccpso_export_tables (host or device),
 * bbo_get, bbo_solution, or bbo_ccpso_phase(h, 1) -- has returned (ShardedCCPSO reuses one
 * buffer per handle and overwrites it only in the next generation's all-gather, which follows the
 * next export).  A kernel error of the merge surfaces at that call.  With host memory the call
 * has copied `gathered` when it returns.  bbo_ccpso_export_tables with device_memory != 0 has
 * finished writing `dst` when it returns (the collective may start at once). */
int bbo_ccpso_set_shard(bbo_handle h, int rank, int world);
/* CCPSO's optional local optimizer (CCPSOSearch(..., local, localfreq), ccpso.cpp:51-70; used at
 * :116-118 and :371-435; py/multivariate_py.cpp:291-295).  `local` is BORROWED, like the
 * reference's pointer (and like `base` of bbo_create_restart): it must outlive h or be detached
 * with bbo_ccpso_set_local(h, NULL, 0).  After generation g with g % localfreq == 0, bbo_iterate /
 * bbo_run / bbo_optimize optimize one weight per swarm with it (objective evaluated on the host:
 * the callback of h's objective, or the built-in's formula), replace the context vector if the
 * result is better and charge the evaluations.  A CMA-ES `local` starts every search afresh
 * (B = C = I, seed = its own seed + search index).  One population; not with bbo_ccpso_set_shard. */
int bbo_ccpso_set_local(bbo_handle h, bbo_handle local, int localfreq);
int bbo_ccpso_phase(bbo_handle h, int phase);
int bbo_ccpso_table_record(bbo_handle h);
int bbo_ccpso_export_tables(bbo_handle h, double *dst, int device_memory);
int bbo_ccpso_merge_tables(bbo_handle h, const double *gathered, int world, int device_memory);

/* ---- JAYA (BBO_ALGO_JAYA): JAYA(mfev,tol,np,npmin,adapt=True,k0=2,mutation=logistic,scale=0.01,
 * beta=1.5,kcheb=2,temper=10.)  py/multivariate_py.cpp:213-234.  `mfev`, `tol`, `np` and `npmin`
 * travel in bbo_params (whose layout stays as it is); the seven other constructor arguments travel
 * here.  bbo_jaya_configure is legal between bbo_create and bbo_init; without it the defaults
 * hold.  BBO_ERR_ARG: not a JAYA handle, k0 outside 1..nks (nks = the number of k >= 1 with
 * np >= npmin k), beta outside (0, 2] or an unknown mutation; BBO_ERR_STATE after bbo_init.
 * `kcheb` is stored and unused, as in the reference. */
typedef enum {
    BBO_JAYA_ORIGINAL = 0,
    BBO_JAYA_LEVY = 1,
    BBO_JAYA_TENT_MAP = 2,
    BBO_JAYA_LOGISTIC = 3
} bbo_jaya_mutation;
typedef struct { int adapt, k0, mutation, kcheb; double scale, beta, temper; } bbo_jaya_params;
void bbo_jaya_params_default(bbo_jaya_params *p);   /* 1, 2, 3 (logistic), 2, 0.01, 1.5, 10. */
int bbo_jaya_configure(bbo_handle h, const bbo_jaya_params *p);

/* ---- DSA (BBO_ALGO_DSA): DSA(mfev,tol,stol,np,adapt=True,nbatch=100)  py/multivariate_py.cpp:189-191,
 * Differential Search with a Rexp3 bandit over its four direction methods (ds.cpp).  `mfev`, `tol`,
 * `stol` and `np` travel in bbo_params (np >= 1, a finite box, `guess` is ignored); `adapt` and
 * `nbatch` travel here.  bbo_dsa_configure is legal between bbo_create and bbo_init; without it the
 * defaults hold.  BBO_ERR_ARG: not a DSA handle or nbatch < 1; BBO_ERR_STATE after bbo_init.
 * Objective programs are refused by bbo_init (BBO_ERR_ARG); DSA is no base of a restart driver. */
typedef struct { int adapt, nbatch; } bbo_dsa_params;
void bbo_dsa_params_default(bbo_dsa_params *p);     /* 1, 100 */
int bbo_dsa_configure(bbo_handle h, const bbo_dsa_params *p);

/* ---- HEES (BBO_ALGO_HEES): HEES(mfev,tol,mres=1,print=False,np=0,sigma0=2.)  py/multivariate_py.cpp:206-211,
 * the Hessian Estimation Evolution Strategy (Glasmachers & Krause 2020; hees.cpp).  `mfev`, `tol`, `np`
 * (0 or less: mu = int(2 + 1.5 ln n)) and `sigma0` travel in bbo_params; `mres` and `print` travel
 * here.  bbo_hees_configure is legal between bbo_create and bbo_init; without it the defaults hold.
 * BBO_ERR_ARG: not a HEES handle; BBO_ERR_STATE after bbo_init.  Limits: n in [1, 512], mu <= 4096
 * (bbo_init returns BBO_ERR_ARG beyond them).  The box is never used to clamp.  bbo_optimize with
 * mres > 1 makes up to mres runs from the remaining budget, mu doubling from run to run, the start
 * points uniform in the box from the second run on (a finite box and populations = 1 are required;
 * run r uses the seed of the handle + r - 1); with `print` it writes the reference's table (iter | f* |
 * fev, one row per run) to stdout and reports converged = 0.  bbo_init / bbo_iterate / bbo_run
 * ignore mres, as the reference's init / iterate do.  Objective programs are refused by bbo_init;
 * HEES is no base of a restart driver.
 * bbo_hees_phase: one part of a generation (0 sample + evaluate, 1 rank, 2 the updates of A, m,
 * p_s and sigma, 3 f(m), the counters and the stop test); the four in order are bbo_iterate.
 * bbo_hees_inject_normals: the normals of the following generations instead of the device's draws,
 * `populations` tables of (B n) x n doubles, B = ceil(mu / n), as the reference draws them: the
 * first mu rows of each are used.  NULL returns to the device generator; bbo_init does the same. */
typedef struct { int mres, print; } bbo_hees_params;
void bbo_hees_params_default(bbo_hees_params *p);   /* 1, 0 */
int bbo_hees_configure(bbo_handle h, const bbo_hees_params *p);
int bbo_hees_phase(bbo_handle h, int phase);
int bbo_hees_inject_normals(bbo_handle h, const double *z, int count);

/* ---- SpiralSearch (BBO_ALGO_SPIRAL): SpiralSearch(mfev,tol,np=20,r=0.95,theta=1.57079632679,taur=0.0,
 * tautheta=0.1,rlow=0.9,rhigh=1.0,thetalow=0.0,thetahigh=6.28318530718)  py/multivariate_py.cpp:344-351,
 * the adaptive spiral optimization algorithm (Tamura & Yasuda 2011; Yuzgec & Inac 2016; spiral.cpp).
 * `mfev`, `tol` (stored and unused, as in the reference) and `np` travel in bbo_params
 * (bbo_params_default gives np = 20); the eight other constructor arguments travel here.
 * bbo_spiral_configure is legal between bbo_create and bbo_init; without it the defaults hold.
 * BBO_ERR_ARG: not a SpiralSearch handle or a value that is not finite; BBO_ERR_STATE after bbo_init.
 * Limits: n in [1, 512], np in [1, 65536], a finite box (it seeds the points and never clamps them);
 * `guess` is ignored; converged is always 0 and "flag" is 0 or 2 (the budget).  Objective programs are
 * refused by bbo_init; SpiralSearch is no base of a restart driver.
 * bbo_spiral_phase: one part of a generation (0 the draws of r and theta, 1 the rotation, 2 the
 * evaluation, 3 the best point, the counters and the budget); the four in order are bbo_iterate.
 * bbo_spiral_inject_uniforms: `populations` tables of np x 4 raw uniforms in [0, 1) -- per point the
 * coin of r, the value of r, the coin of theta, the value of theta -- which the following
 * generations consume instead of the device's draws.  NULL returns to the device generator;
 * bbo_init does the same. */
typedef struct { double r, theta, taur, tautheta, rlow, rhigh, thetalow, thetahigh; } bbo_spiral_params;
void bbo_spiral_params_default(bbo_spiral_params *p);   /* 0.95, 1.57079632679, 0, 0.1, 0.9, 1, 0, 6.28318530718 */
int bbo_spiral_configure(bbo_handle h, const bbo_spiral_params *p);
int bbo_spiral_phase(bbo_handle h, int phase);
int bbo_spiral_inject_uniforms(bbo_handle h, const double *u, int count);

/* ---- NSHS (BBO_ALGO_NSHS): NSHS(mfev,hms,fstdmin=0.0001)  py/multivariate_py.cpp:200-205, the novel
 * self-adaptive harmony search (Luo 2013; nshs.cpp).  `mfev` and `np` (which is hms: required, no
 * default) travel in bbo_params; fstdmin travels here.  For this algorithm bbo_params_default gives
 * poll_every = 0: bbo_run then launches the engine's own chunk of whole ITERATIONS per poll (one
 * iteration is one evaluation), a positive poll_every is that many iterations per launch.
 * bbo_nshs_configure is legal between bbo_create and bbo_init; without it the default holds.
 * BBO_ERR_ARG: not an NSHS handle or a value that is not finite or negative; BBO_ERR_STATE after
 * bbo_init.
 * Limits: n in [1, 512], hms in [1, 4096], a finite box; `guess` is ignored; converged is always 0 and
 * "flag" is 0 or 2 (the budget, reached exactly: fev == mfev).  With mfev <= hms bbo_init evaluates
 * the memory, bbo_run does nothing and bbo_iterate / bbo_nshs_phase return BBO_ERR_STATE (the
 * reference would divide by mfev - hms <= 0).  Objective programs are refused by bbo_init; NSHS is no
 * base of a restart driver.
 * bbo_nshs_phase: one part of an iteration (0 the candidate, 1 its evaluation, 2 the replacement of
 * the worst row with fstd, best, worst, the counters and the budget); the three in order are
 * bbo_iterate.
 * bbo_nshs_inject_uniforms: `populations` tables of n x 4 raw uniforms in [0, 1) -- per coordinate
 * the coin, the row, the fresh value, the adjustment; the row j travels as (j + 0.5) / hms and is
 * mapped back by floor(u hms) -- which the following iterations consume instead of the device's
 * draws.  NULL returns to the device generator; bbo_init does the same. */
typedef struct { double fstdmin; } bbo_nshs_params;
void bbo_nshs_params_default(bbo_nshs_params *p);   /* 0.0001 */
int bbo_nshs_configure(bbo_handle h, const bbo_nshs_params *p);
int bbo_nshs_phase(bbo_handle h, int phase);
int bbo_nshs_inject_uniforms(bbo_handle h, const double *u, int count);

/* ---- LmCMAES (BBO_ALGO_LM_CMAES): LmCMAES(mfev,tol,np,memory=0,sigma0=2,bound=False,
 * rademacher=True,usenew=True)  py/multivariate_py.cpp:123-128, the limited-memory CMA-ES (Loshchilov
 * 2014 / 2015; lm_cmaes.cpp): m direction vectors instead of a covariance matrix, O(m n) per
 * candidate.  mfev, tol, np (lambda), sigma0 and bound travel in bbo_params; memory (<= 0: m =
 * int(2 sqrt(n))), rademacher and usenew travel here.  bbo_lm_configure is legal between bbo_create
 * and bbo_init; without it the defaults hold.  BBO_ERR_ARG: not an LmCMAES handle; BBO_ERR_STATE
 * after bbo_init.
 * Limits, each refused by bbo_init with a message: n in [1, 4096], np in [2, 4096], m in [1, 256], a
 * finite sigma0.  `bound` clamps the mean to the box and never a candidate, as in the reference.
 * "flag": 1 MaxIter, 2 TolHistFun, 3 EqualFunVals (the CMA engines' codes), 11 sigma < 1e-16.
 * Objective programs are refused by bbo_init; LmCMAES is no base of a restart driver.
 * bbo_lm_phase: one part of a generation (0 the sampling, 1 the evaluation, 2 the ranking, 3 the
 * update of the mean, pc, the memory and sigma, 4 the histories, the counters and the stop tests);
 * the five in order are bbo_iterate.
 * bbo_lm_inject_draws: G >= 1 generations of draws, count = G * populations * ceil(np / 2) * (n + 1)
 * doubles as [G][populations][ceil(np / 2)][n + 1]: a row is the z of a "+" candidate (normals, or
 * the +-1 of the Rademacher coin as values) followed by the normal g of selectSubset (ignored where
 * the reference draws none: usenew off, or fewer than two slots in use).  The following G
 * generations consume them; sampling a generation beyond them is BBO_ERR_STATE.  NULL returns to
 * the device generator; bbo_init does the same. */
typedef struct { int memory, rademacher, usenew; } bbo_lm_params;
void bbo_lm_params_default(bbo_lm_params *p);   /* 0, 1, 1 */
int bbo_lm_configure(bbo_handle h, const bbo_lm_params *p);
int bbo_lm_phase(bbo_handle h, int phase);
int bbo_lm_inject_draws(bbo_handle h, const double *table, int count);

/* ---- xNES (BBO_ALGO_XNES): xNES(mfev,tol,a0=1.,etamu=1.), the exponential natural evolution strategy
 * (Glasmachers et al. 2010; xnes.cpp).  mfev and tol travel in bbo_params; a0 (the first sigma), etamu
 * and from_guess travel here.  The population size is 4 + int(3 ln n), no parameter.  As in the
 * reference the mean starts at the ORIGIN and neither `guess` nor the box is used; from_guess = 1 (an
 * extension) starts the mean at `guess`.  bbo_solution returns the best point of the LAST generation
 * (the reference's _points[0]); "xbest" / "fbest" hold the best ever seen.  "stop": 1 |f_best -
 * f_worst| < tol in the ranked generation, 2 fev >= mfev (fev is a multiple of np).
 * bbo_xnes_configure is legal between bbo_create and bbo_init; BBO_ERR_ARG: not an xNES handle, or a0
 * not finite or not positive; BBO_ERR_STATE after bbo_init.  Limits: n in [1, 512]; objective
 * programs are refused by bbo_init; xNES is no base of a restart driver.
 * bbo_xnes_phase: one part of a generation (0 sample + evaluate, 1 rank, 2 the small step: mean,
 * sigma, counters, stop test and the operator of the update of B, 3 the update of B); the four in
 * order are bbo_iterate.
 * bbo_xnes_inject_normals: count = G * populations * np * n doubles as [G][populations][np][n], the
 * normals of the following G generations in sampling order; sampling beyond them is BBO_ERR_STATE.
 * NULL returns to the device generator; bbo_init does the same.
 * "route": 1 the low-rank update (n >= "lowrank_min_n", default 32, settable in [16, 32]), 0 the
 * dense one.  "fact_fail": generations whose low-rank factorisation met a pivot that was not finite
 * or not above 2^-40 of its diagonal (equal or dependent rows); B is left as it is in such a one. */
typedef struct { double a0, etamu; int from_guess; } bbo_xnes_params;
void bbo_xnes_params_default(bbo_xnes_params *p);   /* 1., 1., 0 */
int bbo_xnes_configure(bbo_handle h, const bbo_xnes_params *p);
int bbo_xnes_phase(bbo_handle h, int phase);
int bbo_xnes_inject_normals(bbo_handle h, const double *z, int count);

/* ---- AMALGAM (BBO_ALGO_AMALGAM): AMALGAM(mfev,tol,stol,np=0,iamalgam=True,noparam=True,print=True), the
 * AMaLGaM-IDEA and iAMaLGaM-IDEA of Bosman, Grahl & Thierens 2009 (amalgam.cpp).  mfev, tol, stol and np
 * travel in bbo_params (np <= 0: int(10 sqrt n) for iAMaLGaM, int(17 + 3 n^1.5) for AMaLGaM); the rest
 * travels here.  The population starts uniform in the box: a finite box is mandatory, `guess` is not
 * read.  keep_elite = 1 (an extension) leaves the x of row 0 alone in the sampler; the default, as the
 * reference, resamples it and keeps its old value.  substream (an extension): the sub-stream of
 * population 0; population p draws from substream + p.
 * noparam = 1, the parameter-free mode: bbo_iterate is one stage, runs = 2^(s/2) copies of size
 * (1 + s/2) nbase (s even) or one copy of size 2^(1 + s/2) nbase (s odd), each a complete inner run
 * whose budget is what the copies before it left, plus one evaluation of its result.  populations must
 * be 1.  concurrent = 1 runs the copies of a stage as the populations of one inner handle, copy r on
 * sub-stream (s << 16) + r, and charges the budget afterwards in the sequential order, replaying a
 * copy that ran beyond its cap alone; concurrent = 0 runs them one after another: the same results.
 * print = 1 writes the reference's table to stdout.  Keys of this mode: "stages" (rows of s, runs,
 * pop, f*, best f*, fev), "fbest", "xbest", "s", "budget", "fev", "nbase"; phase and inject are
 * BBO_ERR_STATE.
 * bbo_amalgam_configure is legal between bbo_create and bbo_init.  Limits: n in [1, 512], np in
 * [3, 65536]; objective programs, np < 3 and a non-finite box are refused by bbo_init (BBO_ERR_ARG).
 * bbo_amalgam_phase: 0 distribution (mean, covariance, factor), 1 sample + evaluate, 2 adapt + stop
 * (and the ranking of the new values); the three in order are bbo_iterate.
 * bbo_amalgam_inject_draws: the normals of the following G generations, zcount = G * populations * np
 * * n doubles as [G][populations][np][n] in sampling order (row m is the reference's sorted row m),
 * and the rows that take the anticipated mean shift, rcount = G * populations * nams ints as
 * [G][populations][nams], each in 1 .. np - 1.  Sampling beyond them is BBO_ERR_STATE; z = NULL returns
 * to the device generator.  bbo_amalgam_inject_points: the initial points of the next bbo_init,
 * populations * np * n doubles, before bbo_init.
 * "stop": 1 cmult < 1e-10 or the variance of the np stored values <= stol^2, 2 fev >= mfev; fev counts
 * np per generation as the reference does, though np - 1 points are evaluated.  "route": the slabs
 * of the Gram's K dimension and whether the factorisation ran in LDS.  "fact_fail": factorisations
 * that ended at a non-positive pivot, left unrepaired as in the reference; "fail_at": its step. */
typedef struct { int iamalgam, noparam, print, keep_elite, concurrent, substream; } bbo_amalgam_params;
void bbo_amalgam_params_default(bbo_amalgam_params *p);   /* 1, 1, 1, 0, 1, 0 */
int bbo_amalgam_configure(bbo_handle h, const bbo_amalgam_params *p);
int bbo_amalgam_phase(bbo_handle h, int phase);
int bbo_amalgam_inject_draws(bbo_handle h, const double *z, int zcount, const int *rows, int rcount);
int bbo_amalgam_inject_points(bbo_handle h, const double *x, int count);

/* ---- SLPSO (BBO_ALGO_SLPSO): SLPSO(mfev,stol,np,omegamin=0.4,omegamax=0.9,eta=1.496,gamma=0.01,vmax=0.2,
 * Ufmax=10.)  py/multivariate_py.cpp:292-299, the self-learning particle swarm of Li, Yang & Nguyen 2012
 * (slpso.cpp).  mfev, stol and np travel in bbo_params; the rest travels here.  The swarm starts uniform in
 * the box: a finite box is mandatory, `guess` is not read.  Limits: n in [1, 512], np in [2, 4096];
 * objective programs, np < 2 and a non-finite box are refused (BBO_ERR_ARG).
 * bbo_slpso_configure is legal between bbo_create and bbo_init.
 * One bbo_iterate is one iterate() of the reference: every particle in swarm order, each with its move,
 * its evaluation and, on an improvement, the coordinate walk of Algorithm 2 over abest; then updatePar.
 * The budget is tested between generations only, so fev may pass mfev by up to one generation.
 * bbo_slpso_phase walks the same generation one EVALUATION at a time: 0 advances every population to
 * its next pending point ("cand": a moved particle or an Algorithm 2 trial; "pending" is 0 once the
 * generation is complete and updatePar has run), 1 evaluates "cand" into "fcand", 2 absorbs the value.
 * bbo_slpso_inject_draws: `populations` tables of 1 + np + np * (3 + 4 n) doubles that replace the
 * generator from the next generation on: alpha, the permutation after its shuffle (np values), then per
 * particle step the forcing coin, the roulette uniform and the partner j as (j + 0.5) / np, and per
 * coordinate the uniform r, the normal of operator 1 (its value), the redraw of eq. 11 and the coin of
 * Algorithm 2.  Uniforms are raw canonicals in [0, 1); a draw the generation does not use is padding.
 * NULL returns to the device generator.  "record_draws" keeps the same table of the last generation
 * ("draws").  "dbg" 1 forces the sequential form of Algorithm 2 where the speculative one would run
 * ("speculative": which form runs; the two give the same bits).  "x" loads positions (re-evaluated;
 * pbest, abest in index order and the learning state follow, velocities are zeroed), "perm" the
 * permutation (Uf and Pl follow), "substream" (an extension) the sub-stream of population 0, from which
 * the swarm is drawn again; population p draws from substream + p.
 * "stop": 1 the spread of the particles' norms fell under stol, 2 fev >= mfev. */
typedef struct { double omegamin, omegamax, eta, gamma, vmax, Ufmax; } bbo_slpso_params;
void bbo_slpso_params_default(bbo_slpso_params *p);   /* 0.4, 0.9, 1.496, 0.01, 0.2, 10. */
int bbo_slpso_configure(bbo_handle h, const bbo_slpso_params *p);
int bbo_slpso_phase(bbo_handle h, int phase);
int bbo_slpso_inject_draws(bbo_handle h, const double *table, int count);

/* ---- CRS (BBO_ALGO_CRS): CRS(mfev,np,tol)  py/multivariate_py.cpp:339-342, the controlled random search
 * with local mutation of Kaelo & Ali 2006 (crs.cpp).  mfev, np and tol travel in bbo_params, all three
 * required; `max_depth` and `repair` (extensions) travel here.  The pool starts uniform in the box: a finite
 * box is mandatory, `guess` is not read.  Limits: n in [1, 512], np in [2, 65536]; objective programs and
 * a non-finite box are refused by bbo_init (BBO_ERR_ARG).  CRS is no base of a restart driver and is not
 * sharded over devices.  bbo_crs_configure is legal between bbo_create and bbo_init.
 * One bbo_iterate is one iterate() of the reference: trial(), whose recursion is walked as a state machine
 * over a stack of bits, then update(), which replaces the worst point.  The walk is the reference's, its
 * quirks included: a reflected point that left the box is redrawn and the point accepted in its place is
 * evaluated and counted a second time; after a rejected mutation the inner call's result is overwritten
 * with the mutation computed last, so the worst point may be replaced by one no better ("stale" counts
 * these iterations).  The budget is tested between iterations only, so fev may pass mfev.
 * repair = 1 is the loop of the paper instead: an out-of-box reflection and a rejected pair are redrawn,
 * only an accepted point replaces the worst, the budget is also tested where a pair is rejected.
 * The reference recurses until its stack overflows once every stored value is equal.  Here a push beyond
 * max_depth frames (repair: max_depth out-of-box redraws in a row) ends the run with "flag" 3: the pool is
 * as the last complete iteration left it, fev keeps what was spent.
 * bbo_run advances `poll_every` iterations per population and chunk (0: 256) in launches that end, for a
 * population, after "launch_evals" steps (drawn trials and evaluations; 0, the default: 8 per iteration of
 * the chunk); a population cut there resumes in the next launch with the same bits.
 * bbo_crs_phase walks the iteration one EVALUATION at a time: 0 advances every population to its next
 * pending point ("pending"; "stage" 1: "cand", 2: "cand2"), 1 evaluates it into "value", 2 absorbs the
 * value and advances again; "pending" is 0 once the iteration is complete.
 * bbo_crs_inject_draws: populations * records * 2 n doubles that replace the generator: a record holds
 * the n row indices of a trial (n - 1 for the centroid, then the reflected point; -1 where none is drawn)
 * and n uniforms in [0, 1) for a mutation.  A trial takes the next record; a mutation takes the uniforms
 * of the current record, or of the next one when they are spent or the table is new.  When the table runs
 * out inside an iteration the call returns with "starved" 1 and the next table continues it (bbo_run
 * returns BBO_ERR_STATE instead).  NULL returns to the device generator.  "record_draws" (1: 64 records,
 * or their number) keeps the records of the last iteration in the same layout ("draws", "nrec").
 * Keys: "x" / "f" the pool in RANK order (set: rows in place, re-evaluated / re-ranked, the walk starts
 * over), "order" rank -> row, "rows" the pool in place, "cand" "fcand" "cand2" "fcand2" the trial, the
 * mutation and their values, "fbest" "fworst" "fev" "it" "trials" "muts" "depth" "maxdepth" "stage"
 * "pending" "stale" "flag" "conv", "max_depth" (settable up to the configured depth), "launch_evals".
 * "flag": 1 |f_best - f_worst| < tol after an iteration, 2 fev >= mfev, 3 max_depth.  A NaN value counts
 * as +inf. */
typedef struct { int max_depth; int repair; } bbo_crs_params;
void bbo_crs_params_default(bbo_crs_params *p);   /* 4096, 0 */
int bbo_crs_configure(bbo_handle h, const bbo_crs_params *p);
int bbo_crs_phase(bbo_handle h, int phase);
int bbo_crs_inject_draws(bbo_handle h, const double *table, int count);

/* ---- SSDE (BBO_ALGO_SSDE): SSDE(mfev,npinit,tol,patience=1000,npmin=4,ptop=0.11,h=100,usede=false,
 * repaircr=true)  py/multivariate_py.cpp, the spherical search of Kumar et al. 2019 with the DE fallback
 * of Zhao et al. 2022 (ssde.cpp).  mfev, np (= npinit) and tol travel in bbo_params; the rest travels here
 * (the defaults are the Python binding's: usede = 0).  The pool starts uniform in the box, with usede
 * joined by its opposites lower + upper - x, the best npinit of which stay (fev = 2 npinit): a finite box
 * is mandatory, `guess` is not read.  bbo_init refuses (BBO_ERR_ARG) a box that is not finite, n outside
 * [1, 512], npinit outside [4, 4096], npmin < 4 or > npinit, h < 1 or > 65536, ptop outside (0, 1),
 * patience < 0, usede / repaircr other than 0 or 1, and an objective program.  ptop = 1 is refused because
 * the reference draws pbest from [0, int(ptop np)] inclusive and would read past the pool.
 * bbo_ssde_configure is legal between bbo_create and bbo_init.  SSDE is no base of a restart driver and
 * is not sharded over devices.
 * One bbo_iterate is one iterate() of the reference: the members in rank order, each reading the rows the
 * members before it have replaced, R = fev / mfev read at every member, the spherical trial and, with
 * usede, on its failure the DE trial; then the memory update (L1, L2, LCR), the sort (stable on ties),
 * convcount and the linear shrink of np, which here never falls under 4.  The budget is tested between
 * generations only, so fev may pass mfev by up to one generation.  The pool stays in place: "order" maps
 * a rank to its row, "x" and "f" are in rank order.
 * bbo_ssde_phase walks the same generation one EVALUATION at a time: 0 advances every population to its
 * next pending point ("cand": the spherical or the DE trial; "pending" is 0 once the generation is
 * complete), 1 evaluates "cand" into "fcand", 2 absorbs the value.
 * bbo_ssde_inject_draws: `populations` tables of n + npinit * (9 + 3 n) doubles that replace the generator
 * from the next generation on: the permutation whose consecutive pairs are the rotated planes (n values),
 * then per member i the OUTCOMES of its draws: iL, the normal of prank, p, q, r, pbest, the accepted ci
 * (in (0, 1]), the normal of CRi, j0, then n uniforms of the binary vector, n of the crossover and n of
 * the redraw inside the box.  Uniforms are raw canonicals in [0, 1); a draw the generation does not make
 * is padding.  NULL returns to the device generator, which is Philox keyed by (generation, member,
 * purpose, coordinate, attempt).  Its rejection loops are bounded: after 64 attempts sample3 takes the
 * next free index cyclically and ci becomes min(1, L2[iL]).  "record_draws" keeps the same table of the
 * last generation ("draws").
 * Keys: "x" "f" "order" "L1" "L2" "LCR" (h values each) "k" "kCR" "np" "fev" "gen" "convcount" "perm"
 * "cand" "fcand" "pending" "stage" "member" "stop" "conv" "npinit" "n".  Writable: "x" (m rows, 4 <= m <=
 * npinit: np becomes m; re-evaluated and re-sorted), "L1" "L2" "LCR" "k" "kCR" "fev" "convcount", "perm"
 * (the next generation keeps it instead of drawing one), "cand" "fcand", "substream" (an extension: the
 * sub-stream of population 0, from which the pool is drawn again; population p draws from substream + p).
 * "stop": 1 converged() (the spread of the members' norms under tol, or convcount > patience), 2 fev >=
 * mfev.  A NaN value counts as +inf. */
typedef struct { int patience, npmin; double ptop; int h, usede, repaircr; } bbo_ssde_params;
void bbo_ssde_params_default(bbo_ssde_params *p);   /* 1000, 4, 0.11, 100, 0, 1 */
int bbo_ssde_configure(bbo_handle h, const bbo_ssde_params *p);
int bbo_ssde_phase(bbo_handle h, int phase);
int bbo_ssde_inject_draws(bbo_handle h, const double *table, int count);

/* ---- ACD (BBO_ALGO_ACD): ACD(mfev,ftol,xtol,ksucc=2.,kunsucc=0.5)  py/multivariate_py.cpp:44-48, the
 * adaptive coordinate descent of Loshchilov, Schoenauer & Sebag 2011 (acd.cpp): a coordinate search along
 * the columns of B, an archive of 2 n points, and after every sweep that improved a rank-one covariance
 * update with a symmetric eigendecomposition (adaptive encoding).  mfev travels in bbo_params, ftol in `tol`
 * and xtol in `stol` (bbo_params_default writes the long struct for this algorithm); the rest travels here.
 * x_best starts uniform in the box: a finite box is mandatory; `guess` is read only with from_guess = 1
 * (an extension: population p starts at its row of `guess`).  Limits: n in [1, 128], any `populations`;
 * bbo_init refuses (BBO_ERR_ARG) a box that is not finite, n outside the limits and an objective program;
 * speculate = 1 (the speculative sweep) was built, measured slower at 4096 populations and dropped: it is
 * refused by bbo_acd_configure.
 * bbo_acd_configure is legal between bbo_create and bbo_init.  ACD is no base of a restart driver and is not
 * sharded over devices.
 * One bbo_iterate is one iterate() of the reference: ONE coordinate step (two evaluations, x1 then x2), with
 * the archive ranking, updateAE() and the decomposition behind the last step of a sweep that improved.
 * bbo_run counts coordinate steps; it advances `poll_every` of them per population and poll (0: n, one
 * sweep).  The budget is tested between steps, so fev may pass mfev by 1.
 * bbo_acd_phase walks a step with a host objective's granularity: 0 forms x1 and x2 ("cand", 2 n values;
 * "pending" 1), 1 evaluates them into "value" (2 values), 2 absorbs the values, does the step's bookkeeping
 * and, where due, the update.
 * The archive is ranked stably with respect to the persisting `order` (the reference's std::sort is stable
 * only while 2 n <= 16).  From the second update on C has a degenerate eigenspace whose basis rounding
 * decides, so B is the reference's only up to that choice.
 * Keys: "xbest" "fbest" "sigma" "B" "invB" "C" (n x n, row-major) "p" "m" "mold" "diagd" "colmax", "x" / "f"
 * the archive in place (2 n rows), "order", "ix" "it" "itae" "improved" "fev", "fhist" (the ring, cp values),
 * "cp", "cand" "value" "pending", "flag" (1 converged, 2 fev >= mfev), "rule" (1 ftol, 2 xtol), "conv",
 * "due".  Writable: "xbest" "fbest" "sigma" "B" (recomputes "colmax") "invB" "C" "p" "m" "mold"
 * "diagd" "x" "f" "order" "fhist" "value" "ix" "it" "itae" "improved" "fev", and "substream" (write-only, an
 * extension: x_best of the population is drawn again from that sub-stream); every other key is read-only.
 * The device's history rule takes the newest entry of the ring from "fbest", which is what the last step
 * wrote there: after a set of "fbest", "it" or "fhist" without a step, "conv" and bbo_solution (which read
 * the ring) may say otherwise until the next step.  A NaN value counts as +inf. */
typedef struct { double ksucc, kunsucc; int from_guess; int speculate; } bbo_acd_params;
void bbo_acd_params_default(bbo_acd_params *p);   /* 2., 0.5, 0, 0 */
int bbo_acd_configure(bbo_handle h, const bbo_acd_params *p);
int bbo_acd_phase(bbo_handle h, int phase);

/* ---- Mayfly (BBO_ALGO_MAYFLY): Mayfly(np,mfev,a1=1.,a2=1.5,a3=1.5,beta=2.,dance=5.,ddamp=0.8,fl=1.,
 * fldamp=0.99,gmin=0.8,gmax=0.8,vdamp=0.1,sigma=0.1,pmutdim=0.01,pmutnp=0.05,l=0.95,pgb=false), the mayfly
 * optimizer of Zervoudakis & Tsafarakis 2020 with the PGB-IMA switch (mayfly.cpp; the reference writes the
 * binding out at py/multivariate_py.cpp:236-246 but leaves it commented away).  np and mfev travel in
 * bbo_params, the rest here.  Both swarms start uniform in the box (fev = 2 np): a finite box is mandatory,
 * `guess` is not read.  Limits: n in [1, 512], np even in [2, 4096], mfev > 2 np.  bbo_create refuses an odd
 * np (the reference leaves the last offspring of an odd swarm unwritten: a zero vector of value 0 that wins
 * the selection), np < 2 and mfev <= 2 np (itmax <= 0: g = 0/0); bbo_init refuses a box that is not finite, n
 * outside the limits and an objective program (BBO_ERR_ARG).  No restart base, not sharded over devices.
 * bbo_mayfly_configure is legal between bbo_create and bbo_init.
 * One bbo_iterate is one iterate() of the reference: the females (each against the male of its slot), the
 * males (male j + 1 reads the best that male j wrote: run as rounds of "window" males that are committed up
 * to the first that improves fbest, the rest formed again with the same draws), both swarms sorted (stable
 * on ties), np offspring, nmut mutated flies, the two selections and the schedule.  The reference's selection
 * copies into the swarm in place while its sorted list still points at slots already overwritten, which
 * leaves about half of each swarm an exact duplicate; that is reproduced (repair = 0) by resolving for every
 * slot the record that lands in it.  repair = 1 (an extension) selects from untouched copies, as the paper
 * does, and starts every fly at the point it drew with no velocity (the reference builds its flies with x and v
 * exchanged: every fly starts at the origin, the drawn point is its velocity and, for a male, its own best).
 * substream (an extension): population p draws from Philox sub-stream substream + p, so a batch can be
 * checked against single runs.  The budget is tested between generations, so fev passes mfev by less than one generation (3 np +
 * nmut evaluations); there is no convergence test ("flag" 2 = budget).
 * bbo_mayfly_inject_draws: populations * table_len doubles that replace the generator in every following
 * generation ("table_len" = 2 np n + np + nmut + 2 nmut nmd, nmd = ceil(pmutdim n)): the canonical uniforms
 * in [0, 1) of the females' random flights [np][n] and of the males' dances [np][n] (-1 where the fly takes
 * the attraction form), the shuffle of the offspring and of the mutated flies as permutations (shuffled
 * place -> index), and per mutated fly its nmd displaced genes and their nmd normals.  NULL returns to the
 * device generator (Philox keyed by generation, swarm, individual and coordinate).  "record_draws" keeps
 * the same table of the last generation ("draws").
 * Keys: "males_x" "males_v" "males_bx" "males_f" "males_bf" "females_x" "females_v" "females_f" (slot
 * order), "xbest" "fbest" "g" "dance" "fl" "it" "itmax" "fev" (all writable: a whole state can be set, nothing
 * is evaluated), "nmut" "nmd" "flag" "conv"; of the last generation: "moved_males_x" "moved_males_v"
 * "moved_males_f" "moved_females_x" "moved_females_v" "moved_females_f" (the swarms after their moves, before
 * the selection), "off_x" "off_f" "mut_x" "mut_f", "rank_m" "rank_f" (rank -> slot), "sel_m" "sel_f" (rank ->
 * record of the selection: t < np the swarm's fly of rank t, then np / 2 shuffled offspring, then nmut / 2
 * shuffled mutated flies), "src_m" "src_f" (the record that landed in each slot), "branch_m" "branch_f"
 * (1: attraction, 0: the random form), "perm_o" "perm_u", "took" (the evaluation that took fbest last:
 * females from 0, males from np, offspring from 2 np, mutated flies from 3 np; -1 none), "dropped" "rounds"
 * (male evaluations discarded and rounds run so far).  "window" (writable): the males of a round, 0 = all
 * remaining, default 4; the state does not depend on it.  A NaN value counts as +inf. */
typedef struct {
    double a1, a2, a3, beta, dance, ddamp, fl, fldamp, gmin, gmax, vdamp, sigma, pmutdim, pmutnp, l;
    int pgb, repair, substream;
} bbo_mayfly_params;
void bbo_mayfly_params_default(bbo_mayfly_params *p);   /* 1, 1.5, 1.5, 2, 5, 0.8, 1, 0.99, 0.8, 0.8, 0.1, 0.1, 0.01, 0.05, 0.95, 0, 0, 0 */
int bbo_mayfly_configure(bbo_handle h, const bbo_mayfly_params *p);
int bbo_mayfly_inject_draws(bbo_handle h, const double *table, int count);

/* ---- PIKAIA (BBO_ALGO_PIKAIA): PIKAIA(np,ngen,nd,pcross=0.85,imut=2,pmut=0.005,pmutmn=0.0005,pmutmx=0.25,
 * fdif=1.,irep=1,ielite=0), the genetic algorithm of Charbonneau & Knapp (pikaia.cpp, a translation of the HAO
 * Fortran 77 code; the reference binds it to no Python class, the constructor at pikaia.h:25-27 is the
 * signature).  In bbo_params travel np, ngen (as `mfev`: this engine's budget is generations) and nd (as `h`),
 * the rest here.  Limits: n in [1, 512], np even in [2, 4096], nd in [1, 9], ngen >= 1 with np + ngen (np + 1)
 * <= INT_MAX.  bbo_create refuses an odd np (the reference leaves the last row of the new population a zero
 * vector), nd > 9 (int(ph 10^nd) overflows); bbo_pikaia_configure, legal between bbo_create and bbo_init,
 * refuses irep = 2, 3 (the steady-state plans are a sequential walk with the evaluations inside it: not
 * built), imut outside [1, 6], ielite outside {0, 1}, a probability outside [0, 1], pmutmn > pmutmx and fdif
 * outside [0, 1]; bbo_init refuses a box that is not finite unless raw (BBO_ERR_ARG each, with the reason).
 * The GA's state is the phenotype u in [0, 1)^n.  raw = 0 (the default): the objective is handed
 * x = lower + u (upper - lower), one multiply and one add, and the fitness the GA maximises is -f(x): the
 * reference run on that wrapped function.  raw = 1 is the literal reference: the objective sees u, the box is
 * not read, the fitness is +f.  `guess` is not read.  Reproduced with repair = 0: init stores the value of the
 * last row only, in the last slot, so the first generation selects on np - 1 tied zeros; a generation counts
 * np + 1 evaluations; the relative fitness difference of imut 2 / 5 has a signed denominator, so on a
 * non-negative objective (fitness <= 0) pmut only ever rises to pmutmx.  repair = 1 stores every initial value,
 * counts np per generation, keeps the stored value of the elite row and divides by |f_best + f_median|.
 * Ranking is the library's stable order (fitness ascending, ties by row), not the reference's quicksort: where
 * values tie (after init, repair = 0) runs agree with the reference as distributions, not draw for draw.
 * select's running sums are formed left to right once per generation and looked up by bisection; if rounding
 * leaves the last sum under the dice the device takes the last row (np counting from 1 as the reference does,
 * np - 1 in the 0-based keys; the reference would keep the index of the previous call).  The second parent is drawn at most 64 times and is then the next row cyclically.
 * One bbo_iterate is one iterate() of the reference; the only stop is ig > ngen ("flag" 1, converged, as the
 * reference reports).  bbo_solution returns the mapped best row of the population as it stands.  A host
 * objective is called in the reference's order: new row 1 first when ielite = 1, then rows 1 .. np (np + ielite
 * calls per generation; np under repair).  A NaN value ranks worst.  Objective programs are taken; a program's NaN is stored as +inf
 * ("new_f"), so under raw = 1 a +inf from a program ranks worst as well.
 * substream (an extension): population p draws from Philox sub-stream substream + p.
 * bbo_pikaia_inject_draws: populations * table_len doubles that replace the generator in every following
 * generation.  Per mating ("table_len" = (np / 2) (69 + 2 (1 + 2 n nd))): [0] the uniform of the first parent,
 * [1, 65) those of the second, one per attempt, [65, 69) the crossover's coin, ispl, the coin one- / two-point,
 * ispl2, then per child the coin creep / uniform, n nd locus uniforms and n nd value uniforms (the new digit
 * int(10 u) or the creep step round(u) 2 - 1); -1 wherever the reference draws nothing.  The doubles are
 * compared as the reference compares them.  A table is refused (BBO_ERR_ARG) unless every slot the next
 * generation reads holds a draw: both parents' first slots, the crossover's coin and what it calls for, the
 * coin of every child for imut >= 4, every locus uniform, and the value of every locus whose uniform is below
 * pmut as it stands at the call.  NULL returns to the device generator (Philox keyed by generation,
 * mating, child, purpose and locus; one 32-bit word per locus test).  "record_draws" keeps the same table of
 * the last generation ("draws").
 * Keys: "ph" (phenotypes, row order; writing them writes "x" too) "fitns" "order" (rank -> row, ascending;
 * writable as a permutation, the ranks and the running sums follow) "pmut" "ig" "fev" "fbest" "xbest" (best
 * ever, the objective's scale) -- all writable, nothing is evaluated -- "x" "rank" "cum" "flag" "conv" "rdif"
 * "table_len" "z" "zinv"; of the last generation "parents" (np / 2 x 2 rows) "cross" (np / 2 x 2: ispl, ispl2,
 * 1-based, or -1) "mode" (per child: 1 creep, 0 uniform) "new_ph" "new_x" "new_f" (objective values) "elite". */
typedef struct {
    double pcross, pmut, pmutmn, pmutmx, fdif;
    int imut, irep, ielite;
    int repair, raw, substream;
} bbo_pikaia_params;
void bbo_pikaia_params_default(bbo_pikaia_params *p);   /* 0.85, 0.005, 0.0005, 0.25, 1., 2, 1, 0, 0, 0, 0 */
int bbo_pikaia_configure(bbo_handle h, const bbo_pikaia_params *p);
int bbo_pikaia_inject_draws(bbo_handle h, const double *table, int count);

/* ---- NelderMead (BBO_ALGO_NELDER_MEAD): NelderMead(mfev,tol,rad0,minit=spendley,pinit=mehta2019_refined,
 * checkev=10,eps=1e-3)  py/multivariate_py.cpp:307-337, the simplex search of Nelder & Mead as O'Neill's
 * AS 47 with restarts, the adaptive coefficients of Gao & Han 2012 and Mehta 2020 and four initial simplexes
 * (nelder_mead.cpp).  mfev and tol travel in bbo_params, rad0 in `sigma0`, the rest here.  One workgroup per
 * population, a lane per coordinate; a multi-start is `populations` rows of `guess`.  Limits: n in [1, 128],
 * checkev >= 1, rad0 and eps finite; minit = random (3) draws the simplex from [lower, upper] and needs a
 * finite box, nothing else reads the bounds.  bbo_init refuses an objective program (BBO_ERR_ARG each).
 * bbo_nm_configure is legal between bbo_create and bbo_init.  No restart base, not sharded over devices.
 * Departure from the reference, whose step protocol is broken (its init() builds no simplex, so iterate()
 * after it walks zeros, and solution() returns the scratch vector of the shrink): bbo_init builds and
 * evaluates the first simplex as nelmin()'s first pass does (fev = n + 1), one bbo_iterate is one iterate()
 * of the reference from there (the shrink's n + 1 evaluations included, no stop flag, no factorial test) and
 * bbo_solution gives row ilo, fev and the conv of the last step.  bbo_run counts simplex steps and is
 * nelmin(): the steps while fev < mfev and not converged, then the factorial test (2 n probes at xmin[i] +-
 * step[i] eps, counted up to and including the first below ynl, the coordinates restored by += del, -= 2 del,
 * += del as the reference does), then the restart from the probe that improved or "flag" 1; "flag" 2 where
 * mfev < fev.  bbo_optimize is bbo_init + that, whole, and returns "xmin" as nelmin() leaves it.
 * Reproduced: the centroid is summed over all n + 1 rows in row order, less row ihi, divided by n, every step;
 * ihi is the first maximum, ilo the first minimum; the outside contraction that is refused stores pstar with
 * the value y2star (nelder_mead.cpp:195-197; repair = 1 stores ystar); the shrink runs in place row after
 * row, so row ilo itself moves unless scoef = 0.5 and the rows behind it read the moved one; a shrink
 * returns before the stop test's bookkeeping; the stop test compares the undivided sum of squares with
 * tol^2 n every checkev steps while fev <= mfev.  speculate = 1 (pstar and the three possible second
 * points of a step evaluated at once on four wavefronts) was built, bit-identical, measured slower at 1, 256 and
 * 4096 populations alike and dropped: bbo_nm_configure refuses it.  lds = 1 keeps the simplex in LDS over a launch,
 * 0 in HBM; -1 (the default) takes HBM where the simplex leaves one workgroup per CU in LDS and there are at least
 * four populations per CU, as measured; the state does not depend on it.  substream: population p draws minit = random from sub-stream substream + p.
 * bbo_nm_phase walks with a host objective's granularity: 0 advance to the next pending batch ("pending"
 * points: 1, or n + 1 rows of the simplex, or 2 n probes), 1 evaluate it, 2 absorb the values and advance.
 * A host objective sees exactly the reference's points in its order, the factorial probes up to the first
 * that improved.  A NaN value counts as +inf.
 * Keys: "p" ((n + 1) x n) "y" "ilo" "ihi" (0-based) "ylo" "ynl" "jcount" "fev" "del" "start" "xmin" "step"
 * "conv" "flag" "pending" "stage" "coef" (ccoef, ecoef, rcoef, scoef) "branch" (the last step: 1 expansion
 * kept, 2 expansion refused, 3 reflection, 4 inside contraction, 5 shrink, 6 outside contraction, 7 outside
 * contraction refused) "restarts" "it" "cand" "value" "lds".  Writable: "p" "y" "ilo" "ylo" "jcount" "fev"
 * "start" "del" "value" "lds"; nothing is evaluated. */
typedef struct { int minit, pinit, checkev; double eps; int repair, speculate, lds, substream; } bbo_nm_params;
void bbo_nm_params_default(bbo_nm_params *p);   /* 1, 3, 10, 1e-3, 0, 0, -1, 0 */
int bbo_nm_configure(bbo_handle h, const bbo_nm_params *p);
int bbo_nm_phase(bbo_handle h, int phase);

/* ---- Rosenbrock (BBO_ALGO_ROSENBROCK): Rosenbrock(mfev,tol,step0,decf=0.1)  rosenbrock.h:55, Rosenbrock's
 * rotating-axes search with the line search of Davies, Swann and Campey (doubling, then a Lagrange quadratic
 * through three of four points) and Palmer's orthogonalisation (rosenbrock.cpp; the reference binds it to no
 * Python class).  mfev and tol travel in bbo_params, step0 in `sigma0`, decf here.  No random draw.  One workgroup
 * per population; a multi-start is `populations` rows of `guess`.  Limits: n in [1, 128], step0 and decf finite and not 0, tol >= 0 (with a step of 0 the doubling loop
 * of a search would end on the budget alone, inside one launch);
 * the bounds are stored and never read.  bbo_init refuses an objective program (BBO_ERR_ARG each) and evaluates
 * nothing.  bbo_rosen_configure is legal between bbo_create and bbo_init.  No restart base, not sharded.
 * One bbo_iterate is one iterate() of the reference: a line search from x[i - 1] along v[i] into x[i], d[i] = the
 * step taken, then i++, or the extra search along the stage's displacement, or the step test with the
 * orthogonalisation or the shrink of the step.  bbo_run counts line searches.  bbo_optimize is init() + iterate()
 * until _ierr >= 0 and returns _x1, WHICH ONLY A CONVERGED RUN WRITES: ON A BUDGET EXIT THE RESULT IS THE ZERO
 * VECTOR, as in the reference (rosenbrock.cpp:197 is the only write).  repair = 1 returns the end point of the last
 * completed line search, x[i - 1], where the run has not converged, and changes nothing else.  The budget is
 * tested inside the doubling loop and behind a stage only, so n_evals passes mfev by a few evaluations.
 * wide = 1 evaluates the points of a batch at once, a wavefront each (256 threads); 0 in turn on one wavefront;
 * -1 (the default) takes 1 except at n <= 64 with at least four populations per CU, as measured (DESIGN.md
 * section 3.20); the state does not depend on it.  substream is reserved (the method draws nothing).
 * bbo_rosen_phase walks with a host objective's granularity: 0 advance to the next pending batch ("pending"
 * points: 2 first, then 1 back, 1 per doubling, 4 for the interpolation, 1 final), 1 evaluate it, 2 absorb the
 * values and advance.  A host objective sees exactly the reference's points in its order, the second call at x0
 * included.  Departure: a NaN value counts as +inf.
 * Keys: "x" ((n + 2) x n) "v" ((n + 2) x n) "d" (n + 2) "stepi" "i" "fev" "x1" "flag" (1 converged, 2 budget)
 * "path" (the last search: direction 1 forward / 2 backward / 3 straight to the interpolation, rounds of the
 * doubling loop, imin or -1, end 0 none / 1 kept / 2 restored / 3 budget) "fs" "pending" "value" "cand" (the pending
 * batch; behind a search with a built-in the four interpolation points, whose values are "fs") "stage"
 * "it" "orth" "orths" "walk_ticks" "orth_ticks" (ticks of the constant-rate clock inside rosen_walk, and inside its
 * orthogonalisations) "s" "fx0" "fx" (lineSearch()'s, the last values) "wide".  Writable: "x" "v" "d" "stepi" "i" "fev" "value" "wide"; nothing is evaluated. */
typedef struct { double decf; int repair, wide, substream; } bbo_rosen_params;
void bbo_rosen_params_default(bbo_rosen_params *p);   /* 0.1, 0, -1, 0 */
int bbo_rosen_configure(bbo_handle h, const bbo_rosen_params *p);
int bbo_rosen_phase(bbo_handle h, int phase);

/* ---- BasinHopping (BBO_ALGO_BASIN_HOPPING): BasinHopping(minimizer,stepstrat,print=True,mit=99,temp=1.) with
 * BasinHopping_StepStrategy(stepsize) / BasinHopping_AdaptStrategy(stepsize=1.,accept_rate=0.5,interval=5,factor=0.9)
 * py/multivariate_py.cpp:83-97, basinhopping.cpp.  Metropolis chains whose every hop is a whole local minimisation:
 * a step of stepsize U[-1,1) (upper - lower) per coordinate clamped to the box less 5 % on each side, the minimiser
 * from there, one extra evaluation of what it returned, exp(min(0, -(new - old) / temp)) >= U[0,1).
 * bbo_create_basin borrows `minimizer`, a BBO_ALGO_NELDER_MEAD or BBO_ALGO_ROSENBROCK handle of this library with the
 * same populations and device; it stays owned by the caller, must outlive the handle and is driven by it (its
 * state is the last minimisation's).  One chain per population, re-armed on the device between hops (DESIGN.md
 * section 3.21).  BBO_ERR_ARG: another handle, mismatched populations / device, NelderMead with minit = random (it
 * addresses its draws by the restart count alone and would draw the same simplex on every hop); at bbo_bh_configure
 * interval < 1, factor not finite and positive, temp < 0, mit < 0; at bbo_init a box that is not finite, n > 128,
 * an objective program.  A NaN energy counts as +inf.  params: seed, device, populations, poll_every (rounds of walk
 * chunk + hop between polls of the finished chains; 0: 8).
 * bbo_init is init(): the first minimisation from the guess and log row -1.  bbo_iterate is one hop of every chain
 * that has hops left, bbo_run(g) up to g, bbo_optimize init and hops to mit; converged is always 0, n_evals the sum of
 * the minimisations' counts + 1 each.  With a built-in objective the chains hop asynchronously (lockstep = 1: a hop
 * only when every minimisation has stopped; same results; -1, the default, takes 1 at n > 64 with at least 256
 * chains, as measured); with a callable the minimiser's host loop runs to every
 * population's stop, then one host batch values the energy points.  Every draw is addressed by (seed, substream +
 * population, hop, coordinate or the accept slot): a chain does not depend on scheduling or on `populations`.
 * nstep0 / naccept0: the history of an adaptive strategy that has been used before (the reference's init() resets
 * none of it).  print: the reference's table for population 0, rows as the polls discover them.
 * bbo_bh_phase: 0 every idle chain with hops left takes its step and re-arms its minimiser, 1 collect the stopped
 * minimisations' results, 2 evaluate the pending energy points, 3 decide.
 * bbo_bh_inject_draws (after bbo_init): per hop n step uniforms in [-1, 1) and one accept uniform in [0, 1), consumed
 * by every chain instead of Philox while the table covers the hop; NULL ends it.  bbo_bh_draws: the same n + 1
 * uniforms of (seed, substream, hop) computed on the host; needs no handle and no device.
 * State: "x" "energy" "xbest" "fbest" "stepsize" "nstep" "naccept" "it" "fev" "flag" (0 running, 2 mit reached)
 * "log" ((it + 1) x 7: it, f, conv, step, accept, f*, fev) "log_start" "log_sol" ((it + 1) x n: the start handed to
 * the minimiser and what it returned) "log_fev" "xtrial" "xsol" "stage" "pending" "lockstep" "n" "profile".
 * Writable between hops: "x" "energy" "stepsize" "nstep" "naccept"; "profile".  A minimiser that is initialised again on its own
 * after bbo_init (another problem, a run of its own) leaves the handle stale: every call returns BBO_ERR_STATE until
 * the next bbo_init.  "xtrial" "xsol" "stage" "pending" are what a caller of bbo_bh_phase reads between its steps. */
typedef struct {
    double stepsize; int adaptive; double accept_rate; int interval; double factor, temp;
    int mit, print, lockstep, substream, nstep0, naccept0;
} bbo_bh_params;
void bbo_bh_params_default(bbo_bh_params *p);   /* 1., 1, 0.5, 5, 0.9, 1., 99, 1, -1, 0, 0, 0 */
int bbo_create_basin(const bbo_params *params, bbo_handle minimizer, bbo_handle *out);
int bbo_bh_configure(bbo_handle h, const bbo_bh_params *p);
int bbo_bh_phase(bbo_handle h, int phase);
int bbo_bh_inject_draws(bbo_handle h, const double *table, int count);
int bbo_bh_draws(uint64_t seed, int substream, int hop, int n, double *out);

/* ---- diagnostics -------------------------------------------------------------------------------
 * bbo_probe_objective: built-in `objective` at `rows` points of `n` coordinates (X, rows x n, host
 * memory) through ONE of the device forms the kernels evaluate it in; f_out takes the rows values as
 * the form returns them (no NaN guard).  For tests of the forms at points no optimizer draws.
 *   form 0  eval_row_group<16>, the row in LDS              1  eval_row_group<64>, the row in global
 *        2  eval_row_group<64>, the LDS row swizzled           memory with ld = n rounded up to even
 *        3  eval_row_group<16> unrolled by 4 (CCPSO)        4  eval_frag_rows<8>, MFMA accumulator layout
 * Whatever lies behind a row's n coordinates holds 1e300, in every form.  n in [1, 1024], rows in [1, 65536]; form 4 takes n <= 128 and the
 * objectives without transcendental terms (sphere, rosenbrock, ellipsoid, cigar, discus, schwefel12).
 * BBO_ERR_ARG otherwise, with the reason in bbo_last_error(NULL). */
int bbo_probe_objective(int objective, int form, int n, int rows, const double *X, double *f_out);

const char *bbo_last_error(bbo_handle h);   /* h may be NULL: last creation error */
const char *bbo_version(void);
int bbo_device_count(void);

#ifdef __cplusplus
}
#endif

#endif /* BBOPT_HIP_H_ */
