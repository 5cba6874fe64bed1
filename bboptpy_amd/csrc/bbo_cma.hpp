// bbo_cma.hpp -- device-resident CMA-ES engine: plain, active, separable, Cholesky (declarations).
//
// One generation of the reference (BaseCmaes::iterate, base_cmaes.cpp:150-156:
// samplePopulation -> evaluateAndSortPopulation -> updateDistribution ->
// updateHistory) is a fixed sequence of kernels over state that never leaves HBM.
// See DESIGN.md for the kernel table and the data layout.
#pragma once

#include "bbo_engine.hpp"

namespace bbo {

// per-population scalars, updated by the kernels only
struct CmaScal {
    double sigma;
    double fbest, fworst;     // running best/worst over the history ring (base_cmaes.cpp:201-208)
    double pslen;             // ||ps|| of the last update (diagnostic)
    double ybw[4];            // best, 2nd best, 2nd worst, worst fitness (base_cmaes.cpp:226-229)
    int ibw[4];
    int it, fev;
    int flag;                 // reference stop flag 1..9 (cmaes.cpp:151-227), 0 = none
    int stop;                 // sticky: 1 = stop rule fired, 2 = evaluation budget exhausted
    int hsig;
    int eigenlastev, eigen_done;
    int hist_head, hist_len;
    int basis_ok;             // C^-1/2 = B D^-1 B^T for the (B, D) the sampler uses (see cma_whiten128)
    int eig_stage;            // 128 < n <= 256, split decomposition: 1 = tridiagonal form handed to the next kernels
    int eig_mw_fail;          // sticky: a wavefront of cma_tred_mw gave up waiting for its partners (bbo_eig_mw.hpp)
};

// strategy constants, passed to every kernel by value
struct CmaConst {
    int n, ld;                // dimension, padded leading dimension (multiple of 16)
    int lambda, lambda_pad;   // population size, padded to a multiple of 16
    int mu, mu_pad;
    int variant;              // 0 plain (cmaes.cpp), 1 active (active_cmaes.cpp), 2 separable (sep_cmaes.cpp),
                              // 3 Cholesky (cholesky_cmaes.cpp)
    int bound, obj;
    int use_zn;               // this generation's zn2 is valid and x was not clamped
    int lazy_isc;             // C^-1/2 is not formed after a decomposition (16 < ld <= 256, no box): cma_paths
                              // works from B and D, the whitening takes ||z||^2, readers get it on demand
    int mfev, mit, hlen, ik;
    int honor_stop;           // 1 inside run()/optimize(): stopped populations are frozen
    int splits, rps;          // Gram split-K: number of row slabs, rows per slab
    int npop;
    double mueff, cc, cs, c1, cmu, cneg, alphaold, cm, damps, chi, sigma0, tol, eigenfreq;
    double ccov;              // separable variant (sep_cmaes.cpp:53-62)
    uint64_t seed;
    // extensions, off by default (bbo_set "stop_off" / "ftarget"): bit k of stop_off silences the
    // reference's stop test with flag k; f_best <= ftarget raises the non-reference flag 10
    int stop_off;
    double ftarget;
    // CholeskyCMAES: the radius-spread tolerance of its stop rule; ranked != 0 (extension): the
    // rank-mu term takes the mu best about the old mean instead of the first mu about the new one
    double stol;
    int ranked;
};

// Diagnostic switches: the bits of CmaDev::dbg (bbo_set "dbg", 0 in production).  Each selects an older
// or alternative form of a kernel for A/B tests and timing.  This list is the documentation; the VALUES
// are frozen (tests and scripts pass them as numbers).
enum CmaDbg : int {
    DBG_QL_NO_APPLY      = 1,          // QL stage: the rotations are not applied to the vectors (timing: B is wrong)
    DBG_QL               = 2,          // tridiagonal stage by the reference's implicit QL, not divide and conquer
    DBG_DC_NO_MERGES     = 4,          // divide and conquer: leaves only, no merge level (timing: B is wrong)
    DBG_DC_NO_LEAVES     = 8,          // divide and conquer: the QL leaves are skipped (timing: B is wrong)
    DBG_NO_EIGEN_SMALL   = 16,         // n <= 16: cma_eigen_128 + cma_post, not cma_eigen_small; no fused generations
    DBG_COV_UNFUSED      = 32,         // n = 128 batch: cma_cov, then cma_eigen_fx128u, where cma_eigen_fx128 forms C
    DBG_NO_SMALL_FUSED   = 64,         // n <= 16: the nine-kernel generation, not cma_small_generations
    DBG_RANK_COUNT32     = 128,        // counting rank: cma_rank (32 candidates a workgroup), not cma_rank32 / 64
    DBG_SAMPLE_GUARDED   = 256,        // the guarded builds of the samplers where the lean ones would run
    DBG_GRAM128_LDS      = 512,        // the LDS-staged cma_gram128, not cma_gram128s
    DBG_TRED_L2          = 1024,       // 128 < n <= 256: one kernel (cma_eigen_g), its first n - 128 Householder
                                       // steps streaming from L2; 64 < n <= 128: no split decomposition
    DBG_STAMPS_HALVES    = 2048,       // split decomposition: the phase clocks show cma_eig_halves' first half,
                                       // not the top merge
    DBG_RANK_COUNT_NO64  = 4096,       // counting rank: cma_rank32 where cma_rank64 would run
    DBG_DC_ONE_LEVEL     = 8192,       // divide and conquer stops after its first merge level (phase clocks)
    DBG_DC_TWO_LEVELS    = 16384,      // ... after its second
    DBG_DC_LEAF16        = 32768,      // 16 < n <= 128: leaves of 16 rows, not 8
    DBG_GRAM_NO_PACING   = 65536,      // cma_gram128s without its pacing barrier
    DBG_PATHS_LAZY256    = 131072,     // cma_paths_lazy (256 threads) where cma_paths_lazy1k would run
    DBG_RANK_BITONIC     = 262144,     // cma_rank_sort: the bitonic sort where the merge sort would run
    DBG_DC_LEAF_SINGLE   = 524288,     // one QL leaf per wavefront at a time, not two
    DBG_SEP_ROWS_LDS     = 1048576,    // sep_sample_eval (row in LDS) where sep_sample_sum would run
    DBG_EIG_GENERIC128   = 2097152,    // n = ld = 128: cma_eigen / cma_eigen_r1 where the fixed-shape builds would run
    DBG_EIG_ONE_WG       = 4194304,    // 64 < n <= 256: the whole decomposition on one workgroup (cma_eigen /
                                       // cma_eigen_g), no split over kernels
    DBG_DC_WG_BARRIERS   = 8388608,    // workgroup barriers in the one-wavefront merges
    DBG_TRED_ONE_WG      = 16777216,   // n > 128: the Householder reduction on one workgroup (cma_eigen_g1 /
                                       // cma_eigen_b), not spread
    DBG_TOP_PART2        = 33554432,   // top merge: Loewner vector and F by cma_eigen_g2 part 2, not cma_eig_lowner /
                                       // cma_eig_fcols
    DBG_TOP_ONE_KERNEL   = 67108864,   // 128 < n <= 256 (and the split form): the top merge as one cma_eigen_g2
    DBG_WY_PER_WAVE      = 134217728,  // cma_eig_wy (a tile per wavefront) where cma_eig_wy4 would run
    DBG_SAMPLE_4WAVES    = 268435456,  // n > 128: the four-wavefront cma_sample_eval where <1, 16> would run
    DBG_TRED_ALL_SPREAD  = 536870912,  // spread reduction: no cma_tred_tail (128 < n <= 256), no cma_tred_mw_chain
                                       // (n > 256)
    DBG_GRAM_LOOKUP      = 1073741824, // cma_gram128s looks its coefficients up (rank, then weights and S) where it would
                                       // take cma_rank_sort's table, and cma_rank_sort writes none
    // every bit cma_eigen / cma_eigen_r1 read inside the kernel (bbo_eig.hpp, bbo_eig_dc.hpp), and
    // DBG_EIG_ONE_WG, which asks for them.  The fixed-shape builds of n = ld = 128 read none, so any of these
    // -- and DBG_EIG_GENERIC128 -- keeps the generic kernel: a bit added to those two files belongs in this mask.
    DBG_EIG_IN_KERNEL    = DBG_QL_NO_APPLY | DBG_QL | DBG_DC_NO_MERGES | DBG_DC_NO_LEAVES | DBG_TRED_L2
                           | DBG_STAMPS_HALVES | DBG_DC_ONE_LEVEL | DBG_DC_TWO_LEVELS | DBG_DC_LEAF16
                           | DBG_DC_LEAF_SINGLE | DBG_EIG_ONE_WG | DBG_DC_WG_BARRIERS,
};

struct CmaDev {
    double *X;          // [P][lambda_pad][ld]   candidates (arx)
    double *f;          // [P][lambda_pad]       fitness, +inf on padding rows
    int *rank;          // [P][lambda_pad]       rank of candidate i
    int *order;         // [P][lambda_pad]       candidate with rank r   (= _fitness[r]._index)
    double *xmean, *xold, *pc, *ps;   // [P][ld]
    double *C;          // [P][ld][ld]  covariance, symmetric full (reference keeps the lower half)
    double *B;          // [P][ld][ld]  eigenvectors in columns
    double *D;          // [P][ld]      sqrt(eigenvalues), ascending
    double *isc;        // [P][ld][ld]  C^-1/2
    double *A;          // [P][ld][ld]  CholeskyCMAES: the lower factor, row-major (upper triangle 0)
    int *chol_repairs;  // [P]          CholeskyCMAES, sticky: pivots chol_factor had to lift to a positive value
    double *BDp;        // [P][ld*ld]   (B diag D) in MFMA B-fragment order (CholeskyCMAES: A)
    double *ISp;        // [P][ld*ld]   C^-1/2   in MFMA B-fragment order
    double *S;          // [P][mu_pad]  whitened squared norms of the worst mu
    double *csep;       // [P][ld] diagonal covariance of the separable variant (D = its sqrt)
    double *zn2;        // [P][lambda_pad] ||z||^2 of every candidate (cma_sample_eval128 only)
    double *coef_tab;   // [P][ceil(lambda_pad / 32)][2][32] ld = 128: the Gram coefficient v and the mean weight w of
                        // every ROW, in chunks of 32 rows (v of the 32, then w), written by cma_rank_sort for
                        // cma_gram128s (null: no table); rows >= lambda hold zeros
    int *coef_stamp;    // [P]          it + 1 of the generation whose ranking wrote coef_tab, 0 = never
    double *gram_part;  // [P][splits][ld][ld]
    double *mean_part;  // [P][splits][ld]
    double *hist_best, *hist_kth;     // [P][hlen]
    double *eig_work;   // [P][ld][ldw] scratch for the eigensolver when it does not fit LDS
    const double *weights;            // [mu]
    const double *lower, *upper, *aux;   // [ld]
    const double *zinject;            // [P][lambda][n] or null
    double *zrecord;                  // [P][lambda][n] or null
    CmaScal *scal;                    // [P]
    long long *stamps;                // [16] eigensolver phase clocks (diagnostic) or null
    int dbg;                          // diagnostic switches: CmaDbg bits (0 in production)
    int mw_fault;                     // fault injection of bbo_eig_mw.hpp (-1: none; environment only)
    int *mw_fail_host;                // pinned host word: a spread reduction of this engine timed out
};

// The kernels of one decomposition.  get "eig_route" returns the ids of the last launch_eigen in launch
// order, so this order is that key's contract: append, never renumber.
enum EigKernel : int {
    EK_EIGEN_SMALL = 0, EK_EIGEN_128, EK_EIGEN_256, EK_EIGEN, EK_EIGEN_FX128, EK_EIGEN_FX128U,   // 0 .. 5
    EK_EIGEN_R1, EK_EIGEN_R1_FX128, EK_EIGEN_G1, EK_TRED_MW, EK_TRED_TAIL, EK_EIG_HALVES,        // 6 .. 11
    EK_EIGEN_G2, EK_EIG_SECULAR, EK_EIG_LOWNER, EK_EIG_FCOLS, EK_EIGEN_G,                        // 12 .. 16
    EK_TRED_MW512, EK_TRED_MW_CHAIN, EK_EIGEN_B4, EK_EIGEN_B,                                    // 17 .. 20
    EK_EIG_GEMM1, EK_EIG_GEMM, EK_EIG_WY4, EK_EIG_WY4_512, EK_EIG_WY,                            // 21 .. 25
    EK_POST, EK_POST_MFMA                                                                        // 26, 27
};

// What one launch_eigen does: plain data, computed by CmaEngine::eig_route and by nothing else.
struct EigRoute {
    struct Step {
        EigKernel k;
        int arg;       // cma_tred_mw / _mw512: istop; cma_tred_tail: 1 behind the chain kernel; cma_eigen_g2: part;
                       // cma_eig_gemm: which product; cma_eig_wy4: pack mode
    };
    Step step[12];
    int count;         // steps in all, the trailing EK_POST / EK_POST_MFMA included
    int timed;         // the first `timed` of them are the profile's cma_eigen slot, the rest the top merge's products
    bool split;        // 64 < n <= 128, few matrices: the kernels behind the reduction take eig_plan_split
    bool post;         // launch_post(0) follows
    bool fixed;        // a fixed-shape build of n = ld = 128 (get "eig_fixed128")
    bool forms_c;      // cma_eigen_fx128 forms C on its load: no cma_cov in front (get "cov_fused")
    long mw_workgroups;   // > 0: spread kernels that need this many workgroups reserved (mw_reserve)
};

// The samplers.  get "sample_route" returns the id of the last launch_sample_eval, so this order is that
// key's contract: append, never renumber.  (sep_sample_sum's objective argument is not part of the id.)
enum SampleKernel : int {
    SK_NONE = -1,                                                           // no launch yet
    SK_SEP_16 = 0, SK_SEP_64_512, SK_SEP_64_512_LEAN, SK_SEP_SUM, SK_SEP_SUM4, SK_SEP_64,   // 0 .. 5: sep_sample_eval<16>,
                                    // <64, 512>, <64, 512, true>, sep_sample_sum<256, 0>, <256, 4>, sep_sample_eval<64>
    SK_EVAL128, SK_EVAL128_TRI, SK_TILE8, SK_TILE8_TRI,                     // 6 .. 9: cma_sample_eval128, _tri,
                                                                            // cma_sample_eval<1, 8>, <1, 8, true>
    SK_EVAL64_1_8, SK_EVAL64_1, SK_EVAL64_2,                                // 10 .. 12: cma_sample_eval64<1, 8>, <1>, <2>
    SK_TILE16, SK_EVAL_4, SK_EVAL_8                                         // 13 .. 15: cma_sample_eval<1, 16>, <4>, <8>
};

// What one launch_sample_eval does: plain data, computed by CmaEngine::sample_route and by nothing else.
struct SampleRoute {
    SampleKernel k;
    int gx, gy, block;      // grid (gx, gy), threads of a workgroup
    size_t lds;             // dynamic LDS bytes
    int rows_per_wg;        // cma_sample_eval128 / _tri: kernel argument
    int full;               // the lean build (get "sample_lean"): kernel argument of those two, the template
                            // argument of sep_sample_eval<64, 512, true>, always for sep_sample_sum
    bool writes_zn;         // the kernel hands down ||z||^2 of every candidate
    int transposed;         // cma_sample_eval128 / _tri, lean build: the transposed tile loop (get "sample_transposed"):
                            // kernel argument
};

// The kernels of one launch_update.  get "update_route" returns the ids of the last one in launch order:
// append, never renumber.  (cma_whiten<MAXT> is one id.)
enum UpdateKernel : int {
    UK_CHOL_PATHS = 0, UK_CHOL_CPRIME, UK_CHOL_FACTOR, UK_SEP_MOMENTS, UK_SEP_PATHS,     // 0 .. 4
    UK_WHITEN128, UK_WHITEN, UK_GRAM128S, UK_GRAM128, UK_GRAM,                           // 5 .. 9
    UK_PATHS, UK_PATHS_LAZY, UK_PATHS_LAZY1K, UK_COV                                     // 10 .. 13
};

// What one launch_update does: plain data, computed by CmaEngine::update_route and by nothing else.
struct UpdateRoute {
    struct Step {
        UpdateKernel k;
        int slot;           // the profile's slot of the launch (cma_whiten, cma_gram, cma_paths, cma_cov)
        int gx, gy, gz, block;
        size_t lds;
        int arg;            // chol_factor: in_lds; cma_whiten128: rows per workgroup; cma_whiten: MAXT; cma_gram: ldy
    };
    Step step[4];
    int count;
};

class CmaEngine: public Engine<CmaScal> {
public:
    static constexpr const char *HANDLE_NAME = "not a CMA-ES handle";
    explicit CmaEngine(const bbo_params &p);
    ~CmaEngine() override;

    void init(int n, const double *lower, const double *upper, const double *guess,
            const ObjectiveSpec &obj) override;
    void solution(int population, double *x_out, int *n_evals, int *converged) override;
    // (its own form: max_gen = mfev / lambda + 2, `converged` straight from the stop flag)
    void optimize(int n, const double *lower, const double *upper, const double *guess,
            const ObjectiveSpec &obj, double *x_out, int *n_evals, int *converged) override;
    int get(const std::string &key, int population, double *out, int cap) override;
    int set(const std::string &key, int population, const double *in, int count) override;
    int dimension() const override { return c_.n; }

    // BaseCmaes::setParams (base_cmaes.cpp:136-148), used by the restart drivers
    void set_params(int np, double sigma, int mfev);
    void phase(int which);
    void inject_normals(const double *z, int count);
    // evaluates one point with this engine's objective (restart drivers' extra call)
    double evaluate_point(const double *x);
    int lambda() const { return params_.np; }
    int populations() const { return params_.populations; }
    uint64_t seed() const { return params_.seed; }
    void set_seed(uint64_t s) { params_.seed = s; }
    // the next init() starts like a new object: B = C = I (not the previous run's, cmaes.cpp:53-59)
    void fresh_start(uint64_t s)
    {
        params_.seed = s;
        keep_bc_ = false;
    }

private:
    static const bbo_params &checked(const bbo_params &p);
    void generation(bool honor_stop) override;
    // (c_.mfev: set_params may have moved params_.mfev since init())
    bool budget_spent(const CmaScal &s) const override { return s.fev >= c_.mfev; }
    void inspect(const std::vector<CmaScal> &sc) override;   // basis_maybe_stale_, the spread reduction's flags
    int chunk_limit(int want) override;                      // the fused path: at most 512 generations a launch
    void launch_chunk(int gens) override;                    // the fused path: one launch
    void after_chunk(bool in_run) override;                  // iterate(): a spread reduction that gave up is redone
    bool small_fused_ok() const;
    void launch_small(int gens, bool honor_stop);
    void launch_sample_eval();
    void launch_post(int mode);
    void launch_rank();
    void launch_update(bool with_cov = true);
    SampleRoute sample_route() const;
    // norms_done: the ranking wrote the whitened norms; with_cov: cma_cov is not left to the eigensolver
    UpdateRoute update_route(bool norms_done, bool with_cov) const;
    // spread_ok: the spread reduction may be used; fuse_ok: no cma_cov has gone before (a generation)
    EigRoute eig_route(bool spread_ok = true, bool fuse_ok = false) const;
    void launch_eigen(EigRoute r);
    // the samplers' lean builds: no padding column or row, no box, no injected or recorded normals
    bool nothing_to_guard() const
    {
        return c_.n == c_.ld && !c_.bound && c_.lambda == c_.lambda_pad && !d_.zinject && !d_.zrecord
                && !(d_.dbg & DBG_SAMPLE_GUARDED);
    }
    void launch_history_stop();
    void host_evaluate();
    void program_evaluate();

    CmaConst c_ {};
    CmaDev d_ {};
    bool keep_bc_ = false;    // B and C survive a re-init of the same object (cmaes.cpp:53-54)
    bool basis_maybe_stale_ = false;   // some population's basis_ok may be 0 (refreshed at every poll)
    // the Householder reduction spread over several workgroups (128 < n <= 256, few populations):
    // its exchange buffers, the epoch base of its flags, and 'a wavefront once gave up: do not use it'
    DevBuf<double> mw_buf_;
    unsigned long long mw_launch_ = 0;
    bool mw_disabled_ = false;
    int mw_xcd_ = next_mw_xcd();        // this engine's offset into the XCDs
    static int next_mw_xcd();
    long sample_wide_max_tiles_ = 512;       // n = 128: at most this many 16-row tiles take cma_sample_eval<1, 8>
    long sample128_min_rows_ = 256 * 128;   // candidates in flight from which cma_sample_eval128 is used
    bool chol_tri_ = true;             // CholeskyCMAES, n = 128: the triangular forms of the two wide samplers
    bool sample128_rowlayout_ = false; // cma_sample_eval128 / _tri: the row-layout tile loop where the transposed one would run
    int split_maxp_ = 32;              // 64 < n <= 128: at most this many populations take the split decomposition
    EigRoute last_route_ {};           // what the last launch_eigen did (get "eig_route", "eig_fixed128", "cov_fused")
    SampleRoute last_sample_ { SK_NONE };   // what the last launch_sample_eval did (get "sample_route", "sample_lean",
                                            // "sample_transposed")
    UpdateRoute last_update_ {};       // what the last launch_update did (get "update_route")
    bool small_fused_ = false;         // the last generation or chunk was a cma_small_generations launch (get "small_fused")
    int last_rank_ = -1;               // the form the last launch_rank took: RankKernel (get "rank_route"), -1 before
    bool rank_wrote_norms_ = false;    // this generation's cma_rank_sort wrote S: no whiten launch
    int last_n_ = -1;

    DevBuf<double> zn2_, csep_, A_;
    DevBuf<double> X_, f_, xmean_, xold_, pc_, ps_, C_, B_, D_, isc_, BDp_, ISp_, S_,
            gram_part_, mean_part_, hist_best_, hist_kth_, eig_work_, weights_, zinject_, zrecord_;
    DevBuf<double> coef_tab_;
    DevBuf<int> rank_, order_, chol_repairs_, coef_stamp_;
    void coef_tab_forget();         // no ranking's coefficient table is valid any more (set(), inject_normals())
    DevBuf<long long> stamps_;
    int *mw_fail_host_ = nullptr;   // pinned, device-visible: raised by a spread reduction that timed out
    long mw_reserved_ = 0;          // workgroups this engine holds of the device's MwBudget
    bool mw_launched_ = false;      // a spread kernel went out since the flag was last read
    bool mw_reserve(long workgroups);
    void mw_release();
    bool mw_check_failed();         // after a synchronisation: true once when the flag went up
};

} // namespace bbo
