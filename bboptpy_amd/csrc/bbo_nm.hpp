// bbo_nm.hpp -- device-resident NelderMead: O'Neill's AS 47 simplex search with restarts.
//
// Reference: NelderMead (src/multivariate/simplex/nelder_mead.cpp:41-401).  Steady-state like ACD and CRS:
// a step costs one or two evaluations, a shrink n + 1, so an engine is no wider than a workgroup and pays
// across `populations`: thousands of independent simplexes, a multi-start local search.  nelmin() (:245-304)
// is the state machine
//
//   BUILD     initSimplex() (:312-367) from `start` and `del`; its n + 1 rows await their values
//   IDLE      between steps.  Under bbo_run: converged or fev >= mfev leads to the factorial test
//             (:270-295), 2 n probes formed at once from the drift each coordinate's restore leaves
//   REFLECT   pstar awaits its value (:108-114)
//   SECOND    p2star awaits its value: expansion (:119-125), inside (:151-157) or outside (:183-189)
//   SHRINK    the n + 1 rows of the shrunk simplex await their values (:159-175)
//   FACT      the probes await their values; the first below ynl restarts (:300-302), none converges
//
// nm_walk runs it, one workgroup per population and a lane per coordinate, resumable at every evaluation:
// the stage, the simplex, y and the counters live in global memory between launches.  With a device
// objective a launch evaluates inside and ends at the population's goal of steps; with a host objective
// the same walk is left at every batch and entered again with its values.
// Objective programs are refused at bbo_init; no restart base, no multi-GPU sharding.
#pragma once

#include "bbo_engine.hpp"

namespace bbo {

constexpr int NM_MAX_N = 128;
constexpr int NM_THREADS = 128;          // nm_walk at n > 64 (one wavefront below), nm_eval
// nm_walk's static LDS (y, the values of a batch, seven vectors): what a workgroup takes next to its simplex
constexpr int NM_STATIC_LDS = (NM_MAX_N + 2 + 2 * NM_MAX_N + 7 * NM_MAX_N) * 8;
constexpr int NM_DEFAULT_CHUNK = 64;     // simplex steps per launch of bbo_run

enum NmStage {
    NM_IDLE = 0, NM_WAIT_REFLECT, NM_WAIT_SECOND, NM_WAIT_SHRINK, NM_WAIT_FACT, NM_WAIT_INIT, NM_BUILD
};

// what a launch of the walk does
enum NmMode {
    NM_FUSED = WALK_FUSED, NM_ADVANCE = WALK_ADVANCE,
    NM_ABSORB = WALK_ABSORB  // take the values of the pending batch, then advance (phase 2)
};

// NmScal::kind, the second point of a step
enum NmKind { NM_EXPAND = 1, NM_INSIDE, NM_OUTSIDE };

// "branch": the path of the last step
enum NmBranch {
    NM_BR_NONE = 0, NM_BR_EXPANDED, NM_BR_EXPAND_REFUSED, NM_BR_REFLECTED, NM_BR_INSIDE, NM_BR_SHRINK,
    NM_BR_OUTSIDE, NM_BR_OUTSIDE_REFUSED
};

struct NmScal {
    double ylo, ynl, del, ystar;
    int fev;                 // _icount
    int it;                  // simplex steps completed
    int goal;                // the step count the current bbo_run chunk / bbo_iterate ends at
    int stop;                // sticky: 1 = the factorial test passed, 2 = mfev < fev
    int conv;                // _conv of the last step
    int stage, pending;      // NmStage; the points that await their values
    int ilo, ihi;            // 0-based
    int jcount, kind, branch, restarts;
};

// the scalars of a fresh start (:82-86): what init() uploads and nm_rearm writes
__host__ __device__ inline NmScal nm_fresh_scal(int checkev)
{
    NmScal s = {};
    s.jcount = checkev;
    s.del = 1.;
    s.stage = NM_BUILD;
    return s;
}

struct NmConst {
    int n, ld;
    int obj, mfev, honor_stop, npop;
    int minit, checkev, repair, lds, substream;
    int vs;                  // values per population: 2 n (>= n + 1)
    double ccoef, ecoef, rcoef, scoef, rq, eps;
    double sp, sq;           // spendley's p and q (:325-327)
    uint64_t seed;
};

struct NmDev {
    double *P;               // [P][n + 1][ld] the simplex
    double *y;               // [P][n + 1]
    double *start, *xmin, *step;     // [P][ld]
    double *cand;            // [P][2 n][ld] pstar, p2star; the probes of the factorial test
    double *value;           // [P][vs] the values of the pending batch
    const double *lower, *upper, *aux;
    NmScal *scal;
};

class NmEngine: public WalkEngine<NmScal> {
    friend class BhEngine;      // borrows the handle as its local minimiser (bbo_bh.hpp)
public:
    static constexpr const char *HANDLE_NAME = "not a NelderMead handle";
    explicit NmEngine(const bbo_params &p);
    void init(int n, const double *lower, const double *upper, const double *guess,
            const ObjectiveSpec &obj) override;
    void optimize(int n, const double *lower, const double *upper, const double *guess,
            const ObjectiveSpec &obj, double *x_out, int *n_evals, int *converged) override;
    void solution(int population, double *x_out, int *n_evals, int *converged) override;
    int get(const std::string &key, int population, double *out, int cap) override;
    int set(const std::string &key, int population, const double *in, int count) override;
    int dimension() const override { return c_.n; }

    void configure(const bbo_nm_params &np);

private:
    static const bbo_params &checked(const bbo_params &p);
    void launch_walk(int mode, bool begin) override;
    void launch_eval_device() override;
    PendingPoints pending_points(int p, const NmScal &s) override;
    int &honor_stop() override { return c_.honor_stop; }
    void launch_chunk(int gens) override;
    // nelmin() tests the budget itself, and at fev == mfev still runs the factorial test
    bool budget_spent(const NmScal&) const override { return false; }
    int default_poll() const override { return NM_DEFAULT_CHUNK; }
    void launch_body(int mode, int k, bool begin);
    void coefficients(int n);

    bbo_nm_params np_ {};
    int inits_ = 0;          // bbo_init calls so far: a borrower notices a handle that was initialised behind its back
    NmConst c_ {};
    NmDev d_ {};
    DevBuf<double> P_, y_, start_, xmin_, step_, cand_, value_;
    std::vector<double> ynl_h_;      // the bound of a host-driven factorial batch, per population
};

} // namespace bbo
