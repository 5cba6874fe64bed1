// bbo_rosen.hpp -- device-resident Rosenbrock: the rotating-axes search with the line search of Davies, Swann
// and Campey and Palmer's orthogonalisation.
//
// Reference: Rosenbrock (src/multivariate/rosenbrock/rosenbrock.cpp:49-332).  A local method without a random
// draw: a line search costs about eight evaluations, so an engine is no wider than a workgroup and pays across
// `populations`: independent searches from the rows of `guess`, a multi-start.  lineSearch() (:227-332) is the
// state machine
//
//   IDLE      between searches: iterate()'s bookkeeping is done, the next search has not begun
//   FIRST     x0 and x0 + s v await their values (:233-239)
//   BACK      x0 - s v awaits its value (:244-247)
//   DOUBLE    the doubled step's point awaits its value, one per round (:254-264)
//   INTERP    the four interpolation points await their values (:272-280)
//   FINAL     the interpolated point awaits its value (:316-318)
//
// and iterate() (:95-210) what follows a search: the row count i, the extra search along the stage's
// displacement, the step test, Palmer's orthogonalisation (:144-185), the shrink of the step, the two ends.
// rosen_walk runs both, one workgroup per population, resumable at every batch of evaluations: the stage, the
// rows x, the directions v, d and the counters live in global memory between launches.  With a device objective
// a launch evaluates inside and ends at the population's goal of line searches; with a host objective the same
// walk is left at every batch and entered again with its values.  Objective programs
// are refused at bbo_init; no restart base, no multi-GPU sharding.
#pragma once

#include "bbo_engine.hpp"

namespace bbo {

constexpr int ROSEN_MAX_N = 128;
constexpr int ROSEN_THREADS = 256;        // rosen_walk in its wide form (one wavefront in the narrow), rosen_eval
constexpr int ROSEN_BATCH = 4;            // the most points a batch holds
constexpr int ROSEN_DEFAULT_CHUNK = 64;   // line searches per launch of bbo_run

enum RosenStage {
    ROSEN_IDLE = 0, ROSEN_WAIT_FIRST, ROSEN_WAIT_BACK, ROSEN_WAIT_DOUBLE, ROSEN_WAIT_INTERP, ROSEN_WAIT_FINAL,
    // inside a launch only: never stored with a batch pending
    ROSEN_NEXT_DOUBLE, ROSEN_PREP_INTERP, ROSEN_FINISH
};

// what a launch of the walk does
enum RosenMode {
    ROSEN_FUSED = WALK_FUSED, ROSEN_ADVANCE = WALK_ADVANCE,
    ROSEN_ABSORB = WALK_ABSORB  // take the values of the pending batch, then advance (phase 2)
};

// "path": the direction and the end of the last search
enum RosenDir { ROSEN_FORWARD = 1, ROSEN_BACKWARD, ROSEN_STRAIGHT };
enum RosenEnd { ROSEN_END_NONE = 0, ROSEN_END_KEPT, ROSEN_END_RESTORED, ROSEN_END_BUDGET };

struct RosenScal {
    double stepi, s, fx0, fx, stepf;     // _stepi; lineSearch()'s s, fx0, fx, stepf
    double fs[4];
    int fev;                 // _fev
    int it;                  // line searches completed
    int goal;                // the search count the current bbo_run chunk / bbo_iterate ends at
    int stop;                // sticky: 1 = stepi <= tol, 2 = the budget (_ierr + 1)
    int conv;
    int stage, pending;      // RosenStage; the points that await their values
    int i;                   // _i
    int pdir, prounds, pimin, pend;      // the last search's path
    int orth, orths;         // the last search ended in an orthogonalisation; how many there were
    // ticks of the constant-rate clock the launches of rosen_walk took, and the orthogonalisations of them
    // (copy of v, temp, the n^2 sums; as thread 0 saw them): scripts/bench_rosenbrock.py's share of a stage
    long long walk_ticks, orth_ticks;
};

// the scalars of a fresh start (:85-92): what init() uploads and rosen_rearm writes
__host__ __device__ inline RosenScal rosen_fresh_scal(double step0)
{
    RosenScal s = {};
    s.stepi = step0;
    s.i = 1;
    s.pimin = -1;
    return s;
}

struct RosenConst {
    int n, ld;
    int obj, mfev, honor_stop, npop;
    int wide, repair;
    double tol, decf;
    double step0;            // what a re-arm sets stepi to
};

struct RosenDev {
    double *x, *v, *vold;    // [P][n + 2][ld]
    double *d;               // [P][n + 2]
    double *x0;              // [P][ld] lineSearch()'s x0 (_wx) while a search is under way
    double *x1;              // [P][ld] _x1
    double *cand;            // [P][4][ld] the pending batch
    double *value;           // [P][4]
    const double *aux;
    RosenScal *scal;
};

class RosenEngine: public WalkEngine<RosenScal> {
    friend class BhEngine;      // borrows the handle as its local minimiser (bbo_bh.hpp)
public:
    static constexpr const char *HANDLE_NAME = "not a Rosenbrock handle";
    explicit RosenEngine(const bbo_params &p);
    void init(int n, const double *lower, const double *upper, const double *guess,
            const ObjectiveSpec &obj) override;
    void optimize(int n, const double *lower, const double *upper, const double *guess,
            const ObjectiveSpec &obj, double *x_out, int *n_evals, int *converged) override;
    void solution(int population, double *x_out, int *n_evals, int *converged) override;
    int get(const std::string &key, int population, double *out, int cap) override;
    int set(const std::string &key, int population, const double *in, int count) override;
    int dimension() const override { return c_.n; }

    void configure(const bbo_rosen_params &rp);

private:
    static const bbo_params &checked(const bbo_params &p);
    void launch_walk(int mode, bool begin) override;
    void launch_eval_device() override;
    PendingPoints pending_points(int p, const RosenScal &s) override;
    int &honor_stop() override { return c_.honor_stop; }
    void launch_chunk(int gens) override;
    // iterate() tests the budget itself, behind a stage and inside the doubling loop
    bool budget_spent(const RosenScal&) const override { return false; }
    int default_poll() const override { return ROSEN_DEFAULT_CHUNK; }
    void launch_body(int mode, int k, bool begin);

    bbo_rosen_params rp_ {};
    int inits_ = 0;          // bbo_init calls so far: a borrower notices a handle that was initialised behind its back
    RosenConst c_ {};
    RosenDev d_ {};
    DevBuf<double> x_, v_, vold_, dd_, x0_, x1_, cand_, value_;
};

} // namespace bbo
