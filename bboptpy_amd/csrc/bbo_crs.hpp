// bbo_crs.hpp -- device-resident CRS: the controlled random search with local mutation (Kaelo & Ali 2006).
//
// Reference: CrsSearch (src/multivariate/crs/crs.cpp:46-181).  Steady-state like NSHS: an iteration ends
// with ONE point replacing the worst of the np stored points (:160-166).  What it costs is open: trial()
// (:111-158) calls itself when the reflected point leaves the box (:132-134) and when the mutated point is
// rejected (:150-152), and goes on after the inner call returns.  Its frames hold no locals, so the call
// stack is a stack of bits (B: return to :135, M: return to :155) and the recursion is the state machine
//
//   CALL   centroid of the best point and n - 1 drawn points, reflection of one more drawn point (:114-129);
//          outside the box: push B, CALL again
//   L1     ft = f(t) (:135); ft >= f_worst: the mutation t2 (:142-147), ft2 = f(t2);
//          ft2 >= f_worst: push M, CALL; else t = t2
//   RET    stack empty: the iteration is complete; pop B: L1 (t is evaluated and counted again);
//          pop M: t = t2, ft = ft2 -- whatever mutation was computed LAST -- and RET again
//
// crs_steps runs it, one workgroup per population, resumable at every step: the stage, the bit stack, t,
// t2, ft, ft2 and the counters live in global memory between launches.  A launch ends for a population
// when it has completed its share of iterations or spent `launch_evals` steps (drawn trials and
// evaluations), so no launch's duration depends on the depth of a recursion; the host relaunches while
// one flag says that some population is short of its goal.  The same body, entered to advance to the
// next pending evaluation or to absorb a value, is the path of bbo_crs_phase and of a host objective
// (DESIGN.md section 3.14).
//
// The pool stays in place: order[rank] names the row, the accepted point is written into the worst's row
// and `order` is shifted behind the values that are <= the new one (stable, as the initial ranking is).
// A NaN value counts as +inf.  The reference recurses until its stack overflows once the pool has
// collapsed; here a push beyond `max_depth` ends the run with flag 3.
// Objective programs are refused at bbo_init; CRS is no restart base and has no multi-GPU sharding.
#pragma once

#include "bbo_engine.hpp"

namespace bbo {

constexpr int CRS_MAX_N = 512;
constexpr int CRS_MAX_NP = 65536;
constexpr int CRS_DEFAULT_CHUNK = 256;      // iterations per launch of bbo_run, as NSHS
// Steps (drawn trials + evaluations) a population may spend in one fused launch, as a multiple of the
// chunk of iterations.  An iteration of the recorded runs costs 2 to 4 steps, so a chunk normally ends
// on its iterations; a population deep in a recursion is cut here and resumed by the next launch.
constexpr int CRS_LAUNCH_STEPS_PER_ITERATION = 8;
constexpr int CRS_DEFAULT_RECORD = 64;      // records of draws kept per iteration under record_draws

// where a population stands inside its iteration
enum CrsStage {
    CRS_IDLE = 0,            // between iterations
    CRS_WAIT_TRIAL,          // t awaits its value (pending), or has it and awaits the draws of its mutation
    CRS_WAIT_MUT,            // t2 awaits its value
    CRS_CALL,                // a trial is about to be drawn
    CRS_RET                  // a point was accepted: the stack is being unwound
};

// what a launch of the body does
enum CrsMode {
    CRS_FUSED = WALK_FUSED, CRS_ADVANCE = WALK_ADVANCE,
    CRS_ABSORB = WALK_ABSORB // take the value of the pending evaluation, then advance (phase 2)
};

struct CrsScal {
    double fbest, fworst;    // f[order[0]], f[order[np - 1]]
    double ft, ft2;          // _ftrial, _ftrial2
    int fev;
    int it;                  // iterations completed
    int goal;                // the iteration count the current bbo_run chunk / bbo_iterate ends at
    int stop;                // sticky: 1 = |f_best - f_worst| < tol, 2 = budget, 3 = max_depth
    int conv;                // stop() of the pool
    int stage, depth, pending;
    int trials;              // trials drawn: the counter word of their index draws
    int muts;                // mutations drawn: the counter word of their uniforms
    int stale;               // iterations whose replacement was no better than the worst it replaced
    int maxdepth;            // the deepest stack of the last iteration
    int nrec;                // records of draws the current iteration has made (record_draws)
    int irec;                // records of the injected table consumed
    int wused;               // the current record's uniforms are spent
    int starved;             // the injected table ran out: the iteration waits for the next one
};

struct CrsConst {
    int n, ld, np;
    int obj, mfev, honor_stop, npop;
    int record;              // records of draws kept per iteration (0: none)
    int inject_n;            // records per population in the injected table
    int max_depth, repair, launch_evals, stack_words;
    double tol;
    uint64_t seed;
};

struct CrsDev {
    double *X;               // [P][np][ld] the pool, in place
    double *f;               // [P][np]
    int *order;              // [P][np] rank -> row
    double *cand, *cand2;    // [P][ld] _trial, _trial2
    double *value;           // [P] the value bbo_crs_phase 1 computed for the pending point
    uint32_t *stack;         // [P][stack_words] bit k: the return point of frame k (0 = B, 1 = M)
    double *draws;           // [P][record][2 n] (recording, else null)
    const double *inject;    // [P][inject_n][2 n] draws instead of the generator's (else null)
    int *more;               // [1] some population ended the launch short of its goal
    const double *lower, *upper, *aux;
    CrsScal *scal;
};

class CrsEngine: public WalkEngine<CrsScal> {
public:
    static constexpr const char *HANDLE_NAME = "not a CRS handle";
    explicit CrsEngine(const bbo_params &p);
    void init(int n, const double *lower, const double *upper, const double *guess,
            const ObjectiveSpec &obj) override;
    void solution(int population, double *x_out, int *n_evals, int *converged) override;
    int get(const std::string &key, int population, double *out, int cap) override;
    int set(const std::string &key, int population, const double *in, int count) override;
    int dimension() const override { return c_.n; }

    void configure(const bbo_crs_params &cp);
    // bbo_crs_inject_draws: [P][records][2 n] (n row indices, n uniforms)
    void inject_draws(const double *table, int count);

private:
    static const bbo_params &checked(const bbo_params &p);
    void launch_walk(int mode, bool begin) override;
    void launch_eval_device() override;
    // the point of stage 2 (the mutation) waits in cand2
    PendingPoints pending_points(int p, const CrsScal &s) override
    {
        return { s.stage == CRS_WAIT_MUT ? &cand2_ : &cand_, (size_t) p * c_.ld, 1, c_.ld, &value_ };
    }
    int &honor_stop() override { return c_.honor_stop; }
    void launch_chunk(int gens) override;
    void inspect(const std::vector<CrsScal> &sc) override;
    int default_poll() const override { return CRS_DEFAULT_CHUNK; }
    void launch_init(int p0, int pcount, int mode);
    void launch_rank(int p0, int pcount);
    void launch_body(int mode, int k, bool begin);
    void fused(int k);
    void reset_walk(int p);
    int workgroup() const;
    int launch_evals(int k) const;

    bbo_crs_params cp_ {};
    CrsConst c_ {};
    CrsDev d_ {};
    DevBuf<double> X_, f_, cand_, cand2_, value_;
    DrawTables tables_;      // records of 2 n draws: the injected table and the recorded one
    DevBuf<int> order_, more_;
    DevBuf<uint32_t> stack_;
    int launch_evals_ = 0;           // bbo_set "launch_evals": 0 = CRS_LAUNCH_STEPS_PER_ITERATION per iteration
};

} // namespace bbo
