// bbo_bh.hpp -- device-resident BasinHopping: Metropolis chains whose every hop is a whole local minimisation.
//
// Reference: BasinHopping, StepsizeStrategy, AdaptiveStepsizeStrategy, MetropolisHastings
// (src/multivariate/basin/basinhopping.cpp:46-203).  The engine borrows a NelderMead or a Rosenbrock handle of
// this library, as the restart drivers borrow their CMA-ES base, and runs one chain per population of it.  A chain
// is the state machine
//
//   WAIT_INNER    the minimiser walks from xtrial; bh_collect takes its result when it has stopped
//   WAIT_ENERGY   xsol awaits its value, the one extra evaluation of :136 / :163
//   IDLE          between hops (it < goal is never left idle by a launch: bh_decide takes the next step itself)
//
// bh_decide absorbs the energy (:169-189), takes the next step (:50-88) and re-arms the population of the
// minimiser at xtrial with that engine's own re-arm (nm_rearm, rosen_rearm): no point, value or decision leaves
// the device between hops.  With a built-in objective the host only launches -- a chunk of the minimiser's walk,
// then collect + decide fused -- and polls one counter of finished chains; with a callable the minimiser's own host
// loop runs every population to its stop, then one host batch values the energy points.
#pragma once

#include "bbo_engine.hpp"

namespace bbo {

class NmEngine;
class RosenEngine;

constexpr int BH_MAX_N = 128;
constexpr int BH_THREADS = 128;          // one wavefront at n <= 64
constexpr int BH_LOG_COLS = 7;           // it, f, conv, step, accept, f*, fev

enum BhStage { BH_IDLE = 0, BH_WAIT_INNER, BH_WAIT_ENERGY };

// what a launch of bh_hop does
enum BhMode {
    BH_FUSED = WALK_FUSED,   // collect with the evaluation inside, then decide
    BH_COLLECT = WALK_ADVANCE,       // collect: xsol is left pending (bbo_bh_phase 1)
    BH_DECIDE = WALK_ABSORB, // decide with the value in `evalue` (bbo_bh_phase 3)
    BH_BEGIN,                // the goal becomes min(it + K, mit); an idle chain below it takes its step (bbo_bh_phase 0)
    BH_EVALUATE              // the built-in at every pending xsol (bbo_bh_phase 2)
};

struct BhScal {
    double energy, bestenergy, stepsize;
    int nstep, naccept;      // _nstep, _naccept
    int it;                  // _it; -1 until the first minimisation is absorbed
    int goal;                // the hop count the current run ends at
    int fev;                 // _fev
    int stage, pending;
    int inner_fev, inner_conv;       // of the run bh_collect took
    int rows;                // log rows written
};

struct BhConst {
    int n, ld, npop, mit, substream;
    int adaptive, interval;
    int inject_hops;         // hops the injected table covers
    double accept_rate, factor, beta;
    uint64_t seed;
};

struct BhDev {
    double *x, *xbest, *xtrial, *xsol;       // [P][ld]
    double *evalue;          // [P] the value of xsol
    double *log;             // [P][mit + 1][7]
    double *log_start, *log_sol;     // [P][mit + 1][ld]
    int *log_fev;            // [P][mit + 1]
    const double *lower, *upper;
    const double *inject;    // [inject_hops][n + 1] or null
    int *done;               // chains that reached their goal in this run
    BhScal *scal;
};

// bbo_bh_draws: the n + 1 uniforms of one hop on the host, by the functions the kernels call (bbo_bh_kernels.hpp)
void bh_draws_host(uint64_t seed, int substream, int hop, int n, double *out);

class BhEngine: public Optimizer {
public:
    static constexpr const char *HANDLE_NAME = "not a BasinHopping handle";
    BhEngine(const bbo_params &p, Optimizer *minimizer);
    ~BhEngine() override;
    void init(int n, const double *lower, const double *upper, const double *guess,
            const ObjectiveSpec &obj) override;
    void iterate() override;
    int run(int max_hops) override;
    void optimize(int n, const double *lower, const double *upper, const double *guess,
            const ObjectiveSpec &obj, double *x_out, int *n_evals, int *converged) override;
    void solution(int population, double *x_out, int *n_evals, int *converged) override;
    int get(const std::string &key, int population, double *out, int cap) override;
    int set(const std::string &key, int population, const double *in, int count) override;
    int dimension() const override { return c_.n; }

    void configure(const bbo_bh_params &bp);
    void phase(int which);
    void inject_draws(const double *table, int count);

private:
    void enter(const char *call, int population = 0);
    void require_native_minimizer() const;
    void hops(int k);
    void launch_inner();
    void launch_hop(int mode, int k);
    void host_energies();
    bool inner_all_stopped();
    int finished();
    std::vector<int> hop_counts();
    void print_new_rows();
    template<class Launch> void timed(int slot, Launch launch);

    bbo_params params_;
    bbo_bh_params bp_ {};
    NmEngine *nm_ = nullptr;
    RosenEngine *rosen_ = nullptr;
    Optimizer *min_ = nullptr;
    ObjectiveSpec obj_;
    hipStream_t stream_ = nullptr;       // the minimiser's: its walk and the hops are one queue
    bool inited_ = false;
    bool lockstep_ = false;     // bp_.lockstep resolved at init()
    int inner_inits_ = 0;       // the minimiser's count of bbo_init calls at this engine's init()
    int printed_ = 0;
    KernelTimer timer_;
    BhConst c_ {};
    BhDev d_ {};
    DevBuf<double> x_, xbest_, xtrial_, xsol_, evalue_, log_, log_start_, log_sol_, lower_, upper_, inject_;
    DevBuf<int> log_fev_, done_;
    DevBuf<BhScal> scal_;
};

} // namespace bbo
