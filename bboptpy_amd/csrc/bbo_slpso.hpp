// bbo_slpso.hpp -- device-resident SLPSO: the self-learning particle swarm (Li, Yang & Nguyen 2012).
//
// Reference: SLPSOSearch (src/multivariate/pso/slpso.cpp:42-439).  The swarm is updated one particle
// after another (:107-151): a particle picks one of four learning operators (:112-116), moves itself or,
// in operator 2, its partner (:269-301), and every improving move starts Algorithm 2 (:338-354), a walk
// over the coordinates of the swarm's best point with one evaluation per chosen coordinate.  Nothing in a
// generation is parallel across particles, so the hot path is
//   slpso_generation   one workgroup per population, one whole iterate() per launch: the lanes own the
//                      coordinates, the first wavefront sums the objective from LDS
// and the same body, entered and left at its evaluations, is the path of bbo_iterate with a host
// objective, of bbo_slpso_phase and of the tests.
#pragma once

#include "bbo_engine.hpp"

namespace bbo {

// diagnostic switches: the bits of SlpsoConst::dbg (bbo_set "dbg", 0 in production)
enum SlpsoDbg { SLPSO_DBG_SEQ_ALG2 = 1 };    // Algorithm 2 one trial at a time in workgroups of several wavefronts

constexpr int SLPSO_MAX_N = 512;
constexpr int SLPSO_MAX_NP = 4096;
constexpr int SLPSO_NSTRAT = 4;

// where a population stands inside its generation
enum SlpsoStage {
    SLPSO_IDLE = 0,          // between generations
    SLPSO_MOVE,              // particle kp is about to choose its operator
    SLPSO_WAIT_MOVE,         // the moved particle `mv` awaits its value
    SLPSO_ALG2,              // Algorithm 2 looks for its next chosen coordinate from position `ai` on
    SLPSO_WAIT_ALG2          // the trial of chosen coordinate number `ai` awaits its value
};

// what a launch of the body does
enum SlpsoMode {
    SLPSO_FUSED = WALK_FUSED, SLPSO_ADVANCE = WALK_ADVANCE, SLPSO_ABSORB = WALK_ABSORB
};

struct SlpsoScal {
    double fabest, alpha, omega;
    int mfes;
    int fev;
    int it;                  // generations done: the counter word of the draws
    int stop;                // sticky: 1 = the norms' spread fell under stol, 2 = budget
    int conv;                // converged() of the state
    int stage, kp, mv, iop, ai;
    int pending;             // a point waits in cand
};

struct SlpsoConst {
    int n, ld, np;
    int obj, mfev, honor_stop, npop;
    int record, dbg;
    int sub0;                // the sub-stream of population 0
    double omegamin, omegamax, eta, gamma, vmax, stol;
    uint64_t seed;
};

struct SlpsoDev {
    double *x, *v, *pb;              // [P][np][ld]
    double *fx, *fpb, *fp, *Uf, *Pl; // [P][np]
    double *s, *p;                   // [P][np][4]
    int *g, *G;                      // [P][np][4]
    int *m, *CF, *PF, *perm;         // [P][np]
    double *abest, *vdavg, *cand;    // [P][ld]
    double *fcand;                   // [P]
    double *radius;                  // [P][np] the particles' norms (the stop test)
    double *draws;                   // [P][1 + np + np (3 + 4 n)] (recording, else null)
    const double *inject;            // the same table instead of the generator (else null)
    const double *Uf_tab, *Pl_tab;   // [np] by rank (:383-392, formed on the host)
    const double *lower, *upper, *aux;
    SlpsoScal *scal;
};

class SlpsoEngine: public WalkEngine<SlpsoScal> {
public:
    static constexpr const char *HANDLE_NAME = "not an SLPSO handle";
    explicit SlpsoEngine(const bbo_params &p);
    void init(int n, const double *lower, const double *upper, const double *guess,
            const ObjectiveSpec &obj) override;
    void solution(int population, double *x_out, int *n_evals, int *converged) override;
    int get(const std::string &key, int population, double *out, int cap) override;
    int set(const std::string &key, int population, const double *in, int count) override;
    int dimension() const override { return c_.n; }

    void configure(const bbo_slpso_params &sp);
    void inject_draws(const double *table, int count);

private:
    static const bbo_params &checked(const bbo_params &p);
    void launch_walk(int mode, bool begin) override;
    void launch_eval_device() override;
    PendingPoints pending_points(int p, const SlpsoScal&) override { return { &cand_, (size_t) p * c_.ld, 1, c_.ld, &fcand_ }; }
    int &honor_stop() override { return c_.honor_stop; }
    void launch_init(int p0, int pcount, int mode);
    int workgroup() const;
    size_t table_len() const { return 1 + (size_t) c_.np + (size_t) c_.np * (3 + 4 * (size_t) c_.n); }

    bbo_slpso_params sp_ {};
    SlpsoConst c_ {};
    SlpsoDev d_ {};
    DevBuf<double> x_, v_, pb_, fx_, fpb_, fp_, Uf_, Pl_, s_, p_, abest_, vdavg_, cand_, fcand_, radius_, Uf_tab_, Pl_tab_;
    DevBuf<int> g_, G_, m_, CF_, PF_, perm_;
    DrawTables tables_;
};

} // namespace bbo
