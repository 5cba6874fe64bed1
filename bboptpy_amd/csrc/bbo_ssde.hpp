// bbo_ssde.hpp -- device-resident SSDE: spherical search (Kumar et al. 2019) with the DE fallback of
// Zhao et al. 2022.
//
// Reference: SSDESearch (src/multivariate/de/ssde.cpp:46-472).  iterate() (:134-361) updates the pool in
// place, member after member: member i reads rows the members before it have replaced, R = fev / mfev
// (:173) moves with every evaluation, and with usede a member whose spherical trial loses draws and
// evaluates a DE trial (:250-293).  Nothing in a generation is parallel across members, so the hot path is
//   ssde_generation   one workgroup per population, one whole iterate() per launch: the lanes own the
//                     coordinates, the first wavefront sums the objective from LDS
// and the same body, entered and left at its evaluations, is the path of bbo_iterate with a host
// objective, of bbo_ssde_phase and of the tests.
// randA() (:410-432) builds ONE matrix per generation: the identity with the shuffled coordinates paired
// off two by two, each pair a rotation by pi / 2 - 1e-12.  A row has two non-zeros (one for the leftover
// coordinate of an odd n), so computeTrialPoint's (:434-453) two dense n x n loops are two sparse passes.
#pragma once

#include "bbo_engine.hpp"

namespace bbo {

constexpr int SSDE_MAX_N = 512;
constexpr int SSDE_MAX_NP = 4096;
constexpr int SSDE_MIN_NP = 4;           // sample3 (:459-472) needs three members besides i
constexpr int SSDE_MAX_H = 65536;
constexpr int SSDE_MAX_TRIES = 64;       // the bound of the device generator's rejection loops
constexpr int SSDE_REC_HEAD = 9;         // iL, zr, p, q, r, pbest, ci, zcr, j0

// where a population stands inside its generation
enum SsdeStage {
    SSDE_IDLE = 0,           // between generations
    SSDE_MEMBER,             // member `mi` is about to draw its spherical trial
    SSDE_WAIT_SS,            // the spherical trial awaits its value
    SSDE_DE,                 // the spherical trial lost: member `mi` is about to draw its DE trial
    SSDE_WAIT_DE             // the DE trial awaits its value
};

// what a launch of the body does
enum SsdeMode {
    SSDE_FUSED = WALK_FUSED, SSDE_ADVANCE = WALK_ADVANCE, SSDE_ABSORB = WALK_ABSORB
};

struct SsdeScal {
    double oldbestf;         // _swarm[0]._f when the generation began (:135)
    double prank, ci, R;     // of the member whose trial is pending
    double cr1;              // of its DE trial
    int np;                  // the current pool size
    int fev;
    int gen;                 // generations done: the counter word of the draws
    int stop;                // sticky: 1 = converged(), 2 = budget
    int conv;                // converged() of the state
    int convcount;
    int k, kCR;              // 1-based, as the reference keeps them
    int lenS, lenSCR;        // successes recorded in this generation
    int stage, mi, iL, pi, qi, ri;
    int pending;             // a point waits in cand
    int keep_perm;           // "perm" was set: the next generation does not draw one
};

struct SsdeConst {
    int n, ld, npinit, nrows, H;
    int obj, mfev, honor_stop, npop;
    int record;
    int sub0;                // the sub-stream of population 0
    int patience, npmin, usede, repaircr;
    double ptop, tol;
    uint64_t seed;
};

struct SsdeDev {
    double *x;                       // [P][nrows][ld] the pool in place (nrows = npinit, 2 npinit with usede)
    double *f;                       // [P][nrows] by row
    int *order, *order2;             // [P][nrows] rank -> row, and the sort's scratch
    double *L1, *L2, *LCR;           // [P][H]
    double *SR, *SC, *w, *SCR, *wCR; // [P][npinit] the successes of the generation, in member order
    double *radius;                  // [P][npinit] the members' norms by rank (the stop test)
    int *perm;                       // [P][ld] the generation's permutation
    double *cand;                    // [P][ld]
    double *fcand;                   // [P]
    double *draws;                   // [P][n + npinit (9 + 3 n)] (recording, else null)
    const double *inject;            // the same table instead of the generator (else null)
    const double *lower, *upper, *aux;
    SsdeScal *scal;
};

class SsdeEngine: public WalkEngine<SsdeScal> {
public:
    static constexpr const char *HANDLE_NAME = "not an SSDE handle";
    explicit SsdeEngine(const bbo_params &p);
    void init(int n, const double *lower, const double *upper, const double *guess,
            const ObjectiveSpec &obj) override;
    void solution(int population, double *x_out, int *n_evals, int *converged) override;
    int get(const std::string &key, int population, double *out, int cap) override;
    int set(const std::string &key, int population, const double *in, int count) override;
    int dimension() const override { return c_.n; }

    void configure(const bbo_ssde_params &sp);
    void inject_draws(const double *table, int count);

private:
    static const bbo_params &checked(const bbo_params &p);
    void launch_walk(int mode, bool begin) override;
    void launch_eval_device() override;
    PendingPoints pending_points(int p, const SsdeScal&) override { return { &cand_, (size_t) p * c_.ld, 1, c_.ld, &fcand_ }; }
    int &honor_stop() override { return c_.honor_stop; }
    void seed_pool(int p0, int pcount);
    void launch_init(int p0, int pcount, int mode, int r0, int r1);
    int workgroup() const;
    size_t table_len() const { return (size_t) c_.n + (size_t) c_.npinit * (SSDE_REC_HEAD + 3 * (size_t) c_.n); }
    void set_memory(DevBuf<double> &b, int p, const double *in, int count, const char *what);

    bbo_ssde_params sp_ {};
    SsdeConst c_ {};
    SsdeDev d_ {};
    DevBuf<double> x_, f_, L1_, L2_, LCR_, SR_, SC_, w_, SCR_, wCR_, radius_, cand_, fcand_;
    DevBuf<int> order_, order2_, perm_;
    DrawTables tables_;
};

} // namespace bbo
