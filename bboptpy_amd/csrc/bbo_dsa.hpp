// bbo_dsa.hpp -- device-resident DSA: Differential Search (Civicioglu 2012) with the reference's
// Rexp3 bandit over its four direction methods.
//
// Reference: DSSearch (src/multivariate/pso/ds.cpp:36-365).  Its generation is synchronous already:
// the scalars, the direction rows, the maps, every trial and its box repair are settled before
// any member is replaced (:86-156).  Here a generation is
//   dsa_rank     the pool ranked by f (only under the methods that need it: :245-248, :266-269)
//   dsa_plan     p1, p2, the method, the map strategy, R, the direction row of every member
//                (:91-116, :219-292, :307-333)
//   dsa_evolve   map, trial, box repair, evaluation, greedy selection into the other half of the
//                pool's double buffer (:119-137, :304-365)
//   dsa_finish   successes, the bandit's weights, the stop test, the incumbent (:138-155, :186-217)
// Given the same draws that is the reference's arithmetic operation for operation
// (tests/dsa_model.py); only the random streams differ.
#pragma once

#include "bbo_engine.hpp"

namespace bbo {

struct DsaScal {
    double p[4], w[4];       // the bandit's probabilities and weights (ds.cpp:79-80)
    double fbest;            // fitness of bestx
    double m2;               // radius spread of the last stop test that reached it, else -1
    // the last generation's scalars: raw uniforms (p1, p2, method, coin, strategy, R) and what
    // was decided from them
    double raw[6];
    double p1, p2, R;
    int method, strategy, mapmax;   // 0..3, 0..2 (random-1, differential, random-2)
    int cur;                 // which half of X holds the pool
    int it;                  // the reference's _it (the bandit's batch clock; settable)
    int fev, gen;
    int stop;                // sticky: 1 = converged(), 2 = evaluation budget exhausted
    int conv;                // result of the last stop test
    int nsucc;               // accepted trials of the last generation
};

struct DsaConst {
    int n, ld, np;
    int adapt, nbatch;
    int obj, mfev, honor_stop, npop;
    int record;              // keep the draws and the trials of the generation
    int kb;                  // half the bits of np - 1, rounded up (cso_perm)
    int mcap;                // recorded coordinate draws of the random-2 map per member
    int force_method, force_map;    // -1: as drawn
    double tol, stol, gamma;
    uint64_t seed;
};

struct DsaDev {
    double *X[2];            // [P][np][ld], the pool and its successor
    double *f;               // [P][np]
    double *T;               // [P][np][ld] trials (host objective or recording, else null)
    double *ftrial;          // [P][np]
    double *radius;          // [P][np] norm of the row
    double *bestx;           // [P][ld]
    double *dirdraws;        // [P][np][2] (recording, else null)
    double *mapdraws;        // [P][np][n + 2 + mcap]
    double *bounddraws;      // [P][np][n][2]
    int *map;                // [P][np][n]
    int *order;              // [P][np] rank -> row
    int *dirrow;             // [P][np] the row every member moves towards
    int *acc;                // [P][np] the trial was accepted
    const double *lower, *upper, *aux;
    DsaScal *scal;
};

class DsaEngine: public Engine<DsaScal> {
public:
    static constexpr const char *HANDLE_NAME = "not a DSA handle";
    explicit DsaEngine(const bbo_params &p);
    void init(int n, const double *lower, const double *upper, const double *guess,
            const ObjectiveSpec &obj) override;
    void solution(int population, double *x_out, int *n_evals, int *converged) override;
    int get(const std::string &key, int population, double *out, int cap) override;
    int set(const std::string &key, int population, const double *in, int count) override;
    int dimension() const override { return c_.n; }

    // bbo_dsa_configure: the constructor arguments bbo_params has no field for
    void configure(const bbo_dsa_params &dp);

private:
    static const bbo_params &checked(const bbo_params &p);
    void generation(bool honor_stop) override;
    void alloc_record();

    bbo_dsa_params dp_ {};
    DsaConst c_ {};
    DsaDev d_ {};
    DevBuf<double> X0_, X1_, f_, T_, ftrial_, radius_, bestx_, dirdraws_, mapdraws_, bounddraws_;
    DevBuf<int> map_, order_, dirrow_, acc_;
};

} // namespace bbo
