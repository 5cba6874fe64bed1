// bbo_jaya.hpp -- device-resident JAYA: self-adaptive multi-population Jaya with Levy-flight and
// chaotic mutations (Rao 2016; Rao & Saroj 2017; Yu et al. 2019; Ravipudi & Neebha 2018).
//
// Reference: JayaSearch (src/multivariate/jaya/jaya.cpp:57-377).  The reference evolves one member
// at a time and holds POINTERS to the best and the worst member of a sub-population, so a member
// evolved after the best sees its already replaced coordinates; here a generation is
//   jaya_partition   shuffle, sub-population lengths, best / worst of every sub-population
//                    copied into `bw`, the chaotic chain of the generation (:136-157, :225-239)
//   jaya_evolve      trial / clamp / evaluate / greedy replacement of every member (:260-338)
//   jaya_finish      max f, incumbent, stop test, performance index and the next k (:166-173,
//                    :184-217, :241-252)
// and every member of a sub-population uses that sub-population's best and worst rows as they stood
// at the start of the generation (tests/jaya_model.py states both orders).
#pragma once

#include "bbo_engine.hpp"

namespace bbo {

struct JayaScal {
    double xchaos;           // state of the chaotic map (jaya.cpp:355-377)
    double fgbest;           // fitness of bestx
    double best, pbest;      // the reference's _best / _pbest: fgbest after init, then +inf (jaya.cpp:143)
    double m2;               // radius spread of the last stop test
    double uroul;            // the roulette's uniform of the last generation (recording)
    int k;                   // sub-populations of the NEXT generation
    int fev, gen;
    int stop;                // sticky: 1 = radius test fired, 2 = evaluation budget exhausted
    int conv;                // result of the last stop test
    int nredraw;             // redraws of xchaos so far (the guards of :361, :372)
};

struct JayaConst {
    int n, ld, np, npmin, nks;
    int adapt, mutation, kcheb;
    int obj, mfev, honor_stop, npop;
    int record;              // keep the draws and the trials of the generation
    int kb;                  // half the bits of np - 1, rounded up (cso_perm)
    int ndraw;               // recorded draws per coordinate: r1, r2 (levy: zu, zv, u, r1, r2)
    double tol, scale, beta, temper, sigmau;
    uint64_t seed;
};

struct JayaDev {
    double *X;               // [P][np][ld]
    double *f;               // [P][np]
    double *T;               // [P][np][ld] trials by row (host objective or recording, else null)
    double *ftrial;          // [P][np]
    double *radius;          // [P][np] norm of the row
    double *bw;              // [P][nks][2][ld] best and worst row of every sub-population
    double *chaos;           // [P][nks][n][2] r1, r2 of the best member of every sub-population
    double *pstrat, *perfindex;   // [P][nks]
    double *bestx;           // [P][ld]
    double *draws;           // [P][np][n][ndraw] (recording, else null)
    int *occ, *occ2;         // [P][np] slot -> row
    int *len;                // [P][nks]
    int *off;                // [P][nks + 1] first slot of every sub-population
    int *bwrow;              // [P][nks][2] rows of the best and the worst member
    const double *lower, *upper, *aux;
    JayaScal *scal;
};

class JayaEngine: public Engine<JayaScal> {
public:
    static constexpr const char *HANDLE_NAME = "not a JAYA handle";
    explicit JayaEngine(const bbo_params &p);
    void init(int n, const double *lower, const double *upper, const double *guess,
            const ObjectiveSpec &obj) override;
    void solution(int population, double *x_out, int *n_evals, int *converged) override;
    int get(const std::string &key, int population, double *out, int cap) override;
    int set(const std::string &key, int population, const double *in, int count) override;
    int dimension() const override { return c_.n; }

    // bbo_jaya_configure: the constructor arguments bbo_params has no field for
    void configure(const bbo_jaya_params &jp);
    static int count_ks(int np, int npmin);

private:
    static const bbo_params &checked(const bbo_params &p);
    static void check_jaya(const bbo_params &p, const bbo_jaya_params &jp);
    void generation(bool honor_stop) override;
    void alloc_record();

    bbo_jaya_params jp_ {};
    JayaConst c_ {};
    JayaDev d_ {};
    DevBuf<double> X_, f_, T_, ftrial_, radius_, bw_, chaos_, pstrat_, perfindex_, bestx_, draws_;
    DevBuf<int> occ_, occ2_, len_, off_, bwrow_;
};

} // namespace bbo
