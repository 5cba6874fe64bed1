// bbo_lm.hpp -- device-resident LM-CMA-ES: the limited-memory CMA-ES of Loshchilov (2014 / 2015), the
// reference's one member of the CMA family without a matrix: m ~ 2 sqrt(n) direction vectors stand for
// the Cholesky factor, a candidate costs O(m n) and n goes up to 4096.
//
// Reference: LmCmaes (src/multivariate/cma/lm_cmaes.cpp:42-318 over base_cmaes.cpp).  A generation is
//   lm_draw          z of every "+" candidate and the normal of selectSubset   (:94-106, :314)
//   lm_sample        the dots b_j <v_j, z>, the fold az = sqrt(1 - c1) az + dot pc_j slot by slot from
//                    i0, both mirrored rows x = m +- sigma az                   (:108-124, :304-318)
//   lm_eval          the objective on the rows (a host objective takes X instead); fp <- the last
//                    generation's sorted values                                  (:215-226)
//   lm_rank          the std::sort of base_cmaes.cpp:221 (rank by counting, ties to the lower index)
//   lm_update        mean, pc, updateSet, the v vectors of the slots from imin on (ainvz), b, d, the
//                    population success rule of sigma                            (:129-181, :228-302)
//   lm_history_stop  the histories, the counters, the four stop tests            (:183-213, base :191-209)
// Given the same draws that is the reference's arithmetic up to the order of the dot products over n
// and the sigma rule's numerator, an exact integer here (tests/lm_model.py carries both forms;
// DESIGN.md sections 3.10, 4 and 5).
#pragma once

#include "bbo_engine.hpp"

namespace bbo {

constexpr int LM_MAX_N = 4096;
constexpr int LM_MAX_NP = 4096;
constexpr int LM_MAX_M = 256;
// "+" candidates per workgroup of lm_sample: V and P stream in once for all of them
constexpr int LM_BLOCK = 4;
// the stop flag of sigma < 1e-16 (1, 2, 3 are MaxIter, TolHistFun, EqualFunVals as in bbo_cma.hpp; 10
// is taken there by the target value)
constexpr int LM_FLAG_SIGMA = 11;

struct LmScal {
    double sigma, s;
    double fbest, fworst;    // over the history of the best values, once it is full
    int memlen;              // slots in use
    int it, fev;
    int hist_head, hist_len;
    int flag;                // the stop test that fired: 1, 2, 3 or LM_FLAG_SIGMA
    int stop;                // sticky: 1 = converged(), 2 = evaluation budget exhausted
    int conv;                // result of the last stop test
};

struct LmConst {
    int n, ld, lambda, mu, half;     // half = ceil(lambda / 2), the "+" candidates
    int m, t, nsteps, mit, hlen, ik;
    int obj, mfev, honor_stop, npop;
    int usenew, rademacher, bound;
    double tol, cc, cs, c1, ccc, damps, sqrt1mc1, zstar, stolmin;
    uint64_t seed;
};

struct LmDev {
    double *X;               // [P][lambda][ld] candidates
    double *Z;               // [P][half][ld] z of the "+" candidates
    double *g;               // [P][half] the normal of selectSubset
    double *f;               // [P][lambda]
    double *fsort, *fp;      // [P][lambda] this and the last generation's values in rank order
    int *order, *rank;       // [P][lambda] rank -> index, index -> rank
    double *xmean, *xold, *pc;   // [P][ld]
    double *Pm, *Vm;         // [P][m][ld] pcmat, vmat
    double *b, *d;           // [P][m]
    int *jarr, *larr;        // [P][m]
    double *hist_best, *hist_kth;    // [P][hlen]
    const double *w;         // [mu]
    const double *lower, *upper, *aux;
    LmScal *scal;
};

class LmEngine: public Engine<LmScal> {
public:
    static constexpr const char *HANDLE_NAME = "not an LmCMAES handle";
    explicit LmEngine(const bbo_params &p);
    void init(int n, const double *lower, const double *upper, const double *guess,
            const ObjectiveSpec &obj) override;
    void solution(int population, double *x_out, int *n_evals, int *converged) override;
    int get(const std::string &key, int population, double *out, int cap) override;
    int set(const std::string &key, int population, const double *in, int count) override;
    int dimension() const override { return c_.n; }

    // bbo_lm_configure: the constructor arguments bbo_params has no field for
    void configure(const bbo_lm_params &lp);
    // one part of a generation: 0 sample, 1 evaluate, 2 rank, 3 update, 4 history + stop
    void phase(int which);
    // G generations of draws, [G][P][half][n + 1], or null: the device generator
    void inject_draws(const double *table, int count);

private:
    static const bbo_params &checked(const bbo_params &p);
    void generation(bool honor_stop) override;
    void part_sample();
    void part_eval();
    void part_rank();
    void part_update();
    void part_history();

    bbo_lm_params lp_ {};
    LmConst c_ {};
    LmDev d_ {};
    std::vector<double> draws_;         // the injected table
    int draws_gens_ = 0, draws_next_ = 0;
    DevBuf<double> X_, Z_, g_, f_, fsort_, fp_, xmean_, xold_, pc_, Pm_, Vm_, b_, dd_, hist_best_, hist_kth_, w_;
    DevBuf<int> order_, rank_, jarr_, larr_;
};

} // namespace bbo
