// bbo_amalgam.hpp -- device-resident AMaLGaM-IDEA and iAMaLGaM-IDEA (Bosman, Grahl & Thierens 2009):
// an estimation-of-distribution algorithm with a full covariance model, the anticipated mean shift
// and the adaptive variance multiplier.
//
// Reference: Amalgam (src/multivariate/amalgam/amalgam.cpp:42-528).  Per generation it sorts, takes
// the mean and the covariance of the best ss = int(0.35 np) points (scalar loops, O(ss n^2)), factors
// the covariance with LINPACK's dchdc (O(n^3)), samples np points (O(np n^2)) and adapts the
// multiplier.  The kernels of a generation: bbo_amalgam_kernels.hpp.
// The rows stay where they were sampled: row m of a generation is the m-th point the reference
// samples, i.e. its sorted row m, and order[] carries the ranking.
#pragma once

#include "bbo_engine.hpp"

namespace bbo {

constexpr int AMALGAM_MAX_N = 512;
constexpr int AMALGAM_MAX_NP = 65536;
constexpr int AMALGAM_SLAB = 256;            // ranked rows per slab of the Gram's K dimension
constexpr int AMALGAM_LDS_MAX_LD = 128;      // the factorisation keeps the matrix in LDS up to here

struct AmalgamScal {
    double cmult;
    double sdr;              // the last standard-deviation ratio (0 in a generation without improvement)
    double fbest;            // the best value ever evaluated (an extension: solution() is the reference's)
    double felite;           // the value row 0 carries through the sampler
    int nis, t, it, fev, gen;
    int stop;                // sticky: 1 = cmult < 1e-10 or var(f) <= stol^2, 2 = evaluation budget
    int conv;                // converged() after the last generation
    int fact_fail;           // factorisations that ended at a non-positive pivot
    int fail_at;             // the step of the last one, n if it ran through
    int pad;
};

struct AmalgamConst {
    int n, ld, np, ss, nams, nismax;
    int obj, mfev, honor_stop, npop;
    int slabs;               // ceil(ss / AMALGAM_SLAB)
    int lds_factor;          // the factorisation runs in LDS (ld <= 128)
    int keep_elite;
    int kb;                  // shuffle_key_bits(np - 1)
    int sub0;                // the sub-stream of population 0 (population p draws from sub0 + p)
    double etasigma, etashift, stol;
    uint64_t seed;
};

struct AmalgamDev {
    double *X;               // [P][np][ld] in sampling order
    double *Z;               // [P][np][ld] the normals of the last generation
    double *f;               // [P][np]
    double *mu, *muold, *mushift, *xelite, *xbest;   // [P][ld]
    double *cov, *chol;      // [P][ld][ld] (chol: lower triangular, scaled by sqrt(cmult))
    double *part;            // [P][slabs][ld][ld] the Gram's slabs
    const double *zin;       // [P][np][ld] injected normals of this generation, else null
    const int *shin;         // [P][np] 1: a row the injected table shifts in this generation, else null
    int *shifted;            // [P][np] 1: the row took the anticipated mean shift
    int *order, *rank;       // [P][np] rank -> row, row -> rank
    const double *lower, *upper, *aux;
    const uint64_t *lane_seed;
    AmalgamScal *scal;
};

// the outcome of one stage of the parameter-free driver: a row of the reference's table
struct AmalgamStage {
    int s, runs, np;
    double fbestrun, fbest;
    int fev;
};

class AmalgamEngine: public Engine<AmalgamScal> {
public:
    static constexpr const char *HANDLE_NAME = "not an AMALGAM handle";
    explicit AmalgamEngine(const bbo_params &p);
    void init(int n, const double *lower, const double *upper, const double *guess,
            const ObjectiveSpec &obj) override;
    void iterate() override;
    int run(int max_generations) override;
    void optimize(int n, const double *lower, const double *upper, const double *guess, const ObjectiveSpec &obj,
            double *x_out, int *n_evals, int *converged) override;
    void solution(int population, double *x_out, int *n_evals, int *converged) override;
    int get(const std::string &key, int population, double *out, int cap) override;
    int set(const std::string &key, int population, const double *in, int count) override;
    int dimension() const override { return c_.n; }

    void configure(const bbo_amalgam_params &ap);
    // one part of a generation: 0 distribution, 1 sample + evaluate, 2 adapt + stop
    void phase(int which);
    // the draws of the next G generations: the normals [G][P][np][n] and the shifted rows [G][P][nams]
    void inject_draws(const double *z, int zcount, const int *rows, int rcount);
    // the initial points [P][np][n] of the next bbo_init
    void inject_points(const double *x, int count);

private:
    static const bbo_params &checked(const bbo_params &p);
    void generation(bool honor_stop) override;
    // optimize() iterates before it tests (:246-255): a fresh population takes one generation whatever mfev
    bool budget_spent(const AmalgamScal &s) const override { return s.it > 0 && s.fev >= params_.mfev; }
    void part_distribution();
    void part_sample();
    void part_adapt();
    void launch_rank();
    // ---- the parameter-free driver (:72-98, :180-203, :257-288) ----
    bool driver() const { return ap_.noparam != 0; }
    void driver_init(int n, const double *lower, const double *upper, const ObjectiveSpec &obj);
    void driver_stage();
    bool driver_converged() const;
    double evaluate_point(const double *x);

    bbo_amalgam_params ap_ {};
    AmalgamConst c_ {};
    AmalgamDev d_ {};
    int sub0_ = 0;
    int zin_gens_ = 0, zin_pos_ = 0;
    std::vector<double> xin_;
    DevBuf<double> X_, Z_, f_, mu_, muold_, mushift_, xelite_, xbest_, cov_, chol_, part_, zin_;
    DevBuf<int> shin_, shifted_, order_, rank_, ident_;
    DevBuf<uint64_t> lane_seed_;
    // driver state
    int dn_ = 0, nbase_ = 0, s_ = 0, budget_ = 0, dfev_ = 0;
    double dfbest_ = 0., dfbestrun_ = 0., dfbestrunold_ = 0.;
    std::vector<double> dbest_, dlower_, dupper_;
    std::vector<AmalgamStage> stages_;
};

} // namespace bbo
