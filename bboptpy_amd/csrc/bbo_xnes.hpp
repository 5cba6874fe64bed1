// bbo_xnes.hpp -- device-resident xNES: the exponential natural evolution strategy (Glasmachers,
// Schaul, Yi, Wierstra & Schmidhuber 2010), the reference's rank-based relative of CMA-ES that
// updates a factor B of the covariance multiplicatively, B <- B exp(1/2 eta_B G_B).
//
// Reference: xNES (src/multivariate/nes/xnes.cpp:43-253).  Per generation it forms the dense n x n
// gradient G, diagonalises it (tred2 / tql2) and multiplies twice, O(n^3), for np = 4 + int(3 ln n)
// evaluations.  G has rank <= np: with the ranked normals Z (np x n), U = diag(u), sum u = 0,
//     G_B = Z^T U Z - G_sigma I,   G_sigma = sum_i u_i |z_i|^2 / n
// and with K = Z Z^T = L L^T, S = L^T U L = W Lambda W^T, T = L^-T W, c = eta_B / 2
//     B exp(c G_B) = e^{-c G_sigma} (B + Y^T H Z),   H = T (e^{c Lambda} - 1) T^T   (np x np)
// where the rows of Y = Z B^T are what the sampler has just computed.  Here a generation is
//   xnes_draw     the rows of Z (xnes_settle: the slow ziggurat draws; xnes_take: injected rows)  (:113-116)
//   xnes_points   Y = Z B^T, x = mu + sigma y, the objective                                      (:117-123)
//   xnes_rank     the std::sort of :128 (by counting, ties to the lower index)
//   xnes_step     mu, G_sigma, sigma, the counters and the stop test; then the update operator:
//                 low-rank (n >= lowrank_min_n) H and Q = H Z, or dense (smaller n, where np may
//                 exceed n and K is singular) E = exp(c G_B) through a Jacobi eigensolver          (:131-179)
//   xnes_adapt    B <- e^{-c G_sigma} (B + Y^T Q), or B <- B E                                     (:180-190)
// O(np n^2), no n x n eigenproblem (tests/xnes_model.py carries both forms).
#pragma once

#include "bbo_engine.hpp"

namespace bbo {

constexpr int XNES_MAX_N = 512;
constexpr int XNES_MAX_NP = 22;              // 4 + int(3 ln 512)
constexpr int XNES_NPP = 24;                 // np padded to whole steps of four (the K of the matrix pipe)
constexpr int XNES_EIG_MAX = 32;             // the eigensolver of xnes_step: np x np or n x n, n <= 31
constexpr int XNES_EIG_LD = 33;
// the low-rank route from this n on (settable as "lowrank_min_n" in [16, 32]): n / np > 2 there
constexpr int XNES_LOWRANK_MIN_N = 32;
// Y = Z B^T and the low-rank update of B go through the fp64 matrix instruction from here on
constexpr int XNES_MFMA_MIN_N = 16;

struct XnesScal {
    double sigma;
    double gsigma;           // G_sigma of the last generation
    double escale;           // e^{-c G_sigma}: the factor of xnes_adapt's low-rank form
    double fbest;            // the best value ever seen (an extension: solution() is the reference's)
    int it, fev, gen;
    int stop;                // sticky: 1 = converged(), 2 = evaluation budget exhausted
    int conv;                // result of the last stop test
    int skip;                // the last generation left B untouched (the Cholesky factorisation failed)
    int fact_fail;           // how often that happened
    int pad;
};

struct XnesConst {
    int n, ld, np;
    int obj, mfev, honor_stop, npop;
    int lowrank;             // the route of xnes_step / xnes_adapt: 1 low-rank, 0 dense
    double tol, etamu, etasigma, etab;
    uint64_t seed;
};

struct XnesDev {
    double *B;               // [P][n][ld]
    double *mu, *xbest;      // [P][ld]
    double *Z, *Y, *X, *Q;   // [P][np][ld] in sampling order; Q = H Z (low-rank route)
    double *f;               // [P][np]
    double *E;               // [P][32][32] exp(c G_B) (dense route)
    const double *u;         // [np] the utilities by rank
    const double *zin;       // [P][np][ld] injected normals of this generation, else null
    int *order, *rank;       // [P][np] rank -> index, index -> rank
    const double *aux;
    const uint64_t *lane_seed;   // [64] the seed once per lane (see hees_settle)
    XnesScal *scal;
};

class XnesEngine: public Engine<XnesScal> {
public:
    static constexpr const char *HANDLE_NAME = "not an xNES handle";
    explicit XnesEngine(const bbo_params &p);
    void init(int n, const double *lower, const double *upper, const double *guess,
            const ObjectiveSpec &obj) override;
    void solution(int population, double *x_out, int *n_evals, int *converged) override;
    int get(const std::string &key, int population, double *out, int cap) override;
    int set(const std::string &key, int population, const double *in, int count) override;
    int dimension() const override { return c_.n; }

    // bbo_xnes_configure: the constructor arguments bbo_params has no field for
    void configure(const bbo_xnes_params &xp);
    // one part of a generation: 0 sample + evaluate, 1 rank, 2 small step, 3 adapt
    void phase(int which);
    // the normals of the next G generations, [G][P][np][n], or null
    void inject_normals(const double *z, int count);

private:
    static const bbo_params &checked(const bbo_params &p);
    void generation(bool honor_stop) override;
    void part_sample();
    void part_rank();
    void part_step();
    void part_adapt();

    bbo_xnes_params xp_ {};
    XnesConst c_ {};
    XnesDev d_ {};
    int lowrank_min_n_ = XNES_LOWRANK_MIN_N;
    int zin_gens_ = 0, zin_pos_ = 0;    // injected generations, and how many of them are consumed
    DevBuf<double> B_, mu_, xbest_, Z_, Y_, X_, Q_, f_, E_, u_, zin_;
    DevBuf<int> order_, rank_;
    DevBuf<uint64_t> lane_seed_;
};

} // namespace bbo
