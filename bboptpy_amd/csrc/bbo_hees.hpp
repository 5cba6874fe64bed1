// bbo_hees.hpp -- device-resident HEES: the Hessian Estimation Evolution Strategy (Glasmachers &
// Krause 2020), the reference's one strategy that learns its metric from curvature, not from ranks.
//
// Reference: Hees (src/multivariate/hees/hees.cpp:39-382).  Per generation it draws B n normal
// rows (B = ceil(mu / n)), orthonormalises every batch of n, forms G = (1/B) sum_i c_i b^_i b^_i^T
// over all of them and multiplies A by it -- O(n^3) for 2 mu + 1 evaluations.  Every batch is a
// complete orthonormal basis and c_i = 1 for the rows i >= mu, so
//     A G = A + (1/B) sum_{i < mu} (q_i - 1) / |z_i|^2  (A b_i) b_i^T
// and A b_i is the row y_i the sampler has just computed; row i of a batch depends only on the rows
// before it, so only the first mu rows are ever drawn.  Here a generation is
//   hees_draw     rows r < mu of Z (hees_settle: the slow ziggurat draws, the norms)  (:203-209)
//   hees_ortho    modified Gram-Schmidt per batch, rescaled to |z_r|                  (:211-229)
//   hees_points   Y = b A^T, the objective on m -+ sigma y                            (:231-249)
//   hees_rank     the two std::sorts of :251-259 (rank by counting, ties to the lower index)
//   hees_update   h, q, the weights' differences, m, p_s, g_s, sigma                  (:262-292, :324-364)
//   hees_adapt    A += Y^T diag((q - 1) / (|z|^2 B)) b                                (:294-321)
//   hees_finish   f(m), the incumbent, the counters, converged()                      (:332-340, :366-382)
// O(mu n^2).  Given the same normals that is the reference's arithmetic up to the order of a few
// sums (tests/hees_model.py carries both forms; DESIGN.md sections 3.7, 4 and 5).
#pragma once

#include "bbo_engine.hpp"

namespace bbo {

constexpr int HEES_MAX_N = 512;
constexpr int HEES_MAX_MU = 4096;
// the rows of a batch live in LDS up to this many bytes (beside hees_ortho's 4 KiB of scratch)
constexpr int HEES_ORTHO_LDS = 128 * 1024;
// Y = b A^T and the update of A go through the fp64 matrix instruction from here on: at least one
// whole tile of 16 coordinates and half a tile of rows
constexpr int HEES_MFMA_MIN_N = 16, HEES_MFMA_MIN_MU = 8;

struct HeesScal {
    double sigma, gs;
    double fm;               // f at the mean
    double fbest;            // the best mean so far (hees.cpp:336-339: not the best sample)
    double maxh;             // the largest curvature estimate of the last generation
    double m2;               // spread of the 2 mu values in the last stop test
    double sigma_prev;       // sigma the last candidates were sampled with (get "arx")
    int it, fev, gen;
    int stop;                // sticky: 1 = converged(), 2 = evaluation budget exhausted
    int conv;                // result of the last stop test
    int skip;                // the last generation left A untouched (max h <= 0)
};

struct HeesConst {
    int n, ld, mu, B;
    int obj, mfev, honor_stop, npop;
    int ortho_global;        // 1: hees_ortho keeps its rows in global memory whatever the shape
    int force_fma;           // 1: hees_points / hees_adapt in their plain forms whatever the shape
    double tol, cs, ds, chi, csc, kappa, etaA;
    uint64_t seed;
};

struct HeesDev {
    double *A;               // [P][n][ld]
    double *m, *mprev, *ps, *xbest;     // [P][ld]
    double *b;               // [P][mu][ld] the normals, then the orthogonalised rows
    double *norms;           // [P][mu] |z_r|
    double *Y;               // [P][mu][ld] rows A b_r
    double *X;               // [P][2 mu][ld] candidates (host objective, else null)
    double *f;               // [P][2 mu]
    double *fmh;             // [P] f(m) from a host objective
    double *hess, *q, *coef, *dw;       // [P][mu]
    const double *w;         // [2 mu] the weights by rank
    const double *zin;       // [P][mu][ld] injected normals, else null
    double *zlast;           // [P][mu][ld] the normals of the last generation (recording, else null)
    int *order, *rank;       // [P][2 mu] rank -> index, index -> rank
    const double *aux;
    const uint64_t *lane_seed;   // [64] the seed once per lane
    HeesScal *scal;
};

class HeesEngine: public Engine<HeesScal> {
public:
    static constexpr const char *HANDLE_NAME = "not a HEES handle";
    explicit HeesEngine(const bbo_params &p);
    void init(int n, const double *lower, const double *upper, const double *guess,
            const ObjectiveSpec &obj) override;
    void optimize(int n, const double *lower, const double *upper, const double *guess,
            const ObjectiveSpec &obj, double *x_out, int *n_evals, int *converged) override;
    void solution(int population, double *x_out, int *n_evals, int *converged) override;
    int get(const std::string &key, int population, double *out, int cap) override;
    int set(const std::string &key, int population, const double *in, int count) override;
    int dimension() const override { return c_.n; }

    // bbo_hees_configure: the constructor arguments bbo_params has no field for
    void configure(const bbo_hees_params &hp);
    // one part of a generation: 0 sample + evaluate, 1 rank, 2 update, 3 finish
    void phase(int which);
    // the normals of the next generations (P tables of B n x n, the reference's), or null
    void inject_normals(const double *z, int count);

private:
    static const bbo_params &checked(const bbo_params &p);
    void generation(bool honor_stop) override;
    void part_sample();
    void part_rank();
    void part_update();
    void part_finish(bool init_only);
    void host_mean();
    bool use_mfma() const { return !c_.force_fma && c_.n >= HEES_MFMA_MIN_N && c_.mu >= HEES_MFMA_MIN_MU; }

    bbo_hees_params hp_ {};
    HeesConst c_ {};
    HeesDev d_ {};
    bool record_ = false;
    bool sampled_ = false;              // candidates are out whose generation has not been updated yet
    std::vector<double> runs_;          // optimize() with mres > 1: (mu, fev, fbest) of every run
    DevBuf<double> A_, m_, mprev_, ps_, xbest_, b_, norms_, Y_, X_, f_, fmh_, hess_, q_, coef_, dw_, w_,
            zin_, zlast_;
    DevBuf<int> order_, rank_;
    DevBuf<uint64_t> lane_seed_;
};

} // namespace bbo
