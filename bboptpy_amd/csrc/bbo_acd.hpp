// bbo_acd.hpp -- device-resident ACD: adaptive coordinate descent (Loshchilov, Schoenauer & Sebag 2011).
//
// Reference: ACD (src/multivariate/acd/acd.cpp:54-334).  A coordinate search along the columns of B:
// iterate() (:122-178) forms x1, x2 = clamp(xbest -+ sigma[ix] B[:, ix]), evaluates both, lets each replace
// xbest in turn, scales sigma[ix], stores both points in the archive and moves on to the next coordinate.
// Behind the last coordinate of a sweep that improved, the archive of 2 n points is ranked and updateAE()
// (:236-334) runs: the mean of the n best, the path p, C = (1 - c1) C + c1 p p^T, the symmetric
// eigendecomposition of C with its two repairs, B = V diag(d), invB = diag(1 / d) V^T.
//
//   acd_sweep   one workgroup per population, two wavefronts: one forms and evaluates x1, the other x2.
//               Resumable after every coordinate step; it ends at the population's goal, at the end of the
//               sweep, at a stop rule or the budget, and where an update is due (it raises `due` there and
//               leaves the stop test of that step to acd_post, because converged() reads the new B).
//   acd_ae      one workgroup per due population: the stable ranking of the archive, m, mold, artmp, denom,
//               p and C as sequential chains in the reference's order (bit for bit), and the symmetric
//               copy of C's lower triangle the eigensolver reads (tred2 reads the lower triangle only).
//   (decomposition)  the project's one-workgroup eigensolver over a CmaDev / CmaConst view of that copy
//               (launch_eigen_view, bbo_cma.hip); its repair is ACD's (bbo_eig.hpp against acd.cpp:299-315).
//   acd_post    B, invB, diagd, the shifted diagonal of C, colmax; clears improved and due; the stop test.
//
// B is stored transposed (column ix contiguous) and so is invB (lane i walks row i of invB coalesced).
// fhist is the reference's ring of cp = 10 + int(20 n^1.5) doubles per population in HBM.
// Objective programs are refused at bbo_init; ACD is no restart base and has no multi-GPU sharding.
#pragma once

#include "bbo_engine.hpp"

namespace bbo {

struct CmaDev;
struct CmaConst;
struct CmaScal;
// bbo_cma.hip: the one-workgroup decomposition (n <= 128) of every matrix of the view whose CmaScal says
// fev - eigenlastev > eigenfreq, and the doubles of eig_work one matrix needs
void launch_eigen_view(hipStream_t stream, const CmaDev &d, const CmaConst &c);
size_t eigen_view_scratch(int ld);

constexpr int ACD_MAX_N = 128;
constexpr int ACD_THREADS = 128;     // acd_sweep, acd_ae, acd_post: two wavefronts

// what a launch of acd_sweep does
enum AcdMode {
    ACD_FUSED = 0,           // whole steps, the evaluations inside
    ACD_ADVANCE,             // forms x1 and x2 of the next step (phase 0)
    ACD_ABSORB               // takes their values and completes the step (phase 2)
};

// AcdScal::due
enum AcdDue {
    ACD_DUE_NONE = 0,
    ACD_DUE_AE,              // the sweep ended improved: acd_ae has to run
    ACD_DUE_POST,            // acd_ae has run, no decomposition (the first update): acd_post closes the step
    ACD_DUE_EIG              // acd_ae has run and asked for the decomposition
};

struct AcdScal {
    double fbest;
    int fev;
    int it, itae, ix;
    int improved;
    int due;                 // AcdDue
    int goal;                // the step count the current bbo_run chunk / bbo_iterate ends at
    int stop;                // sticky: 1 = converged(), 2 = budget
    int conv;                // converged() after the last step
    int rule;                // which rule: 1 = ftol over the history, 2 = xtol
    int pending;             // x1 and x2 await their values (host objective, bbo_acd_phase)
};

struct AcdConst {
    int n, ld;
    int obj, mfev, honor_stop, npop;
    int cp;                  // _convergeperiod
    double ftol, xtol, ksucc, kunsucc;
    double c1, cpath;        // 0.5 / n, 1 / sqrt(n)
    uint64_t seed;
};

struct AcdDev {
    double *xbest, *sigma, *p, *m, *mold, *diagd, *colmax;   // [P][ld]
    double *Bt;              // [P][ld][ld]  Bt[j][i] = B[i][j]
    double *invBt;           // [P][ld][ld]  invBt[j][i] = invB[i][j]
    double *C;               // [P][ld][ld]  row-major, every element as the reference computes it
    double *Cw;              // [P][ld][ld]  the lower triangle of C mirrored: the eigensolver's matrix
    double *V;               // [P][ld][ld]  its eigenvectors in columns
    double *Dv;              // [P][ld]      the roots of its eigenvalues, ascending
    double *X;               // [P][2 n][ld] the archive
    double *f;               // [P][2 n]
    int *order;              // [P][2 n]
    double *fhist;           // [P][cp]
    double *cand;            // [P][2][ld]   x1, x2
    double *value;           // [P][2]       f1, f2 (bbo_acd_phase 1)
    int *flags;              // [2] some population ended the launch short of its goal; some update is due
    CmaScal *eigscal;        // [P] the eigensolver's view: fev - eigenlastev says whether a matrix is due
    const double *lower, *upper, *aux;
    AcdScal *scal;
};

class AcdEngine: public Engine<AcdScal> {
public:
    static constexpr const char *HANDLE_NAME = "not an ACD handle";
    explicit AcdEngine(const bbo_params &p);
    ~AcdEngine() override;
    void init(int n, const double *lower, const double *upper, const double *guess,
            const ObjectiveSpec &obj) override;
    void solution(int population, double *x_out, int *n_evals, int *converged) override;
    int get(const std::string &key, int population, double *out, int cap) override;
    int set(const std::string &key, int population, const double *in, int count) override;
    int dimension() const override { return c_.n; }

    void configure(const bbo_acd_params &ap);
    // bbo_acd_phase: 0 form x1 and x2, 1 evaluate, 2 absorb (and update where due)
    void phase(int which);

private:
    struct EigView;          // CmaDev + CmaConst + the buffers behind them (bbo_acd.hip)
    static const bbo_params &checked(const bbo_params &p);
    void generation(bool honor_stop) override;
    void launch_chunk(int gens) override;
    int default_poll() const override { return c_.n; }
    void launch_sweep(int mode, int k, bool begin);
    void launch_eval();
    void launch_update();
    void fused(int k);
    void draw_xbest(uint32_t sub, double *x) const;
    int converged_now(int p, const AcdScal &s, int *rule) const;

    bbo_acd_params ap_ {};
    AcdConst c_ {};
    AcdDev d_ {};
    std::unique_ptr<EigView> eig_;
    DevBuf<double> xbest_, sigma_, p_, m_, mold_, diagd_, colmax_, Bt_, invBt_, C_, X_, f_, fhist_, cand_, value_;
    DevBuf<int> order_, flags_;
};

} // namespace bbo
