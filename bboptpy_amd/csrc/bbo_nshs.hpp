// bbo_nshs.hpp -- device-resident NSHS: the novel self-adaptive harmony search (Luo 2013).
//
// Reference: NSHS (src/multivariate/harmony/nshs.cpp:46-181).  The algorithm is steady-state: one
// iteration improvises ONE candidate coordinate by coordinate (:112-147), evaluates it (:150) and
// overwrites the worst of the hms rows of the harmony memory when it is strictly better
// (:154-170).  A generation-per-launch engine would pay its launches for one evaluation per
// population, so the hot path is
//   nshs_steps      one workgroup per population, K whole iterations per launch; a small harmony
//                   memory and its values in LDS (read from HBM once per launch, accepted rows
//                   written through), a larger one gathered from global memory
// and the iteration also exists in three parts, the path of bbo_iterate, bbo_nshs_phase and a host
// objective:
//   nshs_generate   the candidate (:112-147)
//   nshs_eval       its value (:150)
//   nshs_replace    the replacement (:157-162), fstd, best and worst (:165-169), counters, budget
// Given the same uniforms the candidate's coordinates are the reference's bit for bit; f differs by
// summation order, fstd by its two-pass tree form, which enters the
// algorithm through the comparison fstd > fstdmin alone.
#pragma once

#include "bbo_engine.hpp"

namespace bbo {

// diagnostic switches: the bits of NshsConst::dbg (bbo_set "dbg", 0 in production)
enum NshsDbg { NSHS_DBG_GLOBAL_HM = 1 };     // nshs_steps gathers the harmony memory from global memory

// nshs_steps keeps the harmony memory in LDS while hms * ld * 8 bytes fit this budget.  The kernel is
// a latency chain that only occupancy hides, and its registers allow 16 wavefronts on a CU: the
// budget is what 16 resident workgroups leave each of the CU's 160 KiB next to the candidate and the
// box.  A larger memory is gathered from global memory, which costs a single resident workgroup 5 %
// and a full device nothing (measured with 32 KiB: DESIGN.md section 3.9).  The kernel allocates
// what the shape needs, not the budget.
constexpr int NSHS_LDS_BYTES = 6144;
constexpr int NSHS_MAX_N = 512;
constexpr int NSHS_MAX_HMS = 4096;
constexpr int NSHS_DEFAULT_CHUNK = 256;  // iterations per launch of bbo_run

struct NshsScal {
    double fbest;            // the first minimum of f
    double fworst;           // the first maximum of f: what the next candidate has to beat
    double fstd;             // sqrt(sum (f - mean)^2 / hms), two-pass tree form
    int ibest, iworst;
    int wide;                // fstd > fstdmin: the branch of the NEXT iteration (:122, :136)
    int accepted;            // the last candidate replaced the worst row
    int it;                  // iterations done: the counter word of the draws
    int fev;
    int stop;                // sticky: 2 = evaluation budget exhausted (there is no 1)
    int conv;                // always 0: the reference never converges (:100, :109)
};

struct NshsConst {
    int n, ld, hms;
    int obj, mfev, mit, honor_stop, npop;
    int record;              // keep the four raw uniforms of every coordinate
    int dbg;                 // NshsDbg bits
    double fstdmin, hmcr, tunerange;
    uint64_t seed;
};

struct NshsDev {
    double *X;               // [P][hms][ld] the harmony memory
    double *f;               // [P][hms]
    double *cand;            // [P][ld] the last candidate
    double *fcand;           // [P]
    double *draws;           // [P][n][4] (recording, else null)
    const double *inject;    // [P][n][4] raw uniforms instead of the generator's (else null)
    const double *lower, *upper, *aux;
    NshsScal *scal;
};

class NshsEngine: public Engine<NshsScal> {
public:
    static constexpr const char *HANDLE_NAME = "not an NSHS handle";
    explicit NshsEngine(const bbo_params &p);
    void init(int n, const double *lower, const double *upper, const double *guess,
            const ObjectiveSpec &obj) override;
    void iterate() override;
    void solution(int population, double *x_out, int *n_evals, int *converged) override;
    int get(const std::string &key, int population, double *out, int cap) override;
    int set(const std::string &key, int population, const double *in, int count) override;
    int dimension() const override { return c_.n; }

    // bbo_nshs_configure: the constructor argument bbo_params has no field for
    void configure(const bbo_nshs_params &np);
    // bbo_nshs_phase: 0 generate, 1 evaluate, 2 replace
    void phase(int which);
    // bbo_nshs_inject_uniforms: [P][n][4] (the coin, the row, the fresh value, the adjustment)
    void inject_uniforms(const double *u, int count);

private:
    static const bbo_params &checked(const bbo_params &p);
    void generation(bool honor_stop) override;
    void launch_chunk(int gens) override;
    int default_poll() const override { return NSHS_DEFAULT_CHUNK; }
    void require_iterations(const char *call) const;
    void launch_init(int p0, int pcount, int mode);
    void launch_generate();
    void launch_eval();
    void launch_replace();
    void launch_steps(int k);
    bool hm_in_lds() const;
    int workgroup() const;

    bbo_nshs_params np_ {};
    NshsConst c_ {};
    NshsDev d_ {};
    DevBuf<double> X_, f_, cand_, fcand_;
    DrawTables tables_;      // [P][n][4] uniforms: the injected table and the recorded one
    int wg_ = 0;             // bbo_set "wg": 0 = by n, else 64, 128 or 256 threads for nshs_steps
};

} // namespace bbo
