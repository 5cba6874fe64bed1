// bbo_mayfly.hpp -- device-resident mayfly optimizer (Zervoudakis & Tsafarakis 2020, with the PGB-IMA switch).
//
// Reference: MayflySearch (src/multivariate/mayfly/mayfly.cpp:63-428), a class the reference does not bind to
// Python (its binding is commented away at py/multivariate_py.cpp:236-246).  A generation is
//
//   females (:168-180)   female j reads male j as the last selection left it: attraction a3 exp(-beta r) or,
//                        when the male is no better, a random flight of scale fl; clamp, move, evaluate
//   males (:183-199)     attraction to the own best and to `best` (a1, a2) or, at or below fbest, the nuptial
//                        dance; male j + 1 reads the best and fbest that male j has just written
//   mating (:202-221)    both swarms sorted by f, pair j -> two offspring, evaluated off1, off2
//   mutation (:224-239)  the offspring shuffled, the first nmut each copied into a mutated fly with
//                        ceil(pmutdim n) genes displaced by sigma (up - lo) N(0, 1); the mutated flies shuffled
//   selection (:241-275) males + half the offspring + half the mutated flies sorted, the best np copied into
//                        the male slots IN PLACE while later entries still point at slots already
//                        overwritten; the same for the females with the other halves
//   schedule (:277-281)  g, dance, fl
//
// Every part but the male loop is parallel over the individuals.  The male loop is run as prefix-commit
// rounds: a workgroup forms and evaluates the next `window` males against the current best, commits them up
// to and including the first that improves fbest and redoes the rest.  The draws
// are keyed by (generation, swarm, individual, coordinate), so a male that is redone draws the same.
//
// The in-place selection is reproduced by resolving, per slot, the record that finally lands in it (a chain
// over integers); the rows themselves are copied from the untouched swarm into its second buffer.
// repair = 1 selects from untouched copies, as the paper does.  Odd np (the reference leaves one offspring
// unwritten: a zero vector of value 0 that wins the selection), np < 2 and mfev <= 2 np (itmax <= 0, g = 0/0)
// are refused.  Objective programs are refused at bbo_init; no restart base, no multi-GPU sharding.
#pragma once

#include "bbo_engine.hpp"

namespace bbo {

constexpr int MAYFLY_MAX_N = 512;
constexpr int MAYFLY_MAX_NP = 4096;
constexpr int MAYFLY_WG = 256;              // threads of mayfly_males: four wavefronts
constexpr int MAYFLY_DEFAULT_WINDOW = 4;    // males formed per round: the wavefronts of the workgroup

// what a launch of mayfly_males does
enum MayflyMaleMode {
    MAYFLY_FUSED = 0,        // the whole loop, the evaluations inside
    MAYFLY_FORM,             // host objective: form male `jm` into candidate slot 0
    MAYFLY_ABSORB            // host objective: commit male `jm` with the value in candf
};

struct MayflyScal {
    double fbest;
    double g, dance, fl;     // _g, _dance, _fl
    int fev, it, itmax;
    int stop;                // sticky: 2 = budget (the reference has no convergence test)
    int conv;                // always 0
    int active;              // this generation runs in this population (set by its first kernel)
    int took;                // the evaluation of the last generation that took fbest last (-1: none):
                             // females 0 .. np - 1, males np .., offspring 2 np .., mutated flies 3 np ..
    int jm;                  // the male cursor of a host-driven loop
    int dropped;             // speculative male evaluations discarded so far
    int rounds;              // prefix-commit rounds so far
};

struct MayflyConst {
    int n, ld, np;
    int nmut;                // _nmut
    int nmd;                 // genes displaced per mutated fly: ceil(pmutdim n)
    int cm;                  // records of a selection: np + np / 2 + nmut / 2
    int obj, mfev, honor_stop, npop;
    int pgb, repair;
    int sub0;                // population p draws from sub-stream sub0 + p
    int window;              // males per round (np: all remaining)
    int kb_np, kb_nmut, kb_n;    // key widths of the keyed permutations
    int table;               // doubles of a draw table per population
    double a1, a2, a3, beta, ddamp, fldamp, gmin, gmax, vdamp, sigma, l;
    uint64_t seed;
};

struct MayflyDev {
    double *MX, *MV, *MBX;   // [P][np][ld] males
    double *Mf, *Mbf;        // [P][np]
    double *FX, *FV;         // [P][np][ld] females
    double *Ff;              // [P][np]
    double *MX2, *MV2, *MBX2, *Mf2, *Mbf2, *FX2, *FV2, *Ff2;   // the selection's target: the other buffer
    double *OX, *Of;         // [P][np][ld], [P][np] offspring (v = 0, bx = x, bf = f)
    double *UX, *Uf;         // [P][nmut][ld], [P][nmut] mutated flies
    double *best;            // [P][ld]
    double *candx, *candv;   // [P][window][ld] the males of a round
    double *candf;           // [P][window]
    double *keys;            // [P][2][cm] the values a selection sorts
    int *ordm, *ordf;        // [P][np] rank -> row
    int *ordt;               // [P][2][cm] rank -> record of a selection
    int *srcm, *srcf;        // [P][np] the record that lands in slot j
    int *permo, *permu;      // [P][np], [P][nmut] shuffled place -> offspring / mutated fly
    int *brm, *brf;          // [P][np] 1: the attraction form, 0: the random one
    double *draws;           // [P][table] (recording, else null)
    const double *inject;    // [P][table] draws instead of the generator's (else null)
    const double *lower, *upper, *aux;
    MayflyScal *scal;
};

class MayflyEngine: public Engine<MayflyScal> {
public:
    static constexpr const char *HANDLE_NAME = "not a Mayfly handle";
    explicit MayflyEngine(const bbo_params &p);
    void init(int n, const double *lower, const double *upper, const double *guess,
            const ObjectiveSpec &obj) override;
    void solution(int population, double *x_out, int *n_evals, int *converged) override;
    int get(const std::string &key, int population, double *out, int cap) override;
    int set(const std::string &key, int population, const double *in, int count) override;
    int dimension() const override { return c_.n; }

    void configure(const bbo_mayfly_params &mp);
    // bbo_mayfly_inject_draws: [P][table_len()]
    void inject_draws(const double *table, int count);

private:
    static const bbo_params &checked(const bbo_params &p);
    void generation(bool honor_stop) override;
    void host_evaluate_init();
    void host_male_loop(bool honor_stop);
    void launch_rank(int which, int count);
    void alloc_window();
    void bind();

    bbo_mayfly_params mp_ {};
    MayflyConst c_ {};
    MayflyDev d_ {};
    DevBuf<double> MX_[2], MV_[2], MBX_[2], Mf_[2], Mbf_[2], FX_[2], FV_[2], Ff_[2];
    DevBuf<double> OX_, Of_, UX_, Uf_, best_, candx_, candv_, candf_, keys_;
    DevBuf<int> ordm_, ordf_, ordt_, srcm_, srcf_, permo_, permu_, brm_, brf_;
    DrawTables tables_;
    int cur_ = 0;            // the buffer that holds the swarms
    int window_ = MAYFLY_DEFAULT_WINDOW;    // bbo_set "window": 0 = all remaining males
    bool record_ = false;
};

} // namespace bbo
