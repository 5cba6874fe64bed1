// bbo_pikaia.hpp -- device-resident PIKAIA, the genetic algorithm of Charbonneau & Knapp (HAO, 1995).
//
// Reference: PikaiaSearch (src/multivariate/pikaia/pikaia.cpp:18-593), a C++ translation of the Fortran 77
// code that the reference binds to no Python class.  With irep = 1 (full generational replacement) a
// generation is np / 2 independent matings
//
//   select (:460-472)    two parents by a roulette over the row indices, weights from the ranks; the second
//                        is drawn again until it differs
//   encode (:272-283)    every coordinate of a phenotype in [0, 1) as nd decimal digits, int(ph 10^nd)
//   cross (:298-328)     with probability pcross the digit loci ispl .. ispl2 are exchanged (one- or two-point)
//   mutate (:330-406)    per locus with probability pmut: a fresh digit (imut 1-3), or for imut 4-6 after a
//                        coin +-1 with the carry into the more significant digits of the same gene (creep)
//   decode (:285-296)    ip 10^-nd
//
// followed by newpop (:567-592: elitism, np evaluations, the ranking) and adjmut (:408-434).
//
// A lane owns one coordinate of both children and keeps the gene as the integer it encodes: the digit
// window of the crossover is a div / mod by powers of ten, a creep step adds or subtracts 10^k and clamps
// at 0...0 and 9...9 exactly where the reference's carry loop does.  The draws are keyed by (generation,
// mating, child, purpose, locus), so a mating that is computed again draws the same.
//
// Reproduced by default: the reference maximises over the unit cube; its init stores the value of the last
// row only, in the last slot (:62), so the first generation selects on a ranking of np - 1 tied zeros; a
// generation counts np + 1 evaluations whatever ielite is (:579, :588); the relative fitness difference of
// imut 2 / 5 has a signed denominator (:415-416).  repair = 1 stores every initial value, counts np, keeps the
// stored value of the elite row and divides by |f_best + f_median|.  raw = 0 (the default) hands the
// objective lower + u (upper - lower) and takes -f as the fitness: the reference on the wrapped function.
//
// Ranking is the stable order of bbo_rank.hpp (fitness ascending, ties by row), not rqsort's (:154-250).
// select's running sums (:465) are formed once per generation, left to right, and a mating finds its
// parents by bisection.  If rounding leaves the last sum under the dice, the device takes row np - 1; the
// reference's loop would fall through there and keep the index of the previous call.  The second parent is
// drawn at most PIKAIA_ATTEMPTS times and is then the next row cyclically.
//
// Refused: irep 2 and 3 (the steady-state walk: every child is inserted at once and the next select reads the
// ranks that insertion left), odd np (the reference leaves the last row of the new
// population a zero vector), nd > 9 (int(ph 10^nd) overflows).  No restart base, no multi-GPU sharding.
#pragma once

#include "bbo_engine.hpp"

namespace bbo {

constexpr int PIKAIA_MAX_N = 512;
constexpr int PIKAIA_MAX_NP = 4096;
constexpr int PIKAIA_MAX_ND = 9;
constexpr int PIKAIA_ATTEMPTS = 64;     // draws of the second parent before the cyclic rule

// what a launch of pikaia_newpop does
enum PikaiaNewpopMode {
    PIKAIA_ELITE = 1,        // :574-578 the elite test and copy
    PIKAIA_REST = 2,         // fitness, ranking, adjmut, the running sums, the counters
    PIKAIA_INIT = 4          // the same behind init (:57-68): no elite, no adjmut, fev = np, ig = 1
};

struct PikaiaScal {
    double pmut;             // _pmut
    double fbest;            // the best fitness ever evaluated (the GA's scale: maximised)
    double rdif;             // adjmut's measure of the last generation
    int fev, ig;             // _fev, _ig
    int stop;                // sticky: 1 = ig > ngen (the reference's only stop)
    int conv;                // 1 with it: the reference reports converged = true
    int active;              // the last generation ran in this population
    int elite;               // the last generation replaced new row 0 by the old best
};

struct PikaiaConst {
    int n, ld, np, nd;
    int ngen, imut, ielite;
    int repair, raw;
    int prog;                // the objective is a program: its NaN arrives as +inf
    int obj, honor_stop, npop;
    int sub0;                // population p draws from sub-stream sub0 + p
    int table;               // doubles of a draw table per population
    int zi;                  // 10^nd
    double z, zinv;          // std::pow(10., nd), std::pow(10., -nd) of the host
    double pcross, pmutmn, pmutmx, fdif;
    uint64_t seed;
};

struct PikaiaDev {
    double *ph, *x;          // [P][np][ld] phenotypes in [0, 1) and the points handed to the objective
    double *fitns;           // [P][np] _fitns (maximised)
    double *newph, *newx;    // [P][np][ld] the offspring of the last generation
    double *newf;            // [P][np] their objective values
    double *cum;             // [P][np] select's running sums, by row
    double *best;            // [P][ld] the point of fbest
    int *order, *rank;       // [P][np] rank -> row (ascending fitness), row -> rank
    int *parents;            // [P][np / 2][2]
    int *cross;              // [P][np / 2][2] ispl, ispl2 (1-based, as the reference) or -1, -1
    int *mode;               // [P][np] per child: 1 creep, 0 uniform
    double *draws;           // [P][table] (recording, else null)
    const double *inject;    // [P][table] draws instead of the generator's (else null)
    const double *lower, *upper, *aux;
    PikaiaScal *scal;
};

class PikaiaEngine: public Engine<PikaiaScal> {
public:
    static constexpr const char *HANDLE_NAME = "not a PIKAIA handle";
    explicit PikaiaEngine(const bbo_params &p);
    void init(int n, const double *lower, const double *upper, const double *guess,
            const ObjectiveSpec &obj) override;
    void solution(int population, double *x_out, int *n_evals, int *converged) override;
    int get(const std::string &key, int population, double *out, int cap) override;
    int set(const std::string &key, int population, const double *in, int count) override;
    int dimension() const override { return c_.n; }

    void configure(const bbo_pikaia_params &gp);
    // bbo_pikaia_inject_draws: [P][table_len()]
    void inject_draws(const double *table, int count);

private:
    static const bbo_params &checked(const bbo_params &p);
    void generation(bool honor_stop) override;
    bool budget_spent(const PikaiaScal &s) const override { return s.ig > c_.ngen; }
    void evaluate_new(bool honor_stop, int rows);
    void launch_newpop(int mode);
    void launch_copy();

    bbo_pikaia_params gp_ {};
    PikaiaConst c_ {};
    PikaiaDev d_ {};
    DevBuf<double> ph_, x_, fitns_, newph_, newx_, newf_, cum_, best_;
    DevBuf<int> order_, rank_, parents_, cross_, mode_;
    ProgEval prog_row0_;     // the same program over new row 0 of every population: the elite test's value
    DrawTables tables_;
    bool record_ = false;
};

} // namespace bbo
