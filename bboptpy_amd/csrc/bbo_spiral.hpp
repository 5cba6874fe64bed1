// bbo_spiral.hpp -- device-resident SpiralSearch: the adaptive spiral optimization algorithm
// (Tamura & Yasuda 2011; Yuzgec & Inac 2016).
//
// Reference: SpiralSearch (src/multivariate/spiral/spiral.cpp:46-190).  Its generation is synchronous
// by construction: every point is rotated about the generation's best point by its own angle and
// contracted by its own factor (:111-135), all points are evaluated, the best is chosen (:138-148).
// Here a generation is
//   spiral_draw     the two coins of every point and its new r / theta (:111-118); cos and sin of
//                   the angles that changed (:124-125)
//   spiral_rotate   the composite rotation rotate_n (:184-190) of x_i - xbest, one lane per point,
//                   and x_i = r_i (R d) + xbest (:126-134 with the difference rotated once)
//   spiral_eval     the objective on the new rows (:141)
//   spiral_best     the first strict minimum of this generation's values, xbest, the counters and
//                   the budget (:138-148, :163)
// Given the same cos, sin, r and xbest the rotation is tests/spiral_model.py's device form bit for
// bit; the difference form against the reference's two rotations is rounding alone (DESIGN.md
// section 4).
#pragma once

#include "bbo_engine.hpp"

namespace bbo {

// diagnostic switches: the bits of SpiralConst::dbg (bbo_set "dbg", 0 in production)
enum SpiralDbg { SPIRAL_DBG_GLOBAL_TILE = 1 };     // the whole tile of the rotation in global memory

// the last SPIRAL_LDS_COORDS coordinates of a wavefront's 64 x n tile live in LDS (40 KiB: four
// wavefronts per CU), the ones before them in global memory
constexpr int SPIRAL_LDS_COORDS = 80;
constexpr int SPIRAL_MAX_N = 512;
constexpr int SPIRAL_MAX_NP = 65536;
constexpr int SPIRAL_DEFAULT_K = 8;      // the fastest of 1, 2, 4, 8 at n = 128

struct SpiralScal {
    double fbest;            // f of xbest: the minimum of the LAST generation, not of the run
    int ibest;               // its row
    int it;                  // generations done: the counter word of the draws
    int fev;
    int stop;                // sticky: 2 = evaluation budget exhausted (there is no 1)
    int conv;                // always 0: the reference never converges (spiral.cpp:152, :169)
};

struct SpiralConst {
    int n, ld, np;
    int obj, mfev, honor_stop, npop;
    int record;              // keep the four raw uniforms of every point
    int dbg;                 // SpiralDbg bits
    int kfuse;               // stages fused in registers: 1, 2, 4 or 8 (the same bits)
    double r, theta, taur, tautheta, rlow, rhigh, thetalow, thetahigh;
    uint64_t seed;
};

struct SpiralDev {
    double *X;               // [P][np][ld]
    double *f;               // [P][np]
    double *r, *theta, *cs, *sn;    // [P][np]
    double *xbest;           // [P][ld]
    double *draws;           // [P][np][4] (recording, else null)
    const double *inject;    // [P][np][4] raw uniforms instead of the generator's (else null)
    double *tile;            // [ceil(P np / 64)][split][64]: the tile's coordinates below `split` (else null)
    const double *lower, *upper, *aux;
    SpiralScal *scal;
};

class SpiralEngine: public Engine<SpiralScal> {
public:
    static constexpr const char *HANDLE_NAME = "not a SpiralSearch handle";
    explicit SpiralEngine(const bbo_params &p);
    void init(int n, const double *lower, const double *upper, const double *guess,
            const ObjectiveSpec &obj) override;
    void solution(int population, double *x_out, int *n_evals, int *converged) override;
    int get(const std::string &key, int population, double *out, int cap) override;
    int set(const std::string &key, int population, const double *in, int count) override;
    int dimension() const override { return c_.n; }

    // bbo_spiral_configure: the constructor arguments bbo_params has no field for
    void configure(const bbo_spiral_params &sp);
    // bbo_spiral_phase: 0 draw, 1 rotate, 2 evaluate, 3 best
    void phase(int which);
    // bbo_spiral_inject_uniforms: [P][np][4] (coin of r, value of r, coin of theta, value of theta)
    void inject_uniforms(const double *u, int count);

private:
    static const bbo_params &checked(const bbo_params &p);
    void generation(bool honor_stop) override;
    void launch_draw();
    void launch_rotate();
    void launch_eval(int p0, int pcount);
    void launch_best(int p0, int pcount, int counters);
    int lds_coords() const;
    int tile_split() const;

    bbo_spiral_params sp_ {};
    SpiralConst c_ {};
    SpiralDev d_ {};
    DevBuf<double> X_, f_, r_, theta_, cs_, sn_, xbest_, tile_;
    DrawTables tables_;      // [P][np][4] uniforms: the injected table and the recorded one
    int tile_split_ = 0;     // the split tile_ was allocated for
};

} // namespace bbo
