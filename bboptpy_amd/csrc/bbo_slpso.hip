// bbo_slpso.hip -- host side of the SLPSO engine.  Reference behaviour restated on the host:
// SLPSOSearch::SLPSOSearch / init / optimize / solution (slpso.cpp:42-171), updateParParticle (:383-392).
#include "bbo_slpso_kernels.hpp"

#include <algorithm>
#include <cmath>
#include <limits>

namespace bbo {

namespace {
enum { K_INIT = 0, K_GENERATION, K_EVAL, K_COUNT };
static const char *const K_NAMES[K_COUNT] = { "bbo:slpso_init", "bbo:slpso_generation", "bbo:slpso_eval" };
}

SlpsoEngine::SlpsoEngine(const bbo_params &p) :
        WalkEngine(checked(p), "bbo_slpso_phase", false)
{
    bbo_slpso_params_default(&sp_);
}

// the part of the constructor's arguments that travels in bbo_params
const bbo_params &SlpsoEngine::checked(const bbo_params &p)
{
    BBO_REQUIRE(p.algo == BBO_ALGO_SLPSO, "SlpsoEngine: bad algo");
    // (the reference would draw `jp != p` forever in a swarm of one, :272-275)
    BBO_REQUIRE(p.np >= 2 && p.np <= SLPSO_MAX_NP, "SLPSO: np must be in [2, 4096]");
    BBO_REQUIRE(p.mfev >= 1, "SLPSO: mfev must be positive");
    BBO_REQUIRE(std::isfinite(p.stol), "SLPSO: stol must be finite");
    return p;
}

void SlpsoEngine::configure(const bbo_slpso_params &sp)
{
    if (inited_) throw Error(BBO_ERR_STATE, "bbo_slpso_configure after bbo_init");
    for (double v : { sp.omegamin, sp.omegamax, sp.eta, sp.gamma, sp.vmax, sp.Ufmax })
        BBO_REQUIRE(std::isfinite(v), "SLPSO: the parameters must be finite");
    BBO_REQUIRE(sp.vmax >= 0., "SLPSO: vmax must not be negative");
    sp_ = sp;
}

// the threads of slpso_generation's workgroup: a lane per coordinate, one wavefront up to n = 64
int SlpsoEngine::workgroup() const
{
    return c_.n <= 64 ? 64 : c_.n <= 128 ? 128 : 256;
}

void SlpsoEngine::init(int n, const double *lower, const double *upper, const double *guess,
        const ObjectiveSpec &obj)
{
    (void) guess;   // SLPSO never reads it (slpso.cpp:56-92)
    reject_program(obj, "SLPSO");
    BBO_REQUIRE(n >= 1 && n <= SLPSO_MAX_N, "SLPSO: dimension must be in [1, 512]");
    require_finite_box("SLPSO draws its swarm from [lower, upper] and redraws inside it: the bounds must be finite",
            n, lower, upper);
    BBO_HIP(hipSetDevice(params_.device));
    obj_ = obj;
    const int P = params_.populations, np = params_.np;
    BBO_REQUIRE(P <= (1 << 24), "SLPSO: populations must be <= 2^24");
    const int keep_dbg = c_.dbg, keep_sub = c_.sub0;
    SlpsoConst &c = c_;
    c = SlpsoConst {};
    c.n = n;
    c.ld = round_up(n, 2);
    c.np = np;
    c.obj = obj.fused() ? obj.builtin : OBJ_HOST;
    c.mfev = params_.mfev;
    c.npop = P;
    c.dbg = keep_dbg;
    c.sub0 = keep_sub;
    c.omegamin = sp_.omegamin;
    c.omegamax = sp_.omegamax;
    c.eta = sp_.eta;
    c.gamma = sp_.gamma;
    c.vmax = sp_.vmax;
    c.stol = params_.stol;
    c.seed = params_.seed;

    const size_t rows = (size_t) P * np;
    x_.alloc(rows * c.ld);
    v_.alloc(rows * c.ld);
    pb_.alloc(rows * c.ld);
    fx_.alloc(rows); fpb_.alloc(rows); fp_.alloc(rows); Uf_.alloc(rows); Pl_.alloc(rows); radius_.alloc(rows);
    s_.alloc(rows * 4); p_.alloc(rows * 4); g_.alloc(rows * 4); G_.alloc(rows * 4);
    m_.alloc(rows); CF_.alloc(rows); PF_.alloc(rows); perm_.alloc(rows);
    abest_.alloc((size_t) P * c.ld); vdavg_.alloc((size_t) P * c.ld); cand_.alloc((size_t) P * c.ld);
    fcand_.alloc(P);
    tables_.clear();
    scal_.alloc(P);
    upload_box(n, c.ld, lower, upper, obj);
    {
        // updateParParticle (:383-392) by rank: std::exp / std::pow of the host, the reference's values
        std::vector<double> uf(np), pl(np);
        for (int k = 0; k < np; k++) {
            const double progress = std::exp(-std::pow(1.6 * k / np, 4.));
            uf[k] = std::max(1., sp_.Ufmax * progress);
            pl[k] = std::max(0.05, 1. - progress);
        }
        Uf_tab_.alloc(np);
        Pl_tab_.alloc(np);
        Uf_tab_.upload(uf.data(), np);
        Pl_tab_.upload(pl.data(), np);
    }
    {
        std::vector<double> zx(rows * c.ld, 0.), zf(P, 0.);
        x_.upload(zx.data(), zx.size());        // (the padding columns)
        fcand_.upload(zf.data(), P);
        std::vector<SlpsoScal> sc(P);
        std::memset(sc.data(), 0, sizeof(SlpsoScal) * P);
        scal_.upload(sc.data(), P);
    }

    SlpsoDev &d = d_;
    d = SlpsoDev {};
    d.x = x_.p; d.v = v_.p; d.pb = pb_.p;
    d.fx = fx_.p; d.fpb = fpb_.p; d.fp = fp_.p; d.Uf = Uf_.p; d.Pl = Pl_.p;
    d.s = s_.p; d.p = p_.p; d.g = g_.p; d.G = G_.p;
    d.m = m_.p; d.CF = CF_.p; d.PF = PF_.p; d.perm = perm_.p;
    d.abest = abest_.p; d.vdavg = vdavg_.p; d.cand = cand_.p; d.fcand = fcand_.p; d.radius = radius_.p;
    d.Uf_tab = Uf_tab_.p; d.Pl_tab = Pl_tab_.p;
    d.lower = lower_.p; d.upper = upper_.p; d.aux = aux_.p; d.scal = scal_.p;
    inited_ = true;
    mid_generation_ = false;

    if (obj_.needs_host()) {
        launch_init(0, P, SLPSO_INIT_DRAW);
        host_evaluate_range(x_, fx_, 0, P, c.np, 0, c.np, n, c.ld);     // (in swarm order: :84-91)
        launch_init(0, P, SLPSO_INIT_RESET | SLPSO_INIT_PAR);
    } else {
        launch_init(0, P, SLPSO_INIT_DRAW | SLPSO_INIT_EVAL | SLPSO_INIT_RESET | SLPSO_INIT_PAR);
    }
    BBO_HIP(hipStreamSynchronize(stream_));
}

void SlpsoEngine::launch_init(int p0, int pcount, int mode)
{
    timed(K_INIT, [&] { hipLaunchKernelGGL(slpso_init, dim3(pcount), dim3(256), 0, stream_, d_, c_, p0, mode); });
}

// one iterate() of every population (SLPSO_FUSED), or the same body from evaluation to evaluation
void SlpsoEngine::launch_walk(int mode, bool begin)
{
    const int b = begin ? 1 : 0;
    const int T = workgroup(), W = T / 64;
    const size_t bytes = (size_t) (5 + (W > 1 ? W : 0)) * c_.ld * sizeof(double) + (size_t) c_.ld * sizeof(int);
    timed(K_GENERATION, [&] {
        switch (T) {
        case 64: hipLaunchKernelGGL((slpso_generation<64>), dim3(c_.npop), dim3(64), bytes, stream_, d_, c_, mode, b); break;
        case 128: hipLaunchKernelGGL((slpso_generation<128>), dim3(c_.npop), dim3(128), bytes, stream_, d_, c_, mode, b); break;
        default: hipLaunchKernelGGL((slpso_generation<256>), dim3(c_.npop), dim3(256), bytes, stream_, d_, c_, mode, b); break;
        }
    });
}

void SlpsoEngine::launch_eval_device()
{
    timed(K_EVAL, [&] { hipLaunchKernelGGL(slpso_eval, dim3(c_.npop), dim3(64), 0, stream_, d_, c_); });
}

void SlpsoEngine::inject_draws(const double *table, int count)
{
    enter("bbo_slpso_inject_draws");
    BBO_HIP(hipStreamSynchronize(stream_));
    if (!table) {
        d_.inject = nullptr;
        return;
    }
    const int n = c_.n, np = c_.np;
    const size_t len = table_len(), want = (size_t) c_.npop * len;
    BBO_REQUIRE(count >= 0 && (size_t) count == want,
            "bbo_slpso_inject_draws: populations * (1 + np + np * (3 + 4 n)) values");
    auto unit = [](double u) { return u >= 0. && u < 1.; };
    for (int p = 0; p < c_.npop; p++) {
        const double *t = table + (size_t) p * len;
        BBO_REQUIRE(unit(t[0]), "bbo_slpso_inject_draws: uniforms lie in [0, 1)");
        permutation_of(t + 1, np, "bbo_slpso_inject_draws: perm is a permutation of 0 .. np - 1");
        for (int k = 0; k < np; k++) {
            const double *st = t + 1 + np + (size_t) k * (3 + 4 * (size_t) n);
            BBO_REQUIRE(unit(st[0]) && unit(st[1]) && unit(st[2]), "bbo_slpso_inject_draws: uniforms lie in [0, 1)");
            for (int j = 0; j < n; j++) {
                const double *cd = st + 3 + 4 * (size_t) j;
                BBO_REQUIRE(unit(cd[0]) && unit(cd[2]) && unit(cd[3]) && std::isfinite(cd[1]),
                        "bbo_slpso_inject_draws: uniforms lie in [0, 1), normals are finite");
            }
        }
    }
    d_.inject = tables_.load(table, want);
}

void SlpsoEngine::solution(int population, double *x_out, int *n_evals, int *converged)
{
    enter_population("solution()", population);
    SlpsoScal s;
    scal_.download(&s, 1, population);
    report_solution(s, abest_, (size_t) population * c_.ld, c_.n, c_.ld, x_out, n_evals, converged);
}

int SlpsoEngine::get(const std::string &k, int p, double *out, int cap)
{
    enter_population("get()", p);
    const SlpsoConst &c = c_;
    SlpsoScal s;
    scal_.download(&s, 1, p);
    const size_t pr = (size_t) p * c.np;
    const StateOut o { out, cap };
    if (k == "profile") return profile_report(out, cap);
    if (k == "x") return o.rows(x_, pr, c.np, c.n, c.ld);
    if (k == "v") return o.rows(v_, pr, c.np, c.n, c.ld);
    if (k == "pb") return o.rows(pb_, pr, c.np, c.n, c.ld);
    if (k == "fx") return o.vec(fx_, pr, c.np);
    if (k == "fpb") return o.vec(fpb_, pr, c.np);
    if (k == "fp") return o.vec(fp_, pr, c.np);
    if (k == "Uf") return o.vec(Uf_, pr, c.np);
    if (k == "Pl") return o.vec(Pl_, pr, c.np);
    if (k == "s") return o.vec(s_, pr * 4, c.np * 4);
    if (k == "p") return o.vec(p_, pr * 4, c.np * 4);
    if (k == "g") return o.ints(g_, pr * 4, c.np * 4);
    if (k == "G") return o.ints(G_, pr * 4, c.np * 4);
    if (k == "m") return o.ints(m_, pr, c.np);
    if (k == "CF") return o.ints(CF_, pr, c.np);
    if (k == "PF") return o.ints(PF_, pr, c.np);
    if (k == "perm") return o.ints(perm_, pr, c.np);
    if (k == "abest") return o.vec(abest_, (size_t) p * c.ld, c.n);
    if (k == "vdavg") return o.vec(vdavg_, (size_t) p * c.ld, c.n);
    if (k == "cand") return o.vec(cand_, (size_t) p * c.ld, c.n);
    if (k == "fcand") return o.vec(fcand_, p, 1);
    if (k == "draws") {
        require_record(c.record, k);
        return o.vec(tables_.draws, (size_t) p * table_len(), (int) table_len());
    }
    if (k == "fabest") return o.one(s.fabest);
    if (k == "alpha") return o.one(s.alpha);
    if (k == "omega") return o.one(s.omega);
    if (k == "mfes") return o.one(s.mfes);
    if (k == "fev") return o.one(s.fev);
    if (k == "it") return o.one(s.it);
    if (k == "flag" || k == "stop") return o.one(s.stop);
    if (k == "conv") return o.one(s.conv);
    if (k == "pending") return o.one(s.pending);
    if (k == "stage") return o.one(s.stage);
    if (k == "kp") return o.one(s.kp);
    if (k == "mv") return o.one(s.mv);
    if (k == "iop") return o.one(s.iop);
    if (k == "record_draws") return o.one(c.record);
    if (k == "dbg") return o.one(c.dbg);
    if (k == "substream") return o.one(c.sub0);
    if (k == "wg") return o.one(workgroup());
    if (k == "speculative") return o.one(workgroup() > 64 && !(c.dbg & SLPSO_DBG_SEQ_ALG2) ? 1. : 0.);
    if (k == "np") return o.one(c.np);
    if (k == "n") return o.one(c.n);
    throw Error(BBO_ERR_KEY, "unknown state key '" + k + "'");
}

int SlpsoEngine::set(const std::string &k, int p, const double *in, int count)
{
    enter_population("set()", p);
    const SlpsoConst &c = c_;
    const size_t pr = (size_t) p * c.np;
    if (k == "profile") return profile_enable(in, K_COUNT, K_NAMES);
    if (k == "record_draws") {      // (the whole handle: every population)
        BBO_REQUIRE(count == 1, "record_draws: one value");
        c_.record = in[0] != 0. ? 1 : 0;
        d_.draws = tables_.record(c_.record, (size_t) c.npop * table_len());
        return 1;
    }
    if (k == "dbg") {
        BBO_REQUIRE(count == 1 && (in[0] == 0. || in[0] == 1.), "dbg: 0, or 1 (Algorithm 2 one trial at a time)");
        c_.dbg = (int) in[0];
        return 1;
    }
    if (k == "substream") {     // the sub-stream of population 0; the swarm is drawn again from it
        BBO_REQUIRE(count == 1 && in[0] >= 0. && in[0] == std::floor(in[0]) && in[0] + c.npop <= (1 << 24),
                "substream: one integer in [0, 2^24 - populations]");
        c_.sub0 = (int) in[0];
        mid_generation_ = false;
        if (obj_.needs_host()) {
            launch_init(0, c.npop, SLPSO_INIT_DRAW);
            host_evaluate_range(x_, fx_, 0, c.npop, c.np, 0, c.np, c.n, c.ld);
            launch_init(0, c.npop, SLPSO_INIT_RESET | SLPSO_INIT_PAR);
        } else {
            launch_init(0, c.npop, SLPSO_INIT_DRAW | SLPSO_INIT_EVAL | SLPSO_INIT_RESET | SLPSO_INIT_PAR);
        }
        BBO_HIP(hipStreamSynchronize(stream_));
        return 1;
    }
    if (k == "x") {             // values, pbest, abest (index order) and the learning state follow; v = 0
        BBO_REQUIRE(count == c.np * c.n, "x: np * n values");
        upload_rows(x_, pr, c.np, c.n, c.ld, in);
        if (c.npop == 1) mid_generation_ = false;   // (the generation in progress, if any, is abandoned)
        if (obj_.needs_host()) {
            host_evaluate_range(x_, fx_, p, 1, c.np, 0, c.np, c.n, c.ld);
            launch_init(p, 1, SLPSO_INIT_RESET | SLPSO_INIT_PAR);
        } else {
            launch_init(p, 1, SLPSO_INIT_EVAL | SLPSO_INIT_RESET | SLPSO_INIT_PAR);
        }
        BBO_HIP(hipStreamSynchronize(stream_));
        return count;
    }
    if (k == "perm") {          // Uf and Pl follow
        BBO_REQUIRE(count == c.np, "perm: np values");
        perm_.upload(permutation_of(in, c.np, "perm: a permutation of 0 .. np - 1").data(), c.np, pr);
        launch_init(p, 1, SLPSO_INIT_PAR);
        BBO_HIP(hipStreamSynchronize(stream_));
        return count;
    }
    if (k == "cand") {          // (what bbo_slpso_phase 1 evaluates)
        BBO_REQUIRE(count == c.n, "cand: n values");
        cand_.upload(in, c.n, (size_t) p * c.ld);
        return count;
    }
    if (k == "fcand") {         // (what bbo_slpso_phase 2 absorbs)
        BBO_REQUIRE(count == 1, "fcand: one value");
        double v = in[0];
        nan_to_inf(&v, 1);
        fcand_.upload(&v, 1, p);
        return 1;
    }
    if (k == "fev") {           // (the budget test looks at fev after the next generation)
        BBO_REQUIRE(count == 1 && in[0] >= 0. && in[0] == std::floor(in[0]) && in[0] < 2147483647.,
                "fev: one non-negative integer");
        SlpsoScal s;
        scal_.download(&s, 1, p);
        s.fev = (int) in[0];
        scal_.upload(&s, 1, p);
        return 1;
    }
    throw Error(BBO_ERR_KEY, "unknown or read-only state key '" + k + "'");
}

Optimizer* make_slpso_engine(const bbo_params &p)
{
    return new SlpsoEngine(p);
}

} // namespace bbo
