// bbo_lm.hip -- host side of the LM-CMA-ES engine.  Reference behaviour restated on the host:
// LmCmaes::LmCmaes / init (lm_cmaes.h:56-65, lm_cmaes.cpp:42-86) over BaseCmaes::init
// (base_cmaes.cpp:54-134), optimize and solution (base_cmaes.cpp:158-174, :232-238).
#include "bbo_lm_kernels.hpp"

#include <algorithm>
#include <cmath>
#include <limits>

namespace bbo {

namespace {
enum { K_DRAW = 0, K_SAMPLE, K_EVAL, K_RANK, K_UPDATE, K_HISTORY, K_COUNT };
static const char *const K_NAMES[K_COUNT] = { "bbo:lm_draw", "bbo:lm_sample", "bbo:lm_eval", "bbo:lm_rank",
        "bbo:lm_update", "bbo:lm_history_stop" };

// lm_sample / lm_update with NR = the power of two >= ceil(n / 256) columns per thread
template<class... A>
void launch_sample(int n, dim3 grid, hipStream_t s, A... a)
{
    const int nr = (n + 255) / 256;
    if (nr <= 1) hipLaunchKernelGGL(lm_sample<1>, grid, dim3(256), 0, s, a...);
    else if (nr <= 2) hipLaunchKernelGGL(lm_sample<2>, grid, dim3(256), 0, s, a...);
    else if (nr <= 4) hipLaunchKernelGGL(lm_sample<4>, grid, dim3(256), 0, s, a...);
    else if (nr <= 8) hipLaunchKernelGGL(lm_sample<8>, grid, dim3(256), 0, s, a...);
    else hipLaunchKernelGGL(lm_sample<16>, grid, dim3(256), 0, s, a...);
}

template<class... A>
void launch_update(int n, dim3 grid, hipStream_t s, A... a)
{
    const int nr = (n + 255) / 256;
    if (nr <= 1) hipLaunchKernelGGL(lm_update<1>, grid, dim3(256), 0, s, a...);
    else if (nr <= 2) hipLaunchKernelGGL(lm_update<2>, grid, dim3(256), 0, s, a...);
    else if (nr <= 4) hipLaunchKernelGGL(lm_update<4>, grid, dim3(256), 0, s, a...);
    else if (nr <= 8) hipLaunchKernelGGL(lm_update<8>, grid, dim3(256), 0, s, a...);
    else hipLaunchKernelGGL(lm_update<16>, grid, dim3(256), 0, s, a...);
}
}

LmEngine::LmEngine(const bbo_params &p) :
        Engine(checked(p))
{
    bbo_lm_params_default(&lp_);
}

const bbo_params &LmEngine::checked(const bbo_params &p)
{
    BBO_REQUIRE(p.algo == BBO_ALGO_LM_CMAES, "LmEngine: bad algo");
    return p;
}

void LmEngine::configure(const bbo_lm_params &lp)
{
    if (inited_) throw Error(BBO_ERR_STATE, "bbo_lm_configure after bbo_init");
    lp_ = lp;
}

void LmEngine::init(int n, const double *lower, const double *upper, const double *guess,
        const ObjectiveSpec &obj)
{
    reject_program(obj, "LmCMAES");
    BBO_REQUIRE(n >= 1 && n <= LM_MAX_N, "LmCMAES: dimension must be in [1, 4096]");
    const int lambda = params_.np;
    BBO_REQUIRE(lambda >= 2 && lambda <= LM_MAX_NP, "LmCMAES: np (lambda) must be in [2, 4096]");
    // memory <= 0: large_size(n) = int(2 sqrt(n)) (lm_cmaes.h:60-62, lm_cmaes.cpp:46-48)
    const int m = lp_.memory > 0 ? lp_.memory : static_cast<int>(2. * std::sqrt(1. * n));
    BBO_REQUIRE(m >= 1 && m <= LM_MAX_M, "LmCMAES: memory (or int(2 sqrt(n))) must be in [1, 256]");
    BBO_REQUIRE(std::isfinite(params_.sigma0), "LmCMAES: sigma0 must be finite");
    BBO_HIP(hipSetDevice(params_.device));
    obj_ = obj;
    const int P = params_.populations;
    LmConst &c = c_;
    c = LmConst {};
    c.n = n;
    c.ld = round_up(n, 4);
    c.lambda = lambda;
    c.mu = lambda / 2;
    c.half = (lambda + 1) / 2;
    c.m = m;
    c.obj = obj.fused() ? obj.builtin : OBJ_HOST;
    c.mfev = params_.mfev;
    c.mit = params_.mfev / lambda;
    c.npop = P;
    c.usenew = lp_.usenew ? 1 : 0;
    c.rademacher = lp_.rademacher ? 1 : 0;
    c.bound = params_.bound ? 1 : 0;
    c.tol = params_.tol;
    c.seed = params_.seed;

    // weights and mueff, base_cmaes.cpp:93-105
    std::vector<double> w(c.mu);
    double sum = 0.;
    for (int i = 0; i < c.mu; i++) {
        w[i] = std::log(0.5 * (lambda + 1.)) - std::log(i + 1.);
        sum += w[i];
    }
    const double scale = 1. / sum;
    double lenw = 0.;
    for (int i = 0; i < c.mu; i++) {
        w[i] *= scale;
        lenw += w[i] * w[i];
    }
    const double mueff = 1. / lenw;
    // lm_cmaes.cpp:50-66
    if (c.usenew) {
        c.nsteps = n;
        c.t = std::max(1, static_cast<int>(std::log(1. * n)));
        c.cc = 0.5 / std::sqrt(1. * n);
    } else {
        c.nsteps = m;
        c.t = 1;
        c.cc = 1. / m;
    }
    c.cs = 0.3;
    c.c1 = 0.1 / std::log(n + 1.);
    c.ccc = std::sqrt(c.cc * (2. - c.cc) * mueff);
    c.damps = 1.;
    c.sqrt1mc1 = std::sqrt(1. - c.c1);
    c.zstar = 0.25;
    c.stolmin = 1e-16;
    // base_cmaes.cpp:128-129
    c.hlen = 10 + static_cast<int>(std::ceil((30. * n) / lambda));
    c.ik = static_cast<int>(std::ceil(0.1 + lambda / 4.));

    const size_t ld = c.ld, rows = (size_t) P * lambda;
    X_.alloc(rows * ld);
    Z_.alloc((size_t) P * c.half * ld);
    g_.alloc((size_t) P * c.half);
    f_.alloc(rows);
    fsort_.alloc(rows);
    fp_.alloc(rows);
    order_.alloc(rows);
    rank_.alloc(rows);
    xmean_.alloc(P * ld);
    xold_.alloc(P * ld);
    pc_.alloc(P * ld);
    Pm_.alloc((size_t) P * m * ld);
    Vm_.alloc((size_t) P * m * ld);
    b_.alloc((size_t) P * m);
    dd_.alloc((size_t) P * m);
    jarr_.alloc((size_t) P * m);
    larr_.alloc((size_t) P * m);
    hist_best_.alloc((size_t) P * c.hlen);
    hist_kth_.alloc((size_t) P * c.hlen);
    w_.alloc(c.mu);
    scal_.alloc(P);
    upload_box(n, c.ld, lower, upper, obj);
    w_.upload(w.data(), c.mu);
    {
        std::vector<double> mm(P * ld, 0.);
        for (int p = 0; p < P; p++)
            std::copy(guess + (size_t) p * n, guess + (size_t) (p + 1) * n, mm.begin() + p * ld);
        xmean_.upload(mm.data(), mm.size());
    }
    std::vector<LmScal> sc(P);
    for (auto &s : sc) {
        std::memset(&s, 0, sizeof(s));
        s.sigma = params_.sigma0;
        s.hist_head = -1;
        s.fbest = -std::numeric_limits<double>::infinity();
        s.fworst = std::numeric_limits<double>::infinity();
    }
    scal_.upload(sc.data(), P);

    LmDev &d = d_;
    d = LmDev {};
    d.X = X_.p; d.Z = Z_.p; d.g = g_.p; d.f = f_.p; d.fsort = fsort_.p; d.fp = fp_.p;
    d.order = order_.p; d.rank = rank_.p; d.xmean = xmean_.p; d.xold = xold_.p; d.pc = pc_.p;
    d.Pm = Pm_.p; d.Vm = Vm_.p; d.b = b_.p; d.d = dd_.p; d.jarr = jarr_.p; d.larr = larr_.p;
    d.hist_best = hist_best_.p; d.hist_kth = hist_kth_.p; d.w = w_.p;
    d.lower = lower_.p; d.upper = upper_.p; d.aux = aux_.p; d.scal = scal_.p;
    c.honor_stop = 0;
    draws_.clear();
    draws_gens_ = draws_next_ = 0;
    inited_ = true;
}

void LmEngine::part_sample()
{
    const LmConst &c = c_;
    const int P = c.npop;
    if (draws_gens_ > 0) {
        if (draws_next_ >= draws_gens_)
            throw Error(BBO_ERR_STATE, "LmCMAES: the injected draws are used up (bbo_lm_inject_draws)");
        BBO_HIP(hipStreamSynchronize(stream_));
        const size_t rows = (size_t) P * c.half, width = (size_t) c.n + 1;
        const double *tab = draws_.data() + (size_t) draws_next_ * rows * width;
        std::vector<double> z(rows * c.ld, 0.), g(rows);
        for (size_t r = 0; r < rows; r++) {
            std::copy(tab + r * width, tab + r * width + c.n, z.begin() + r * c.ld);
            g[r] = tab[r * width + c.n];
        }
        Z_.upload(z.data(), z.size());
        g_.upload(g.data(), g.size());
        draws_next_++;
    } else {
        timed(K_DRAW, [&] { hipLaunchKernelGGL(lm_draw, dim3((c.half + 3) / 4, P), dim3(256), 0, stream_, d_, c_); });
    }
    timed(K_SAMPLE, [&] { launch_sample(c.n, dim3((c.half + LM_BLOCK - 1) / LM_BLOCK, P), stream_, d_, c_); });
}

void LmEngine::part_eval()
{
    timed(K_EVAL, [&] {
        hipLaunchKernelGGL(lm_eval, dim3((c_.lambda + 3) / 4, c_.npop), dim3(256), 0, stream_, d_, c_);
    });
    if (obj_.needs_host()) host_evaluate_rows(X_, f_, c_.lambda, c_.n, c_.ld, c_.honor_stop);
}

void LmEngine::part_rank()
{
    timed(K_RANK, [&] {
        hipLaunchKernelGGL(lm_rank, dim3((c_.lambda + 31) / 32, c_.npop), dim3(256), 0, stream_, d_, c_);
    });
}

void LmEngine::part_update()
{
    timed(K_UPDATE, [&] { launch_update(c_.n, dim3(c_.npop), stream_, d_, c_); });
}

void LmEngine::part_history()
{
    timed(K_HISTORY, [&] { hipLaunchKernelGGL(lm_history_stop, dim3(c_.npop), dim3(64), 0, stream_, d_, c_); });
}

void LmEngine::generation(bool honor_stop)
{
    c_.honor_stop = honor_stop ? 1 : 0;
    part_sample();
    part_eval();
    part_rank();
    part_update();
    part_history();
}

void LmEngine::phase(int which)
{
    run_phase("phase()", which, 5, "LmCMAES phase: 0 sample, 1 evaluate, 2 rank, 3 update, 4 history + stop", [&] {
        c_.honor_stop = 0;
        if (which == 0) part_sample();
        else if (which == 1) part_eval();
        else if (which == 2) part_rank();
        else if (which == 3) part_update();
        else part_history();
    });
}

void LmEngine::inject_draws(const double *table, int count)
{
    enter("inject_draws()");
    BBO_HIP(hipStreamSynchronize(stream_));
    draws_.clear();
    draws_gens_ = draws_next_ = 0;
    if (!table) return;
    const size_t per_gen = (size_t) c_.npop * c_.half * ((size_t) c_.n + 1);
    BBO_REQUIRE(count > 0 && (size_t) count % per_gen == 0,
            "LmCMAES inject_draws: G x populations x ceil(np / 2) rows of n + 1 values (z of a \"+\" candidate, then "
            "the subset normal)");
    draws_.assign(table, table + count);
    draws_gens_ = (int) ((size_t) count / per_gen);
}

void LmEngine::solution(int population, double *x_out, int *n_evals, int *converged)
{
    enter_population("solution()", population);
    LmScal s;
    scal_.download(&s, 1, population);
    // bestSolution(), base_cmaes.cpp:232-238: the mean before the first generation, else the best
    // candidate of the last one
    if (s.it <= 0) {
        report_solution(s, xmean_, (size_t) population * c_.ld, c_.n, c_.ld, x_out, n_evals, converged);
        return;
    }
    int best = 0;
    order_.download(&best, 1, (size_t) population * c_.lambda);
    best = std::min(std::max(best, 0), c_.lambda - 1);
    report_solution(s, X_, ((size_t) population * c_.lambda + best) * c_.ld, c_.n, c_.ld, x_out, n_evals, converged);
}

int LmEngine::get(const std::string &k, int p, double *out, int cap)
{
    enter_population("get()", p);
    const LmConst &c = c_;
    LmScal s;
    scal_.download(&s, 1, p);
    const size_t pf = (size_t) p * c.lambda, pv = (size_t) p * c.ld, pm = (size_t) p * c.m;
    const StateOut o { out, cap };
    if (k == "profile") return profile_report(out, cap);
    if (k == "arx") return o.rows(X_, pf, c.lambda, c.n, c.ld);
    if (k == "fit_val") return o.vec(fsort_, pf, c.lambda);
    if (k == "fit_idx") return o.ints(order_, pf, c.lambda);
    if (k == "fit_rank") return o.ints(rank_, pf, c.lambda);
    if (k == "f") return o.vec(f_, pf, c.lambda);
    if (k == "fp") return o.vec(fp_, pf, c.lambda);
    if (k == "xmean") return o.vec(xmean_, pv, c.n);
    if (k == "xold") return o.vec(xold_, pv, c.n);
    if (k == "pc") return o.vec(pc_, pv, c.n);
    if (k == "pcmat") return o.rows(Pm_, pm, c.m, c.n, c.ld);
    if (k == "vmat") return o.rows(Vm_, pm, c.m, c.n, c.ld);
    if (k == "b") return o.vec(b_, pm, c.m);
    if (k == "d") return o.vec(dd_, pm, c.m);
    if (k == "jarr") return o.ints(jarr_, pm, c.m);
    if (k == "larr") return o.ints(larr_, pm, c.m);
    if (k == "z") return o.rows(Z_, (size_t) p * c.half, c.half, c.n, c.ld);
    if (k == "g") return o.vec(g_, (size_t) p * c.half, c.half);
    if (k == "weights") return o.vec(w_, 0, c.mu);
    if (k == "sigma") return o.one(s.sigma);
    if (k == "s") return o.one(s.s);
    if (k == "memlen") return o.one(s.memlen);
    if (k == "fbest") return o.one(s.fbest);
    if (k == "fworst") return o.one(s.fworst);
    if (k == "it") return o.one(s.it);
    if (k == "fev") return o.one(s.fev);
    if (k == "flag") return o.one(s.flag);
    if (k == "stop") return o.one(s.stop);
    if (k == "conv") return o.one(s.conv);
    if (k == "n") return o.one(c.n);
    if (k == "lambda") return o.one(c.lambda);
    if (k == "mu") return o.one(c.mu);
    if (k == "memory") return o.one(c.m);
    if (k == "t") return o.one(c.t);
    if (k == "nsteps") return o.one(c.nsteps);
    if (k == "hlen") return o.one(c.hlen);
    if (k == "cc") return o.one(c.cc);
    if (k == "c1") return o.one(c.c1);
    if (k == "ccc") return o.one(c.ccc);
    throw Error(BBO_ERR_KEY, "unknown state key '" + k + "'");
}

int LmEngine::set(const std::string &k, int p, const double *in, int count)
{
    enter_population("set()", p);
    if (k == "profile") return profile_enable(in, K_COUNT, K_NAMES);
    if (k == "xmean") {
        BBO_REQUIRE(count == c_.n, "xmean: n values");
        xmean_.upload(in, c_.n, (size_t) p * c_.ld);
        return count;
    }
    if (k == "sigma") {
        BBO_REQUIRE(count == 1 && in[0] > 0., "sigma: one positive value");
        LmScal s;
        scal_.download(&s, 1, p);
        s.sigma = in[0];
        scal_.upload(&s, 1, p);
        return 1;
    }
    throw Error(BBO_ERR_KEY, "unknown or read-only state key '" + k + "'");
}

Optimizer* make_lm_engine(const bbo_params &p)
{
    return new LmEngine(p);
}

} // namespace bbo
