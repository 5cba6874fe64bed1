// bbo_xnes.hip -- host side of the xNES engine.  Reference behaviour restated on the host:
// xNES::xNES / init / optimize / solution (xnes.cpp:43-108, :193-219).
#include "bbo_xnes_kernels.hpp"

#include <algorithm>
#include <cmath>
#include <limits>

namespace bbo {

namespace {
enum { K_DRAW = 0, K_POINTS, K_RANK, K_STEP, K_ADAPT, K_COUNT };
static const char *const K_NAMES[K_COUNT] = { "bbo:xnes_draw", "bbo:xnes_points", "bbo:xnes_rank",
        "bbo:xnes_step", "bbo:xnes_adapt" };
}

XnesEngine::XnesEngine(const bbo_params &p) :
        Engine(checked(p))
{
    bbo_xnes_params_default(&xp_);
}

const bbo_params &XnesEngine::checked(const bbo_params &p)
{
    BBO_REQUIRE(p.algo == BBO_ALGO_XNES, "XnesEngine: bad algo");
    return p;
}

void XnesEngine::configure(const bbo_xnes_params &xp)
{
    if (inited_) throw Error(BBO_ERR_STATE, "bbo_xnes_configure after bbo_init");
    BBO_REQUIRE(std::isfinite(xp.a0) && xp.a0 > 0., "xNES: a0 must be finite and positive");
    BBO_REQUIRE(std::isfinite(xp.etamu), "xNES: etamu must be finite");
    xp_ = xp;
}

void XnesEngine::init(int n, const double *lower, const double *upper, const double *guess,
        const ObjectiveSpec &obj)
{
    reject_program(obj, "xNES");
    BBO_REQUIRE(n >= 1 && n <= XNES_MAX_N, "xNES: dimension must be in [1, 512]");
    BBO_HIP(hipSetDevice(params_.device));
    obj_ = obj;
    const int P = params_.populations;
    XnesConst &c = c_;
    c = XnesConst {};
    c.n = n;
    c.ld = round_up(n, 4);
    // xnes.cpp:63-65
    c.np = 4 + static_cast<int>(3. * std::log(1. * n));
    c.etasigma = 3. * (3. + std::log(1. * n)) / (5. * n * std::sqrt(1. * n));
    c.etab = c.etasigma;
    c.etamu = xp_.etamu;
    c.obj = obj.fused() ? obj.builtin : OBJ_HOST;
    c.mfev = params_.mfev;
    c.npop = P;
    c.tol = params_.tol;
    c.seed = params_.seed;
    c.lowrank = n >= lowrank_min_n_ ? 1 : 0;
    const int np = c.np;

    // the utilities, xnes.cpp:68-77
    std::vector<double> u(np);
    double sumu = 0.;
    for (int i = 1; i <= np; i++) {
        u[i - 1] = std::max(0., std::log(1 + 0.5 * np) - std::log(1. * i));
        sumu += u[i - 1];
    }
    for (int i = 0; i < np; i++) u[i] = u[i] / sumu - (1. / np);

    const size_t ld = c.ld, rows = (size_t) P * np;
    B_.alloc((size_t) P * n * ld);
    mu_.alloc(P * ld);
    xbest_.alloc(P * ld);
    Z_.alloc(rows * ld);
    Y_.alloc(rows * ld);
    X_.alloc(rows * ld);
    Q_.alloc(rows * ld);
    f_.alloc(rows);
    E_.alloc((size_t) P * XNES_EIG_MAX * XNES_EIG_MAX);
    u_.alloc(np);
    u_.upload(u.data(), np);
    zin_.alloc(0);
    zin_gens_ = zin_pos_ = 0;
    order_.alloc(rows);
    rank_.alloc(rows);
    scal_.alloc(P);
    upload_box(n, c.ld, lower, upper, obj);
    if (xp_.from_guess) {
        // (an extension: the reference starts at the origin whatever the guess, xnes.cpp:80)
        std::vector<double> mm(P * ld, 0.);
        for (int p = 0; p < P; p++)
            std::copy(guess + (size_t) p * n, guess + (size_t) (p + 1) * n, mm.begin() + p * ld);
        mu_.upload(mm.data(), mm.size());
    }
    {
        const std::vector<uint64_t> seeds(64, c.seed);
        lane_seed_.alloc(64);
        lane_seed_.upload(seeds.data(), 64);
    }
    std::vector<XnesScal> sc(P);
    for (auto &s : sc) {
        std::memset(&s, 0, sizeof(s));
        s.sigma = xp_.a0;
        s.escale = 1.;
        s.fbest = std::numeric_limits<double>::infinity();
        // solution() before the first generation: the points are zeros, so converged() is 0 < tol (:211-219)
        s.conv = 0. < params_.tol ? 1 : 0;
    }
    scal_.upload(sc.data(), P);

    XnesDev &d = d_;
    d = XnesDev {};
    d.B = B_.p; d.mu = mu_.p; d.xbest = xbest_.p; d.Z = Z_.p; d.Y = Y_.p; d.X = X_.p; d.Q = Q_.p;
    d.f = f_.p; d.E = E_.p; d.u = u_.p; d.zin = nullptr; d.order = order_.p; d.rank = rank_.p;
    d.aux = aux_.p; d.lane_seed = lane_seed_.p; d.scal = scal_.p;
    c.honor_stop = 0;
    allow_lds((const void*) xnes_points_mfma, XNES_MAX_NP * XNES_MAX_N * (int) sizeof(double));
    inited_ = true;
    hipLaunchKernelGGL(xnes_eye, dim3(P), dim3(256), 0, stream_, d_, c_);      // (alloc zeroed B)
    BBO_HIP(hipGetLastError());
    BBO_HIP(hipStreamSynchronize(stream_));
}

void XnesEngine::part_sample()
{
    const XnesConst &c = c_;
    const int P = c.npop;
    const dim3 rows((c.np + 3) / 4, P);
    if (zin_gens_ > 0 && zin_pos_ >= zin_gens_)
        throw Error(BBO_ERR_STATE, "xNES: the injected normals are used up (inject more, or NULL for the "
                "device's draws)");
    const bool take = zin_gens_ > 0;    // the next generation of the injected table
    if (take) d_.zin = zin_.p + (size_t) zin_pos_++ * P * c.np * c.ld;
    timed(K_DRAW, [&] {
        if (take) {
            hipLaunchKernelGGL(xnes_take, rows, dim3(256), 0, stream_, d_, c_);
        } else {
            hipLaunchKernelGGL(xnes_draw, rows, dim3(256), 0, stream_, d_, c_);
            hipLaunchKernelGGL(xnes_settle, rows, dim3(256), 0, stream_, d_, c_);
        }
    });
    timed(K_POINTS, [&] {
        if (c.n >= XNES_MFMA_MIN_N)
            hipLaunchKernelGGL(xnes_points_mfma, dim3(P), dim3(256), (size_t) c.np * c.ld * sizeof(double), stream_,
                    d_, c_);
        else
            hipLaunchKernelGGL(xnes_points, rows, dim3(256), (size_t) 8 * c.ld * sizeof(double), stream_, d_, c_);
    });
    if (obj_.needs_host()) host_evaluate_rows(X_, f_, c.np, c.n, c.ld, c.honor_stop);
}

void XnesEngine::part_rank()
{
    timed(K_RANK, [&] { hipLaunchKernelGGL(xnes_rank, dim3(c_.npop), dim3(64), 0, stream_, d_, c_); });
}

void XnesEngine::part_step()
{
    timed(K_STEP, [&] { hipLaunchKernelGGL(xnes_step, dim3(c_.npop), dim3(256), 0, stream_, d_, c_); });
}

void XnesEngine::part_adapt()
{
    timed(K_ADAPT, [&] {
        if (c_.lowrank)
            hipLaunchKernelGGL(xnes_adapt_lr, dim3((c_.n + 15) / 16, c_.npop), dim3(256), 0, stream_, d_, c_);
        else
            hipLaunchKernelGGL(xnes_adapt_dense, dim3(c_.npop), dim3(256), 0, stream_, d_, c_);
    });
}

void XnesEngine::generation(bool honor_stop)
{
    c_.honor_stop = honor_stop ? 1 : 0;
    part_sample();
    part_rank();
    part_step();
    part_adapt();
}

void XnesEngine::phase(int which)
{
    run_phase("phase()", which, 4, "xNES phase: 0 sample, 1 rank, 2 small step, 3 adapt", [&] {
        c_.honor_stop = 0;
        if (which == 0) part_sample();
        else if (which == 1) part_rank();
        else if (which == 2) part_step();
        else part_adapt();
    });
}

void XnesEngine::inject_normals(const double *z, int count)
{
    enter("inject_normals()");
    BBO_HIP(hipStreamSynchronize(stream_));
    zin_gens_ = zin_pos_ = 0;
    d_.zin = nullptr;
    if (!z) {
        zin_.alloc(0);
        return;
    }
    const XnesConst &c = c_;
    const size_t gen = (size_t) c.npop * c.np * c.n;
    BBO_REQUIRE(count > 0 && (size_t) count % gen == 0,
            "xNES inject_normals: G * populations * np * n normals, G >= 1");
    const size_t G = (size_t) count / gen, nrows = G * c.npop * c.np;
    std::vector<double> rows(nrows * c.ld, 0.);
    for (size_t r = 0; r < nrows; r++) std::copy(z + r * c.n, z + (r + 1) * c.n, rows.begin() + r * c.ld);
    zin_.alloc(rows.size());
    zin_.upload(rows.data(), rows.size());
    zin_gens_ = (int) G;
}

// xnes.cpp:193-195: the best point of the last generation, not the best ever
void XnesEngine::solution(int population, double *x_out, int *n_evals, int *converged)
{
    enter_population("solution()", population);
    XnesScal s;
    scal_.download(&s, 1, population);
    int first = 0;
    order_.download(&first, 1, (size_t) population * c_.np);
    report_solution(s, X_, ((size_t) population * c_.np + first) * c_.ld, c_.n, c_.ld, x_out, n_evals, converged);
}

int XnesEngine::get(const std::string &k, int p, double *out, int cap)
{
    enter_population("get()", p);
    const XnesConst &c = c_;
    XnesScal s;
    scal_.download(&s, 1, p);
    const size_t pb = (size_t) p * c.np, pv = (size_t) p * c.ld;
    const StateOut o { out, cap };
    if (k == "profile") return profile_report(out, cap);
    if (k == "B") return o.rows(B_, (size_t) p * c.n, c.n, c.n, c.ld);
    if (k == "xmean") return o.vec(mu_, pv, c.n);
    if (k == "xbest") return o.vec(xbest_, pv, c.n);
    if (k == "arx") return o.rows(X_, pb, c.np, c.n, c.ld);
    if (k == "arz") return o.rows(Z_, pb, c.np, c.n, c.ld);
    if (k == "ary") return o.rows(Y_, pb, c.np, c.n, c.ld);
    if (k == "fit_val") return o.vec(f_, pb, c.np);
    if (k == "fit_idx") return o.ints(order_, pb, c.np);
    if (k == "u") return o.vec(u_, 0, c.np);
    if (k == "sigma") return o.one(s.sigma);
    if (k == "gsigma") return o.one(s.gsigma);
    if (k == "fbest") return o.one(s.fbest);
    if (k == "np") return o.one(c.np);
    if (k == "n") return o.one(c.n);
    if (k == "it") return o.one(s.it);
    if (k == "fev") return o.one(s.fev);
    if (k == "flag" || k == "stop") return o.one(s.stop);
    if (k == "conv") return o.one(s.conv);
    if (k == "fact_fail") return o.one(s.fact_fail);
    if (k == "route") return o.one(c.lowrank);
    if (k == "lowrank_min_n") return o.one(lowrank_min_n_);
    if (k == "etasigma") return o.one(c.etasigma);
    throw Error(BBO_ERR_KEY, "unknown state key '" + k + "'");
}

int XnesEngine::set(const std::string &k, int p, const double *in, int count)
{
    if (k == "lowrank_min_n") {     // (the whole handle; legal before bbo_init too)
        BBO_REQUIRE(count == 1 && in[0] == std::floor(in[0]) && in[0] >= XNES_MFMA_MIN_N && in[0] <= XNES_EIG_MAX,
                "lowrank_min_n: an integer in [16, 32]");
        if (inited_) BBO_HIP(hipStreamSynchronize(stream_));
        lowrank_min_n_ = (int) in[0];
        if (inited_) c_.lowrank = c_.n >= lowrank_min_n_ ? 1 : 0;
        return 1;
    }
    enter_population("set()", p);
    const XnesConst &c = c_;
    if (k == "profile") return profile_enable(in, K_COUNT, K_NAMES);
    if (k == "B") {
        BBO_REQUIRE(count == c.n * c.n, "B: n * n values");
        upload_rows(B_, (size_t) p * c.n, c.n, c.n, c.ld, in);
        return count;
    }
    if (k == "xmean") {
        BBO_REQUIRE(count == c.n, "xmean: n values");
        mu_.upload(in, c.n, (size_t) p * c.ld);
        return count;
    }
    if (k == "sigma") {
        BBO_REQUIRE(count == 1 && in[0] > 0., "sigma: one positive value");
        XnesScal s;
        scal_.download(&s, 1, p);
        s.sigma = in[0];
        scal_.upload(&s, 1, p);
        return 1;
    }
    throw Error(BBO_ERR_KEY, "unknown or read-only state key '" + k + "'");
}

Optimizer* make_xnes_engine(const bbo_params &p)
{
    return new XnesEngine(p);
}

} // namespace bbo
