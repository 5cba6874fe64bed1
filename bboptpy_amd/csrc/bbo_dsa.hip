// bbo_dsa.hip -- host side of the DSA engine.  Reference behaviour restated on the host:
// DSSearch::DSSearch / init / optimize / solution (ds.cpp:36-84, :158-184).
#include "bbo_dsa_kernels.hpp"

#include <algorithm>
#include <cmath>
#include <limits>

namespace bbo {

namespace {
enum { K_RANK = 0, K_PLAN, K_EVOLVE, K_FINISH, K_COUNT };
static const char *const K_NAMES[K_COUNT] = { "bbo:dsa_rank", "bbo:dsa_plan", "bbo:dsa_evolve", "bbo:dsa_finish" };
constexpr int N_SCALARS = 12;
}

DsaEngine::DsaEngine(const bbo_params &p) :
        Engine(checked(p))
{
    bbo_dsa_params_default(&dp_);
}

// the part of the constructor's arguments that travels in bbo_params
const bbo_params &DsaEngine::checked(const bbo_params &p)
{
    BBO_REQUIRE(p.algo == BBO_ALGO_DSA, "DsaEngine: bad algo");
    BBO_REQUIRE(p.np >= 1, "DSA needs at least 1 member");
    return p;
}

void DsaEngine::configure(const bbo_dsa_params &dp)
{
    if (inited_) throw Error(BBO_ERR_STATE, "bbo_dsa_configure after bbo_init");
    BBO_REQUIRE(dp.nbatch >= 1, "DSA: nbatch must be >= 1");
    dp_ = dp;
}

void DsaEngine::init(int n, const double *lower, const double *upper, const double *guess,
        const ObjectiveSpec &obj)
{
    (void) guess;   // DSA never reads it (ds.cpp:46-84)
    reject_program(obj, "DSA");
    BBO_REQUIRE(n >= 1 && n <= 1024, "DSA: dimension must be in [1, 1024]");
    require_finite_box("DSA draws its pool from [lower, upper]: the bounds must be finite", n,
            lower, upper);
    BBO_HIP(hipSetDevice(params_.device));
    obj_ = obj;
    const int P = params_.populations;
    DsaConst &c = c_;
    c = DsaConst {};
    c.n = n;
    c.ld = round_up(n, 2);
    c.np = params_.np;
    c.adapt = dp_.adapt ? 1 : 0;
    c.nbatch = dp_.nbatch;
    c.obj = obj.fused() ? obj.builtin : OBJ_HOST;
    c.mfev = params_.mfev;
    c.npop = P;
    c.tol = params_.tol;
    c.stol = params_.stol;
    // ds.cpp:81-82
    c.gamma = std::min(1.0, std::sqrt(4 * std::log(4) / ((std::exp(1) - 1) * c.nbatch)));
    c.seed = params_.seed;
    c.force_method = c.force_map = -1;
    c.mcap = round_up((int) std::ceil(0.3 * n) + 1, 4);     // mapmax = ceil(p2 n), p2 < 0.3
    c.kb = shuffle_key_bits(c.np);

    const size_t rows = (size_t) P * c.np, ld = c.ld;
    X0_.alloc(rows * ld);
    X1_.alloc(rows * ld);
    f_.alloc(rows);
    ftrial_.alloc(rows);
    radius_.alloc(rows);
    order_.alloc(rows);
    dirrow_.alloc(rows);
    acc_.alloc(rows);
    T_.alloc(obj_.needs_host() ? rows * ld : 0);
    dirdraws_.alloc(0);
    mapdraws_.alloc(0);
    bounddraws_.alloc(0);
    map_.alloc(0);
    bestx_.alloc(P * ld);
    scal_.alloc(P);
    upload_box(n, c.ld, lower, upper, obj);
    std::vector<DsaScal> sc(P);
    for (auto &s : sc) {
        std::memset(&s, 0, sizeof(s));
        s.fev = c.np;          // the initial pool is evaluated (ds.cpp:301)
        for (int q = 0; q < 4; q++) {
            s.w[q] = 1.;
            s.p[q] = 0.25;
        }
        s.fbest = std::numeric_limits<double>::infinity();
    }
    scal_.upload(sc.data(), P);

    DsaDev &d = d_;
    d = DsaDev {};
    d.X[0] = X0_.p; d.X[1] = X1_.p; d.f = f_.p; d.T = T_.p; d.ftrial = ftrial_.p; d.radius = radius_.p;
    d.bestx = bestx_.p; d.order = order_.p; d.dirrow = dirrow_.p; d.acc = acc_.p;
    d.lower = lower_.p; d.upper = upper_.p; d.aux = aux_.p; d.scal = scal_.p;
    c.honor_stop = 0;
    c.record = 0;
    inited_ = true;

    hipLaunchKernelGGL(dsa_init, dim3((c.np + 3) / 4, P), dim3(256), 4 * ld * sizeof(double),
            stream_, d_, c_);
    BBO_HIP(hipGetLastError());
    // host objective: the pool, and in generation() the trials, in row order like the reference's loop
    if (obj_.needs_host()) host_evaluate_rows(X0_, f_, c.np, c.n, c.ld, c.honor_stop);
    hipLaunchKernelGGL(dsa_finish, dim3(P), dim3(256), 0, stream_, d_, c_, 1);
    BBO_HIP(hipGetLastError());
    BBO_HIP(hipStreamSynchronize(stream_));
}

void DsaEngine::generation(bool honor_stop)
{
    DsaConst &c = c_;
    c.honor_stop = honor_stop ? 1 : 0;
    const int P = c.npop;
    const dim3 members((c.np + 3) / 4, P);
    timed(K_RANK, [&] { hipLaunchKernelGGL(dsa_rank, dim3((c.np + 31) / 32, P), dim3(256), 0, stream_, d_, c_); });
    timed(K_PLAN, [&] { hipLaunchKernelGGL(dsa_plan, dim3(P), dim3(256), 0, stream_, d_, c_); });
    timed(K_EVOLVE, [&] {
        hipLaunchKernelGGL(dsa_evolve, members, dim3(256), (size_t) 4 * c.ld * sizeof(double), stream_, d_, c_);
    });
    if (obj_.needs_host()) {
        host_evaluate_rows(T_, ftrial_, c.np, c.n, c.ld, c.honor_stop);
        hipLaunchKernelGGL(dsa_select, members, dim3(256), 0, stream_, d_, c_);
        BBO_HIP(hipGetLastError());
    }
    timed(K_FINISH, [&] { hipLaunchKernelGGL(dsa_finish, dim3(P), dim3(256), 0, stream_, d_, c_, 0); });
}

void DsaEngine::solution(int population, double *x_out, int *n_evals, int *converged)
{
    enter_population("solution()", population);
    DsaScal s;
    scal_.download(&s, 1, population);
    report_solution(s, bestx_, (size_t) population * c_.ld, c_.n, c_.ld, x_out, n_evals, converged);
}

// the buffers of "record_draws": the draws, the maps and the trial rows of a generation
void DsaEngine::alloc_record()
{
    const size_t rows = (size_t) c_.npop * c_.np;
    if (!dirdraws_.p) dirdraws_.alloc(rows * 2);
    if (!mapdraws_.p) mapdraws_.alloc(rows * (c_.n + 2 + c_.mcap));
    if (!bounddraws_.p) bounddraws_.alloc(rows * c_.n * 2);
    if (!map_.p) map_.alloc(rows * c_.n);
    if (!T_.p) T_.alloc(rows * c_.ld);
}

int DsaEngine::get(const std::string &k, int p, double *out, int cap)
{
    enter_population("get()", p);
    const DsaConst &c = c_;
    DsaScal s;
    scal_.download(&s, 1, p);
    const size_t pb = (size_t) p * c.np;
    const StateOut o { out, cap };
    if (k == "profile") return profile_report(out, cap);
    if (k == "X") return o.rows(s.cur ? X1_ : X0_, pb, c.np, c.n, c.ld);
    if (k == "f") return o.vec(f_, pb, c.np);
    if (k == "fit_idx") return o.ints(order_, pb, c.np);     // rank -> row, as the last dsa_rank that sorted left it
    if (k == "p") return o.copy(s.p, 4);
    if (k == "w") return o.copy(s.w, 4);
    if (k == "bestx") return o.vec(bestx_, (size_t) p * c.ld, c.n);
    if (k == "scalars" || k == "dirdraws" || k == "dirrow" || k == "mapdraws" || k == "map"
            || k == "bounddraws" || k == "trial" || k == "ftrial" || k == "nsucc") {
        require_record(c.record, k);
        if (k == "trial") return o.rows(T_, pb, c.np, c.n, c.ld);
        if (k == "ftrial") return o.vec(ftrial_, pb, c.np);
        if (k == "nsucc") return o.one(s.nsucc);
        if (k == "dirrow") return o.ints(dirrow_, pb, c.np);
        if (k == "map") return o.ints(map_, pb * c.n, c.np * c.n);
        if (k == "dirdraws") return o.vec(dirdraws_, pb * 2, c.np * 2);
        if (k == "mapdraws") return o.vec(mapdraws_, pb * (c.n + 2 + c.mcap), c.np * (c.n + 2 + c.mcap));
        if (k == "bounddraws") return o.vec(bounddraws_, pb * c.n * 2, c.np * c.n * 2);
        // the raw uniforms behind p1, p2, the method, the coin, the strategy and R; then what
        // was decided: p1, p2, method, strategy, mapmax, R
        if (o.fits(N_SCALARS)) {
            std::copy(s.raw, s.raw + 6, out);
            out[6] = s.p1;
            out[7] = s.p2;
            out[8] = s.method;
            out[9] = s.strategy;
            out[10] = s.mapmax;
            out[11] = s.R;
        }
        return N_SCALARS;
    }
    if (k == "record_draws") return o.one(c.record);
    if (k == "force_method") return o.one(c.force_method);
    if (k == "force_map") return o.one(c.force_map);
    if (k == "mcap") return o.one(c.mcap);
    if (k == "it") return o.one(s.it);
    if (k == "fev") return o.one(s.fev);
    if (k == "gen") return o.one(s.gen);
    if (k == "stop") return o.one(s.stop);
    if (k == "conv") return o.one(s.conv);
    if (k == "m2") return o.one(s.m2);
    if (k == "np") return o.one(c.np);
    if (k == "n") return o.one(c.n);
    if (k == "gamma") return o.one(c.gamma);
    if (k == "fbest") return o.one(s.fbest);
    throw Error(BBO_ERR_KEY, "unknown state key '" + k + "'");
}

int DsaEngine::set(const std::string &k, int p, const double *in, int count)
{
    enter_population("set()", p);
    const DsaConst &c = c_;
    const size_t pb = (size_t) p * c.np;
    if (k == "profile") return profile_enable(in, K_COUNT, K_NAMES);
    if (k == "record_draws") {
        BBO_REQUIRE(count == 1, "record_draws: one value");
        c_.record = in[0] != 0. ? 1 : 0;
        if (c_.record) alloc_record();
        d_.dirdraws = c_.record ? dirdraws_.p : nullptr;
        d_.mapdraws = c_.record ? mapdraws_.p : nullptr;
        d_.bounddraws = c_.record ? bounddraws_.p : nullptr;
        d_.map = c_.record ? map_.p : nullptr;
        d_.T = c_.record || obj_.needs_host() ? T_.p : nullptr;
        return 1;
    }
    if (k == "force_method" || k == "force_map") {      // (the whole handle: every population)
        const int top = k == "force_method" ? 3 : 2;
        BBO_REQUIRE(count == 1 && in[0] >= -1. && in[0] <= top && in[0] == std::floor(in[0]),
                "force_method: -1 or 0..3, force_map: -1 or 0..2");
        (k == "force_method" ? c_.force_method : c_.force_map) = (int) in[0];
        return 1;
    }
    DsaScal s;
    scal_.download(&s, 1, p);
    if (k == "X") {             // the radii follow, f does not
        BBO_REQUIRE(count == c.np * c.n, "X: np * n values");
        upload_rows(s.cur ? X1_ : X0_, pb, c.np, c.n, c.ld, in, &radius_);
        return count;
    }
    if (k == "f") {
        BBO_REQUIRE(count == c.np, "f: np values");
        f_.upload(in, c.np, pb);
        return count;
    }
    if (k == "p" || k == "w") {
        BBO_REQUIRE(count == 4, "four values");
        std::copy(in, in + 4, k == "p" ? s.p : s.w);
        scal_.upload(&s, 1, p);
        return 4;
    }
    if (k == "it") {
        BBO_REQUIRE(count == 1 && in[0] >= 0. && in[0] == std::floor(in[0]) && in[0] < 2147483647.,
                "it: one non-negative integer");
        s.it = (int) in[0];
        scal_.upload(&s, 1, p);
        return 1;
    }
    throw Error(BBO_ERR_KEY, "unknown or read-only state key '" + k + "'");
}

Optimizer* make_dsa_engine(const bbo_params &p)
{
    return new DsaEngine(p);
}

} // namespace bbo
