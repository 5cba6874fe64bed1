// bbo_jaya.hip -- host side of the JAYA engine.  Reference behaviour restated on the host:
// JayaSearch::JayaSearch / init / optimize / solution (jaya.cpp:57-134, :176-198).
#include "bbo_jaya_kernels.hpp"

#include <algorithm>
#include <cmath>
#include <limits>

namespace bbo {

namespace {
enum { K_PARTITION = 0, K_EVOLVE, K_FINISH, K_COUNT };
static const char *const K_NAMES[K_COUNT] = { "bbo:jaya_partition", "bbo:jaya_evolve", "bbo:jaya_finish" };
}

JayaEngine::JayaEngine(const bbo_params &p) :
        Engine(checked(p))
{
    bbo_jaya_params_default(&jp_);
}

int JayaEngine::count_ks(int np, int npmin)
{
    int nks = 0;
    for (int k = 1; k <= np && np >= (long) npmin * k; k++) nks++;     // jaya.cpp:128-131
    return nks;
}

// the part of the constructor's arguments that travels in bbo_params
const bbo_params &JayaEngine::checked(const bbo_params &p)
{
    BBO_REQUIRE(p.algo == BBO_ALGO_JAYA, "JayaEngine: bad algo");
    BBO_REQUIRE(p.np >= 2, "JAYA needs at least 2 members");
    BBO_REQUIRE(p.npmin >= 1, "JAYA: npmin must be >= 1");
    BBO_REQUIRE(p.npmin <= p.np, "JAYA: npmin must not exceed np");
    return p;
}

// the part that travels in bbo_jaya_params
void JayaEngine::check_jaya(const bbo_params &p, const bbo_jaya_params &jp)
{
    const int nks = count_ks(p.np, p.npmin);
    BBO_REQUIRE(jp.k0 >= 1 && jp.k0 <= nks, "JAYA: k0 must be in [1, nks], nks = #{k >= 1 : np >= npmin k}");
    BBO_REQUIRE(jp.beta > 0. && jp.beta <= 2., "JAYA: beta must be in (0, 2]");
    BBO_REQUIRE(jp.mutation >= BBO_JAYA_ORIGINAL && jp.mutation <= BBO_JAYA_LOGISTIC, "JAYA: unknown mutation");
}

void JayaEngine::configure(const bbo_jaya_params &jp)
{
    if (inited_) throw Error(BBO_ERR_STATE, "bbo_jaya_configure after bbo_init");
    check_jaya(params_, jp);
    jp_ = jp;
}

void JayaEngine::init(int n, const double *lower, const double *upper, const double *guess,
        const ObjectiveSpec &obj)
{
    (void) guess;   // JAYA never reads it (jaya.cpp:73-134)
    reject_program(obj, "JAYA");
    BBO_REQUIRE(n >= 1 && n <= 1024, "JAYA: dimension must be in [1, 1024]");
    require_finite_box("JAYA draws its pool from [lower, upper]: the bounds must be finite", n,
            lower, upper);
    check_jaya(params_, jp_);
    BBO_HIP(hipSetDevice(params_.device));
    obj_ = obj;
    const int P = params_.populations;
    JayaConst &c = c_;
    c = JayaConst {};
    c.n = n;
    c.ld = round_up(n, 2);
    c.np = params_.np;
    c.npmin = params_.npmin;
    c.nks = count_ks(c.np, c.npmin);
    c.adapt = jp_.adapt ? 1 : 0;
    c.mutation = jp_.mutation;
    c.kcheb = jp_.kcheb;
    c.obj = obj.fused() ? obj.builtin : OBJ_HOST;
    c.mfev = params_.mfev;
    c.npop = P;
    c.tol = params_.tol;
    c.scale = jp_.scale;
    c.beta = jp_.beta;
    c.temper = jp_.temper;
    c.seed = params_.seed;
    c.ndraw = c.mutation == JAYA_LEVY ? 5 : 2;
    // jaya.cpp:86-89
    c.sigmau = std::pow((std::tgamma(1. + c.beta) * std::sin(c.beta * M_PI / 2.))
            / (std::tgamma((1. + c.beta) / 2.) * c.beta * std::pow(2., (c.beta - 1.) / 2.)), 1. / c.beta);
    c.kb = shuffle_key_bits(c.np);

    const size_t rows = (size_t) P * c.np, ld = c.ld, sub = (size_t) P * c.nks;
    X_.alloc(rows * ld);
    f_.alloc(rows);
    ftrial_.alloc(rows);
    radius_.alloc(rows);
    occ_.alloc(rows);
    occ2_.alloc(rows);
    T_.alloc(obj_.needs_host() ? rows * ld : 0);
    draws_.alloc(0);
    bw_.alloc(sub * 2 * ld);
    chaos_.alloc(c.mutation >= JAYA_TENT ? sub * n * 2 : 1);
    pstrat_.alloc(sub);
    perfindex_.alloc(sub);
    len_.alloc(sub);
    off_.alloc(sub + P);
    bwrow_.alloc(sub * 2);
    bestx_.alloc(P * ld);
    scal_.alloc(P);
    upload_box(n, c.ld, lower, upper, obj);
    std::vector<JayaScal> sc(P);
    for (auto &s : sc) {
        std::memset(&s, 0, sizeof(s));
        s.fev = c.np;          // the initial pool is evaluated (jaya.cpp:125)
        s.k = jp_.k0;
        s.fgbest = s.best = s.pbest = std::numeric_limits<double>::infinity();
    }
    scal_.upload(sc.data(), P);

    JayaDev &d = d_;
    d = JayaDev {};
    d.X = X_.p; d.f = f_.p; d.T = T_.p; d.ftrial = ftrial_.p; d.radius = radius_.p;
    d.bw = bw_.p; d.chaos = chaos_.p; d.pstrat = pstrat_.p; d.perfindex = perfindex_.p;
    d.bestx = bestx_.p; d.draws = nullptr;
    d.occ = occ_.p; d.occ2 = occ2_.p; d.len = len_.p; d.off = off_.p; d.bwrow = bwrow_.p;
    d.lower = lower_.p; d.upper = upper_.p; d.aux = aux_.p; d.scal = scal_.p;
    c.honor_stop = 0;
    c.record = 0;
    inited_ = true;

    hipLaunchKernelGGL(jaya_seed, dim3(P), dim3(64), 0, stream_, d_, c_);
    hipLaunchKernelGGL(jaya_init_eval, dim3((c.np + 3) / 4, P), dim3(256), 4 * ld * sizeof(double),
            stream_, d_, c_);
    BBO_HIP(hipGetLastError());
    // host objective: the pool, and in generation() the trials, in slot order like the reference's loop
    if (obj_.needs_host()) host_evaluate_rows(X_, f_, c.np, c.n, c.ld, c.honor_stop, &occ_);
    hipLaunchKernelGGL(jaya_finish, dim3(P), dim3(256), 0, stream_, d_, c_, 1);
    BBO_HIP(hipGetLastError());
    BBO_HIP(hipStreamSynchronize(stream_));
}

void JayaEngine::generation(bool honor_stop)
{
    JayaConst &c = c_;
    c.honor_stop = honor_stop ? 1 : 0;
    const int P = c.npop;
    timed(K_PARTITION, [&] { hipLaunchKernelGGL(jaya_partition, dim3(P), dim3(256), 0, stream_, d_, c_); });
    timed(K_EVOLVE, [&] {
        const dim3 grid((c.np + 3) / 4, P);
        const size_t lds = (size_t) 4 * c.ld * sizeof(double);
        if (c.mutation == JAYA_LEVY) hipLaunchKernelGGL(jaya_evolve<true>, grid, dim3(256), lds, stream_, d_, c_);
        else hipLaunchKernelGGL(jaya_evolve<false>, grid, dim3(256), lds, stream_, d_, c_);
    });
    if (obj_.needs_host()) {
        host_evaluate_rows(T_, ftrial_, c.np, c.n, c.ld, c.honor_stop, &occ_);
        hipLaunchKernelGGL(jaya_select, dim3((c.np + 3) / 4, P), dim3(256), 0, stream_, d_, c_);
        BBO_HIP(hipGetLastError());
    }
    timed(K_FINISH, [&] { hipLaunchKernelGGL(jaya_finish, dim3(P), dim3(256), 0, stream_, d_, c_, 0); });
}

void JayaEngine::solution(int population, double *x_out, int *n_evals, int *converged)
{
    enter_population("solution()", population);
    JayaScal s;
    scal_.download(&s, 1, population);
    report_solution(s, bestx_, (size_t) population * c_.ld, c_.n, c_.ld, x_out, n_evals, converged);
}

// the buffers of "record_draws": the draws and the trial rows of a generation
void JayaEngine::alloc_record()
{
    const size_t rows = (size_t) c_.npop * c_.np;
    if (!draws_.p) draws_.alloc(rows * c_.n * c_.ndraw);
    if (!T_.p) T_.alloc(rows * c_.ld);
}

int JayaEngine::get(const std::string &k, int p, double *out, int cap)
{
    enter_population("get()", p);
    const JayaConst &c = c_;
    JayaScal s;
    scal_.download(&s, 1, p);
    const size_t pb = (size_t) p * c.np;
    const StateOut o { out, cap };
    if (k == "profile") return profile_report(out, cap);
    // per-member arrays are reported by ROW; "occ" maps the reference's slots to rows
    if (k == "X") return o.rows(X_, pb, c.np, c.n, c.ld);
    if (k == "f") return o.vec(f_, pb, c.np);
    if (k == "occ") return o.ints(occ_, pb, c.np);
    if (k == "len") return o.ints(len_, (size_t) p * c.nks, c.nks);
    if (k == "pstrat") return o.vec(pstrat_, (size_t) p * c.nks, c.nks);
    if (k == "perfindex") return o.vec(perfindex_, (size_t) p * c.nks, c.nks);
    if (k == "bestx") return o.vec(bestx_, (size_t) p * c.ld, c.n);
    if (k == "trial" || k == "draws" || k == "ftrial") {
        require_record(c.record, k);
        if (k == "trial") return o.rows(T_, pb, c.np, c.n, c.ld);
        if (k == "ftrial") return o.vec(ftrial_, pb, c.np);
        const int cnt = c.np * c.n * c.ndraw + 1;
        if (o.fits(cnt)) {
            draws_.download(out, cnt - 1, pb * c.n * c.ndraw);
            out[cnt - 1] = s.uroul;        // the roulette's uniform (0 without `adapt`)
        }
        return cnt;
    }
    if (k == "record_draws") return o.one(c.record);
    if (k == "k") return o.one(s.k);
    if (k == "nks") return o.one(c.nks);
    if (k == "xchaos") return o.one(s.xchaos);
    if (k == "best") return o.one(s.best);
    if (k == "pbest") return o.one(s.pbest);
    if (k == "fgbest") return o.one(s.fgbest);
    if (k == "sigmau") return o.one(c.sigmau);
    if (k == "fev") return o.one(s.fev);
    if (k == "gen") return o.one(s.gen);
    if (k == "stop") return o.one(s.stop);
    if (k == "conv") return o.one(s.conv);
    if (k == "m2") return o.one(s.m2);
    if (k == "np") return o.one(c.np);
    if (k == "n") return o.one(c.n);
    throw Error(BBO_ERR_KEY, "unknown state key '" + k + "'");
}

int JayaEngine::set(const std::string &k, int p, const double *in, int count)
{
    enter_population("set()", p);
    const JayaConst &c = c_;
    const size_t pb = (size_t) p * c.np;
    if (k == "profile") return profile_enable(in, K_COUNT, K_NAMES);
    if (k == "record_draws") {
        BBO_REQUIRE(count == 1, "record_draws: one value");
        c_.record = in[0] != 0. ? 1 : 0;
        if (c_.record) alloc_record();
        d_.draws = c_.record ? draws_.p : nullptr;
        d_.T = c_.record || obj_.needs_host() ? T_.p : nullptr;
        return 1;
    }
    if (k == "X") {             // by row; the radii follow, f does not
        BBO_REQUIRE(count == c.np * c.n, "X: np * n values");
        upload_rows(X_, pb, c.np, c.n, c.ld, in, &radius_);
        return count;
    }
    if (k == "f") {
        BBO_REQUIRE(count == c.np, "f: np values");
        f_.upload(in, c.np, pb);
        return count;
    }
    if (k == "k" || k == "xchaos") {
        BBO_REQUIRE(count == 1, "one value");
        JayaScal s;
        scal_.download(&s, 1, p);
        if (k == "k") {
            BBO_REQUIRE(in[0] >= 1. && in[0] <= c.nks && in[0] == std::floor(in[0]), "k must be in [1, nks]");
            s.k = (int) in[0];
        } else {
            s.xchaos = in[0];
        }
        scal_.upload(&s, 1, p);
        return 1;
    }
    throw Error(BBO_ERR_KEY, "unknown or read-only state key '" + k + "'");
}

Optimizer* make_jaya_engine(const bbo_params &p)
{
    return new JayaEngine(p);
}

} // namespace bbo
