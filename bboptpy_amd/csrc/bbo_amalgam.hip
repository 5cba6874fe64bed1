// bbo_amalgam.hip -- host side of the (i)AMaLGaM engine.  Reference behaviour restated on the host:
// Amalgam::Amalgam / init / iterate / optimize / runParallel / converged (amalgam.cpp:42-328).
#include "bbo_amalgam_kernels.hpp"

#include <algorithm>
#include <cmath>
#include <limits>

namespace bbo {

namespace {
enum { K_MOMENTS = 0, K_FACTOR, K_DRAW, K_POINTS, K_EVAL, K_ADAPT, K_RANK, K_COUNT };
static const char *const K_NAMES[K_COUNT] = { "bbo:amalgam_moments", "bbo:amalgam_factor", "bbo:amalgam_draw",
        "bbo:amalgam_points", "bbo:amalgam_eval", "bbo:amalgam_adapt", "bbo:amalgam_rank" };

// :75-79, :102-106
int default_np(int n, bool iamalgam)
{
    return iamalgam ? static_cast<int>(10. * std::sqrt(1. * n)) : static_cast<int>(17. + 3. * std::pow(1. * n, 1.5));
}
}

AmalgamEngine::AmalgamEngine(const bbo_params &p) :
        Engine(checked(p))
{
    bbo_amalgam_params_default(&ap_);
}

const bbo_params &AmalgamEngine::checked(const bbo_params &p)
{
    BBO_REQUIRE(p.algo == BBO_ALGO_AMALGAM, "AmalgamEngine: bad algo");
    return p;
}

void AmalgamEngine::configure(const bbo_amalgam_params &ap)
{
    if (inited_) throw Error(BBO_ERR_STATE, "bbo_amalgam_configure after bbo_init");
    BBO_REQUIRE(ap.substream >= 0 && ap.substream < (1 << 24), "AMALGAM: substream must be in [0, 2^24)");
    ap_ = ap;
    sub0_ = ap.substream;
}

void AmalgamEngine::init(int n, const double *lower, const double *upper, const double *guess,
        const ObjectiveSpec &obj)
{
    (void) guess;       // (never read: :53-175; runParallel passes nullptr)
    reject_program(obj, "AMALGAM");
    BBO_REQUIRE(n >= 1 && n <= AMALGAM_MAX_N, "AMALGAM: dimension must be in [1, 512]");
    require_finite_box("AMALGAM: the initial population is uniform in the box: every bound must be finite", n,
            lower, upper);
    BBO_HIP(hipSetDevice(params_.device));
    obj_ = obj;
    if (driver()) {
        BBO_REQUIRE(params_.populations == 1, "AMALGAM: the parameter-free mode (noparam) takes populations = 1; "
                "its copies are the populations of an inner handle");
        driver_init(n, lower, upper, obj);
        return;
    }
    const int P = params_.populations;
    const bool iam = ap_.iamalgam != 0;
    const int np = params_.np > 0 ? params_.np : default_np(n, iam);
    BBO_REQUIRE(np >= 3, "AMALGAM: np must be at least 3 (the selection int(0.35 np) would be empty)");
    BBO_REQUIRE(np <= AMALGAM_MAX_NP, "AMALGAM: np must be at most 65536");
    AmalgamConst &c = c_;
    c = AmalgamConst {};
    c.n = n;
    c.ld = round_up(n, 4);
    c.np = np;
    // :112-131
    c.ss = static_cast<int>(0.35 * np);
    if (iam) {
        const double es = -1.1 * std::pow(c.ss, 1.2) / std::pow(1. * n, 1.6);
        const double esh = -1.2 * std::pow(c.ss, 0.31) / std::sqrt(1. * n);
        c.etasigma = 1. - std::exp(es);
        c.etashift = 1. - std::exp(esh);
    } else {
        c.etasigma = 1.;
        c.etashift = 1.;
    }
    const double alphaams = (0.5 * 0.35 * np) / (np - 1);
    c.nams = static_cast<int>(alphaams * (np - 1));
    c.nismax = 25 + n;
    c.obj = obj.fused() ? obj.builtin : OBJ_HOST;
    c.mfev = params_.mfev;
    c.npop = P;
    c.slabs = (c.ss + AMALGAM_SLAB - 1) / AMALGAM_SLAB;
    c.lds_factor = c.ld <= AMALGAM_LDS_MAX_LD ? 1 : 0;
    c.keep_elite = ap_.keep_elite ? 1 : 0;
    c.kb = shuffle_key_bits(np - 1);
    c.sub0 = sub0_;
    c.stol = params_.stol;
    c.seed = params_.seed;

    const size_t ld = c.ld, rows = (size_t) P * np, img = ld * ld;
    X_.alloc(rows * ld);
    Z_.alloc(rows * ld);
    f_.alloc(rows);
    mu_.alloc(P * ld);
    muold_.alloc(P * ld);
    mushift_.alloc(P * ld);
    xelite_.alloc(P * ld);
    xbest_.alloc(P * ld);
    cov_.alloc(P * img);
    chol_.alloc(P * img);
    part_.alloc((size_t) P * c.slabs * img);
    shifted_.alloc(rows);
    order_.alloc(rows);
    rank_.alloc(rows);
    zin_.alloc(0);
    shin_.alloc(0);
    zin_gens_ = zin_pos_ = 0;
    scal_.alloc(P);
    upload_box(n, c.ld, lower, upper, obj);
    {
        const std::vector<uint64_t> seeds(64, c.seed);
        lane_seed_.alloc(64);
        lane_seed_.upload(seeds.data(), 64);
    }
    std::vector<AmalgamScal> sc(P);
    for (auto &s : sc) {
        std::memset(&s, 0, sizeof(s));
        s.cmult = 1.;
        s.fbest = std::numeric_limits<double>::infinity();
        s.fail_at = n;
    }
    scal_.upload(sc.data(), P);

    AmalgamDev &d = d_;
    d = AmalgamDev {};
    d.X = X_.p; d.Z = Z_.p; d.f = f_.p; d.mu = mu_.p; d.muold = muold_.p; d.mushift = mushift_.p;
    d.xelite = xelite_.p; d.xbest = xbest_.p; d.cov = cov_.p; d.chol = chol_.p; d.part = part_.p;
    d.zin = nullptr; d.shin = nullptr; d.shifted = shifted_.p; d.order = order_.p; d.rank = rank_.p;
    d.lower = lower_.p; d.upper = upper_.p; d.aux = aux_.p; d.lane_seed = lane_seed_.p; d.scal = scal_.p;
    c.honor_stop = 0;
    if (c.lds_factor)
        allow_lds((const void*) amalgam_factor, AMALGAM_LDS_MAX_LD * AMALGAM_LDS_MAX_LD * (int) sizeof(double));
    inited_ = true;

    // the population (:137-147), mu and the diagonal of cov (:161-174)
    DevBuf<double> xin;
    if (!xin_.empty()) {
        BBO_REQUIRE(xin_.size() == rows * (size_t) n, "AMALGAM: the injected initial points are populations * np * n values");
        std::vector<double> padded(rows * ld, 0.);
        for (size_t r = 0; r < rows; r++)
            std::copy(xin_.begin() + r * n, xin_.begin() + (r + 1) * n, padded.begin() + r * ld);
        xin.alloc(padded.size());
        xin.upload(padded.data(), padded.size());
        xin_.clear();
    }
    const dim3 rowgrid((np + 3) / 4, P);
    hipLaunchKernelGGL(amalgam_init, rowgrid, dim3(256), (size_t) 4 * ld * sizeof(double), stream_, d_, c_,
            (const double*) xin.p);
    BBO_HIP(hipGetLastError());
    if (obj_.needs_host()) host_evaluate_rows(X_, f_, np, n, c.ld, false);
    launch_rank();
    hipLaunchKernelGGL(amalgam_init_mom, dim3(P), dim3(256), 0, stream_, d_, c_);
    BBO_HIP(hipGetLastError());
    BBO_HIP(hipStreamSynchronize(stream_));
}

void AmalgamEngine::launch_rank()
{
    timed(K_RANK, [&] {
        hipLaunchKernelGGL(amalgam_rank, dim3((c_.np + 31) / 32, c_.npop), dim3(256), 0, stream_, d_, c_);
    });
}

// updateDistribution, :358-416 (the sort is the ranking the previous phase left)
void AmalgamEngine::part_distribution()
{
    const AmalgamConst &c = c_;
    const int P = c.npop, T = (c.n + 15) / 16, tiles = T * (T + 1) / 2;
    timed(K_MOMENTS, [&] {
        hipLaunchKernelGGL(amalgam_mean, dim3(P), dim3(256), 0, stream_, d_, c_);
        hipLaunchKernelGGL(amalgam_gram, dim3((tiles + 3) / 4, c.slabs, P), dim3(256), 0, stream_, d_, c_);
        hipLaunchKernelGGL(amalgam_cov, dim3((c.n * c.n + 255) / 256, P), dim3(256), 0, stream_, d_, c_);
    });
    timed(K_FACTOR, [&] {
        hipLaunchKernelGGL(amalgam_factor, dim3(P), dim3(1024),
                c.lds_factor ? (size_t) c.ld * c.ld * sizeof(double) : (size_t) 0, stream_, d_, c_);
    });
}

// samplePopulation, :418-453
void AmalgamEngine::part_sample()
{
    const AmalgamConst &c = c_;
    const int P = c.npop;
    const dim3 rows((c.np + 3) / 4, P);
    if (zin_gens_ > 0 && zin_pos_ >= zin_gens_)
        throw Error(BBO_ERR_STATE, "AMALGAM: the injected draws are used up (inject more, or NULL for the "
                "device's draws)");
    const bool take = zin_gens_ > 0;    // the next generation of the injected table
    d_.zin = take ? zin_.p + (size_t) zin_pos_ * P * c.np * c.ld : nullptr;
    d_.shin = take ? shin_.p + (size_t) zin_pos_ * P * c.np : nullptr;
    if (take) zin_pos_++;
    timed(K_DRAW, [&] {
        if (take) {
            hipLaunchKernelGGL(amalgam_take, rows, dim3(256), 0, stream_, d_, c_);
        } else {
            hipLaunchKernelGGL(amalgam_draw, rows, dim3(256), 0, stream_, d_, c_);
            hipLaunchKernelGGL(amalgam_settle, rows, dim3(256), 0, stream_, d_, c_);
        }
    });
    timed(K_POINTS, [&] {
        hipLaunchKernelGGL(amalgam_points, dim3((c.np + 15) / 16, P), dim3(256), 0, stream_, d_, c_);
    });
    timed(K_EVAL, [&] {
        hipLaunchKernelGGL(amalgam_eval, rows, dim3(256), (size_t) 4 * c.ld * sizeof(double), stream_, d_, c_);
    });
    if (obj_.needs_host()) {
        // rows 1 .. in sampling order; row 0 keeps the value amalgam_eval gave it
        if (ident_.count != (size_t) P * c.np) {
            std::vector<int> id((size_t) P * c.np);
            for (size_t i = 0; i < id.size(); i++) id[i] = (int) (i % c.np);
            ident_.alloc(id.size());
            ident_.upload(id.data(), id.size());
        }
        host_evaluate_rows(X_, f_, c.np, c.n, c.ld, c.honor_stop, &ident_, [](int s) { return s == 0; });
    }
}

// the multiplier rules and the stop tests (:213-233, :290-328), then the ranking of the new values
void AmalgamEngine::part_adapt()
{
    timed(K_ADAPT, [&] { hipLaunchKernelGGL(amalgam_adapt, dim3(c_.npop), dim3(256), 0, stream_, d_, c_); });
    launch_rank();
}

void AmalgamEngine::generation(bool honor_stop)
{
    c_.honor_stop = honor_stop ? 1 : 0;
    part_distribution();
    part_sample();
    part_adapt();
}

void AmalgamEngine::phase(int which)
{
    enter("phase()");       // (here too: the refusal comes behind it and before the range check)
    if (driver()) throw Error(BBO_ERR_STATE, "AMALGAM phase: not in the parameter-free mode (noparam)");
    run_phase("phase()", which, 3, "AMALGAM phase: 0 distribution, 1 sample + evaluate, 2 adapt + stop", [&] {
        c_.honor_stop = 0;
        if (which == 0) part_distribution();
        else if (which == 1) part_sample();
        else part_adapt();
    });
}

void AmalgamEngine::inject_points(const double *x, int count)
{
    if (inited_ && !driver()) BBO_HIP(hipStreamSynchronize(stream_));
    if (driver()) throw Error(BBO_ERR_STATE, "AMALGAM inject: not in the parameter-free mode (noparam)");
    xin_.clear();
    if (!x) return;
    BBO_REQUIRE(count > 0, "AMALGAM inject_points: populations * np * n values");
    xin_.assign(x, x + count);
}

void AmalgamEngine::inject_draws(const double *z, int zcount, const int *rows, int rcount)
{
    enter("inject_draws()");
    if (driver()) throw Error(BBO_ERR_STATE, "AMALGAM inject: not in the parameter-free mode (noparam)");
    BBO_HIP(hipStreamSynchronize(stream_));
    zin_gens_ = zin_pos_ = 0;
    d_.zin = nullptr;
    d_.shin = nullptr;
    if (!z) {
        zin_.alloc(0);
        shin_.alloc(0);
        return;
    }
    const AmalgamConst &c = c_;
    const size_t gen = (size_t) c.npop * c.np * c.n;
    BBO_REQUIRE(zcount > 0 && (size_t) zcount % gen == 0,
            "AMALGAM inject_draws: G * populations * np * n normals, G >= 1");
    const size_t G = (size_t) zcount / gen, nrows = G * c.npop * c.np;
    BBO_REQUIRE((size_t) rcount == G * c.npop * c.nams && (rows || rcount == 0),
            "AMALGAM inject_draws: G * populations * nams shifted rows");
    std::vector<double> zr(nrows * c.ld, 0.);
    for (size_t r = 0; r < nrows; r++) std::copy(z + r * c.n, z + (r + 1) * c.n, zr.begin() + r * c.ld);
    std::vector<int> flags(nrows, 0);
    for (size_t g = 0; g < G * c.npop; g++)
        for (int k = 0; k < c.nams; k++) {
            const int r = rows[g * c.nams + k];
            BBO_REQUIRE(r >= 1 && r < c.np && !flags[g * c.np + r],
                    "AMALGAM inject_draws: the shifted rows are nams different rows of 1 .. np - 1");
            flags[g * c.np + r] = 1;
        }
    zin_.alloc(zr.size());
    zin_.upload(zr.data(), zr.size());
    shin_.alloc(flags.size());
    shin_.upload(flags.data(), flags.size());
    zin_gens_ = (int) G;
}

// ---- the parameter-free driver -----------------------------------------------------------------------

double AmalgamEngine::evaluate_point(const double *x)
{
    if (obj_.fused()) return builtin_objective_host(obj_.builtin, dn_, x, aux_h_.data());
    double f = 0.;
    obj_.eval_host(x, 1, dn_, dn_, &f);
    nan_to_inf(&f, 1);
    return f;
}

namespace {
void print_row(const std::string &a, const std::string &b, const std::string &c, const std::string &d,
        const std::string &e, const std::string &f)
{
    printf(" | %5s | %5s | %10s | %25s | %25s | %10s | \n", a.c_str(), b.c_str(), c.c_str(), d.c_str(), e.c_str(),
            f.c_str());
}
std::string full(double v)
{
    char buf[64];
    snprintf(buf, sizeof(buf), "%.17g", v);
    return buf;
}
}

// :72-98
void AmalgamEngine::driver_init(int n, const double *lower, const double *upper, const ObjectiveSpec &obj)
{
    dn_ = n;
    dlower_.assign(lower, lower + n);
    dupper_.assign(upper, upper + n);
    aux_h_.assign(n, 0.);
    fill_objective_aux(obj.fused() ? obj.builtin : -1, n, aux_h_.data());
    nbase_ = default_np(n, ap_.iamalgam != 0);
    BBO_REQUIRE(nbase_ >= 3, "AMALGAM: np must be at least 3 (the selection int(0.35 np) would be empty)");
    const double inf = std::numeric_limits<double>::infinity();
    dfbest_ = dfbestrun_ = dfbestrunold_ = inf;
    dbest_.assign(n, 0.);
    s_ = 0;
    budget_ = params_.mfev;
    dfev_ = 0;
    stages_.clear();
    c_ = AmalgamConst {};
    c_.n = n;
    inited_ = true;
    if (ap_.print) {
        print_row("iter", "runs", "pop", "f*", "best f*", "fev");
        printf(" |%s| \n", std::string(5 + 5 + 10 + 25 + 25 + 10 + 3 * 5 + 2, '=').c_str());
        fflush(stdout);
    }
}

// iterate() of the parameter-free mode (:180-203) with runParallel (:257-288).  The copies of a stage
// run as the populations of one inner handle, copy r on sub-stream (s << 16) + r, every one with the
// budget the stage starts with; the budget is then charged in the reference's order.  A copy whose
// cap in that order is smaller and that ran a generation beyond it is replayed alone with that cap:
// the same sub-stream, so the same generations up to the cap.
void AmalgamEngine::driver_stage()
{
    const int floorS = s_ >> 1;
    BBO_REQUIRE(floorS < 15, "AMALGAM: the parameter-free mode ends after 30 stages");
    int np, runs;
    if ((s_ & 1) == 0) {
        np = (1 + floorS) * nbase_;
        runs = 1 << floorS;
    } else {
        np = (1 << (1 + floorS)) * nbase_;
        runs = 1;
    }
    BBO_REQUIRE(np <= AMALGAM_MAX_NP, "AMALGAM: np must be at most 65536");
    dfbestrunold_ = dfbestrun_;
    dfbestrun_ = std::numeric_limits<double>::infinity();

    bbo_amalgam_params ip = ap_;
    ip.noparam = 0;
    std::vector<double> guess((size_t) runs * dn_, 0.);
    auto make = [&](int pops, int sub, int cap) {
        bbo_params q = params_;
        q.populations = pops;
        q.np = np;
        q.mfev = cap;
        std::unique_ptr<AmalgamEngine> e(new AmalgamEngine(q));
        ip.substream = sub;
        e->configure(ip);
        e->init(dn_, dlower_.data(), dupper_.data(), guess.data(), obj_);
        e->run(std::numeric_limits<int>::max());
        return e;
    };
    const int sub = (s_ << 16);
    std::unique_ptr<AmalgamEngine> all;
    if (ap_.concurrent && runs > 1) all = make(runs, sub, budget_);
    std::vector<double> x(dn_);
    for (int r = 0; r < runs; r++) {
        int fev = 0, conv = 0;
        bool have = false;
        if (all) {
            all->solution(r, x.data(), &fev, &conv);
            have = fev == 2 * np || fev - np < budget_;
        }
        if (!have) {
            auto one = make(1, sub + r, budget_);
            one->solution(0, x.data(), &fev, &conv);
        }
        dfev_ += fev;
        budget_ -= fev;
        const double fitr = evaluate_point(x.data());
        dfev_++;
        budget_--;
        dfbestrun_ = std::min(dfbestrun_, fitr);
        if (fitr < dfbest_) {
            dfbest_ = fitr;
            dbest_ = x;
        }
    }
    stages_.push_back(AmalgamStage { s_, runs, np, dfbestrun_, dfbest_, dfev_ });
    if (ap_.print) {
        print_row(std::to_string(s_), std::to_string(runs), std::to_string(np), full(dfbestrun_), full(dfbest_),
                std::to_string(dfev_));
        fflush(stdout);
    }
    s_++;
}

// :292-308
bool AmalgamEngine::driver_converged() const
{
    if (dfev_ >= params_.mfev) return true;
    return dfbestrun_ != dfbestrunold_ && std::fabs(dfbestrun_ - dfbestrunold_) <= params_.tol;
}

void AmalgamEngine::iterate()
{
    if (!driver()) {
        Engine::iterate();
        return;
    }
    enter("iterate()");
    driver_stage();
}

int AmalgamEngine::run(int max_generations)
{
    if (!driver()) return Engine::run(max_generations);
    enter("run()");
    int done = 0;
    // optimize() iterates before it tests (:246-255); a later call goes on only while not converged
    while (done < max_generations && (s_ == 0 || !driver_converged())) {
        driver_stage();
        done++;
    }
    return done;
}

void AmalgamEngine::optimize(int n, const double *lower, const double *upper, const double *guess,
        const ObjectiveSpec &obj, double *x_out, int *n_evals, int *converged)
{
    if (!driver()) {
        Engine::optimize(n, lower, upper, guess, obj, x_out, n_evals, converged);
        return;
    }
    init(n, lower, upper, guess, obj);
    run(std::numeric_limits<int>::max());
    solution(0, x_out, n_evals, converged);
}

// :236-244: row 0 of the population -- after a generation the resampled elite row -- or the driver's best
void AmalgamEngine::solution(int population, double *x_out, int *n_evals, int *converged)
{
    if (driver()) {
        enter("solution()");
        BBO_REQUIRE(population == 0, "population index out of range");
        std::copy(dbest_.begin(), dbest_.end(), x_out);
        *n_evals = dfev_;
        *converged = driver_converged() ? 1 : 0;
        return;
    }
    enter_population("solution()", population);
    AmalgamScal s;
    scal_.download(&s, 1, population);
    int first = 0;
    if (s.it == 0) order_.download(&first, 1, (size_t) population * c_.np);    // (the sorted row 0)
    report_solution(s, X_, ((size_t) population * c_.np + first) * c_.ld, c_.n, c_.ld, x_out, n_evals, converged);
}

int AmalgamEngine::get(const std::string &k, int p, double *out, int cap)
{
    const StateOut o { out, cap };
    if (driver()) {
        enter("get()");
        BBO_REQUIRE(p == 0, "population index out of range");
        if (k == "stages") {
            std::vector<double> t;
            for (const auto &st : stages_) {
                const double row[6] = { (double) st.s, (double) st.runs, (double) st.np, st.fbestrun, st.fbest,
                        (double) st.fev };
                t.insert(t.end(), row, row + 6);
            }
            return o.copy(t.data(), (int) t.size());
        }
        if (k == "fbest") return o.one(dfbest_);
        if (k == "xbest") return o.copy(dbest_.data(), dn_);
        if (k == "s") return o.one(s_);
        if (k == "budget") return o.one(budget_);
        if (k == "fev") return o.one(dfev_);
        if (k == "nbase") return o.one(nbase_);
        if (k == "n") return o.one(dn_);
        throw Error(BBO_ERR_KEY, "unknown state key '" + k + "' (parameter-free mode)");
    }
    enter_population("get()", p);
    const AmalgamConst &c = c_;
    AmalgamScal s;
    scal_.download(&s, 1, p);
    const size_t pb = (size_t) p * c.np, pv = (size_t) p * c.ld, pm = (size_t) p * c.ld;
    if (k == "profile") return profile_report(out, cap);
    if (k == "mu") return o.vec(mu_, pv, c.n);
    if (k == "muold") return o.vec(muold_, pv, c.n);
    if (k == "mushift") return o.vec(mushift_, pv, c.n);
    if (k == "xbest") return o.vec(xbest_, pv, c.n);
    if (k == "xelite") return o.vec(xelite_, pv, c.n);
    if (k == "cov") return o.rows(cov_, pm, c.n, c.n, c.ld);
    if (k == "chol") return o.rows(chol_, pm, c.n, c.n, c.ld);
    if (k == "arx") return o.rows(X_, pb, c.np, c.n, c.ld);
    if (k == "arz") return o.rows(Z_, pb, c.np, c.n, c.ld);
    if (k == "fit_val") return o.vec(f_, pb, c.np);
    if (k == "fit_idx") return o.ints(order_, pb, c.np);
    if (k == "shifted") return o.ints(shifted_, pb, c.np);
    if (k == "cmult") return o.one(s.cmult);
    if (k == "sdr") return o.one(s.sdr);
    if (k == "fbest") return o.one(s.fbest);
    if (k == "nis") return o.one(s.nis);
    if (k == "t") return o.one(s.t);
    if (k == "it") return o.one(s.it);
    if (k == "fev") return o.one(s.fev);
    if (k == "np") return o.one(c.np);
    if (k == "ss") return o.one(c.ss);
    if (k == "nams") return o.one(c.nams);
    if (k == "nismax") return o.one(c.nismax);
    if (k == "n") return o.one(c.n);
    if (k == "etasigma") return o.one(c.etasigma);
    if (k == "etashift") return o.one(c.etashift);
    if (k == "flag" || k == "stop") return o.one(s.stop);
    if (k == "conv") return o.one(s.conv);
    if (k == "fact_fail") return o.one(s.fact_fail);
    if (k == "fail_at") return o.one(s.fail_at);
    if (k == "route") {
        const double r[2] = { (double) c.slabs, (double) c.lds_factor };
        return o.copy(r, 2);
    }
    throw Error(BBO_ERR_KEY, "unknown state key '" + k + "'");
}

int AmalgamEngine::set(const std::string &k, int p, const double *in, int count)
{
    if (driver()) throw Error(BBO_ERR_KEY, "unknown or read-only state key '" + k + "' (parameter-free mode)");
    enter_population("set()", p);
    const AmalgamConst &c = c_;
    if (k == "profile") return profile_enable(in, K_COUNT, K_NAMES);
    if (k == "cov") {
        BBO_REQUIRE(count == c.n * c.n, "cov: n * n values");
        upload_rows(cov_, (size_t) p * c.ld, c.n, c.n, c.ld, in);
        return count;
    }
    if (k == "mu") {
        BBO_REQUIRE(count == c.n, "mu: n values");
        mu_.upload(in, c.n, (size_t) p * c.ld);
        return count;
    }
    if (k == "fit_val") {
        BBO_REQUIRE(count == c.np, "fit_val: np values");
        f_.upload(in, c.np, (size_t) p * c.np);
        return count;
    }
    if (k == "etasigma") {      // (the whole handle: 0 keeps a crafted cov through the distribution phase)
        BBO_REQUIRE(count == 1 && in[0] >= 0. && in[0] <= 1., "etasigma: one value in [0, 1]");
        c_.etasigma = in[0];
        return 1;
    }
    if (k == "cmult" || k == "fev" || k == "nis") {
        BBO_REQUIRE(count == 1 && in[0] >= 0., "cmult / fev / nis: one value, not negative");
        AmalgamScal s;
        scal_.download(&s, 1, p);
        if (k == "cmult") s.cmult = in[0];
        else if (k == "fev") s.fev = (int) in[0];
        else s.nis = (int) in[0];
        scal_.upload(&s, 1, p);
        return 1;
    }
    throw Error(BBO_ERR_KEY, "unknown or read-only state key '" + k + "'");
}

Optimizer* make_amalgam_engine(const bbo_params &p)
{
    return new AmalgamEngine(p);
}

} // namespace bbo
