// bbo_hees.hip -- host side of the HEES engine.  Reference behaviour restated on the host:
// Hees::Hees / init / optimize / solution (hees.cpp:39-199).
#include "bbo_hees_kernels.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>

namespace bbo {

namespace {
enum { K_DRAW = 0, K_ORTHO, K_POINTS, K_RANK, K_UPDATE, K_ADAPT, K_FINISH, K_COUNT };
static const char *const K_NAMES[K_COUNT] = { "bbo:hees_draw", "bbo:hees_ortho", "bbo:hees_points",
        "bbo:hees_rank", "bbo:hees_update", "bbo:hees_adapt", "bbo:hees_finish" };

// the reference's adaptive mu (hees.cpp:70)
int adaptive_mu(int n)
{
    return static_cast<int>(2. + 1.5 * std::log(1. * n));
}
}

HeesEngine::HeesEngine(const bbo_params &p) :
        Engine(checked(p))
{
    bbo_hees_params_default(&hp_);
}

const bbo_params &HeesEngine::checked(const bbo_params &p)
{
    BBO_REQUIRE(p.algo == BBO_ALGO_HEES, "HeesEngine: bad algo");
    return p;
}

void HeesEngine::configure(const bbo_hees_params &hp)
{
    if (inited_) throw Error(BBO_ERR_STATE, "bbo_hees_configure after bbo_init");
    hp_ = hp;
}

void HeesEngine::init(int n, const double *lower, const double *upper, const double *guess,
        const ObjectiveSpec &obj)
{
    reject_program(obj, "HEES");
    BBO_REQUIRE(n >= 1 && n <= HEES_MAX_N, "HEES: dimension must be in [1, 512]");
    const int mu = params_.np > 0 ? params_.np : adaptive_mu(n);
    BBO_REQUIRE(mu >= 1 && mu <= HEES_MAX_MU, "HEES: mu (np, or int(2 + 1.5 ln n)) must be at most 4096");
    BBO_HIP(hipSetDevice(params_.device));
    obj_ = obj;
    const int P = params_.populations;
    HeesConst &c = c_;
    const int ortho_global = c.ortho_global, force_fma = c.force_fma;
    c = HeesConst {};
    c.n = n;
    c.ld = round_up(n, 4);
    c.mu = mu;
    c.B = static_cast<int>(std::ceil((1. * mu) / n));
    c.obj = obj.fused() ? obj.builtin : OBJ_HOST;
    c.mfev = params_.mfev;
    c.npop = P;
    c.ortho_global = ortho_global;
    c.force_fma = force_fma;
    c.tol = params_.tol;
    c.kappa = 3.;
    c.etaA = 0.5;
    c.chi = std::sqrt(1. * n) * (1. - 1. / (4. * n) + 1. / (21. * n * n));
    c.seed = params_.seed;

    // weights, hees.cpp:80-97
    std::vector<double> w(2 * mu);
    double wsum = 0.;
    for (int i = 0; i < 2 * mu; i++) {
        w[i] = std::log(mu + 0.5) - std::log(std::min(1. + i, mu + 0.5));
        wsum += w[i];
    }
    const double wscale = 1. / wsum;
    double w2 = 0.;
    for (int i = 0; i < 2 * mu; i++) {
        w[i] *= wscale;
        w2 += w[i] * w[i];
    }
    const double mueff = 1. / w2;
    const double mueffm = 1. / (1. / mueff - 1. / (2. * mu - 1.) * (1. - 1. / mueff));
    c.cs = (mueffm + 2.) / (n + mueffm + 3.);
    c.ds = 1. + c.cs + 2. * std::max(0., std::sqrt((mueff - 1.) / (n + 1.)) - 1.);
    c.csc = std::sqrt(c.cs * (2. - c.cs) * mueffm);

    const size_t ld = c.ld, rows = (size_t) P * mu;
    A_.alloc((size_t) P * n * ld);
    m_.alloc(P * ld);
    mprev_.alloc(P * ld);
    ps_.alloc(P * ld);
    xbest_.alloc(P * ld);
    b_.alloc(rows * ld);
    norms_.alloc(rows);
    Y_.alloc(rows * ld);
    X_.alloc(obj_.needs_host() ? 2 * rows * ld : 0);
    f_.alloc(2 * rows);
    fmh_.alloc(P);
    hess_.alloc(rows);
    q_.alloc(rows);
    coef_.alloc(rows);
    dw_.alloc(rows);
    w_.alloc(2 * mu);
    zin_.alloc(0);
    zlast_.alloc(record_ ? rows * ld : 0);
    order_.alloc(2 * rows);
    rank_.alloc(2 * rows);
    scal_.alloc(P);
    upload_box(n, c.ld, lower, upper, obj);
    w_.upload(w.data(), 2 * mu);
    {
        std::vector<double> mm(P * ld, 0.);
        for (int p = 0; p < P; p++)
            std::copy(guess + (size_t) p * n, guess + (size_t) (p + 1) * n, mm.begin() + p * ld);
        m_.upload(mm.data(), mm.size());
        mprev_.upload(mm.data(), mm.size());
        const std::vector<uint64_t> seeds(64, c.seed);
        lane_seed_.alloc(64);
        lane_seed_.upload(seeds.data(), 64);
    }
    std::vector<HeesScal> sc(P);
    for (auto &s : sc) {
        std::memset(&s, 0, sizeof(s));
        s.sigma = s.sigma_prev = params_.sigma0;
        s.fev = 1;
        s.fbest = std::numeric_limits<double>::infinity();
    }
    scal_.upload(sc.data(), P);

    HeesDev &d = d_;
    d = HeesDev {};
    d.A = A_.p; d.m = m_.p; d.mprev = mprev_.p; d.ps = ps_.p; d.xbest = xbest_.p; d.b = b_.p;
    d.norms = norms_.p; d.Y = Y_.p; d.X = X_.p; d.f = f_.p; d.fmh = fmh_.p; d.hess = hess_.p; d.q = q_.p;
    d.coef = coef_.p; d.dw = dw_.p; d.w = w_.p; d.zin = nullptr; d.zlast = zlast_.p;
    d.order = order_.p; d.rank = rank_.p; d.aux = aux_.p; d.lane_seed = lane_seed_.p; d.scal = scal_.p;
    c.honor_stop = 0;
    allow_lds((const void*) hees_ortho, HEES_ORTHO_LDS);
    allow_lds((const void*) hees_points_mfma, 32 * HEES_MAX_N * (int) sizeof(double));
    inited_ = true;
    sampled_ = false;
    hipLaunchKernelGGL(hees_eye, dim3(P), dim3(256), 0, stream_, d_, c_);      // (alloc zeroed A)
    BBO_HIP(hipGetLastError());
    part_finish(true);
    BBO_HIP(hipStreamSynchronize(stream_));
}

// f at the mean through a host objective (hees.cpp:332)
void HeesEngine::host_mean()
{
    BBO_HIP(hipStreamSynchronize(stream_));
    const int P = c_.npop, ld = c_.ld;
    std::vector<HeesScal> sc(P);
    scal_.download(sc.data(), P);
    std::vector<double> mh((size_t) P * ld), fh(P);
    m_.download(mh.data(), mh.size());
    fmh_.download(fh.data(), P);
    for (int p = 0; p < P; p++) {
        if (c_.honor_stop && sc[p].stop) continue;
        obj_.eval_host(mh.data() + (size_t) p * ld, 1, c_.n, ld, &fh[p]);
        nan_to_inf(&fh[p], 1);
    }
    fmh_.upload(fh.data(), P);
}

void HeesEngine::part_sample()
{
    const HeesConst &c = c_;
    const int P = c.npop;
    const dim3 rows((c.mu + 3) / 4, P);
    timed(K_DRAW, [&] {
        if (d_.zin) hipLaunchKernelGGL(hees_take, rows, dim3(256), 0, stream_, d_, c_);
        else {
            hipLaunchKernelGGL(hees_draw, rows, dim3(256), 0, stream_, d_, c_);
            hipLaunchKernelGGL(hees_settle, rows, dim3(256), 0, stream_, d_, c_);
        }
    });
    const size_t batch = (size_t) std::min(c.n, c.mu) * c.ld * sizeof(double);
    const int use_lds = !c.ortho_global && batch <= (size_t) HEES_ORTHO_LDS ? 1 : 0;
    timed(K_ORTHO, [&] {
        // (a batch of 64 rows and more: 16 wavefronts, whose rows hide one another's latency)
        hipLaunchKernelGGL(hees_ortho, dim3(c.B, P), dim3(std::min(c.n, c.mu) >= 64 ? 1024 : 256),
                use_lds ? batch : 0, stream_, d_, c_, use_lds);
    });
    timed(K_POINTS, [&] {
        if (use_mfma())
            hipLaunchKernelGGL(hees_points_mfma, dim3((c.mu + 15) / 16, P), dim3(256),
                    (size_t) 32 * c.ld * sizeof(double), stream_, d_, c_);
        else
            hipLaunchKernelGGL(hees_points, rows, dim3(256), (size_t) 12 * c.ld * sizeof(double), stream_, d_, c_);
    });
    if (obj_.needs_host()) host_evaluate_rows(X_, f_, 2 * c.mu, c.n, c.ld, c.honor_stop);
    sampled_ = true;
}

void HeesEngine::part_rank()
{
    timed(K_RANK, [&] {
        hipLaunchKernelGGL(hees_rank, dim3((2 * c_.mu + 31) / 32, c_.npop), dim3(256), 0, stream_, d_, c_);
    });
}

void HeesEngine::part_update()
{
    const int t = (c_.n + 15) / 16;
    timed(K_UPDATE, [&] { hipLaunchKernelGGL(hees_update, dim3(c_.npop), dim3(256), 0, stream_, d_, c_); });
    sampled_ = false;
    timed(K_ADAPT, [&] {
        if (use_mfma()) hipLaunchKernelGGL(hees_adapt_mfma, dim3(t, t, c_.npop), dim3(256), 0, stream_, d_, c_);
        else hipLaunchKernelGGL(hees_adapt, dim3(t, t, c_.npop), dim3(256), 0, stream_, d_, c_);
    });
}

void HeesEngine::part_finish(bool init_only)
{
    if (obj_.needs_host()) host_mean();
    timed(K_FINISH, [&] {
        hipLaunchKernelGGL(hees_finish, dim3(c_.npop), dim3(256), 0, stream_, d_, c_, init_only ? 1 : 0);
    });
}

void HeesEngine::generation(bool honor_stop)
{
    c_.honor_stop = honor_stop ? 1 : 0;
    part_sample();
    part_rank();
    part_update();
    part_finish(false);
}

void HeesEngine::phase(int which)
{
    run_phase("phase()", which, 4, "HEES phase: 0 sample, 1 rank, 2 update, 3 finish", [&] {
        c_.honor_stop = 0;
        if (which == 0) part_sample();
        else if (which == 1) part_rank();
        else if (which == 2) part_update();
        else part_finish(false);
    });
}

void HeesEngine::inject_normals(const double *z, int count)
{
    enter("inject_normals()");
    BBO_HIP(hipStreamSynchronize(stream_));
    if (!z) {
        zin_.alloc(0);
        d_.zin = nullptr;
        return;
    }
    const HeesConst &c = c_;
    const size_t table = (size_t) c.B * c.n * c.n;
    BBO_REQUIRE(count >= 0 && (size_t) count == table * c.npop,
            "HEES inject_normals: populations tables of (B n) x n normals, B = ceil(mu / n)");
    // the first mu rows of every table are taken, the rest is what the reference draws and never uses
    std::vector<double> rows((size_t) c.npop * c.mu * c.ld, 0.);
    for (int p = 0; p < c.npop; p++)
        for (int r = 0; r < c.mu; r++)
            std::copy(z + p * table + (size_t) r * c.n, z + p * table + (size_t) (r + 1) * c.n,
                    rows.begin() + ((size_t) p * c.mu + r) * c.ld);
    if (zin_.count != rows.size()) zin_.alloc(rows.size());
    zin_.upload(rows.data(), rows.size());
    d_.zin = zin_.p;
}

// hees.cpp:136-199.  mres <= 1: the base's init + loop.  Else runs of a fresh HEES from the
// remaining budget, mu doubling, the restart points uniform in the box from the second run on.
void HeesEngine::optimize(int n, const double *lower, const double *upper, const double *guess,
        const ObjectiveSpec &obj, double *x_out, int *n_evals, int *converged)
{
    if (hp_.mres <= 1) {
        Engine::optimize(n, lower, upper, guess, obj, x_out, n_evals, converged);
        return;
    }
    BBO_REQUIRE(params_.populations == 1, "HEES: restarts (mres > 1) work on populations = 1 only");
    BBO_REQUIRE(n >= 1 && n <= HEES_MAX_N, "HEES: dimension must be in [1, 512]");
    require_finite_box("HEES: restarts (mres > 1) draw their start points from [lower, upper]: the bounds "
            "must be finite", n, lower, upper);
    const bbo_params saved = params_;
    auto row = [](const std::string &a, const std::string &b, const std::string &c) {
        printf(" | %5s | %25s | %10s | \n", a.c_str(), b.c_str(), c.c_str());
    };
    if (hp_.print) {
        row("iter", "f*", "fev");
        printf(" |%s| \n", std::string(5 + 25 + 10 + 3 * 2 + 2, '=').c_str());
        fflush(stdout);
    }
    int mu = saved.np > 0 ? saved.np : adaptive_mu(n);
    int fev = 0;
    double fbest = std::numeric_limits<double>::infinity();
    std::vector<double> x0(guess, guess + n), xbest(guess, guess + n);
    runs_.clear();
    try {
        for (int res = 1; res <= hp_.mres; res++) {
            params_.mfev = saved.mfev - fev;
            params_.np = mu;
            params_.seed = saved.seed + (uint64_t) (res - 1);
            init(n, lower, upper, x0.data(), obj);
            run(std::numeric_limits<int>::max());
            HeesScal s;
            scal_.download(&s, 1, 0);
            if (s.fbest < fbest) {
                fbest = s.fbest;
                std::vector<double> xb(c_.ld);
                xbest_.download(xb.data(), c_.ld, 0);
                std::copy(xb.begin(), xb.begin() + n, xbest.begin());
            }
            fev += s.fev;
            runs_.push_back(mu);
            runs_.push_back(s.fev);
            runs_.push_back(s.fbest);
            if (hp_.print) {
                char buf[64];
                snprintf(buf, sizeof(buf), "%.17g", fbest);
                row(std::to_string(res), buf, std::to_string(fev));
                fflush(stdout);
            }
            if (fev >= saved.mfev) break;
            mu <<= 1;
            // the next start point: coordinate j of restart `res` (hees.cpp:194-196)
            for (int j = 0; j < n; j++) {
                const u32x4 wd = philox4x32_10_uniform(saved.seed, (uint32_t) j, 0, (uint32_t) res,
                        stream_word(STREAM_RESTART, 0));
                x0[j] = u01(wd.x, wd.y) * (upper[j] - lower[j]) + lower[j];
            }
        }
    } catch (...) {
        params_ = saved;
        throw;
    }
    params_ = saved;
    std::copy(xbest.begin(), xbest.end(), x_out);
    *n_evals = fev;
    *converged = 0;
}

void HeesEngine::solution(int population, double *x_out, int *n_evals, int *converged)
{
    enter_population("solution()", population);
    HeesScal s;
    scal_.download(&s, 1, population);
    report_solution(s, xbest_, (size_t) population * c_.ld, c_.n, c_.ld, x_out, n_evals, converged);
}

int HeesEngine::get(const std::string &k, int p, double *out, int cap)
{
    enter_population("get()", p);
    const HeesConst &c = c_;
    HeesScal s;
    scal_.download(&s, 1, p);
    const size_t pb = (size_t) p * c.mu, pv = (size_t) p * c.ld;
    const StateOut o { out, cap };
    if (k == "profile") return profile_report(out, cap);
    if (k == "A") return o.rows(A_, (size_t) p * c.n, c.n, c.n, c.ld);
    if (k == "xmean") return o.vec(m_, pv, c.n);
    if (k == "xbest") return o.vec(xbest_, pv, c.n);
    if (k == "ps") return o.vec(ps_, pv, c.n);
    if (k == "b") return o.rows(b_, pb, c.mu, c.n, c.ld);
    if (k == "y") return o.rows(Y_, pb, c.mu, c.n, c.ld);
    if (k == "norms") return o.vec(norms_, pb, c.mu);
    if (k == "hess") return o.vec(hess_, pb, c.mu);
    if (k == "q") return o.vec(q_, pb, c.mu);
    if (k == "fit_val") return o.vec(f_, 2 * pb, 2 * c.mu);
    if (k == "fit_idx") return o.ints(order_, 2 * pb, 2 * c.mu);
    if (k == "fit_rank") return o.ints(rank_, 2 * pb, 2 * c.mu);
    if (k == "arx") {
        // x_r = m - sigma y_r, x_{r + mu} = m + sigma y_r about the mean and with the sigma they
        // were sampled with: the arithmetic of hees_points.  Between the sampling and the update
        // of a generation (bbo_hees_phase) those are still the current ones.
        const int cnt = 2 * c.mu * c.n;
        if (o.fits(cnt)) {
            std::vector<double> y((size_t) c.mu * c.ld), m0(c.ld);
            Y_.download(y.data(), y.size(), pb * c.ld);
            const bool current = sampled_ || s.gen == 0;
            const double sig = current ? s.sigma : s.sigma_prev;
            (current ? m_ : mprev_).download(m0.data(), c.ld, pv);
            for (int r = 0; r < c.mu; r++)
                for (int j = 0; j < c.n; j++) {
                    const double sy = sig * y[(size_t) r * c.ld + j];
                    out[(size_t) r * c.n + j] = m0[j] - sy;
                    out[(size_t) (r + c.mu) * c.n + j] = m0[j] + sy;
                }
        }
        return cnt;
    }
    if (k == "zlast") {
        if (!record_) throw Error(BBO_ERR_STATE, "'zlast' needs record_normals");
        return o.rows(zlast_, pb, c.mu, c.n, c.ld);
    }
    if (k == "runs") return o.copy(runs_.data(), (int) runs_.size());
    if (k == "record_normals") return o.one(record_ ? 1. : 0.);
    if (k == "hees_ortho_global") return o.one(c.ortho_global);
    if (k == "hees_force_fma") return o.one(c.force_fma);
    if (k == "hees_mfma") return o.one(use_mfma() ? 1. : 0.);
    if (k == "sigma") return o.one(s.sigma);
    if (k == "gs") return o.one(s.gs);
    if (k == "fm") return o.one(s.fm);
    if (k == "fbest") return o.one(s.fbest);
    if (k == "maxh") return o.one(s.maxh);
    if (k == "m2") return o.one(s.m2);
    if (k == "it") return o.one(s.it);
    if (k == "fev") return o.one(s.fev);
    if (k == "flag" || k == "stop") return o.one(s.stop);
    if (k == "conv") return o.one(s.conv);
    if (k == "mu") return o.one(c.mu);
    if (k == "B") return o.one(c.B);
    if (k == "n") return o.one(c.n);
    if (k == "cs") return o.one(c.cs);
    if (k == "ds") return o.one(c.ds);
    throw Error(BBO_ERR_KEY, "unknown state key '" + k + "'");
}

int HeesEngine::set(const std::string &k, int p, const double *in, int count)
{
    if (k == "hees_ortho_global" || k == "hees_force_fma") {    // (the whole handle; legal before bbo_init too)
        BBO_REQUIRE(count == 1 && (in[0] == 0. || in[0] == 1.), "hees_ortho_global, hees_force_fma: 0 or 1");
        if (inited_) BBO_HIP(hipStreamSynchronize(stream_));
        (k == "hees_ortho_global" ? c_.ortho_global : c_.force_fma) = (int) in[0];
        return 1;
    }
    if (k == "record_normals" && !inited_) {
        BBO_REQUIRE(count == 1, "record_normals: one value");
        record_ = in[0] != 0.;
        return 1;
    }
    enter_population("set()", p);
    const HeesConst &c = c_;
    const size_t pv = (size_t) p * c.ld;
    if (k == "profile") return profile_enable(in, K_COUNT, K_NAMES);
    if (k == "record_normals") {
        BBO_REQUIRE(count == 1, "record_normals: one value");
        record_ = in[0] != 0.;
        if (record_ && !zlast_.p) zlast_.alloc((size_t) c.npop * c.mu * c.ld);
        d_.zlast = record_ ? zlast_.p : nullptr;
        return 1;
    }
    if (k == "A") {
        BBO_REQUIRE(count == c.n * c.n, "A: n * n values");
        upload_rows(A_, (size_t) p * c.n, c.n, c.n, c.ld, in);
        return count;
    }
    if (k == "xmean") {
        BBO_REQUIRE(count == c.n, "xmean: n values");
        m_.upload(in, c.n, pv);
        return count;
    }
    if (k == "sigma") {
        BBO_REQUIRE(count == 1 && in[0] > 0., "sigma: one positive value");
        HeesScal s;
        scal_.download(&s, 1, p);
        s.sigma = in[0];
        scal_.upload(&s, 1, p);
        return 1;
    }
    throw Error(BBO_ERR_KEY, "unknown or read-only state key '" + k + "'");
}

Optimizer* make_hees_engine(const bbo_params &p)
{
    return new HeesEngine(p);
}

} // namespace bbo
