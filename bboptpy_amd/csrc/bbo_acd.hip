// bbo_acd.hip -- host side of the ACD engine.  Reference behaviour restated on the host:
// ACD::ACD / init / optimize / solution (acd.cpp:46-120, :180-196).
#include "bbo_acd_kernels.hpp"
#include "bbo_rng.hpp"

#include <algorithm>
#include <cmath>
#include <limits>

namespace bbo {

namespace {
enum { K_SWEEP = 0, K_EVAL, K_AE, K_EIGEN, K_POST, K_COUNT };
static const char *const K_NAMES[K_COUNT] = { "bbo:acd_sweep", "bbo:acd_eval", "bbo:acd_ae", "bbo:acd_eigen",
        "bbo:acd_post" };
}

// the eigensolver's view of the engine: Cw as its C, V as its B, Dv as its D (bbo_cma.hpp)
struct AcdEngine::EigView {
    CmaDev d {};
    CmaConst c {};
    DevBuf<double> Cw, V, Dv, work;
    DevBuf<CmaScal> scal;
};

AcdEngine::AcdEngine(const bbo_params &p) :
        Engine(checked(p)), eig_(new EigView())
{
    bbo_acd_params_default(&ap_);
}

AcdEngine::~AcdEngine() = default;

// the part of the constructor's arguments that travels in bbo_params
const bbo_params &AcdEngine::checked(const bbo_params &p)
{
    BBO_REQUIRE(p.algo == BBO_ALGO_ACD, "AcdEngine: bad algo");
    BBO_REQUIRE(p.mfev >= 1, "ACD: mfev must be positive");
    BBO_REQUIRE(p.tol == p.tol && p.stol == p.stol, "ACD: ftol and xtol must not be NaN");
    return p;
}

void AcdEngine::configure(const bbo_acd_params &ap)
{
    if (inited_) throw Error(BBO_ERR_STATE, "bbo_acd_configure after bbo_init");
    BBO_REQUIRE(ap.ksucc >= 0. && ap.kunsucc >= 0., "ACD: ksucc and kunsucc must not be negative");
    BBO_REQUIRE(ap.from_guess == 0 || ap.from_guess == 1, "ACD: from_guess is 0 or 1");
    // (built, bit-identical and measured: faster for one population, slower for 4096, so dropped as the
    // issue rules; DESIGN.md section 3.16 has both timings)
    BBO_REQUIRE(ap.speculate == 0, "ACD: the speculative sweep was measured and dropped (speculate must be 0)");
    ap_ = ap;
}

// Random::get(lower, upper) over the raw uniform (random.hpp:329-337), as crs_init draws its pool
void AcdEngine::draw_xbest(uint32_t sub, double *x) const
{
    for (int j = 0; j < c_.n; j++) {
        const u32x4 w = philox4x32_10(c_.seed, 0u, (uint32_t) j, 0u, stream_word(STREAM_ACD_INIT, sub));
        const double a = lower_h_[j], b = upper_h_[j];
        const double lo = a < b ? a : b, hi = a < b ? b : a;
        x[j] = u01(w.x, w.y) * (hi - lo) + lo;
    }
}

void AcdEngine::init(int n, const double *lower, const double *upper, const double *guess,
        const ObjectiveSpec &obj)
{
    reject_program(obj, "ACD");
    BBO_REQUIRE(n >= 1 && n <= ACD_MAX_N, "ACD: dimension must be in [1, 128]");
    require_finite_box("ACD draws x_best from [lower, upper] and takes sigma from its width: the bounds must be finite",
            n, lower, upper);
    BBO_HIP(hipSetDevice(params_.device));
    obj_ = obj;
    const int P = params_.populations;
    BBO_REQUIRE(P <= (1 << 24), "ACD: populations must be <= 2^24");
    AcdConst &c = c_;
    c = AcdConst {};
    c.n = n;
    c.ld = round_up(n, 16);
    c.obj = obj.fused() ? obj.builtin : OBJ_HOST;
    c.mfev = params_.mfev;
    c.npop = P;
    c.cp = 10 + static_cast<int>(20 * std::pow(1. * n, 1.5));      // :118
    c.ftol = params_.tol;
    c.xtol = params_.stol;
    c.ksucc = ap_.ksucc;
    c.kunsucc = ap_.kunsucc;
    c.c1 = 0.5 / n;
    c.cpath = 1. / std::sqrt(1. * n);
    c.seed = params_.seed;

    const size_t ld = c.ld, vec = (size_t) P * ld, mat = vec * ld;
    xbest_.alloc(vec); sigma_.alloc(vec); p_.alloc(vec); m_.alloc(vec); mold_.alloc(vec); diagd_.alloc(vec);
    colmax_.alloc(vec);
    Bt_.alloc(mat); invBt_.alloc(mat); C_.alloc(mat);
    X_.alloc((size_t) P * 2 * n * ld);
    f_.alloc((size_t) P * 2 * n);
    order_.alloc((size_t) P * 2 * n);
    fhist_.alloc((size_t) P * c.cp);
    cand_.alloc((size_t) P * 2 * ld);
    value_.alloc((size_t) P * 2);
    flags_.alloc(2);
    scal_.alloc(P);
    EigView &e = *eig_;
    e.Cw.alloc(mat); e.V.alloc(mat); e.Dv.alloc(vec);
    e.work.alloc(n > 1 ? (size_t) P * eigen_view_scratch(c.ld) : 0);
    e.scal.alloc(P);
    upload_box(n, c.ld, lower, upper, obj);
    {
        std::vector<double> xb(vec, 0.), sg(vec, 0.);
        for (int p = 0; p < P; p++) {
            if (ap_.from_guess) std::copy(guess + (size_t) p * n, guess + (size_t) (p + 1) * n, xb.begin() + p * ld);
            else draw_xbest((uint32_t) p, xb.data() + p * ld);                       // :82
            for (int j = 0; j < n; j++) sg[p * ld + j] = (upper[j] - lower[j]) / 4.;    // :83
        }
        xbest_.upload(xb.data(), vec);
        sigma_.upload(sg.data(), vec);
        std::vector<int> ord((size_t) P * 2 * n);
        for (size_t k = 0; k < ord.size(); k++) ord[k] = (int) (k % (2 * n));           // :93
        order_.upload(ord.data(), ord.size());
        std::vector<AcdScal> sc(P);
        std::memset(sc.data(), 0, sizeof(AcdScal) * P);
        for (auto &s : sc) s.fbest = std::numeric_limits<double>::infinity();           // :76
        scal_.upload(sc.data(), P);
    }

    AcdDev &d = d_;
    d = AcdDev {};
    d.xbest = xbest_.p; d.sigma = sigma_.p; d.p = p_.p; d.m = m_.p; d.mold = mold_.p; d.diagd = diagd_.p;
    d.colmax = colmax_.p; d.Bt = Bt_.p; d.invBt = invBt_.p; d.C = C_.p; d.Cw = e.Cw.p; d.V = e.V.p; d.Dv = e.Dv.p;
    d.X = X_.p; d.f = f_.p; d.order = order_.p; d.fhist = fhist_.p; d.cand = cand_.p; d.value = value_.p;
    d.flags = flags_.p; d.eigscal = e.scal.p;
    d.lower = lower_.p; d.upper = upper_.p; d.aux = aux_.p; d.scal = scal_.p;
    e.d = CmaDev {};
    e.d.C = e.Cw.p; e.d.B = e.V.p; e.d.D = e.Dv.p; e.d.eig_work = e.work.p; e.d.scal = e.scal.p;
    e.d.mw_fault = -1;
    e.c = CmaConst {};
    e.c.n = n; e.c.ld = c.ld; e.c.npop = P; e.c.eigenfreq = 0.5;
    inited_ = true;

    hipLaunchKernelGGL(acd_init, dim3(P), dim3(ACD_THREADS), 0, stream_, d_, c_);
    BBO_HIP(hipGetLastError());
    BBO_HIP(hipStreamSynchronize(stream_));
}

void AcdEngine::launch_sweep(int mode, int k, bool begin)
{
    timed(K_SWEEP, [&] {
        hipLaunchKernelGGL(acd_sweep, dim3(c_.npop), dim3(ACD_THREADS), 0, stream_, d_, c_, mode, k, begin ? 1 : 0);
    });
}

// the values of every population's pending pair, x1 then x2
void AcdEngine::launch_eval()
{
    if (!obj_.needs_host()) {
        timed(K_EVAL, [&] { hipLaunchKernelGGL(acd_eval, dim3(c_.npop), dim3(ACD_THREADS), 0, stream_, d_, c_); });
        return;
    }
    // in population order, f1 then f2 (:131-132)
    host_evaluate_pending(c_.honor_stop != 0, [&](int p, const AcdScal&) {
        return PendingPoints { &cand_, (size_t) p * 2 * c_.ld, 2, c_.ld, &value_ };
    });
}

// acd_ae, the decomposition and acd_post: no-ops for the populations that are not due
void AcdEngine::launch_update()
{
    timed(K_AE, [&] { hipLaunchKernelGGL(acd_ae, dim3(c_.npop), dim3(ACD_THREADS), 0, stream_, d_, c_); });
    if (c_.n > 1) {
        eig_->c.honor_stop = 0;
        timed(K_EIGEN, [&] { launch_eigen_view(stream_, eig_->d, eig_->c); });
    }
    timed(K_POST, [&] { hipLaunchKernelGGL(acd_post, dim3(c_.npop), dim3(ACD_THREADS), 0, stream_, d_, c_); });
}

// k coordinate steps of every population with a device objective: a launch ends with the sweep or where an
// update is due, so the host relaunches while a flag says that some population is short of its goal
void AcdEngine::fused(int k)
{
    for (bool begin = true;; begin = false) {
        BBO_HIP(hipMemsetAsync(flags_.p, 0, 2 * sizeof(int), stream_));
        launch_sweep(ACD_FUSED, k, begin);
        BBO_HIP(hipStreamSynchronize(stream_));
        int fl[2] = { 0, 0 };
        flags_.download(fl, 2);
        if (fl[1]) launch_update();
        if (!fl[0]) break;
    }
}

// one iterate() of every population; with a host objective the same step entered and left at its evaluations
void AcdEngine::generation(bool honor_stop)
{
    c_.honor_stop = honor_stop ? 1 : 0;
    if (!obj_.needs_host()) {
        fused(1);
        return;
    }
    BBO_HIP(hipMemsetAsync(flags_.p, 0, 2 * sizeof(int), stream_));
    launch_sweep(ACD_ADVANCE, 1, true);
    launch_eval();
    launch_sweep(ACD_ABSORB, 1, false);
    BBO_HIP(hipStreamSynchronize(stream_));
    int fl[2] = { 0, 0 };
    flags_.download(fl, 2);
    if (fl[1]) launch_update();
}

// bbo_run: `gens` coordinate steps per population
void AcdEngine::launch_chunk(int gens)
{
    if (obj_.needs_host()) {
        Engine::launch_chunk(gens);
        return;
    }
    c_.honor_stop = 1;
    fused(gens);
}

void AcdEngine::phase(int which)
{
    run_phase("bbo_acd_phase", which, 3, "bbo_acd_phase: 0 form x1 and x2, 1 evaluate, 2 absorb", [&] {
        c_.honor_stop = 0;
        if (which == 0) {
            launch_sweep(ACD_ADVANCE, 1, true);
        } else if (which == 1) {
            launch_eval();
        } else {
            launch_sweep(ACD_ABSORB, 1, false);
            launch_update();
        }
    });
}

// converged() (:204-228) of population p as it stands, on the host: solution() asks again, and before
// the first step nothing on the device has
int AcdEngine::converged_now(int p, const AcdScal &s, int *rule) const
{
    const int n = c_.n, cp = c_.cp;
    *rule = 0;
    if (s.it > cp) {
        double f0 = 0., f1 = 0.;
        fhist_.download(&f0, 1, (size_t) p * cp + (size_t) ((s.it - 1 + cp) % cp));
        fhist_.download(&f1, 1, (size_t) p * cp + (size_t) (s.it % cp));
        if (std::fabs(f1 - f0) < c_.ftol) {
            *rule = 1;
            return 1;
        }
    }
    std::vector<double> sg(n), cm(n);
    sigma_.download(sg.data(), n, (size_t) p * c_.ld);
    colmax_.download(cm.data(), n, (size_t) p * c_.ld);
    double dxmax = 0.;
    for (int j = 0; j < n; j++) dxmax = std::max(dxmax, std::fabs(sg[j] * cm[j]));
    if (dxmax < c_.xtol) {
        *rule = 2;
        return 1;
    }
    return 0;
}

void AcdEngine::solution(int population, double *x_out, int *n_evals, int *converged)
{
    enter_population("solution()", population);
    AcdScal s;
    scal_.download(&s, 1, population);
    int rule = 0;
    s.conv = converged_now(population, s, &rule);       // :180-182
    report_solution(s, xbest_, (size_t) population * c_.ld, c_.n, c_.ld, x_out, n_evals, converged);
}

namespace {
// [n][n] row-major of the caller <-> the transposed [ld][ld] of the device
void transpose_out(const std::vector<double> &T, int n, int ld, double *out)
{
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) out[(size_t) i * n + j] = T[(size_t) j * ld + i];
}
std::vector<double> transpose_in(const double *in, int n, int ld)
{
    std::vector<double> T((size_t) ld * ld, 0.);
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) T[(size_t) j * ld + i] = in[(size_t) i * n + j];
    return T;
}
}

int AcdEngine::get(const std::string &k, int p, double *out, int cap)
{
    enter_population("get()", p);
    const AcdConst &c = c_;
    AcdScal s;
    scal_.download(&s, 1, p);
    const size_t pv = (size_t) p * c.ld, pm = pv * c.ld;
    const int n = c.n, ld = c.ld;
    const StateOut o { out, cap };
    if (k == "profile") return profile_report(out, cap);
    if (k == "xbest") return o.vec(xbest_, pv, n);
    if (k == "sigma") return o.vec(sigma_, pv, n);
    if (k == "p") return o.vec(p_, pv, n);
    if (k == "m") return o.vec(m_, pv, n);
    if (k == "mold") return o.vec(mold_, pv, n);
    if (k == "diagd") return o.vec(diagd_, pv, n);
    if (k == "colmax") return o.vec(colmax_, pv, n);
    if (k == "B" || k == "invB") {
        if (o.fits(n * n)) {
            std::vector<double> T((size_t) ld * ld);
            (k == "B" ? Bt_ : invBt_).download(T.data(), T.size(), pm);
            transpose_out(T, n, ld, out);
        }
        return n * n;
    }
    if (k == "C") return o.rows(C_, pv, n, n, ld);
    if (k == "V") return o.rows(eig_->V, pv, n, n, ld);
    if (k == "x") return o.rows(X_, (size_t) p * 2 * n, 2 * n, n, ld);
    if (k == "f") return o.vec(f_, (size_t) p * 2 * n, 2 * n);
    if (k == "order") return o.ints(order_, (size_t) p * 2 * n, 2 * n);
    if (k == "fhist") return o.vec(fhist_, (size_t) p * c.cp, c.cp);
    if (k == "cand") return o.rows(cand_, (size_t) p * 2, 2, n, ld);
    if (k == "value") return o.vec(value_, (size_t) 2 * p, 2);
    if (k == "fbest") return o.one(s.fbest);
    if (k == "fev") return o.one(s.fev);
    if (k == "it") return o.one(s.it);
    if (k == "itae") return o.one(s.itae);
    if (k == "ix") return o.one(s.ix);
    if (k == "improved") return o.one(s.improved);
    if (k == "due") return o.one(s.due);
    if (k == "pending") return o.one(s.pending);
    if (k == "flag" || k == "stop") return o.one(s.stop);
    if (k == "rule") return o.one(s.rule);
    if (k == "conv") {
        int rule = 0;
        return o.one(converged_now(p, s, &rule));
    }
    if (k == "cp") return o.one(c.cp);
    if (k == "chunk") return o.one(params_.poll_every > 0 ? params_.poll_every : default_poll());
    if (k == "n") return o.one(n);
    throw Error(BBO_ERR_KEY, "unknown state key '" + k + "'");
}

int AcdEngine::set(const std::string &k, int p, const double *in, int count)
{
    enter_population("set()", p);
    const AcdConst &c = c_;
    const size_t pv = (size_t) p * c.ld, pm = pv * c.ld;
    const int n = c.n, ld = c.ld;
    auto whole = [&](double lo, double hi) {
        return count == 1 && in[0] == std::floor(in[0]) && in[0] >= lo && in[0] <= hi;
    };
    if (k == "profile") return profile_enable(in, K_COUNT, K_NAMES);
    DevBuf<double> *vecs[] = { &xbest_, &sigma_, &p_, &m_, &mold_, &diagd_ };
    const char *const vec_names[] = { "xbest", "sigma", "p", "m", "mold", "diagd" };
    for (int v = 0; v < 6; v++)
        if (k == vec_names[v]) {
            BBO_REQUIRE(count == n, "xbest, sigma, p, m, mold, diagd: n values");
            if (v == 1)
                for (int j = 0; j < n; j++) BBO_REQUIRE(in[j] >= 0., "sigma: no negative value");
            vecs[v]->upload(in, n, pv);
            return count;
        }
    if (k == "B" || k == "invB") {      // row-major [n][n]; B: colmax follows
        BBO_REQUIRE(count == n * n, "B, invB: n * n values");
        const std::vector<double> T = transpose_in(in, n, ld);
        (k == "B" ? Bt_ : invBt_).upload(T.data(), T.size(), pm);
        if (k == "B") {
            std::vector<double> cm(n, 0.);
            for (int j = 0; j < n; j++)
                for (int i = 0; i < n; i++) cm[j] = std::max(cm[j], std::fabs(T[(size_t) j * ld + i]));
            colmax_.upload(cm.data(), n, pv);
        }
        return count;
    }
    if (k == "C") {
        BBO_REQUIRE(count == n * n, "C: n * n values");
        upload_rows(C_, pv, n, n, ld, in);
        return count;
    }
    if (k == "x") {                     // the archive in place; nothing is evaluated
        BBO_REQUIRE(count == 2 * n * n, "x: 2 n * n values");
        upload_rows(X_, (size_t) p * 2 * n, 2 * n, n, ld, in);
        return count;
    }
    if (k == "f") {
        BBO_REQUIRE(count == 2 * n, "f: 2 n values");
        std::vector<double> fh(in, in + count);
        nan_to_inf(fh.data(), count);
        f_.upload(fh.data(), count, (size_t) p * 2 * n);
        return count;
    }
    if (k == "order") {
        BBO_REQUIRE(count == 2 * n, "order: 2 n values");
        order_.upload(permutation_of(in, count, "order: a permutation of 0 .. 2 n - 1").data(), count, (size_t) p * 2 * n);
        return count;
    }
    if (k == "fhist") {
        BBO_REQUIRE(count == c.cp, "fhist: cp values");
        fhist_.upload(in, count, (size_t) p * c.cp);
        return count;
    }
    if (k == "value") {                 // (what bbo_acd_phase 2 absorbs)
        BBO_REQUIRE(count == 2, "value: two values");
        double v[2] = { in[0], in[1] };
        nan_to_inf(v, 2);
        value_.upload(v, 2, (size_t) 2 * p);
        return count;
    }
    if (k == "substream") {             // x_best of this population again, from another sub-stream
        BBO_REQUIRE(whole(0., 16777215.), "substream: an integer in [0, 2^24)");
        std::vector<double> xb(n);
        draw_xbest((uint32_t) in[0], xb.data());
        xbest_.upload(xb.data(), n, pv);
        return 1;
    }
    if (k == "fbest" || k == "fev" || k == "it" || k == "itae" || k == "ix" || k == "improved") {
        AcdScal s;
        scal_.download(&s, 1, p);
        if (k == "fbest") {
            BBO_REQUIRE(count == 1 && in[0] == in[0], "fbest: one value, not NaN");
            s.fbest = in[0];
        } else {
            BBO_REQUIRE(whole(0., 2147483646.), "fev, it, itae, ix, improved: one non-negative integer");
            BBO_REQUIRE(k != "ix" || in[0] < n, "ix: below n");
            BBO_REQUIRE(k != "improved" || in[0] <= 1., "improved: 0 or 1");
            (k == "fev" ? s.fev : k == "it" ? s.it : k == "itae" ? s.itae : k == "ix" ? s.ix : s.improved) = (int) in[0];
        }
        scal_.upload(&s, 1, p);
        return 1;
    }
    throw Error(BBO_ERR_KEY, "unknown or read-only state key '" + k + "'");
}

Optimizer* make_acd_engine(const bbo_params &p)
{
    return new AcdEngine(p);
}

} // namespace bbo
