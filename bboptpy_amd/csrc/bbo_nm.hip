// bbo_nm.hip -- host side of the NelderMead engine.  Reference behaviour restated on the host:
// NelderMead::NelderMead / init / initParameters / optimize (nelder_mead.cpp:41-87, :232-237, :369-401).
#include "bbo_nm_kernels.hpp"

#include <algorithm>
#include <cmath>
#include <limits>

namespace bbo {

namespace {
enum { K_WALK = 0, K_EVAL, K_COUNT };
static const char *const K_NAMES[K_COUNT] = { "bbo:nm_walk", "bbo:nm_eval" };
constexpr double NM_PI = 3.14159265358979323846;    // M_PI

// the walk may hold the largest simplex in dynamic LDS
void allow_walk_lds()
{
    allow_lds((const void*) nm_walk, (NM_MAX_N + 1) * NM_MAX_N * (int) sizeof(double));
}
}

NmEngine::NmEngine(const bbo_params &p) :
        WalkEngine(checked(p), "bbo_nm_phase", true)
{
    bbo_nm_params_default(&np_);
}

// the part of the constructor's arguments that travels in bbo_params
const bbo_params &NmEngine::checked(const bbo_params &p)
{
    BBO_REQUIRE(p.algo == BBO_ALGO_NELDER_MEAD, "NmEngine: bad algo");
    BBO_REQUIRE(p.mfev >= 1, "NelderMead: mfev must be positive");
    BBO_REQUIRE(p.tol == p.tol, "NelderMead: tol must not be NaN");
    BBO_REQUIRE(std::isfinite(p.sigma0), "NelderMead: rad0 must be finite");
    return p;
}

void NmEngine::configure(const bbo_nm_params &np)
{
    if (inited_) throw Error(BBO_ERR_STATE, "bbo_nm_configure after bbo_init");
    BBO_REQUIRE(np.minit >= 0 && np.minit <= 3, "NelderMead: minit is 0 coordinate_axis, 1 spendley, 2 pfeffer or 3 random");
    BBO_REQUIRE(np.pinit >= 0 && np.pinit <= 3,
            "NelderMead: pinit is 0 original, 1 gao2010, 2 mehta2019_crude or 3 mehta2019_refined");
    BBO_REQUIRE(np.checkev >= 1, "NelderMead: checkev must be >= 1");
    BBO_REQUIRE(std::isfinite(np.eps), "NelderMead: eps must be finite");
    BBO_REQUIRE(np.repair == 0 || np.repair == 1, "NelderMead: repair is 0 or 1");
    BBO_REQUIRE(np.lds >= -1 && np.lds <= 1, "NelderMead: lds is 1, 0 or -1 (the engine chooses)");
    BBO_REQUIRE(np.substream >= 0 && np.substream < (1 << 24), "NelderMead: substream must be in [0, 2^24)");
    // (built -- pstar and the three possible second points on four wavefronts, the unused values dropped --
    // bit-identical and measured: slower at 1, 256 and 4096 populations alike, so dropped as the issue rules;
    // DESIGN.md section 3.19 has both timings)
    BBO_REQUIRE(np.speculate == 0, "NelderMead: the speculative step was measured and dropped (speculate must be 0)");
    np_ = np;
}

// initParameters() (:369-401)
void NmEngine::coefficients(int n)
{
    NmConst &c = c_;
    switch (np_.pinit) {
    case 0:
        c.ccoef = 0.5; c.ecoef = 2.0; c.rcoef = 1.0; c.scoef = 0.5;
        break;
    case 1:
        c.ccoef = 0.75 - 0.5 / n; c.ecoef = 1. + 2. / n; c.rcoef = 1.; c.scoef = 1. - 1. / n;
        break;
    case 2:
        c.ccoef = 1. + std::cos((n + 3. + (n % 2)) * NM_PI / (2. * n));
        c.ecoef = 1. + std::cos((n - 3. - (n % 2)) * NM_PI / (2. * n));
        c.rcoef = 1. + std::cos((n - 1. - (n % 2)) * NM_PI / (2. * n));
        c.scoef = 1. + std::cos((n + 1. + (n % 2)) * NM_PI / (2. * n));
        break;
    default: {
        const int nc = 2 * (9 + (n - 1) / 5);
        c.ccoef = 1. + std::cos((nc + 5.) * NM_PI / (2. * nc));
        c.ecoef = 1. + std::cos((nc - 3.) * NM_PI / (2. * nc));
        c.rcoef = 1. + std::cos((nc - 1.) * NM_PI / (2. * nc));
        c.scoef = 1. + std::cos((nc + 3.) * NM_PI / (2. * nc));
    }
    }
}

void NmEngine::init(int n, const double *lower, const double *upper, const double *guess,
        const ObjectiveSpec &obj)
{
    reject_program(obj, "NelderMead");
    BBO_REQUIRE(n >= 1 && n <= NM_MAX_N, "NelderMead: dimension must be in [1, 128]");
    if (np_.minit == 3)
        require_finite_box("NelderMead: minit = random draws the simplex from [lower, upper]: the bounds must be finite",
                n, lower, upper);
    BBO_HIP(hipSetDevice(params_.device));
    obj_ = obj;
    const int P = params_.populations;
    BBO_REQUIRE(P <= (1 << 24) - np_.substream, "NelderMead: substream + populations must be <= 2^24");
    NmConst &c = c_;
    c = NmConst {};
    c.n = n;
    c.ld = round_up(n, 2);
    c.obj = obj.fused() ? obj.builtin : OBJ_HOST;
    c.mfev = params_.mfev;
    c.npop = P;
    c.minit = np_.minit;
    c.checkev = np_.checkev;
    c.repair = np_.repair;
    c.lds = np_.lds;
    if (c.lds < 0) {
        // Measured: the simplex in LDS is faster while several workgroups share a CU
        // (n = 32) and, where its size leaves one workgroup per CU (n = 96, 128), below four populations per
        // CU; from four per CU on (1024 populations on 256 CUs) the rows in HBM are faster.  Sizes that leave
        // two workgroups per CU (n = 64 .. 93) were not measured and stay in LDS.
        int cus = 0;
        BBO_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, params_.device));
        const size_t bytes = (size_t) (n + 1) * c.ld * sizeof(double);
        const bool one_per_cu = 2 * (bytes + NM_STATIC_LDS) > 160 * 1024;
        c.lds = one_per_cu && P >= 4 * cus ? 0 : 1;
    }
    c.substream = np_.substream;
    c.vs = 2 * n;
    c.eps = np_.eps;
    c.rq = params_.tol * params_.tol * n;                           // :85
    c.sp = 1. / (n * std::sqrt(2.)) * (n - 1. + std::sqrt(n - 1.));    // :325-327
    c.sq = 1. / (n * std::sqrt(2.)) * (std::sqrt(n + 1.) - 1.);
    c.seed = params_.seed;
    coefficients(n);
    mid_generation_ = false;

    const size_t ld = c.ld, vec = (size_t) P * ld;
    P_.alloc(vec * (n + 1));
    y_.alloc((size_t) P * (n + 1));
    start_.alloc(vec); xmin_.alloc(vec); step_.alloc(vec);
    cand_.alloc(vec * 2 * n);
    value_.alloc((size_t) P * c.vs);
    scal_.alloc(P);
    ynl_h_.assign(P, 0.);
    // (the bounds may be infinite: only minit = random reads them)
    upload_box(n, c.ld, lower, upper, obj);
    {
        std::vector<double> st(vec, 0.), sp(vec, 0.), z(vec * 2 * n, 0.);
        for (int p = 0; p < P; p++)
            for (int j = 0; j < n; j++) {
                st[p * ld + j] = guess[(size_t) p * n + j];           // :63
                sp[p * ld + j] = params_.sigma0;                       // :78-79
            }
        start_.upload(st.data(), vec);
        step_.upload(sp.data(), vec);
        std::fill(st.begin(), st.end(), 0.);
        xmin_.upload(st.data(), vec);
        cand_.upload(z.data(), z.size());
        z.assign(vec * (n + 1), 0.);
        P_.upload(z.data(), z.size());
        z.assign((size_t) P * std::max(c.vs, n + 1), 0.);
        value_.upload(z.data(), (size_t) P * c.vs);
        y_.upload(z.data(), (size_t) P * (n + 1));
        std::vector<NmScal> sc(P);
        std::memset(sc.data(), 0, sizeof(NmScal) * P);
        for (auto &s : sc) s = nm_fresh_scal(np_.checkev);
        scal_.upload(sc.data(), P);
    }

    NmDev &d = d_;
    d = NmDev {};
    d.P = P_.p; d.y = y_.p; d.start = start_.p; d.xmin = xmin_.p; d.step = step_.p; d.cand = cand_.p;
    d.value = value_.p;
    d.lower = lower_.p; d.upper = upper_.p; d.aux = aux_.p; d.scal = scal_.p;
    if (c.lds) allow_walk_lds();
    inited_ = true;
    inits_++;

    // the first simplex and its n + 1 values, as nelmin()'s first pass (:251-260): no step
    c.honor_stop = 0;
    if (!obj_.needs_host()) {
        launch_body(NM_FUSED, 0, true);
    } else {
        launch_body(NM_ADVANCE, 0, true);
        host_evaluate_pending(false, [this](int p, const NmScal &s) { return pending_points(p, s); });
        launch_body(NM_ABSORB, 0, false);
    }
    BBO_HIP(hipStreamSynchronize(stream_));
}

void NmEngine::launch_body(int mode, int k, bool begin)
{
    const int threads = c_.n <= 64 ? 64 : NM_THREADS;
    const size_t bytes = c_.lds ? (size_t) (c_.n + 1) * c_.ld * sizeof(double) : 0;
    timed(K_WALK, [&] {
        hipLaunchKernelGGL(nm_walk, dim3(c_.npop), dim3(threads), bytes, stream_, d_, c_, mode, k, begin ? 1 : 0);
    });
}

void NmEngine::launch_eval_device()
{
    timed(K_EVAL, [&] { hipLaunchKernelGGL(nm_eval, dim3(c_.npop), dim3(NM_THREADS), 0, stream_, d_, c_); });
}

// the batch a population has pending: one point, the rows of a fresh or a shrunk simplex, or the probes of
// the factorial test, which the callable sees up to the first below ynl
PendingPoints NmEngine::pending_points(int p, const NmScal &s)
{
    const size_t ld = c_.ld;
    PendingPoints pt { &cand_, (size_t) p * 2 * c_.n * ld, s.pending, c_.ld, &value_ };
    pt.value_off = (long long) p * c_.vs;
    if (s.stage == NM_WAIT_INIT || s.stage == NM_WAIT_SHRINK) {
        pt.cand = &P_;
        pt.off = (size_t) p * (c_.n + 1) * ld;
    } else if (s.stage == NM_WAIT_SECOND) {
        pt.off += ld;
    } else if (s.stage == NM_WAIT_FACT) {
        ynl_h_[p] = s.ynl;
        pt.stop_below = &ynl_h_[p];
    }
    return pt;
}

// one simplex step of every population (NM_FUSED), or the same walk from batch to batch
void NmEngine::launch_walk(int mode, bool begin)
{
    launch_body(mode, 1, begin);
}

// bbo_run: `gens` simplex steps per population, and what nelmin() does between them
void NmEngine::launch_chunk(int gens)
{
    if (obj_.needs_host()) {
        Engine::launch_chunk(gens);
        return;
    }
    c_.honor_stop = 1;
    launch_body(NM_FUSED, gens, true);
    mid_generation_ = false;
}

// init() + nelmin() (:232-237): xmin as nelmin() leaves it, converged = (ifault == 0)
void NmEngine::optimize(int n, const double *lower, const double *upper, const double *guess,
        const ObjectiveSpec &obj, double *x_out, int *n_evals, int *converged)
{
    init(n, lower, upper, guess, obj);
    run(std::numeric_limits<int>::max());
    NmScal s;
    scal_.download(&s, 1, 0);
    std::vector<double> x(c_.ld);
    xmin_.download(x.data(), c_.ld, 0);
    std::copy(x.begin(), x.begin() + n, x_out);
    *n_evals = s.fev;
    *converged = s.stop == 1 ? 1 : 0;
}

void NmEngine::solution(int population, double *x_out, int *n_evals, int *converged)
{
    enter_population("solution()", population);
    NmScal s;
    scal_.download(&s, 1, population);
    report_solution(s, P_, ((size_t) population * (c_.n + 1) + s.ilo) * c_.ld, c_.n, c_.ld, x_out, n_evals, converged);
}

int NmEngine::get(const std::string &k, int p, double *out, int cap)
{
    enter_population("get()", p);
    const NmConst &c = c_;
    NmScal s;
    scal_.download(&s, 1, p);
    const int n = c.n, ld = c.ld;
    const size_t pv = (size_t) p * ld;
    const StateOut o { out, cap };
    if (k == "profile") return profile_report(out, cap);
    if (k == "p") return o.rows(P_, (size_t) p * (n + 1), n + 1, n, ld);
    if (k == "y") return o.vec(y_, (size_t) p * (n + 1), n + 1);
    if (k == "start") return o.vec(start_, pv, n);
    if (k == "xmin") return o.vec(xmin_, pv, n);
    if (k == "step") return o.vec(step_, pv, n);
    if (k == "cand") return o.rows(cand_, (size_t) p * 2 * n, 2 * n, n, ld);
    if (k == "value") return o.vec(value_, (size_t) p * c.vs, c.vs);
    if (k == "coef") {
        const double v[4] = { c.ccoef, c.ecoef, c.rcoef, c.scoef };
        return o.copy(v, 4);
    }
    if (k == "ilo") return o.one(s.ilo);
    if (k == "ihi") return o.one(s.ihi);
    if (k == "ylo") return o.one(s.ylo);
    if (k == "ynl") return o.one(s.ynl);
    if (k == "ystar") return o.one(s.ystar);
    if (k == "jcount") return o.one(s.jcount);
    if (k == "fev") return o.one(s.fev);
    if (k == "it") return o.one(s.it);
    if (k == "del") return o.one(s.del);
    if (k == "conv") return o.one(s.conv);
    if (k == "flag" || k == "stop") return o.one(s.stop);
    if (k == "pending") return o.one(s.pending);
    if (k == "stage") return o.one(s.stage);
    if (k == "branch") return o.one(s.branch);
    if (k == "restarts") return o.one(s.restarts);
    if (k == "rq") return o.one(c.rq);
    if (k == "lds") return o.one(c.lds);
    if (k == "repair") return o.one(c.repair);
    if (k == "chunk") return o.one(params_.poll_every > 0 ? params_.poll_every : default_poll());
    if (k == "n") return o.one(n);
    throw Error(BBO_ERR_KEY, "unknown state key '" + k + "'");
}

int NmEngine::set(const std::string &k, int p, const double *in, int count)
{
    enter_population("set()", p);
    const NmConst &c = c_;
    const int n = c.n, ld = c.ld;
    const size_t pv = (size_t) p * ld;
    auto whole = [&](double lo, double hi) {
        return count == 1 && in[0] == std::floor(in[0]) && in[0] >= lo && in[0] <= hi;
    };
    if (k == "profile") return profile_enable(in, K_COUNT, K_NAMES);
    if (k == "lds") {           // (the whole handle) where a launch keeps the simplex
        BBO_REQUIRE(whole(0., 1.), "lds: 0 or 1");
        c_.lds = (int) in[0];
        if (c_.lds) allow_walk_lds();
        return 1;
    }
    if (k == "p") {             // the simplex in place; nothing is evaluated
        BBO_REQUIRE(count == (n + 1) * n, "p: (n + 1) * n values");
        upload_rows(P_, (size_t) p * (n + 1), n + 1, n, ld, in);
        return count;
    }
    if (k == "y") {
        BBO_REQUIRE(count == n + 1, "y: n + 1 values");
        std::vector<double> fh(in, in + count);
        nan_to_inf(fh.data(), count);
        y_.upload(fh.data(), count, (size_t) p * (n + 1));
        return count;
    }
    if (k == "start") {
        BBO_REQUIRE(count == n, "start: n values");
        start_.upload(in, n, pv);
        return count;
    }
    if (k == "value") {         // (what bbo_nm_phase 2 absorbs: as many values as points are pending)
        NmScal s;
        scal_.download(&s, 1, p);
        BBO_REQUIRE(count >= 1 && count <= c.vs && count == std::max(s.pending, 1), "value: one value per pending point");
        std::vector<double> fh(in, in + count);
        nan_to_inf(fh.data(), count);
        value_.upload(fh.data(), count, (size_t) p * c.vs);
        return count;
    }
    if (k == "ilo" || k == "jcount" || k == "fev" || k == "ylo" || k == "del") {
        NmScal s;
        scal_.download(&s, 1, p);
        if (k == "ylo" || k == "del") {
            BBO_REQUIRE(count == 1 && in[0] == in[0], "ylo, del: one value, not NaN");
            (k == "ylo" ? s.ylo : s.del) = in[0];
        } else if (k == "jcount") {
            BBO_REQUIRE(whole(-2147483647., 2147483646.), "jcount: one integer");
            s.jcount = (int) in[0];
        } else {
            BBO_REQUIRE(whole(0., 2147483646.), "ilo, fev: one non-negative integer");
            BBO_REQUIRE(k != "ilo" || in[0] <= n, "ilo: at most n");
            (k == "ilo" ? s.ilo : s.fev) = (int) in[0];
        }
        scal_.upload(&s, 1, p);
        return 1;
    }
    throw Error(BBO_ERR_KEY, "unknown or read-only state key '" + k + "'");
}

Optimizer* make_nm_engine(const bbo_params &p)
{
    return new NmEngine(p);
}

} // namespace bbo
