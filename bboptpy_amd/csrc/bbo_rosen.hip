// bbo_rosen.hip -- host side of the Rosenbrock engine.  Reference behaviour restated on the host:
// Rosenbrock::Rosenbrock / init / solution / optimize (rosenbrock.cpp:49-93, :212-225).
#include "bbo_rosen_kernels.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

namespace bbo {

namespace {
enum { K_WALK = 0, K_EVAL, K_COUNT };
static const char *const K_NAMES[K_COUNT] = { "bbo:rosen_walk", "bbo:rosen_eval" };
}

RosenEngine::RosenEngine(const bbo_params &p) :
        WalkEngine(checked(p), "bbo_rosen_phase", true)
{
    bbo_rosen_params_default(&rp_);
}

// the part of the constructor's arguments that travels in bbo_params
const bbo_params &RosenEngine::checked(const bbo_params &p)
{
    BBO_REQUIRE(p.algo == BBO_ALGO_ROSENBROCK, "RosenEngine: bad algo");
    BBO_REQUIRE(p.mfev >= 1, "Rosenbrock: mfev must be positive");
    // (with a step of 0 the doubling loop of a search ends on the budget alone, inside one launch: step0 = 0, or
    // a step that underflows to 0 because no tol >= 0 stopped the run before)
    BBO_REQUIRE(p.tol >= 0., "Rosenbrock: tol must be >= 0 (and not NaN)");
    BBO_REQUIRE(std::isfinite(p.sigma0) && p.sigma0 != 0., "Rosenbrock: step0 must be finite and not 0");
    return p;
}

void RosenEngine::configure(const bbo_rosen_params &rp)
{
    if (inited_) throw Error(BBO_ERR_STATE, "bbo_rosen_configure after bbo_init");
    BBO_REQUIRE(std::isfinite(rp.decf) && rp.decf != 0., "Rosenbrock: decf must be finite and not 0");
    BBO_REQUIRE(rp.repair == 0 || rp.repair == 1, "Rosenbrock: repair is 0 or 1");
    BBO_REQUIRE(rp.wide >= -1 && rp.wide <= 1, "Rosenbrock: wide is 1, 0 or -1 (the engine chooses)");
    BBO_REQUIRE(rp.substream >= 0 && rp.substream < (1 << 24), "Rosenbrock: substream must be in [0, 2^24)");
    rp_ = rp;
}

void RosenEngine::init(int n, const double *lower, const double *upper, const double *guess,
        const ObjectiveSpec &obj)
{
    reject_program(obj, "Rosenbrock");
    BBO_REQUIRE(n >= 1 && n <= ROSEN_MAX_N, "Rosenbrock: dimension must be in [1, 128]");
    BBO_HIP(hipSetDevice(params_.device));
    obj_ = obj;
    const int P = params_.populations;
    RosenConst &c = c_;
    c = RosenConst {};
    c.n = n;
    c.ld = round_up(n, 2);
    c.obj = obj.fused() ? obj.builtin : OBJ_HOST;
    c.mfev = params_.mfev;
    c.npop = P;
    c.repair = rp_.repair;
    c.wide = rp_.wide;
    if (c.wide < 0) {
        // Measured: the wide form is faster at n = 32 and n = 128 with 1 and with 256
        // populations and level at n = 128 with 4096; at n = 32 with 4096 populations (16 per CU) the narrow form
        // is twice as fast.  Between 256 and 4096 nothing was measured: the switch is put at four populations per
        // CU, where NelderMead's lies.  n = 64 is the largest size a single wavefront covers in one pass.
        int cus = 0;
        BBO_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, params_.device));
        c.wide = n <= 64 && P >= 4 * cus ? 0 : 1;
    }
    c.tol = params_.tol;
    c.decf = rp_.decf;
    c.step0 = params_.sigma0;
    mid_generation_ = false;

    const size_t ld = c.ld, vec = (size_t) P * ld, mat = vec * (n + 2);
    x_.alloc(mat); v_.alloc(mat); vold_.alloc(mat);
    dd_.alloc((size_t) P * (n + 2));
    x0_.alloc(vec); x1_.alloc(vec);
    cand_.alloc(vec * ROSEN_BATCH);
    value_.alloc((size_t) P * ROSEN_BATCH);
    scal_.alloc(P);
    // (the bounds are stored and never read, as in the reference)
    upload_box(n, c.ld, lower, upper, obj);
    {
        std::vector<double> X(mat, 0.), V(mat, 0.), z(std::max(mat, vec * ROSEN_BATCH), 0.);
        for (int p = 0; p < P; p++) {
            for (int j = 0; j < n; j++) {
                X[(size_t) p * (n + 2) * ld + j] = guess[(size_t) p * n + j];       // :84
                V[((size_t) p * (n + 2) + j + 1) * ld + j] = 1.;                    // :86-88
            }
        }
        x_.upload(X.data(), mat);
        v_.upload(V.data(), mat);
        vold_.upload(z.data(), mat);
        dd_.upload(z.data(), (size_t) P * (n + 2));
        x0_.upload(z.data(), vec);
        x1_.upload(z.data(), vec);
        cand_.upload(z.data(), vec * ROSEN_BATCH);
        value_.upload(z.data(), (size_t) P * ROSEN_BATCH);
        std::vector<RosenScal> sc(P);
        std::memset(sc.data(), 0, sizeof(RosenScal) * P);
        for (auto &s : sc) s = rosen_fresh_scal(params_.sigma0);
        scal_.upload(sc.data(), P);
    }

    RosenDev &d = d_;
    d = RosenDev {};
    d.x = x_.p; d.v = v_.p; d.vold = vold_.p; d.d = dd_.p; d.x0 = x0_.p; d.x1 = x1_.p;
    d.cand = cand_.p; d.value = value_.p;
    d.aux = aux_.p; d.scal = scal_.p;
    inited_ = true;
    inits_++;
}

void RosenEngine::launch_body(int mode, int k, bool begin)
{
    const int threads = c_.wide ? ROSEN_THREADS : 64;
    timed(K_WALK, [&] {
        hipLaunchKernelGGL(rosen_walk, dim3(c_.npop), dim3(threads), 0, stream_, d_, c_, mode, k, begin ? 1 : 0);
    });
}

void RosenEngine::launch_eval_device()
{
    timed(K_EVAL, [&] { hipLaunchKernelGGL(rosen_eval, dim3(c_.npop), dim3(ROSEN_THREADS), 0, stream_, d_, c_); });
}

// the batch a population has pending: 2, 1 or 4 rows of cand, in the reference's order
PendingPoints RosenEngine::pending_points(int p, const RosenScal &s)
{
    PendingPoints pt { &cand_, (size_t) p * ROSEN_BATCH * c_.ld, s.pending, c_.ld, &value_ };
    pt.value_off = (long long) p * ROSEN_BATCH;
    return pt;
}

// one line search of every population with iterate()'s bookkeeping (ROSEN_FUSED), or the same walk from batch
// to batch
void RosenEngine::launch_walk(int mode, bool begin)
{
    launch_body(mode, 1, begin);
}

// bbo_run: `gens` line searches per population
void RosenEngine::launch_chunk(int gens)
{
    if (obj_.needs_host()) {
        Engine::launch_chunk(gens);
        return;
    }
    c_.honor_stop = 1;
    launch_body(ROSEN_FUSED, gens, true);
    mid_generation_ = false;
}

// init() + iterate() until _ierr >= 0 (:216-225)
void RosenEngine::optimize(int n, const double *lower, const double *upper, const double *guess,
        const ObjectiveSpec &obj, double *x_out, int *n_evals, int *converged)
{
    init(n, lower, upper, guess, obj);
    run(std::numeric_limits<int>::max());
    solution(0, x_out, n_evals, converged);
}

// solution() (:212-214): _x1, which only a converged run has written; under repair the end point of the last
// completed search where the run has not converged
void RosenEngine::solution(int population, double *x_out, int *n_evals, int *converged)
{
    enter_population("solution()", population);
    RosenScal s;
    scal_.download(&s, 1, population);
    s.conv = s.stop == 1 ? 1 : 0;
    if (c_.repair && s.stop != 1)
        report_solution(s, x_, ((size_t) population * (c_.n + 2) + s.i - 1) * c_.ld, c_.n, c_.ld, x_out, n_evals, converged);
    else
        report_solution(s, x1_, (size_t) population * c_.ld, c_.n, c_.ld, x_out, n_evals, converged);
}

int RosenEngine::get(const std::string &k, int p, double *out, int cap)
{
    enter_population("get()", p);
    const RosenConst &c = c_;
    RosenScal s;
    scal_.download(&s, 1, p);
    const int n = c.n, ld = c.ld;
    const StateOut o { out, cap };
    if (k == "profile") return profile_report(out, cap);
    if (k == "x") return o.rows(x_, (size_t) p * (n + 2), n + 2, n, ld);
    if (k == "v") return o.rows(v_, (size_t) p * (n + 2), n + 2, n, ld);
    if (k == "d") return o.vec(dd_, (size_t) p * (n + 2), n + 2);
    if (k == "x1") return o.vec(x1_, (size_t) p * ld, n);
    if (k == "cand") return o.rows(cand_, (size_t) p * ROSEN_BATCH, ROSEN_BATCH, n, ld);
    if (k == "value") return o.vec(value_, (size_t) p * ROSEN_BATCH, ROSEN_BATCH);
    if (k == "fs") return o.copy(s.fs, 4);
    if (k == "path") {
        const double v[4] = { (double) s.pdir, (double) s.prounds, (double) s.pimin, (double) s.pend };
        return o.copy(v, 4);
    }
    if (k == "stepi") return o.one(s.stepi);
    if (k == "s") return o.one(s.s);
    if (k == "fx") return o.one(s.fx);
    if (k == "fx0") return o.one(s.fx0);
    if (k == "i") return o.one(s.i);
    if (k == "fev") return o.one(s.fev);
    if (k == "it") return o.one(s.it);
    if (k == "flag" || k == "stop") return o.one(s.stop);
    if (k == "pending") return o.one(s.pending);
    if (k == "stage") return o.one(s.stage);
    if (k == "orth") return o.one(s.orth);
    if (k == "orths") return o.one(s.orths);
    if (k == "walk_ticks") return o.one((double) s.walk_ticks);
    if (k == "orth_ticks") return o.one((double) s.orth_ticks);
    if (k == "wide") return o.one(c.wide);
    if (k == "repair") return o.one(c.repair);
    if (k == "chunk") return o.one(params_.poll_every > 0 ? params_.poll_every : default_poll());
    if (k == "n") return o.one(n);
    throw Error(BBO_ERR_KEY, "unknown state key '" + k + "'");
}

int RosenEngine::set(const std::string &k, int p, const double *in, int count)
{
    enter_population("set()", p);
    const RosenConst &c = c_;
    const int n = c.n, ld = c.ld;
    auto whole = [&](double lo, double hi) {
        return count == 1 && in[0] == std::floor(in[0]) && in[0] >= lo && in[0] <= hi;
    };
    if (k == "profile") return profile_enable(in, K_COUNT, K_NAMES);
    if (k == "wide") {          // (the whole handle) the form of the following launches
        BBO_REQUIRE(whole(0., 1.), "wide: 0 or 1");
        c_.wide = (int) in[0];
        return 1;
    }
    if (k == "x" || k == "v") {     // in place; nothing is evaluated
        BBO_REQUIRE(count == (n + 2) * n, "x, v: (n + 2) * n values");
        upload_rows(k == "x" ? x_ : v_, (size_t) p * (n + 2), n + 2, n, ld, in);
        return count;
    }
    if (k == "d") {
        BBO_REQUIRE(count == n + 2, "d: n + 2 values");
        dd_.upload(in, count, (size_t) p * (n + 2));
        return count;
    }
    if (k == "value") {         // (what bbo_rosen_phase 2 absorbs: as many values as points are pending)
        RosenScal s;
        scal_.download(&s, 1, p);
        BBO_REQUIRE(count >= 1 && count <= ROSEN_BATCH && count == std::max(s.pending, 1), "value: one value per pending point");
        std::vector<double> fh(in, in + count);
        nan_to_inf(fh.data(), count);
        value_.upload(fh.data(), count, (size_t) p * ROSEN_BATCH);
        return count;
    }
    if (k == "stepi" || k == "i" || k == "fev") {
        RosenScal s;
        scal_.download(&s, 1, p);
        BBO_REQUIRE(s.stage == ROSEN_IDLE, "stepi, i, fev: not while a search is under way");
        if (k == "stepi") {
            BBO_REQUIRE(count == 1 && std::isfinite(in[0]) && in[0] != 0., "stepi: one value, finite and not 0");
            s.stepi = in[0];
        } else if (k == "i") {
            BBO_REQUIRE(whole(1., n + 1.), "i: one integer in [1, n + 1]");
            s.i = (int) in[0];
        } else {
            BBO_REQUIRE(whole(0., 2147483646.), "fev: one non-negative integer");
            s.fev = (int) in[0];
        }
        scal_.upload(&s, 1, p);
        return 1;
    }
    throw Error(BBO_ERR_KEY, "unknown or read-only state key '" + k + "'");
}

Optimizer* make_rosen_engine(const bbo_params &p)
{
    return new RosenEngine(p);
}

} // namespace bbo
