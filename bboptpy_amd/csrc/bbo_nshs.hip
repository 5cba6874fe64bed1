// bbo_nshs.hip -- host side of the NSHS engine.  Reference behaviour restated on the host:
// NSHS::NSHS / init / optimize / solution (nshs.cpp:40-110).
#include "bbo_nshs_kernels.hpp"

#include <algorithm>
#include <cmath>
#include <limits>

namespace bbo {

namespace {
enum { K_INIT = 0, K_GENERATE, K_EVAL, K_REPLACE, K_STEPS, K_COUNT };
static const char *const K_NAMES[K_COUNT] = { "bbo:nshs_init", "bbo:nshs_generate", "bbo:nshs_eval",
        "bbo:nshs_replace", "bbo:nshs_steps" };

template<int T>
void launch_steps_t(bool lds, int P, size_t bytes, hipStream_t s, const NshsDev &d, const NshsConst &c, int k)
{
    if (lds) hipLaunchKernelGGL((nshs_steps<T, true>), dim3(P), dim3(T), bytes, s, d, c, k);
    else hipLaunchKernelGGL((nshs_steps<T, false>), dim3(P), dim3(T), bytes, s, d, c, k);
}
}

NshsEngine::NshsEngine(const bbo_params &p) :
        Engine(checked(p))
{
    bbo_nshs_params_default(&np_);
}

// the part of the constructor's arguments that travels in bbo_params
const bbo_params &NshsEngine::checked(const bbo_params &p)
{
    BBO_REQUIRE(p.algo == BBO_ALGO_NSHS, "NshsEngine: bad algo");
    BBO_REQUIRE(p.np >= 1 && p.np <= NSHS_MAX_HMS, "NSHS: hms must be in [1, 4096]");
    return p;
}

void NshsEngine::configure(const bbo_nshs_params &np)
{
    if (inited_) throw Error(BBO_ERR_STATE, "bbo_nshs_configure after bbo_init");
    BBO_REQUIRE(std::isfinite(np.fstdmin) && np.fstdmin >= 0., "NSHS: fstdmin must be finite and not negative");
    np_ = np;
}

// the route of nshs_steps: the memory in LDS while it fits the budget
bool NshsEngine::hm_in_lds() const
{
    if (c_.dbg & NSHS_DBG_GLOBAL_HM) return false;
    return (size_t) c_.hms * c_.ld * sizeof(double) <= (size_t) NSHS_LDS_BYTES;
}

// the threads of nshs_steps' workgroup: a lane per coordinate up to 256
int NshsEngine::workgroup() const
{
    if (wg_) return wg_;
    return c_.n <= 128 ? 64 : c_.n <= 256 ? 128 : 256;
}

void NshsEngine::init(int n, const double *lower, const double *upper, const double *guess,
        const ObjectiveSpec &obj)
{
    (void) guess;   // NSHS never reads it (nshs.cpp:46-91)
    reject_program(obj, "NSHS");
    BBO_REQUIRE(n >= 1 && n <= NSHS_MAX_N, "NSHS: dimension must be in [1, 512]");
    require_finite_box("NSHS draws its memory from [lower, upper] and clamps to it: the bounds must be finite", n,
            lower, upper);
    BBO_HIP(hipSetDevice(params_.device));
    obj_ = obj;
    const int P = params_.populations;
    BBO_REQUIRE(P <= (1 << 24), "NSHS: populations must be <= 2^24");
    const int keep_dbg = c_.dbg;
    NshsConst &c = c_;
    c = NshsConst {};
    c.n = n;
    c.ld = round_up(n, 2);
    c.hms = params_.np;
    c.obj = obj.fused() ? obj.builtin : OBJ_HOST;
    c.mfev = params_.mfev;
    c.mit = params_.mfev - params_.np;          // :83
    c.npop = P;
    c.dbg = keep_dbg;
    c.fstdmin = np_.fstdmin;
    c.hmcr = 1.0 - 1.0 / (n + 1);               // :86
    c.tunerange = 0.0;                          // :87-90
    for (int j = 0; j < n; j++) c.tunerange = std::max(c.tunerange, (upper[j] - lower[j]) / 2);
    c.seed = params_.seed;

    const size_t rows = (size_t) P * c.hms;
    X_.alloc(rows * c.ld);
    f_.alloc(rows);
    cand_.alloc((size_t) P * c.ld);
    fcand_.alloc(P);
    tables_.clear();
    scal_.alloc(P);
    upload_box(n, c.ld, lower, upper, obj);
    std::vector<NshsScal> sc(P);
    for (auto &s : sc) {
        std::memset(&s, 0, sizeof(s));
        s.fev = c.hms;          // the memory is evaluated (:81)
    }
    scal_.upload(sc.data(), P);

    NshsDev &d = d_;
    d = NshsDev {};
    d.X = X_.p; d.f = f_.p; d.cand = cand_.p; d.fcand = fcand_.p;
    d.lower = lower_.p; d.upper = upper_.p; d.aux = aux_.p; d.scal = scal_.p;
    inited_ = true;

    if (obj_.needs_host()) {
        launch_init(0, P, NSHS_INIT_DRAW);
        host_evaluate_range(X_, f_, 0, P, c.hms, 0, c.hms, n, c.ld);    // (in row order, like :60-67)
        launch_init(0, P, 0);
    } else {
        launch_init(0, P, NSHS_INIT_DRAW | NSHS_INIT_EVAL);
    }
    BBO_HIP(hipStreamSynchronize(stream_));
}

void NshsEngine::launch_init(int p0, int pcount, int mode)
{
    timed(K_INIT, [&] { hipLaunchKernelGGL(nshs_init, dim3(pcount), dim3(256), 0, stream_, d_, c_, p0, mode); });
}

void NshsEngine::launch_generate()
{
    timed(K_GENERATE, [&] { hipLaunchKernelGGL(nshs_generate, dim3(c_.npop), dim3(256), 0, stream_, d_, c_); });
}

void NshsEngine::launch_eval()
{
    if (obj_.needs_host()) {
        // one candidate row per population, in population order
        host_evaluate_rows(cand_, fcand_, 1, c_.n, c_.ld, c_.honor_stop != 0);
        return;
    }
    timed(K_EVAL, [&] { hipLaunchKernelGGL(nshs_eval, dim3(c_.npop), dim3(64), 0, stream_, d_, c_); });
}

void NshsEngine::launch_replace()
{
    timed(K_REPLACE, [&] { hipLaunchKernelGGL(nshs_replace, dim3(c_.npop), dim3(64), 0, stream_, d_, c_); });
}

void NshsEngine::launch_steps(int k)
{
    const bool lds = hm_in_lds();
    const size_t bytes = ((size_t) 3 * c_.ld + (lds ? (size_t) c_.hms * (c_.ld + 1) : 0)) * sizeof(double);
    timed(K_STEPS, [&] {
        switch (workgroup()) {
        case 64: launch_steps_t<64>(lds, c_.npop, bytes, stream_, d_, c_, k); break;
        case 128: launch_steps_t<128>(lds, c_.npop, bytes, stream_, d_, c_, k); break;
        default: launch_steps_t<256>(lds, c_.npop, bytes, stream_, d_, c_, k); break;
        }
    });
}

// one iteration in its three parts: the path of bbo_iterate and of a host objective
void NshsEngine::generation(bool honor_stop)
{
    c_.honor_stop = honor_stop ? 1 : 0;
    launch_generate();
    launch_eval();
    launch_replace();
}

// bbo_run: `gens` whole iterations in one launch
void NshsEngine::launch_chunk(int gens)
{
    if (obj_.needs_host()) {
        Engine::launch_chunk(gens);
        return;
    }
    c_.honor_stop = 1;
    launch_steps(gens);
}

// the reference would divide by mit <= 0 (:138)
void NshsEngine::require_iterations(const char *call) const
{
    if (inited_ && c_.mit <= 0)
        throw Error(BBO_ERR_STATE, std::string(call) + ": mfev <= hms leaves no iteration (the memory spent the budget)");
}

void NshsEngine::iterate()
{
    require_iterations("iterate()");
    Engine::iterate();
}

// the three parts of iterate(), one at a time
void NshsEngine::phase(int which)
{
    run_phase("bbo_nshs_phase", which, 3, "bbo_nshs_phase: 0 generate, 1 evaluate, 2 replace", [&] {
        require_iterations("bbo_nshs_phase");
        c_.honor_stop = 0;
        if (which == 0) launch_generate();
        else if (which == 1) launch_eval();
        else launch_replace();
    });
}

void NshsEngine::inject_uniforms(const double *u, int count)
{
    enter("bbo_nshs_inject_uniforms");
    BBO_HIP(hipStreamSynchronize(stream_));
    if (!u) {
        d_.inject = nullptr;
        return;
    }
    const size_t want = (size_t) c_.npop * c_.n * 4;
    BBO_REQUIRE(count >= 0 && (size_t) count == want, "bbo_nshs_inject_uniforms: populations * n * 4 values");
    for (size_t q = 0; q < want; q++)
        BBO_REQUIRE(u[q] >= 0. && u[q] < 1., "bbo_nshs_inject_uniforms: uniforms lie in [0, 1)");
    d_.inject = tables_.load(u, want);
}

void NshsEngine::solution(int population, double *x_out, int *n_evals, int *converged)
{
    enter_population("solution()", population);
    NshsScal s;
    scal_.download(&s, 1, population);
    report_solution(s, X_, ((size_t) population * c_.hms + s.ibest) * c_.ld, c_.n, c_.ld, x_out, n_evals, converged);
}

int NshsEngine::get(const std::string &k, int p, double *out, int cap)
{
    enter_population("get()", p);
    const NshsConst &c = c_;
    NshsScal s;
    scal_.download(&s, 1, p);
    const size_t pb = (size_t) p * c.hms;
    const StateOut o { out, cap };
    if (k == "profile") return profile_report(out, cap);
    if (k == "x") return o.rows(X_, pb, c.hms, c.n, c.ld);
    if (k == "f") return o.vec(f_, pb, c.hms);
    if (k == "cand") return o.vec(cand_, (size_t) p * c.ld, c.n);
    if (k == "fcand") return o.vec(fcand_, p, 1);
    if (k == "xbest") return o.vec(X_, (pb + s.ibest) * c.ld, c.n);
    if (k == "draws") {
        require_record(c.record, k);
        return o.vec(tables_.draws, (size_t) p * c.n * 4, c.n * 4);
    }
    if (k == "fbest") return o.one(s.fbest);
    if (k == "fworst") return o.one(s.fworst);
    if (k == "fstd") return o.one(s.fstd);
    if (k == "ibest") return o.one(s.ibest);
    if (k == "iworst") return o.one(s.iworst);
    if (k == "wide") return o.one(s.wide);
    if (k == "accepted") return o.one(s.accepted);
    if (k == "fev") return o.one(s.fev);
    if (k == "it") return o.one(s.it);
    if (k == "flag" || k == "stop") return o.one(s.stop);
    if (k == "record_draws") return o.one(c.record);
    if (k == "dbg") return o.one(c.dbg);
    if (k == "hm_in_lds") return o.one(hm_in_lds() ? 1. : 0.);
    if (k == "lds_bytes") return o.one(NSHS_LDS_BYTES);
    if (k == "wg") return o.one(workgroup());
    if (k == "chunk") return o.one(params_.poll_every > 0 ? params_.poll_every : default_poll());
    if (k == "fstdmin") return o.one(c.fstdmin);
    if (k == "hmcr") return o.one(c.hmcr);
    if (k == "tunerange") return o.one(c.tunerange);
    if (k == "mit") return o.one(c.mit);
    if (k == "hms" || k == "np") return o.one(c.hms);
    if (k == "n") return o.one(c.n);
    throw Error(BBO_ERR_KEY, "unknown state key '" + k + "'");
}

int NshsEngine::set(const std::string &k, int p, const double *in, int count)
{
    enter_population("set()", p);
    const NshsConst &c = c_;
    const size_t pb = (size_t) p * c.hms;
    if (k == "profile") return profile_enable(in, K_COUNT, K_NAMES);
    if (k == "record_draws") {      // (the whole handle: every population)
        BBO_REQUIRE(count == 1, "record_draws: one value");
        c_.record = in[0] != 0. ? 1 : 0;
        d_.draws = tables_.record(c_.record != 0, (size_t) c.npop * c.n * 4);
        return 1;
    }
    if (k == "dbg") {
        BBO_REQUIRE(count == 1 && (in[0] == 0. || in[0] == 1.), "dbg: 0, or 1 (nshs_steps gathers the memory from global memory)");
        c_.dbg = (int) in[0];
        return 1;
    }
    if (k == "wg") {
        BBO_REQUIRE(count == 1 && (in[0] == 0. || in[0] == 64. || in[0] == 128. || in[0] == 256.),
                "wg: 0 (by n), 64, 128 or 256 threads");
        wg_ = (int) in[0];
        return 1;
    }
    if (k == "x") {             // f, fstd, the best and the worst follow; fev does not move
        BBO_REQUIRE(count == c.hms * c.n, "x: hms * n values");
        upload_rows(X_, pb, c.hms, c.n, c.ld, in);
        if (obj_.needs_host()) {
            host_evaluate_range(X_, f_, p, 1, c.hms, 0, c.hms, c.n, c.ld);
            launch_init(p, 1, 0);
        } else {
            launch_init(p, 1, NSHS_INIT_EVAL);
        }
        BBO_HIP(hipStreamSynchronize(stream_));
        return count;
    }
    if (k == "f") {             // fstd, the best and the worst follow; nothing is evaluated
        BBO_REQUIRE(count == c.hms, "f: hms values");
        std::vector<double> fh(in, in + count);
        nan_to_inf(fh.data(), count);
        f_.upload(fh.data(), c.hms, pb);
        launch_init(p, 1, 0);
        BBO_HIP(hipStreamSynchronize(stream_));
        return count;
    }
    if (k == "cand") {          // (what bbo_nshs_phase 1 evaluates)
        BBO_REQUIRE(count == c.n, "cand: n values");
        cand_.upload(in, c.n, (size_t) p * c.ld);
        return count;
    }
    if (k == "fcand") {         // (what bbo_nshs_phase 2 holds against the worst)
        BBO_REQUIRE(count == 1, "fcand: one value");
        double v = in[0];
        nan_to_inf(&v, 1);
        fcand_.upload(&v, 1, p);
        return 1;
    }
    if (k == "fev" || k == "it") {      // (the budget test looks at fev after the next iteration)
        BBO_REQUIRE(count == 1 && in[0] >= 0. && in[0] == std::floor(in[0]) && in[0] < 2147483647.,
                "fev, it: one non-negative integer");
        NshsScal s;
        scal_.download(&s, 1, p);
        (k == "fev" ? s.fev : s.it) = (int) in[0];
        scal_.upload(&s, 1, p);
        return 1;
    }
    throw Error(BBO_ERR_KEY, "unknown or read-only state key '" + k + "'");
}

Optimizer* make_nshs_engine(const bbo_params &p)
{
    return new NshsEngine(p);
}

} // namespace bbo
